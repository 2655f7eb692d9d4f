"""Scenes for KeyFrame::UpdateConnections (tests/test_covis_ref.py, tests/test_gpu_covis.py): hand-built ones, one per rule of the
reference that is easy to get wrong, each with the outputs it must give written out by hand (`want`, checked against the checker
tests/covis_ref.py before anything else is), sized scenes for the kernels' edges, broken snapshots and a random generator.
CASES: (name, scene, args, want). In `want`, conn / ord are {slot: [(key frame, weight), ...]} for the rows named, the rest are whole arrays."""
import numpy as np
from viorb_amd import covisibility as M
import covis_ref as T


def kf(pts=(), **k):
    return dict(pts=list(pts), **k)


def pt(*obs, bad=False):
    return dict(obs=list(obs), bad=bad)


def rows(r, what, slot):
    """Row `slot` of conn / ord of a result as [(key frame, weight)], cut to its count."""
    n = int(r[what + "_n_out"][slot])
    return list(zip(r[what + "_kf_out"][slot][:n].tolist(), r[what + "_w_out"][slot][:n].tolist()))


def _cases():
    C = []
    add = lambda name, scene, want, **args: C.append((name, scene, args, want))
    # 1. votes: point 0 sits on two keypoints of the target and votes twice for its observer 1 (the target's own observation gives none); point 1
    # is bad and gives none; the null keypoint gives none; point 2 votes for 1 and 2, point 3 for 3. Nobody reaches 15: pKFmax = 1 alone is added
    add("votes", M.scene_from_lists([kf([0, 0, 1, -1, 2, 3]), kf(), kf(), kf()], [pt(0, 1), pt(2, bad=True), pt(1, 2), pt(3)], [0]),
        dict(t_observers=[3], t_max_kf=[1], t_max_w=[3], t_added=[1], conn={0: [(1, 3), (2, 1), (3, 1)], 1: [(0, 3)], 2: [], 3: []}, ord={0: [(1, 3)], 1: [(0, 3)], 2: []},
             kf_touched=[3, 3, 0, 0], t_parent=[1], kf_parent_out=[1, -1, -1, -1]))
    # 2. no observers: the target's only good point is observed by itself alone. Nothing changes, the first-connection flag included
    add("no_observers", M.scene_from_lists([kf([0, -1, 1], conn={1: 5}, ord=[(1, 5)]), kf([1])], [pt(0), pt(1, bad=True)], [0]),
        dict(t_observers=[0], t_max_kf=[-1], t_max_w=[0], t_added=[0], t_parent=[-1], conn={0: [(1, 5)], 1: []}, ord={0: [(1, 5)]}, kf_touched=[0, 0], kf_flags_out=[2, 2],
             kf_parent_out=[-1, -1], n_loop_conn=[0]))
    # 3. nmax / pKFmax: slots 0 and 2 have two votes each; pointer order is 2, 0, 1, 3: slot 2 is walked first and the strict > keeps it
    add("tie_lowest_key_wins", M.scene_from_lists([kf(), kf(), kf(), kf([0, 1, 2])], [pt(0, 2), pt(0, 2), pt(1)], [3], by_key=[2, 0, 1, 3]),
        dict(t_observers=[3], t_max_kf=[2], t_max_w=[2], t_added=[1], conn={3: [(2, 2), (0, 2), (1, 1)], 2: [(3, 2)], 0: []}, ord={3: [(2, 2)]}, t_parent=[2]))
    # 4. the threshold: 15 votes are added, 14 are not (they stay in the target's map only) ...
    add("threshold_15_and_14", M.scene_from_lists([kf([0] * 15 + [1] * 14), kf(), kf()], [pt(1), pt(2)], [0]),
        dict(t_observers=[2], t_max_kf=[1], t_max_w=[15], t_added=[1], conn={0: [(1, 15), (2, 14)], 1: [(0, 15)], 2: []}, ord={0: [(1, 15)], 2: []}, kf_touched=[3, 3, 0]))
    # ... unless nobody reaches 15: then pKFmax alone, with nmax = 14
    add("threshold_14_fallback", M.scene_from_lists([kf([1] * 14 + [0] * 3), kf(), kf()], [pt(1), pt(2)], [0]),
        dict(t_observers=[2], t_max_kf=[2], t_max_w=[14], t_added=[1], conn={0: [(1, 3), (2, 14)], 1: [], 2: [(0, 14)]}, ord={0: [(2, 14)], 2: [(0, 14)]}, kf_touched=[3, 0, 3]))
    # 5. the target's own state: its map is the whole counter in key order (pointer order 0, 3, 1, 2, 4), the sub-threshold slot 4 included; its
    # list holds the added ones by descending weight and, at 15 each, slot 2 (key 3) before slot 1 (key 2)
    add("own_state_order", M.scene_from_lists([kf([0] * 15 + [1] * 15 + [2] * 20 + [3] * 3), kf(), kf(), kf(), kf()], [pt(1), pt(2), pt(3), pt(4)], [0], by_key=[0, 3, 1, 2, 4]),
        dict(t_observers=[4], t_max_kf=[3], t_max_w=[20], t_added=[3], conn={0: [(3, 20), (1, 15), (2, 15), (4, 3)]}, ord={0: [(3, 20), (2, 15), (1, 15)]}, t_parent=[3]))
    # the parent is the front of the list, not pKFmax: 15 votes each for slots 1 and 2, pKFmax is the lower key 1, the front the higher key 2
    add("parent_is_front_not_pkfmax", M.scene_from_lists([kf([0] * 15 + [1] * 15), kf(), kf()], [pt(1), pt(2)], [0]),
        dict(t_max_kf=[1], t_parent=[2], kf_parent_out=[2, -1, -1], ord={0: [(2, 15), (1, 15)]}))
    # 6. AddConnection: slots 1 and 2 were targets earlier and hold a thresholded list beside a map with the sub-threshold slot 3. The target's
    # weight in slot 1 is unchanged (20): early return, the list stays as it is. In slot 2 it changes (20 -> 21): the rebuild pulls slot 3 in
    add("add_connection_kept_and_rebuilt",
        M.scene_from_lists([kf([0] * 20 + [1] * 21), kf(conn={0: 20, 3: 3}, ord=[(0, 20)]), kf(conn={0: 20, 3: 3}, ord=[(0, 20)]), kf()], [pt(1), pt(2)], [0]),
        dict(conn={1: [(0, 20), (3, 3)], 2: [(0, 21), (3, 3)]}, ord={1: [(0, 20)], 2: [(0, 21), (3, 3)], 0: [(2, 21), (1, 20)]}, kf_touched=[3, 0, 3, 0], t_added=[2]))
    # 7. stale entries: slot 1 was connected to the target and observes none of its points any more: it keeps the target in its map and list
    add("stale_entry_kept", M.scene_from_lists([kf([0] * 15, conn={1: 16}, ord=[(1, 16)]), kf(conn={0: 16}, ord=[(0, 16)]), kf()], [pt(2)], [0]),
        dict(conn={0: [(2, 15)], 1: [(0, 16)], 2: [(0, 15)]}, ord={0: [(2, 15)], 1: [(0, 16)]}, kf_touched=[3, 0, 3]))
    # 8. the first connection: slot 0 has mnId 0 and never gets a parent, its flag stays; slot 1 takes the front of its new list and clears it
    add("first_connection", M.scene_from_lists([kf([0] * 15, id0=True), kf([0] * 15)], [pt(0, 1)], [0, 1]),
        dict(kf_parent_out=[-1, 0], kf_flags_out=[3, 0], t_parent=[-1, 0], ord={0: [(1, 15)], 1: [(0, 15)]}))
    add("no_first_connection_keeps_parent", M.scene_from_lists([kf([0] * 15, first=False, parent=2), kf(), kf()], [pt(1)], [0]),
        dict(kf_parent_out=[2, -1, -1], kf_flags_out=[0, 2, 2], t_parent=[-1]))
    # 9. LoopConnections of the group 0, 1. Target 0: the map after the call {1, 2, 3} without its list before the call {2}: {1, 3}, and
    # without the group: {3}. Target 1: its list before its own call already holds 0, put there by target 0's AddConnection (its input list is
    # empty): {0, 4} without {0} = {4}
    loop = lambda: M.scene_from_lists([kf([0] * 15 + [1] * 16 + [2] * 15, conn={2: 30}, ord=[(2, 30)]), kf([0] * 15 + [3] * 15), kf(), kf(), kf()],
                                      [pt(0, 1), pt(2), pt(3), pt(4)], [0, 1])
    add("loop_connections", loop(), dict(loop_conn=[[1, 3], [4]], n_loop_conn=[2, 1], ord={1: [(4, 15), (0, 15)]}))
    add("loop_connections_erase_targets", loop(), dict(loop_conn=[[3], [4]], n_loop_conn=[1, 1]), erase_targets=1)
    # a repeated target: the second call finds every weight unchanged (early returns) and no first connection left
    add("repeated_target", M.scene_from_lists([kf([0] * 15 + [1] * 2), kf(), kf()], [pt(1), pt(2)], [0, 0]),
        dict(t_observers=[2, 2], t_added=[1, 1], t_parent=[1, -1], kf_parent_out=[1, -1, -1], conn={0: [(1, 15), (2, 2)], 1: [(0, 15)]}, n_loop_conn=[2, 1]))
    add("stream_without_targets", M.scene_from_lists([kf([0], conn={1: 4}, ord=[(1, 4)]), kf()], [pt(1)], []), dict(conn={0: [(1, 4)]}, ord={0: [(1, 4)]}, kf_touched=[0, 0]))
    add("empty_stream", M.scene_from_lists([], [], []), dict(t_observers=[], kf_touched=[]))
    add("only_target_without_observers", M.scene_from_lists([kf([-1, 0])], [pt(bad=True)], [0]), dict(t_observers=[0], kf_flags_out=[2], n_loop_conn=[0]))
    # one more entry than ccap, in the target's own map and in the map of a key frame it adds itself to; and exactly ccap
    add("overflow_own_map", M.scene_from_lists([kf([0, 1, 2]), kf(), kf(), kf()], [pt(1), pt(2), pt(3)], [0]), dict(status=T.OVERFLOW, need=3), ccap=2)
    add("own_map_exact", M.scene_from_lists([kf([0, 1, 2]), kf(), kf(), kf()], [pt(1), pt(2), pt(3)], [0]), dict(status=T.OK, need=0, t_observers=[3]), ccap=3)
    add("overflow_added_map", M.scene_from_lists([kf([0] * 15), kf(conn={2: 1, 3: 1}), kf(), kf()], [pt(1)], [0]), dict(status=T.OVERFLOW, need=3), ccap=2)
    add("added_map_exact", M.scene_from_lists([kf([0] * 15), kf(conn={2: 1, 3: 1}), kf(), kf()], [pt(1)], [0]),
        dict(status=T.OK, conn={1: [(0, 15), (2, 1), (3, 1)]}, ord={1: [(0, 15), (3, 1), (2, 1)]}), ccap=3)
    return C


def compare_want(r, want):
    """The entries of `want` that result r does not meet."""
    bad = []
    for f, v in want.items():
        if f in ("conn", "ord"):
            bad += [(f, k, rows(r, f, k)) for k, row in v.items() if rows(r, f, k) != row]
        elif f == "loop_conn":
            got = [r[f][t][:r["n_loop_conn"][t]].tolist() for t in range(len(v))]
            bad += [(f, got)] if got != v else []
        elif f in ("status", "need"):
            bad += [(f, r[f])] if r[f] != v else []
        elif np.asarray(r[f]).tolist() != v:
            bad.append((f, np.asarray(r[f]).tolist()))
    return bad


def sized_scene(seed, nk, nkp, n_targets=3, n_pt=40):
    """nk key frames, the first n_targets of them the targets with nkp keypoints each (the rest have none: only the targets' are read), random
    maps and lists of a few entries: for the strides of the vote and scan loops."""
    rng = np.random.default_rng(seed)
    pts = [pt(*rng.choice(nk, size=min(nk, int(rng.integers(0, 5))), replace=False).tolist(), bad=bool(rng.random() < 0.1)) for _ in range(n_pt)]
    kfs = []
    for k in range(nk):
        others = [o for o in rng.choice(nk, size=min(nk, 4), replace=False).tolist() if o != k]
        conn = {o: int(rng.integers(1, 40)) for o in others}
        kfs.append(kf([int(p) if rng.random() < 0.9 else -1 for p in rng.integers(0, n_pt, nkp)] if k < n_targets else [], conn=conn,
                      ord=[(o, w) for o, w in conn.items() if w >= 15], first=bool(rng.random() < 0.5), id0=(k == 1)))
    return M.scene_from_lists(kfs, pts, list(range(min(n_targets, nk))), by_key=rng.permutation(nk).tolist())


def insert_scene(seed, row, where):
    """Key frame 1 holds a map of `row` entries (slots 2 ..) and its full list; the target 0 gives it 15 votes and is not in the map: the insert
    lands at the front, in the middle or at the end of the row as the target's key is the lowest, the median or the highest."""
    rng = np.random.default_rng(seed)
    nk = row + 2
    conn = {k: int(rng.integers(1, 40)) for k in range(2, nk)}
    order = rng.permutation(np.arange(1, nk)).tolist()
    order.insert({"front": 0, "middle": len(order) // 2, "end": len(order)}[where], 0)
    rank = {k: j for j, k in enumerate(order)}
    full = sorted(conn.items(), key=lambda kv: (kv[1], rank[kv[0]]), reverse=True)
    kfs = [kf([0] * 15), kf(conn=conn, ord=full)] + [kf() for _ in range(row)]
    return M.scene_from_lists(kfs, [pt(1)], [0], by_key=order)


def sized_scenes():
    """(name, scene, ccap or None): keypoint counts around the threads of the vote phase, rows of 63, 64 and 65 entries before and after
    an insert at the front, in the middle and at the end, a row that reaches exactly ccap and one that needs ccap + 1, key-frame counts around
    the threads of the scans and at and above the LDS limit."""
    thr, wave, lds_kf, _ = M.shape()
    out = []
    for d in (-1, 0, 1):
        out.append(("kp_%d" % (thr + d), sized_scene(10 + d, 6, thr + d), None))
        out.append(("kf_%d" % (thr + d), sized_scene(20 + d, thr + d, 40, n_pt=300), None))
    for i, row in enumerate((wave - 2, wave - 1, wave, wave + 1, 2 * wave - 1, 2 * wave)):
        for j, where in enumerate(("front", "middle", "end")):
            out.append(("insert_%s_%d" % (where, row), insert_scene(100 + 3 * i + j, row, where), None))
    out.append(("row_reaches_ccap", insert_scene(150, wave, "middle"), wave + 1))
    out.append(("row_needs_ccap_plus_1", insert_scene(150, wave, "middle"), wave))
    for d in (0, 1):
        out.append(("kf_%d" % (lds_kf + d), sized_scene(30 + d, lds_kf + d, 70, n_targets=4, n_pt=600), 300))
    return out


def random_scene(rng, min_kf=2, max_kf=40, max_targets=6):
    """A random stream of min_kf .. max_kf key frames and 1 .. max_targets targets (now and then one twice). Few points on many keypoints, so
    that weights pass 15; the maps and lists are what a history could have left: weights that are the votes of now (early returns) or others,
    entries for key frames that share nothing any more (stale), lists that are the whole map in order, thresholded, or empty."""
    nk = int(rng.integers(min_kf, max_kf + 1))
    n_pt = int(rng.integers(1, 25))
    p_bad = rng.choice([0.0, 0.1])
    pts = [pt(*rng.choice(nk, size=min(nk, int(rng.integers(0, 5))), replace=False).tolist(), bad=bool(rng.random() < p_bad)) for _ in range(n_pt)]
    by_key = rng.permutation(nk).tolist()
    rank = {k: j for j, k in enumerate(by_key)}
    tabs = [[int(p) if rng.random() < 0.9 else -1 for p in rng.integers(0, n_pt, int(rng.integers(0, 90)))] for _ in range(nk)]
    votes = []
    for k in range(nk):
        c = {}
        for p in tabs[k]:
            if p >= 0 and not pts[p]["bad"]:
                for o in pts[p]["obs"]:
                    if o != k:
                        c[o] = c.get(o, 0) + 1
        votes.append(c)
    kfs = []
    for k in range(nk):
        conn = {}
        for o in range(nk):
            if o == k or rng.random() < 0.6:
                continue
            now = votes[o].get(k, 0)                                    # what o as a target would hand to k
            conn[o] = now if now and rng.random() < 0.5 else int(rng.integers(1, 40))
        full = sorted(conn.items(), key=lambda kv: (kv[1], rank[kv[0]]), reverse=True)
        mode = rng.random()
        order = full if mode < 0.4 else [e for e in full if e[1] >= 15] if mode < 0.8 else []
        first = bool(rng.random() < 0.5)                                # as in the reference, a key frame has no parent before its first connection
        kfs.append(kf(tabs[k], conn=conn, ord=order, first=first, id0=bool(k == 0 and rng.random() < 0.5), parent=-1 if first else int(rng.integers(-1, nk))))
    targets = rng.choice(nk, size=min(nk, int(rng.integers(1, max_targets + 1))), replace=False).tolist()
    if rng.random() < 0.15:
        targets.append(targets[0])
    return M.scene_from_lists(kfs, pts, targets, by_key=by_key)


_RANDOM = {}
RANDOM_CCAP = 39                                                      # the most key frames of a random stream - 1: nothing overflows


def random_streams(seed=5, n=300):
    """n random streams, the checker's outputs with erase_targets = 1 and rows of RANDOM_CCAP, and the counts of the situations of covis_ref.EVENTS, computed once and
    shared (nobody changes them)."""
    if (seed, n) not in _RANDOM:
        rng = np.random.default_rng(seed)
        scenes = [random_scene(rng) for _ in range(n)]
        events = {}
        _RANDOM[(seed, n)] = (scenes, [T.update_connections(s, ccap=RANDOM_CCAP, erase_targets=1, events=events) for s in scenes], events)
    return _RANDOM[(seed, n)]


def broken(scene):
    """(what, scene) for every kind of broken snapshot the validator refuses, made from breakable_scene()."""
    nk, n_pt = len(scene["kf_flags"]), len(scene["pt_bad"])
    out = []

    def brk(what, field, index, value):
        s = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
        s[field][index] = value
        out.append((what, s))
    brk("a point index at the end of the stream in a target's keypoints", "kp_point", 0, n_pt)
    brk("a point index below -1 in a target's keypoints", "kp_point", 1, -2)
    brk("an observation slot at the end", "obs", 0, nk)
    brk("descending keypoint offsets", "kp_start", 1, int(scene["kp_start"][2]) + 1)
    brk("a negative observation offset", "obs_start", 1, -4)
    brk("a conn offset past the total", "conn_start", 1, 1 << 28)
    brk("descending ord offsets", "ord_start", 2, int(scene["ord_start"][1]) - 1)
    brk("a parent outside the snapshot", "kf_parent", 1, nk)
    brk("kf_by_key with a slot twice", "kf_by_key", 0, int(scene["kf_by_key"][1]))
    brk("kf_by_key with a slot out of range", "kf_by_key", 1, nk)
    brk("a conn slot past the end", "conn_kf", 0, nk)
    brk("a conn row out of key order", "conn_kf", slice(0, 2), scene["conn_kf"][1::-1].copy())
    brk("a conn row with a slot twice", "conn_kf", 0, int(scene["conn_kf"][1]))
    brk("a conn row that names its own key frame", "conn_kf", 0, 0)
    brk("an ord slot below 0", "ord_kf", 0, -1)
    brk("an ord row with a slot twice", "ord_kf", 0, int(scene["ord_kf"][1]))
    brk("a target outside the snapshot", "targets", 0, nk)
    brk("a negative target", "targets", 1, -1)
    return out


def breakable_scene():
    """Four key frames in pointer order 2, 0, 3, 1; key frame 0 has a map and a list of two entries (2 before 3 in key order)."""
    return M.scene_from_lists([kf([0, 1, 0], conn={2: 3, 3: 16}, ord=[(3, 16), (2, 3)]), kf([1, 2], conn={0: 2}, parent=0), kf([2, -1], conn={1: 20}, ord=[(1, 20)]), kf([0])],
                              [pt(0, 3), pt(0, 1), pt(1, 2)], [0, 2], by_key=[2, 0, 3, 1])


CASES = _cases()


def expected(name):
    _, scene, args, _ = next(c for c in CASES if c[0] == name)
    return T.update_connections(scene, ccap=args.get("ccap"), erase_targets=args.get("erase_targets", 0))
