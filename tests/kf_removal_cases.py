"""Scenes for key-frame removal (tests/test_kf_removal_ref.py, tests/test_gpu_kf_removal.py): hand-built ones, one per rule of the reference
that is easy to get wrong, each with the outputs that rule decides written out by hand (`want`, checked against the checker
tests/kf_removal_ref.py before anything else is), sized scenes for the kernels' edges, broken snapshots and the seeded random set, whose
maps and lists are the history that tests/covis_ref.py's UpdateConnections leaves on random observation scenes.
CASES: (name, scene, want). In `want`, conn / ord are {slot: [(key frame, weight), ...]} for the rows named, the rest are whole arrays."""
import numpy as np
from viorb_amd import kf_removal as M
from viorb_amd import covisibility as CV
import kf_removal_ref as T
import covis_ref as CT


def kf(pts=(), **k):
    return dict(pts=list(pts), **k)


def pt(*obs, **k):
    return dict(obs=list(obs), **k)


def rows(r, what, slot):
    n = int(r[what + "_n_out"][slot])
    return list(zip(r[what + "_kf_out"][slot][:n].tolist(), r[what + "_w_out"][slot][:n].tolist()))


def _cases():
    C = []
    add = lambda name, scene, want: C.append((name, scene, want))
    R, A, F, D, L = T.REMOVED, T.ALREADY_BAD, T.FIRST_KF, T.DEFERRED, T.RELEASED
    # 1. three children of X = 1 (parent 0): A = 2 is linked to the parent, B = 3 only to A, C = 4 to no candidate: A -> 0 in the first round, B -> A in
    # the second, C -> 0 by the fallback
    add("three_children", M.scene_from_lists([kf(id0=True), kf(parent=0), kf(parent=1, conn={0: 20}, ord=[(0, 20)]), kf(parent=1, conn={2: 10}, ord=[(2, 10)]), kf(parent=1)], [], [1]),
        dict(kf_parent_out=[-1, 0, 0, 2, 0], op_reason=[R], op_children=[3], op_fallback=[1], kf_touched=[0, 3, 4, 4, 4], kf_flags_out=[1, 2, 0, 0, 0]))
    # 2. a tie: children 2 and 3 both reach the parent 0 with weight 7. Pointer order is 3, 0, 1, 2: child 3 is searched first and the strict > keeps
    # it; child 2 then prefers the new candidate 3 (weight 9). In slot order child 2 would have won the first round and both would end under 0
    tie = lambda by_key: M.scene_from_lists([kf(id0=True), kf(parent=0), kf(parent=1, conn={0: 7, 3: 9}, ord=[(3, 9), (0, 7)]), kf(parent=1, conn={0: 7}, ord=[(0, 7)])], [], [1], by_key=by_key)
    add("tie_permuted_keys", tie([3, 0, 1, 2]), dict(kf_parent_out=[-1, 0, 3, 0], op_children=[2], op_fallback=[0]))
    add("tie_slot_order", tie(None), dict(kf_parent_out=[-1, 0, 0, 0], op_children=[2], op_fallback=[0]))
    # 3. a stale list entry: child 2's list names the parent 0 but its map does not: weight 0. It loses the first round to child 3 (weight 1), and in the
    # second it loses to child 2's own entry for the new candidate 3 (weight 5); had 0 > -1 not counted at all the child would fall back to 0 ...
    add("stale_list_entry_loses", M.scene_from_lists([kf(id0=True), kf(parent=0), kf(parent=1, conn={3: 5}, ord=[(0, 30), (3, 5)]), kf(parent=1, conn={0: 1}, ord=[(0, 1)])], [], [1]),
        dict(kf_parent_out=[-1, 0, 3, 0], op_fallback=[0]))
    # ... and alone it still beats -1: the child is taken in a round, not by the fallback
    add("stale_list_entry_beats_minus_one", M.scene_from_lists([kf(id0=True), kf(parent=0), kf(parent=1, ord=[(0, 30)])], [], [1]),
        dict(kf_parent_out=[-1, 0, 0], op_children=[1], op_fallback=[0]))
    # 4. key frame 2 holds X = 1 while X's own map does not hold it: it is not visited, its entry stays. Key frame 3 is in X's map and forgets it; its
    # rebuilt list pulls the sub-threshold 0 in
    add("one_sided_neighbour", M.scene_from_lists([kf(id0=True), kf(parent=0, conn={3: 16}, ord=[(3, 16)]), kf(parent=0, conn={1: 20}, ord=[(1, 20)]),
                                                   kf(parent=0, conn={1: 16, 0: 3}, ord=[(1, 16)])], [], [1]),
        dict(conn={1: [], 2: [(1, 20)], 3: [(0, 3)]}, ord={1: [], 2: [(1, 20)], 3: [(0, 3)]}, op_rebuilt=[1], kf_touched=[0, 3, 0, 3]))
    # 5. points of X = 1. p0: three mono observers, mpRefKF = X: nObs 2, bad, mpRefKF -> 0, its entries at 0 and 2 nulled. p1: a stereo observer 0 makes
    # nObs 4 -> 3: it survives. p2: bad on input with observers X and 2: the erase runs all the same, nObs 1, SetBadFlag again. p3 does not list X:
    # untouched. p4: X's own observation is the stereo one: 5 -> 3, survives
    add("points", M.scene_from_lists([kf([0, 1, 4], id0=True), kf([0, 1, 2, 3, -1, 4], parent=0), kf([0, 1, 2, 3, 4], parent=0), kf([3, 4], parent=0), kf([3], parent=0)],
                                     [pt(0, 1, 2, ref=1), pt((0, True), 1, 2), pt(1, 2, bad=True), pt(2, 3, 4), pt(0, (1, True), 2, 3, ref=1)], [1]),
        dict(pt_nobs_out=[2, 3, 1, 3, 3], pt_bad_out=[1, 0, 1, 0, 0], pt_ref_out=[0, 0, 2, 2, 0], obs_alive=[0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 0, 1, 1],
             kp_point_out=[-1, 1, 4, 0, 1, 2, 3, -1, 4, -1, 1, -1, 3, 4, 3, 4, 3], op_points_bad=[2]))
    # the erase empties mObservations: mpRefKF is begin() == end(), reported as -1
    add("last_observer", M.scene_from_lists([kf(id0=True), kf([0], parent=0)], [pt(1)], [1]), dict(pt_ref_out=[-1], pt_nobs_out=[0], pt_bad_out=[1], obs_alive=[0], kp_point_out=[0]))
    # 6. every guard, and the same slot twice
    add("guards", M.scene_from_lists([kf(id0=True), kf(bad=True, parent=0), kf(not_erase=True, parent=0), kf(parent=0)], [], [0, 1, 2, 3, 3]),
        dict(op_reason=[F, A, D, R, A], kf_flags_out=[1, 2, 12, 2], kf_parent_out=[-1, 0, 0, 0]))
    # 7. SetErase: with loop edges mbNotErase stays and the deferred removal is deferred again; without them it runs; a key frame never deferred is only released
    add("set_erase", M.scene_from_lists([kf(id0=True), kf(parent=0, not_erase=True, to_be_erased=True, loop_edges=True), kf(parent=0, not_erase=True, to_be_erased=True),
                                         kf(parent=0, not_erase=True), kf(parent=0)], [], [(1, 1), (2, 1), (3, 1), (4, 1), (3, 0)]),
        dict(op_reason=[D, R, L, L, R], kf_flags_out=[1, 28, 10, 2, 0]))
    # 8. the links 1 - 2 - 3 - 4: without prev, without next, and two adjacent removals in the middle
    chain = lambda ops: M.scene_from_lists([kf(id0=True)] + [kf(parent=0, prev=k - 1 if k > 1 else -1, next=k + 1 if k < 4 else -1) for k in range(1, 5)], [], ops)
    add("links_without_prev", chain([1]), dict(kf_prev_out=[-1, -1, -1, 2, 3], kf_next_out=[-1, -1, 3, 4, -1], kf_repreint=[0, 0, 0, 0, 0]))
    add("links_without_next", chain([4]), dict(kf_prev_out=[-1, -1, 1, 2, -1], kf_next_out=[-1, 2, 3, -1, -1], kf_repreint=[0, 0, 0, 0, 0]))
    add("links_adjacent", chain([2, 3]), dict(kf_prev_out=[-1, -1, -1, -1, 1], kf_next_out=[-1, 4, -1, -1, -1], kf_repreint=[0, 0, 0, 1, 1]))
    # 9. mTcp of a child removed under a parent that an earlier operation of the call gave it
    pose = lambda a, t: [np.cos(a), -np.sin(a), 0, np.sin(a), np.cos(a), 0, 0, 0, 1] + list(t)
    add("parent_assigned_earlier", M.scene_from_lists([kf(id0=True, pose=pose(0.1, [1, 2, 3])), kf(parent=0, pose=pose(0.2, [0, 1, 0])), kf(parent=1, pose=pose(-0.7, [3, -1, 0.5]))], [], [1, 2]),
        dict(kf_parent_out=[-1, 0, 0], op_reason=[R, R], op_children=[1, 0]))
    add("stream_without_operations", M.scene_from_lists([kf([0], conn={1: 4}, ord=[(1, 4)]), kf([0])], [pt(1)], []), dict(conn={0: [(1, 4)]}, kf_touched=[0, 0], pt_nobs_out=[1]))
    add("empty_stream", M.scene_from_lists([], [], []), dict(kf_touched=[], op_reason=[]))
    return C


def compare_want(r, want):
    """The entries of `want` that result r does not meet."""
    bad = []
    for f, v in want.items():
        if f in ("conn", "ord"):
            bad += [(f, k, rows(r, f, k)) for k, row in v.items() if rows(r, f, k) != row]
        elif np.asarray(r[f]).tolist() != v:
            bad.append((f, np.asarray(r[f]).tolist()))
    return bad


def random_pose(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    Rm = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
          2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    return np.array(Rm + (rng.normal(size=3) * 3).tolist(), np.float32)


def history(rng, tabs, n_pt, by_key, passes=2):
    """(conn, ord, final lists) per key frame after tests/covis_ref.py's UpdateConnections has run over the observation scene `tabs` (the
    points of every key frame), every key frame a target in slot order and then a random few again."""
    nk = len(tabs)
    obs = [[k for k in range(nk) if p in tabs[k]] for p in range(n_pt)]
    kfs = [dict(pts=tabs[k], first=False) for k in range(nk)]
    targets = list(range(nk)) + rng.choice(nk, size=min(nk, 3), replace=False).tolist()
    s = CV.scene_from_lists(kfs, [dict(obs=o) for o in obs], targets, by_key=by_key)
    r = CT.update_connections(s, ccap=nk)
    assert r["status"] == CT.OK
    return [dict(rows(r, "conn", k)) for k in range(nk)], [rows(r, "ord", k) for k in range(nk)], obs


def random_scene(rng, min_kf=6, max_kf=14, max_ops=6):
    """A random stream as the issue describes it: min_kf .. max_kf key frames with dense covisibility (every point has 3 to 5 observers, in half the
    streams from a run of 3 to 6 consecutive key frames; a key frame holds a point once), maps and lists from the covisibility checker's history (weights around the threshold 15, so ties and
    sub-threshold entries occur), a spanning tree in which a key frame's parent is its best older covisible, one prev / next chain in slot
    order, and 1 .. max_ops operations."""
    nk = int(rng.integers(min_kf, max_kf + 1))
    n_pt = int(rng.integers(2, 13)) * nk
    tabs = [[] for _ in range(nk)]
    window = int(rng.integers(3, 7)) if rng.random() < 0.5 else nk     # half the streams see a point only from a run of consecutive key frames
    for p in range(n_pt):
        first = int(rng.integers(0, nk - window + 1))
        for k in (first + rng.choice(window, size=min(window, int(rng.integers(3, 6))), replace=False)).tolist():
            tabs[k].append(p)
    for t in tabs:
        rng.shuffle(t)
        for i in rng.choice(len(t) + 1, size=2).tolist():
            t.insert(i, -1)
    by_key = rng.permutation(nk).tolist()
    conn, order, obs = history(rng, tabs, n_pt, by_key)
    kfs = []
    for k in range(nk):
        older = [c for c, _ in order[k] if c < k] or [c for c in conn[k] if c < k]
        not_erase = bool(k and rng.random() < 0.25)
        kfs.append(kf(tabs[k], conn=conn[k], ord=order[k], id0=(k == 0), parent=-1 if k == 0 else (older[0] if older else int(rng.integers(0, k))),
                      prev=k - 1, next=k + 1 if k + 1 < nk else -1, not_erase=not_erase, to_be_erased=bool(not_erase and rng.random() < 0.5),
                      loop_edges=bool(not_erase and rng.random() < 0.4), pose=random_pose(rng)))
    pts = []
    for p in range(n_pt):
        o = [(k, bool(rng.random() < 0.3)) for k in obs[p]]
        pts.append(pt(*o, ref=int(rng.choice(obs[p])) if rng.random() < 0.5 else obs[p][0]))
    n_ops = int(rng.integers(1, max_ops + 1))
    ops = [(0 if rng.random() < 0.08 else int(rng.integers(1, nk)), int(rng.random() < 0.3)) for _ in range(n_ops)]
    if rng.random() < 0.3:
        ops.append((ops[0][0], 0))
    return M.scene_from_lists(kfs, pts, ops, by_key=by_key)


SEEDS = tuple(range(100, 160))                                        # the seeds of the random set: one stream each
RANDOM_CCAP = 13                                                      # the most key frames of a random stream - 1
_RANDOM = {}


def random_streams():
    """The random set, the checker's outputs with rows of RANDOM_CCAP and the counts of the situations of kf_removal_ref.EVENTS, computed
    once and shared (nobody changes them)."""
    if not _RANDOM:
        scenes = [random_scene(np.random.default_rng(seed)) for seed in SEEDS]
        events = {}
        _RANDOM["set"] = (scenes, [T.remove_key_frames(s, ccap=RANDOM_CCAP, events=events) for s in scenes], events)
    return _RANDOM["set"]


def sparse_scene(seed, nk, n_pt=120, n_ops=5, degree=3):
    """nk key frames with a random tree, maps of at most 2 * degree entries with their full lists, a chain, n_pt points of 3 or 4 observers
    among the first 40 key frames, operations among them too: for the key-frame strides and the LDS limit."""
    rng = np.random.default_rng(seed)
    conn = [dict() for _ in range(nk)]
    for k in range(1, nk):
        for c in rng.integers(max(0, k - 50), k, degree).tolist():
            if len(conn[k]) < 2 * degree and len(conn[c]) < 2 * degree:
                conn[k][c] = conn[c][k] = int(rng.integers(1, 30))
    by_key = rng.permutation(nk).tolist()
    rank = {k: j for j, k in enumerate(by_key)}
    m = min(nk, 40)
    obs = [sorted(rng.choice(m, size=min(m, int(rng.integers(3, 5))), replace=False).tolist()) for _ in range(n_pt)]
    kfs = [kf([p for p in range(n_pt) if k in obs[p]] if k < m else [], conn=conn[k], ord=sorted(conn[k].items(), key=lambda kv: (kv[1], rank[kv[0]]), reverse=True),
              id0=(k == 0), parent=-1 if k == 0 else int(rng.integers(max(0, k - 6), k)), prev=k - 1, next=k + 1 if k + 1 < nk else -1, pose=random_pose(rng)) for k in range(nk)]
    ops = [int(x) for x in rng.choice(np.arange(1, m), size=min(n_ops, m - 1), replace=False)]
    return M.scene_from_lists(kfs, [pt(*o) for o in obs], ops, by_key=by_key)


def star_scene(seed, n_neigh, row, n_kp, n_child):
    """X = 1 under the first key frame 0. Its map holds n_neigh key frames (slots 2 ..), each of which holds X in a map of `row` entries; the
    first n_child of all the others are its children, each with a list over the parent, other children and strangers; X has n_kp keypoints
    on distinct points of 3 or 4 observers: for the strides over neighbours, rows, keypoints and children."""
    rng = np.random.default_rng(seed)
    nk = max(2 + n_neigh, 2 + n_child, row + 3, 8)
    by_key = rng.permutation(nk).tolist()
    rank = {k: j for j, k in enumerate(by_key)}
    full = lambda c: sorted(c.items(), key=lambda kv: (kv[1], rank[kv[0]]), reverse=True)
    conn = [dict() for _ in range(nk)]
    for k in range(2, 2 + n_neigh):
        conn[k][1] = conn[1][k] = int(rng.integers(1, 30))
        others = [o for o in rng.permutation(nk).tolist() if o not in (1, k)][:row - 1]
        for o in others:
            conn[k][o] = int(rng.integers(1, 30))
    for k in range(2, 2 + n_child):                                   # children: links to the parent or to another child, now and then in the list only
        for o in [0] * int(rng.random() < 0.4) + rng.integers(2, 2 + n_child, 2).tolist():
            if o != k and len(conn[k]) < nk - 2:
                conn[k].setdefault(o, int(rng.integers(1, 6)))
    obs = [[1] + rng.choice(np.array([0] + list(range(2, nk))), size=int(rng.integers(2, 4)), replace=False).tolist() for _ in range(n_kp)]
    kfs = [kf([p for p in range(n_kp) if k in obs[p]], conn=conn[k], ord=full(conn[k]), id0=(k == 0), parent=-1 if k == 0 else 1 if 2 <= k < 2 + n_child else 0,
              pose=random_pose(rng)) for k in range(nk)]
    return M.scene_from_lists(kfs, [pt(*o, ref=1 if rng.random() < 0.5 else None) for o in obs], [1], by_key=by_key)


def sized_scenes():
    """(name, scene, ccap or None) around the kernels' strides, read from viorb_remove_key_frames_shape."""
    thr, wave, lds_kf, waves = M.shape()
    out = []
    for d in (-1, 0, 1):
        out.append(("neighbours_%d" % (waves + d), star_scene(40 + d, waves + d, 4, 10, 2), None))
        out.append(("row_%d" % (wave + d), star_scene(50 + d, 3, wave + d, 10, 2), None))
        out.append(("keypoints_%d" % (thr + d), star_scene(60 + d, 3, 4, thr + d, 2), None))
    for n in (0, 1, wave + 1):
        out.append(("children_%d" % n, star_scene(70 + n, 3, 4, 10, n), None))
    for d in (0, 1):
        out.append(("kf_%d" % (lds_kf + d), sparse_scene(80 + d, lds_kf + d), 8))
    return out


def breakable_scene():
    """Five key frames in pointer order 2, 0, 3, 1, 4 under the first one; 1 and 3 are removed; 1 has a child, a map and a list of two entries."""
    pose = random_pose(np.random.default_rng(1))
    return M.scene_from_lists([kf([0, 1], id0=True, next=1, pose=pose), kf([0, 1, 2], parent=0, prev=0, next=2, conn={2: 3, 3: 16}, ord=[(3, 16), (2, 3)], pose=pose),
                               kf([1, 2], parent=1, prev=1, next=3, conn={1: 3}, ord=[(1, 3)]), kf([2, -1, 0], parent=0, prev=2, next=4, conn={1: 16}, ord=[(1, 16)], pose=pose),
                               kf([0], parent=3, prev=3)], [pt(0, 1, 3, 4), pt(0, (1, True), 2), pt(1, 2, 3, ref=3)], [1, (3, 1), 3], by_key=[2, 0, 3, 1, 4])


def broken(scene):
    """(what, scene) for every kind of broken snapshot the validator refuses, made from breakable_scene()."""
    nk, n_pt = len(scene["kf_flags"]), len(scene["pt_bad"])
    out = []

    def brk(what, field, index, value):
        s = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
        s[field][index] = value
        out.append((what, s))
    k1 = int(scene["kp_start"][1])
    brk("a point index at the end of the stream in an operation's keypoints", "kp_point", k1, n_pt)
    brk("a point index below -1 in an operation's keypoints", "kp_point", k1 + 1, -2)
    brk("an observation slot at the end", "obs", 0, nk)
    brk("descending keypoint offsets", "kp_start", 1, int(scene["kp_start"][2]) + 1)
    brk("a negative observation offset", "obs_start", 1, -4)
    brk("a conn offset past the total", "conn_start", 1, 1 << 28)
    brk("descending ord offsets", "ord_start", 2, int(scene["ord_start"][1]) - 1)
    brk("a parent outside the snapshot", "kf_parent", 2, nk)
    brk("kf_by_key with a slot twice", "kf_by_key", 0, int(scene["kf_by_key"][1]))
    brk("kf_by_key with a slot out of range", "kf_by_key", 1, nk)
    brk("a conn slot past the end", "conn_kf", 0, nk)
    brk("a conn row out of key order", "conn_kf", slice(0, 2), scene["conn_kf"][1::-1].copy())
    brk("a conn row with a slot twice", "conn_kf", 0, int(scene["conn_kf"][1]))
    brk("a conn row that names its own key frame", "conn_kf", 0, 1)
    brk("an ord slot below 0", "ord_kf", 0, -1)
    brk("an ord row with a slot twice", "ord_kf", 0, int(scene["ord_kf"][1]))
    brk("an operation outside the snapshot", "op_kf", 0, nk)
    brk("a negative operation", "op_kf", 1, -1)
    brk("an operation kind above 1", "op_kind", 1, 2)
    brk("a prev outside the snapshot", "kf_prev", 4, nk)
    brk("a next below -1", "kf_next", 0, -2)
    brk("an mpRefKF outside the snapshot", "pt_ref", 1, nk)
    brk("an observation count of 2^29", "pt_nobs", 2, 1 << 29)
    brk("an operation's key frame without a parent", "kf_parent", 3, -1)
    brk("a cycle of parents through an operation's key frame", "kf_parent", 0, 3)
    brk("a parent that is the operation's key frame itself", "kf_parent", 1, 1)
    brk("a non-finite pose of an operation's key frame", "kf_pose12", (3, 10), np.inf)
    brk("a non-finite pose of an operation's parent", "kf_pose12", (0, 4), np.nan)
    return out


CASES = _cases()


def expected(name):
    _, scene, _ = next(c for c in CASES if c[0] == name)
    return T.remove_key_frames(scene)


# ---- the chains: culling -> removal -> covisibility ------------------------------------------------------------------------------------------
def chain_in_scene(seed):
    """(culling scene, removal scene without operations) over one map that is valid for both entries: every point has 4 to 6 observers at
    octave 0, so most candidates are redundant; a chain in slot order, the last key frame the current one, a few with mbNotErase."""
    from viorb_amd import culling as CU
    rng = np.random.default_rng(seed)
    nk = int(rng.integers(8, 13))
    n_pt = 10 * nk
    obs = [sorted(rng.choice(nk, size=int(rng.integers(4, 7)), replace=False).tolist()) for _ in range(n_pt)]
    stereo = [[bool(rng.random() < 0.3) for _ in o] for o in obs]
    tabs = [[p for p in range(n_pt) if k in obs[p]] for k in range(nk)]
    for t in tabs:
        rng.shuffle(t)
        t.insert(int(rng.integers(0, len(t) + 1)), -1)
    not_erase = [bool(0 < k and rng.random() < 0.25) for k in range(nk)]
    link = lambda k: dict(prev=k - 1, next=k + 1 if k + 1 < nk else -1)
    cands = [int(c) for c in rng.permutation(nk - 1)]
    cull = CU.scene_from_lists([dict(t=float(k), first=(k == 0), not_erase=not_erase[k], **link(k)) for k in range(nk)], nk - 1,
                               [(c, [(p, 0, 1.0) for p in tabs[c]]) for c in cands], [dict(obs=[(k, 0, st) for k, st in zip(o, s)]) for o, s in zip(obs, stereo)], vins_inited=True)
    removal = lambda ops: M.scene_from_lists([kf(tabs[k], id0=(k == 0), not_erase=not_erase[k], parent=k - 1, pose=random_pose(rng), **link(k)) for k in range(nk)],
                                             [pt(*zip(o, s)) for o, s in zip(obs, stereo)], ops, by_key=rng.permutation(nk).tolist())
    return cull, removal


def chain_in_operations(cull, cr):
    """The operations the culling's result asks for: SetBadFlag on the culled and the deferred candidates, in candidate order."""
    from viorb_amd import culling as CU
    return [int(c) for c, why in zip(cull["cand_kf"], cr["cand_reason"]) if why in (CU.CULLED, CU.DEFERRED)]


def chain_in_differences(cr, r):
    """The outputs of the removal r that differ from the culling's own cr."""
    bad = [f for f in ("pt_nobs_out", "pt_bad_out", "obs_alive", "kf_prev_out", "kf_next_out", "kf_repreint") if not np.array_equal(cr[f], r[f])]
    bad += ["mbBad"] if not np.array_equal(cr["kf_bad"] != 0, (r["kf_flags_out"] & M.KF_BAD) != 0) else []
    bad += ["mbToBeErased"] if not np.array_equal(cr["kf_to_be_erased"] != 0, (r["kf_flags_out"] & M.KF_TO_BE_ERASED) != 0) else []
    return bad


def covis_scene_after(s, r, targets):
    """The covisibility scene (viorb_amd/covisibility.py) a removal's result r leaves of the removal scene s: the rows, kf_parent_out, pt_bad_out,
    the keypoint tables after EraseMapPointMatch and the observations that are still in mObservations; no first connection is pending."""
    nk = len(s["kf_flags"])
    cn, on = r["conn_n_out"], r["ord_n_out"]
    c = dict(targets=np.array(targets, np.int32), kf_by_key=s["kf_by_key"], kf_flags=(s["kf_flags"] & M.KF_ID0).astype(np.uint8), kf_parent=r["kf_parent_out"],
             kp_start=s["kp_start"], kp_point=r["kp_point_out"], pt_bad=r["pt_bad_out"])
    alive = r["obs_alive"] != 0
    per_pt = np.add.reduceat(np.concatenate([alive, [False]]).astype(np.int64), np.minimum(s["obs_start"][:-1], len(alive))) if len(s["pt_bad"]) else np.zeros(0, np.int64)
    per_pt = np.where(s["obs_start"][1:] > s["obs_start"][:-1], per_pt, 0)
    c["obs_start"], c["obs"] = np.concatenate([[0], np.cumsum(per_pt)]).astype(np.int32), s["obs"][alive]
    for what, n in (("conn", cn), ("ord", on)):
        keep = np.arange(r[what + "_kf_out"].shape[1])[None, :] < n[:, None]
        c[what + "_start"] = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        c[what + "_kf"], c[what + "_w"] = r[what + "_kf_out"][keep], r[what + "_w_out"][keep]
    assert len(c["conn_start"]) == nk + 1
    return c


def surviving_targets(s, r, rng, n=4):
    good = np.where((r["kf_flags_out"] & M.KF_BAD) == 0)[0]
    return [int(k) for k in rng.choice(good, size=min(n, len(good)), replace=False)]
