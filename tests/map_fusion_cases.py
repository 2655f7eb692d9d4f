"""Scenes for the map-fusion tests: hand-built ones with hand-written expectations, scenes sized around the strides viorb_apply_fuse_shape
reports, every kind of broken snapshot in the middle of three streams, and a seeded random set. The expectations of the sized, broken
and random scenes come from the checker tests/map_fusion_ref.py."""
import numpy as np
from viorb_amd import map_fusion as M
import map_fusion_ref as T

A, RK, RC, CO, SB, SI, NO, NU = T.ADDED, T.REPLACED_KF_POINT, T.REPLACED_CANDIDATE, T.COUNTED_ONLY, T.SKIP_BAD, T.SKIP_IN_KF, T.NONE, T.NULL_POINT


def K(*pts, **kw):
    return dict(pts=list(pts), **kw)


def P(*obs, **kw):
    return dict(obs=list(obs), **kw)


def _case(name, kfs, pts, calls, want, **kw):
    return name, M.scene_from_lists(kfs, pts, calls, **kw), want


def _cases():
    c = []
    # a candidate lands on an empty feature: AddObservation + AddMapPoint, 1 for a mono keypoint and 2 for a stereo one
    add_kfs = [K(-1, -1, 0, stereo=[0, 1, 0], octave=[0, 3, 1]), K(0, 1), K(1, 2)]
    add_pts = [P((0, 2), (1, 0)), P((1, 1), (2, 0)), P((2, 1))]
    c.append(_case("add", add_kfs, add_pts, [(0, T.POSE, [1, 2], [0, 1])],
                   dict(kp=[[1, 2, 0], [0, 1], [1, 2]], bad=[0, 0, 0], nobs=[2, 3, 3], reason=[A, A], other=[-1, -1], nfused=[1 + 1], dirty=[0, 0, 0],
                        obs=[[(0, 2), (1, 0)], [(0, 0), (1, 1), (2, 0)], [(0, 1), (2, 1)]], words={(2, 0): (0, 3, 1, 1)})))
    # the key frame's point has no more observations than the candidate: it is replaced, found / visible move over
    c.append(_case("replace_kf_point", [K(0), K(1), K(1)], [P((0, 0), found=5, visible=7), P((1, 0), (2, 0), found=10, visible=20)], [(0, T.POSE, [1], [0])],
                   dict(kp=[[1], [1], [1]], bad=[1, 0], nobs=[1, 3], reason=[RK], other=[0], nfused=[1], dirty=[0, 1], replaced=[1, -1], found=[5, 15], visible=[7, 27],
                        obs=[[], [(0, 0), (1, 0), (2, 0)]], dirty_lists=[[], [(0, 0), (1, 0), (2, 0)]], touched=[1, 0, 0])))
    # the key frame's point has more: the candidate is replaced
    rc_kfs, rc_pts = [K(0), K(0), K(0), K(1)], [P((0, 0), (1, 0), (2, 0)), P((3, 0))]
    c.append(_case("replace_candidate", rc_kfs, rc_pts, [(0, T.POSE, [1], [0])],
                   dict(kp=[[0], [0], [0], [0]], bad=[0, 1], nobs=[4, 1], reason=[RC], other=[0], nfused=[1], dirty=[1, 0], replaced=[-1, 0],
                        obs=[[(0, 0), (1, 0), (2, 0), (3, 0)], []])))
    # equal counts: the key frame's point goes
    tie_kfs, tie_pts = [K(0), K(0), K(1), K(1)], [P((0, 0), (1, 0)), P((2, 0), (3, 0))]
    c.append(_case("tie", tie_kfs, tie_pts, [(0, T.POSE, [1], [0])],
                   dict(kp=[[1], [1], [1], [1]], bad=[1, 0], nobs=[2, 4], reason=[RK], other=[0], nfused=[1], obs=[[], [(0, 0), (1, 0), (2, 0), (3, 0)]])))
    # the key frame's point is bad: counted and nothing else
    c.append(_case("bad_in_kf", [K(0), K(1)], [P((0, 0), bad=True), P((1, 0))], [(0, T.POSE, [1], [0])],
                   dict(kp=[[0], [1]], bad=[1, 0], nobs=[1, 1], reason=[CO], other=[0], nfused=[1], dirty=[0, 0], obs=[[(0, 0)], [(1, 0)]])))
    # the survivor already lists one of the replaced point's observers: EraseMapPointMatch there
    c.append(_case("shared_observer", [K(0), K(0, 1), K(1), K(1)], [P((0, 0), (1, 0)), P((1, 1), (2, 0), (3, 0))], [(0, T.POSE, [1], [0])],
                   dict(kp=[[1], [-1, 1], [1], [1]], bad=[1, 0], nobs=[2, 4], reason=[RK], nfused=[1], obs=[[], [(0, 0), (1, 1), (2, 0), (3, 0)]], touched=[1, 1, 0, 0, 0])))
    # the key frame's table holds the candidate although its observations do not name the key frame: Replace returns at once
    c.append(_case("same_point", [K(1), K(1)], [P(), P((1, 0))], [(0, T.POSE, [1], [0])],
                   dict(kp=[[1], [1]], bad=[0, 0], nobs=[0, 1], reason=[RK], other=[1], nfused=[1], dirty=[0, 0], replaced=[-1, -1], obs=[[], [(1, 0)]])))
    # a listed duplicate: the first entry makes the point bad, the second sees it
    c.append(_case("duplicate_goes_bad", rc_kfs, rc_pts, [(0, T.POSE, [1, 1], [0, 0])],
                   dict(kp=[[0], [0], [0], [0]], bad=[0, 1], nobs=[4, 1], reason=[RC, SB], other=[0, -1], nfused=[1])))
    # a listed duplicate: the first entry puts the point into the key frame, the second sees it
    c.append(_case("duplicate_enters_kf", add_kfs, add_pts, [(0, T.POSE, [1, 1], [0, 1])],
                   dict(kp=[[1, -1, 0], [0, 1], [1, 2]], nobs=[2, 3, 1], reason=[A, SI], nfused=[1])))
    c.append(_case("null_entry", add_kfs, add_pts, [(0, T.POSE, [-1, 1, 0], [0, 0, -1])],
                   dict(kp=[[1, -1, 0], [0, 1], [1, 2]], nobs=[2, 3, 1], reason=[NU, A, SI], nfused=[1])))
    # SIM3: the second entry lands on the feature the first one filled; the replace runs after the loop
    c.append(_case("sim3_lands_on_filled", [K(-1), K(0), K(1)], [P((1, 0)), P((2, 0))], [(0, T.SIM3, [0, 1], [0, 0])],
                   dict(kp=[[1], [1], [1]], bad=[1, 0], nobs=[2, 3], reason=[A, RK], other=[-1, 0], nfused=[2], replaced=[1, -1], obs=[[], [(0, 0), (1, 0), (2, 0)]])))
    # SIM3: two entries record the same live point; the second Replace runs on a point that is already bad
    c.append(_case("sim3_replace_of_bad", [K(0), K(1), K(2)], [P((0, 0), found=3, visible=4), P((1, 0), found=10), P((2, 0), found=100)],
                   [(0, T.SIM3, [1, 2], [0, 0])],
                   dict(kp=[[1], [1], [2]], bad=[1, 0, 0], nobs=[1, 2, 1], reason=[RK, RK], other=[0, 0], nfused=[2], replaced=[2, -1, -1], found=[3, 13, 103], visible=[4, 4, 4],
                        dirty=[0, 1, 1], obs=[[], [(0, 0), (1, 0)], [(2, 0)]])))
    # SIM3: spAlreadyFound is taken when the call starts: a point added by the call is not in it (AddObservation returns early), one that was there is
    c.append(_case("sim3_already_found", [K(-1, -1, 1), K(0)], [P((1, 0)), P((0, 2))], [(0, T.SIM3, [0, 0, 1], [0, 1, 0])],
                   dict(kp=[[0, 0, 1], [0]], bad=[0, 0], nobs=[2, 1], reason=[A, A, SI], nfused=[2], obs=[[(0, 0), (1, 0)], [(0, 2)]])))
    # the pointer order of the key frames is the order of a point's observations
    c.append(_case("permuted_keys", tie_kfs, tie_pts, [(0, T.POSE, [1], [0])], dict(kp=[[1], [1], [1], [1]], obs=[[], [(3, 0), (2, 0), (1, 0), (0, 0)]]), by_key=[3, 2, 1, 0]))
    # the second call reads the count the first one raised: without it the replace would go the other way
    c.append(_case("two_calls", [K(-1), K(0), K(1), K(1)], [P((1, 0)), P((2, 0), (3, 0))], [(0, T.POSE, [0], [0]), (2, T.POSE, [0], [0])],
                   dict(kp=[[0], [0], [0], [0]], bad=[0, 1], nobs=[4, 2], reason=[A, RK], other=[-1, 1], nfused=[1, 1], obs=[[(0, 0), (1, 0), (2, 0), (3, 0)], []])))
    return c


CASES = _cases()


def compare_want(e, want):
    """The keys of `want` that a result (the checker's or the library's) contradicts."""
    d = []
    row = lambda rows: [p for r in rows for p in r]
    for key, field in (("bad", "pt_bad_out"), ("nobs", "pt_nobs_out"), ("reason", "op_reason"), ("other", "op_other"), ("nfused", "call_nfused"), ("dirty", "pt_dirty"),
                       ("replaced", "pt_replaced_out"), ("found", "pt_found_out"), ("visible", "pt_visible_out"), ("touched", "obs_touched")):
        if key in want and list(np.asarray(e[field])) != list(want[key]):
            d.append(key)
    if "kp" in want and list(e["kp_point_out"]) != row(want["kp"]):
        d.append("kp")
    if "obs" in want and [[(k, f) for k, _, _, f in o] for o in e["obs"]] != want["obs"]:
        d.append("obs")
    if "dirty_lists" in want and e["dirty"] != want["dirty_lists"]:
        d.append("dirty_lists")
    for (p, i), word in want.get("words", {}).items():
        if e["obs"][p][i] != word:
            d.append("words")
    return d


def expected(name):
    return T.apply_fuse(next(c[1] for c in CASES if c[0] == name))


# ---- scenes sized around the kernels' strides -----------------------------------------------------------------------------------------------
def observers_scene(n):
    """Point 0 has n observers and is replaced by point 1 (whose nObs says more), which shares every third of them."""
    kfs = [K(0, 1 if k % 3 == 0 else -1, stereo=[k % 2, 0]) for k in range(n)] + [K(-1, 1)]
    pts = [P(*[(k, 0) for k in range(n)]), P(*([(k, 1) for k in range(0, n, 3)] + [(n, 1)]), nobs=100000)]
    return M.scene_from_lists(kfs, pts, [(1, T.POSE, [1], [0])], by_key=list(range(n, -1, -1)))


def entries_scene(n):
    """A call with n live entries: n points, each added to its own empty feature of key frame 0; then a second call that replaces them."""
    kfs = [K(*([-1] * n), stereo=[i % 2 for i in range(n)]), K(*range(n)), K(*range(n, 2 * n))]
    pts = [P((1, i)) for i in range(n)] + [P((2, i)) for i in range(n)]
    return M.scene_from_lists(kfs, pts, [(0, T.POSE, list(range(n)), list(range(n))), (0, T.SIM3, list(range(n, 2 * n)), list(range(n)))])


def sized_scenes():
    thr, wave, lds_kf, _ = M.shape()
    assert lds_kf == 0                                               # no state in LDS: no key-frame limit to probe
    out = []
    for stride in (wave, thr):
        for d in (-1, 0, 1):
            out.append(("observers_%d" % (stride + d), observers_scene(stride + d)))
            out.append(("entries_%d" % (stride + d), entries_scene(stride + d)))
    return out


# ---- broken snapshots ------------------------------------------------------------------------------------------------------------------------
def breakable_scene():
    """Four key frames, five points, two calls: every array has an entry to break."""
    kfs = [K(-1, 0, 3), K(0, 1, -1), K(1, 2), K(2, 4, -1)]
    pts = [P((0, 1), (1, 0)), P((1, 1), (2, 0)), P((2, 1), (3, 0)), P((0, 2)), P((3, 1))]
    return M.scene_from_lists(kfs, pts, [(0, T.POSE, [1, 2, -1], [0, 1, -1]), (1, T.SIM3, [3, 4], [2, 0])])


def broken(other, good):
    """(name, packed batch [other, a broken copy of good, good], the statuses expected): each kind breaks one entry of the middle stream."""
    base = M.pack([other, good, good])
    g = M._ranges(base, 1)
    nk, npt = g["k1"] - g["k0"], g["p1"] - g["p0"]
    nkp0 = int(base["kp_start"][g["k0"] + 1] - base["kp_start"][g["k0"]])
    kinds = [
        ("kp_start_descending", "kp_start", g["k0"] + 1, int(base["kp_start"][g["k0"] + 2]) + 1),
        ("kp_start_beyond", "kp_start", g["k0"] + 2, base["n_kp"] + 1),
        ("obs_start_descending", "obs_start", g["p0"] + 1, int(base["obs_start"][g["p0"] + 2]) + 1),
        ("obs_start_negative", "obs_start", g["p0"] + 1, -1),
        ("call_op_disagrees", "call_op", g["c0"] + 1, int(base["call_op"][g["c0"] + 1]) - 1),
        ("kf_by_key_twice", "kf_by_key", g["k0"], int(base["kf_by_key"][g["k0"] + 1])),
        ("kf_by_key_outside", "kf_by_key", g["k0"], nk),
        ("kp_point_beyond", "kp_point", g["i0"], npt),
        ("kp_point_below", "kp_point", g["i0"], -2),
        ("obs_slot_beyond", "obs", g["o0"], nk),
        ("obs_feat_beyond", "obs_feat", g["o0"], nkp0),
        ("obs_feat_negative", "obs_feat", g["o0"], -1),
        ("obs_names_kf_twice", "obs", g["o0"] + 1, int(base["obs"][g["o0"]])),
        ("op_feat_beyond", "op_feat", int(base["call_feat"][g["c0"]]), nkp0),
        ("op_feat_below", "op_feat", int(base["call_feat"][g["c0"]]), -2),
        ("list_point_beyond", "list_point", int(base["call_list"][g["c0"]]), npt),
        ("list_point_below", "list_point", int(base["call_list"][g["c0"]]), -2),
        ("call_kf_beyond", "call_kf", g["c0"], nk),
        ("call_kf_negative", "call_kf", g["c0"], -1),
        ("call_kind_unknown", "call_kind", g["c0"], 2),
        ("call_list_negative", "call_list", g["c0"], -1),
        ("call_list_beyond", "call_list", g["c0"] + 1, base["n_list"] - 1),
        ("call_n_negative", "call_n", g["c0"], -1),
        ("call_n_huge", "call_n", g["c0"], 2 ** 31 - 1),
        ("call_feat_negative", "call_feat", g["c0"], -3),
        ("call_feat_beyond", "call_feat", g["c0"] + 1, base["n_feat"] - 1),
    ]
    out = []
    for name, f, at, value in kinds:
        Pk = M.pack([other, good, good])
        Pk[f][at] = value
        out.append((name, Pk, [T.OK, T.INVALID, T.OK]))
    # a boundary of a batch-level array belongs to two streams: the stream behind the broken one checks it too
    Pk = M.pack([other, good, good])
    Pk["obs_out_start"][2] = int(Pk["obs_out_start"][1]) - 1
    out.append(("obs_out_start_descending", Pk, [T.OK, T.INVALID, T.INVALID]))
    return out


# ---- the seeded random set -------------------------------------------------------------------------------------------------------------------
SEEDS = tuple(range(200, 260))


def random_scene(seed):
    """6-10 key frames of 6-12 keypoints, 10-24 points, 2-4 calls of both kinds with duplicates, NULL entries, bad points, bad key frames,
    tables that disagree with the observations, shared lists and counters near the wrap."""
    r = np.random.RandomState(seed)
    nk, npt = int(r.randint(6, 11)), int(r.randint(10, 25))
    nkp = [int(r.randint(6, 13)) for _ in range(nk)]
    table = [[-1] * n for n in nkp]
    pts = []
    for p in range(npt):
        obs = []
        for k in r.permutation(nk)[:int(r.randint(0, 5))]:
            free = [i for i, q in enumerate(table[k]) if q < 0]
            if len(free) > 3:
                f = int(free[r.randint(len(free))])
                table[k][f] = p
                obs.append((int(k), f))
        big = r.rand() < 0.1
        pts.append(dict(obs=obs, bad=bool(r.rand() < 0.12), found=int(0xfffffff0 if big else r.randint(0, 50)), visible=int(0xfffffffa if big else r.randint(0, 90))))
    for k in range(nk):                                              # an inconsistent map: a table entry its point does not list, a listed entry the table lost
        if r.rand() < 0.3:
            table[k][int(r.randint(nkp[k]))] = int(r.randint(-1, npt))
    kfs = [dict(pts=table[k], stereo=[int(v) for v in r.randint(0, 2, nkp[k])], octave=[int(v) for v in r.randint(0, 8, nkp[k])], bad=bool(r.rand() < 0.15)) for k in range(nk)]
    shared = r.rand() < 0.4
    n_call = int(r.randint(2, 5))
    listed = lambda: [int(v) if r.rand() > 0.06 else -1 for v in r.randint(0, npt, int(r.randint(3, 12)))]
    shared_list = listed() if shared else None
    calls = []
    for c in range(n_call):
        k = int(r.randint(nk))
        points = shared_list if shared else listed()
        feats = [int(r.randint(nkp[k])) if r.rand() < 0.75 else -1 for _ in points]
        if len(points) > 3 and r.rand() < 0.6:                      # a duplicate of a listed point, often on the same feature
            i, j = int(r.randint(len(points))), int(r.randint(len(points)))
            if not shared:
                points[j] = points[i]
            if r.rand() < 0.5:
                feats[j] = feats[i]
        kind = T.SIM3 if (shared or r.rand() < 0.4) else T.POSE
        calls.append((k, kind, feats) if shared else (k, kind, points, feats))
    return M.scene_from_lists(kfs, pts, calls, by_key=[int(v) for v in r.permutation(nk)], shared_list=shared_list)


_RANDOM = None


def random_streams():
    """(scenes, the checker's results, the event counts over the set), computed once."""
    global _RANDOM
    if _RANDOM is None:
        scenes = [random_scene(s) for s in SEEDS]
        exp = [T.apply_fuse(s) for s in scenes]
        events = {}
        for e in exp:
            for k, v in e["events"].items():
                events[k] = events.get(k, 0) + v
        _RANDOM = (scenes, exp, events)
    return _RANDOM
