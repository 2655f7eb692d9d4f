"""Scenes for the map correction of loop closing (tests/test_map_correction_ref.py, tests/test_gpu_map_correction.py): hand-built ones, one
per rule of the reference that is easy to get wrong, each with the outputs it must give written out by hand (`want`, checked against the
checker tests/map_correction_ref.py before anything else is), sized scenes for the kernels' edges, broken snapshots and a random
generator.

The hand-built scenes use poses without rotation, or with half turns, and coordinates that are small integers, so that every expected
number is exact and can be written down: a key frame at centre C has the pose [I | -C]; mg2oScw = (identity, (1, 0, 0), 1) on a current
key frame at the origin moves the world by -1 in x (points and centres alike), and (identity, 0, 2) halves it.
CASES: (name, scene, want); `want` names whole output arrays."""
import numpy as np
from viorb_amd import map_correction as M
import map_correction_ref as T

f32 = np.float32
I9 = [1, 0, 0, 0, 1, 0, 0, 0, 1]
CUR_ID = 7
SHIFT = [0, 0, 0, 1, 1, 0, 0, 1]          # mg2oScw: r = identity, t = (1, 0, 0), s = 1
HALVE = [0, 0, 0, 1, 0, 0, 0, 2]          # r = identity, t = 0, s = 2
SF = [f32(1.0)]
for _ in range(15):
    SF.append(f32(SF[-1] * f32(1.2)))


def kf(C=(0, 0, 0), pts=(), R=I9):
    """A key frame with rotation R (row-major) whose translation is -C: for R = identity its centre is C."""
    return dict(pts=list(pts), pose=list(R) + [0.0 - C[0], 0.0 - C[1], 0.0 - C[2]])


def pt(P, *obs, ref=-1, bad=False, by=0, normal=(9, 9, 9), rng=(5, 50)):
    """A point at P with observations (slot, octave); its normal and range on entry are recognisable junk."""
    return dict(P=list(P) + list(normal) + list(rng), obs=list(obs), ref=ref, bad=bad, by=by)


def _cases():
    C = []
    add = lambda name, scene, **want: C.append((name, scene, want))
    third = f32(1.0 / 3.0)
    # 1. a point held by two members goes to the lower key, not to the lower slot or the earlier list entry: pointer order is 2, 0, 1; the list
    # is 1, 2; point 0 sits in slots 1 and 2. Slot 2 (key 0) corrects it. Its only observer, slot 1 (key 2, above), still has its input centre
    # (0, 3, 0): the point lands on (0, 0, 0), the normal is (0, -1, 0), the distance 3 at octave 1
    add("two_members_lower_key_wins",
        M.scene_from_lists([kf(), kf((0, 3, 0), [0]), kf((0, 0, 5), [0])], [pt((1, 0, 0), (1, 1), ref=1)], 0, [1, 2], SHIFT, CUR_ID, by_key=[2, 0, 1]),
        member_kf=[2, 0, 1], n_member=3, pt_corrected_ref_out=[2], pt_corrected_by_out=[CUR_ID], pt_touched=[1],
        pts_f_out=[[0, 0, 0, 0, -1, 0, f32(3) * SF[1] / SF[7], f32(3) * SF[1]]],
        Ow_out=[[-1, 0, 0], [-1, 3, 0], [-1, 0, 5]], pose12_out=[I9 + [1, 0, 0], I9 + [1, -3, 0], I9 + [1, 0, -5]])
    # 2. a point held twice in one member moves once
    add("twice_in_one_member", M.scene_from_lists([kf(pts=[0, 0, 0])], [pt((4, 0, 0), (0, 0), ref=0)], 0, [], SHIFT, CUR_ID),
        pt_touched=[1], pts_f_out=[[3, 0, 0, 1, 0, 0, f32(3) / SF[7], 3]], pt_corrected_ref_out=[0])
    # 3. a point that already carries this loop's mnCorrectedByKF is left alone; so are a bad point and a null keypoint
    add("already_corrected_bad_and_null",
        M.scene_from_lists([kf(pts=[0, -1, 1, 2])], [pt((4, 0, 0), (0, 0), ref=0, by=CUR_ID), pt((4, 0, 0), (0, 0), ref=0, bad=True), pt((1, 4, 0), (0, 0), ref=0, by=3)],
                           0, [], SHIFT, CUR_ID),
        pt_touched=[0, 0, 1], pt_corrected_by_out=[CUR_ID, 0, CUR_ID], pt_corrected_ref_out=[-1, -1, 0],
        pts_f_out=[[4, 0, 0, 9, 9, 9, 5, 50], [4, 0, 0, 9, 9, 9, 5, 50], [0, 4, 0, 0, 1, 0, f32(4) / SF[7], 4]])
    # 4. a point without observations is moved and keeps its normal and range (its reference key frame is not looked at)
    add("no_observations", M.scene_from_lists([kf(pts=[0])], [pt((4, 0, 0), ref=-1)], 0, [], SHIFT, CUR_ID),
        pt_touched=[1], pts_f_out=[[3, 0, 0, 9, 9, 9, 5, 50]])
    # 5. three centres in one normal. Pointer order = slot order; members 0 (below), 1 (the claimer), 2 (above); slot 3 is the current key
    # frame, at the origin and above. Point 0 = (1, 0, 4) sits in slots 1 and 2 and lands on (0, 0, 4). Slot 0 has been SetPose'd: its centre is
    # (1, 0, 0) - (1, 0, 0) = (0, 0, 0), the term (0, 0, 1); slot 1 is being walked: still (0, 3, 4), the term (0, -1, 0); slot 2 comes later:
    # (-4, 0, 4), the term (1, 0, 0). The reference key frame 1 is on the claimer's side: distance 3. Point 1 is the same with the reference
    # key frame 0, below: distance 4 from the corrected centre. The observations are listed out of key order
    three = [kf((1, 0, 0)), kf((0, 3, 4), [0, 1]), kf((-4, 0, 4), [0, 1]), kf()]
    add("three_centres_and_both_reference_sides",
        M.scene_from_lists(three, [pt((1, 0, 4), (2, 0), (0, 3), (1, 2), ref=1), pt((1, 0, 4), (1, 0), (2, 0), (0, 3), ref=0)], 3, [2, 1, 0], SHIFT, CUR_ID),
        member_kf=[0, 1, 2, 3], pt_corrected_ref_out=[1, 1],
        pts_f_out=[[0, 0, 4, third, -third, third, f32(3) * SF[2] / SF[7], f32(3) * SF[2]], [0, 0, 4, third, -third, third, f32(4) * SF[3] / SF[7], f32(4) * SF[3]]],
        Ow_out=[[0, 0, 0], [-1, 3, 4], [-5, 0, 4], [-1, 0, 0]])
    # 6. a scale of 2: points and centres are halved, the poses get t / s, the Sim3 rows keep t and s, Scw_f12 is the three rows of [s R | t]
    add("scale_2", M.scene_from_lists([kf(pts=[0]), kf((0, 8, 0))], [pt((0, 0, 6), (0, 0), ref=0)], 0, [1], HALVE, CUR_ID),
        member_kf=[0, 1], pts_f_out=[[0, 0, 3, 0, 0, 1, f32(3) / SF[7], 3]],                                   # the observer is the claimer: its input centre, the origin
        pose12_out=[I9 + [0, 0, 0], I9 + [0, -4, 0]], Ow_out=[[0, 0, 0], [0, 4, 0]],
        Scw_out=[[0, 0, 0, 1, 0, 0, 0, 2], [0, 0, 0, 1, 0, -8, 0, 2]], Smeas_out=[[0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0, 1, 0, -8, 0, 1]],
        Scw_f12=[[2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0], [2, 0, 0, 0, 0, 2, 0, -8, 0, 0, 2, 0]])
    # 7. the four branches of Quaterniond(Matrix3d): the identity (trace), and the half turns about x, y and z
    turns = [kf(), kf(R=[1, 0, 0, 0, -1, 0, 0, 0, -1]), kf(R=[-1, 0, 0, 0, 1, 0, 0, 0, -1]), kf(R=[-1, 0, 0, 0, -1, 0, 0, 0, 1])]
    add("mat2q_branches", M.scene_from_lists(turns, [], 0, [1, 2, 3], SHIFT, CUR_ID),
        Smeas_out=[[0, 0, 0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 0, 1], [0, 0, 1, 0, 0, 0, 0, 1]],
        Scw_out=[[0, 0, 0, 1, 1, 0, 0, 1], [1, 0, 0, 0, 1, 0, 0, 1], [0, 1, 0, 0, -1, 0, 0, 1], [0, 0, 1, 0, -1, 0, 0, 1]])
    # 8. an empty covisible list: the current key frame alone; a key frame that is not a member passes through
    add("empty_list", M.scene_from_lists([kf((2, 0, 0)), kf(pts=[0])], [pt((0, 0, 1), (1, 0), ref=1)], 1, [], SHIFT, CUR_ID),
        n_member=1, member_kf=[1], pt_touched=[1], Ow_out=[[2, 0, 0], [-1, 0, 0]], pose12_out=[I9 + [-2, 0, 0], I9 + [1, 0, 0]],
        Scw_out=[[0, 0, 0, 1, -2, 0, 0, 1], [0, 0, 0, 1, 1, 0, 0, 1]], Smeas_out=[[0, 0, 0, 1, -2, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0, 1]])
    # 9. a stream without points
    add("no_points", M.scene_from_lists([kf(pts=[-1]), kf()], [], 0, [1], SHIFT, CUR_ID), member_kf=[0, 1], pts_f_out=np.zeros((0, 8)), pt_touched=[])
    return C


def compare_want(r, want):
    """The entries of `want` that result r does not meet: the values written by hand are exact, the sign of a zero is not written."""
    bad = []
    for f, v in want.items():
        got = np.asarray(r[f])
        w = np.asarray(v, got.dtype).reshape(got.shape) if np.size(v) == got.size else np.asarray(v)
        if got.shape != w.shape or not np.array_equal(got, w):
            bad.append((f, got.tolist()))
    return bad


CASES = _cases()
_expected = {}


def expected(name):
    """The checker's result for a hand-built scene, computed once."""
    if name not in _expected:
        _expected[name] = T.correct_loop(next(c for c in CASES if c[0] == name)[1])
    return _expected[name]


# ---- random scenes ---------------------------------------------------------------------------------------------------------------------------
def random_rotation(rng, kind):
    """A rotation matrix as float32 [9]: kind 0 a small rotation (trace branch), 1-3 close to a half turn about x, y, z."""
    w = rng.normal(size=3) * 0.2
    if kind:
        w[kind - 1] += np.pi
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K).astype(np.float32).ravel()


def random_scene(seed, nk=None, n_pt=None, n_kp=None, max_obs=6, n_members=None, exact_obs=()):
    """A random stream: nk key frames in a random pointer order, a current key frame with a random list of covisibles, points with up to
    max_obs observers in a random order (the reference key frame among them; the first points have exactly exact_obs observers and are
    good), keypoints with null, bad, repeated and already corrected points."""
    rng = np.random.default_rng(seed)
    nk = nk or int(rng.integers(1, 13))
    n_pt = int(rng.integers(0, 30)) if n_pt is None else n_pt
    cur = int(rng.integers(0, nk))
    others = [k for k in rng.permutation(nk).tolist() if k != cur]
    conn = others[:int(rng.integers(0, len(others) + 1)) if n_members is None else min(n_members, len(others))]
    pts = []
    for j in range(n_pt):
        n = int(rng.integers(0, min(nk, max_obs) + 1)) if rng.random() < 0.92 else 0
        n = exact_obs[j] if j < len(exact_obs) else n
        obs = [(int(k), int(rng.integers(0, 8))) for k in rng.choice(nk, size=n, replace=False)]
        pts.append(dict(P=rng.normal(size=8).astype(np.float32) * 4, obs=obs, ref=obs[int(rng.integers(0, n))][0] if n else -1, bad=bool(rng.random() < 0.1) and j >= len(exact_obs),
                        by=CUR_ID if rng.random() < 0.1 and j >= len(exact_obs) else int(rng.integers(0, 5))))
    kfs = []
    for k in range(nk):
        m = (int(rng.integers(0, 12)) if n_kp is None else n_kp) if n_pt else int(rng.integers(0, 3))
        kp = [int(rng.integers(0, n_pt)) if n_pt and rng.random() < 0.85 else -1 for _ in range(m)]
        kp[:len(exact_obs)] = range(min(len(exact_obs), len(kp)))
        if len(kp) > 1 and kp[0] >= 0 and rng.random() < 0.3:
            kp[-1] = kp[0]
        R = random_rotation(rng, int(rng.integers(0, 4)) if rng.random() < 0.5 else 0)
        kfs.append(dict(pts=kp, pose=list(R) + list((rng.normal(size=3) * 3).astype(np.float32))))
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    Scw = list(q) + list(rng.normal(size=3) * 2) + [1.0 if rng.random() < 0.3 else float(rng.uniform(0.5, 2.0))]
    return M.scene_from_lists(kfs, pts, cur, conn, Scw, CUR_ID, by_key=rng.permutation(nk).tolist())


_random = {}


def random_streams(n=300):
    """(scenes, the checker's results, how often each situation of T.EVENTS occurred), computed once."""
    if n not in _random:
        events = {}
        scenes = [random_scene(1000 + i) for i in range(n)]
        _random[n] = (scenes, [T.correct_loop(s, events=events) for s in scenes], events)
    return _random[n]


def sized_scenes():
    """(name, scene) around the strides the kernels report: keypoints of a member and key frames around the threads of the key-frame
    phase, points around a wavefront's pass and around the point phase's threads, observers of a point around the wavefront."""
    thr_kf, thr_pt, wave, lds_kf = M.shape()
    out = []
    for d in (-1, 0, 1):
        out.append(("kp_%d" % (thr_kf + d), random_scene(50 + d, nk=4, n_pt=40, n_kp=thr_kf + d, n_members=3)))
        out.append(("kf_%d" % (thr_kf + d), random_scene(60 + d, nk=thr_kf + d, n_pt=30, n_kp=2, n_members=thr_kf + d)))
        out.append(("pt_%d" % (wave + d), random_scene(70 + d, nk=5, n_pt=wave + d, n_kp=40, n_members=4)))
        out.append(("pt_%d" % (thr_pt + d), random_scene(80 + d, nk=5, n_pt=thr_pt + d, n_kp=150, n_members=4)))
        out.append(("obs_%d" % (wave + d), random_scene(90 + d, nk=wave + 6, n_pt=12, n_kp=3, max_obs=wave + d, n_members=wave + 5, exact_obs=(wave + d, wave + d))))
    return out


def full_observers(scene):
    """The most observers a point of the scene has."""
    return int(np.diff(scene["obs_start"]).max()) if len(scene["pt_bad"]) else 0


# ---- broken snapshots ----------------------------------------------------------------------------------------------------------------------
def breakable_scene():
    """Three members, a key frame outside, four points: every array has entries to break."""
    kfs = [kf((0, 0, 0), [0, 1, -1]), kf((0, 3, 0), [1, 2]), kf((2, 0, 0), [2, 0]), kf((9, 9, 9), [3])]
    pts = [pt((1, 0, 4), (0, 0), (1, 1), ref=0), pt((1, 2, 4), (1, 0), (2, 2), (0, 1), ref=2), pt((0, 2, 1), (2, 3), ref=2), pt((5, 5, 5), (3, 0), ref=3)]
    return M.scene_from_lists(kfs, pts, 0, [2, 1], SHIFT, CUR_ID, by_key=[1, 3, 0, 2])


def broken(s):
    """[(what, scene)]: every kind of broken snapshot of one stream."""
    def put(f, i, v):
        a = s[f].copy()
        a.reshape(-1)[i] = v
        return dict(s, **{f: a})
    out = [("kp_start descends", put("kp_start", 1, 7)), ("kp_start negative", put("kp_start", 2, -1)), ("kp_start beyond", put("kp_start", 2, 1 << 20)),
           ("obs_start descends", put("obs_start", 2, 0)), ("obs_start beyond", put("obs_start", 2, 1 << 20)),
           ("kf_by_key out of range", put("kf_by_key", 1, 4)), ("kf_by_key negative", put("kf_by_key", 1, -1)), ("kf_by_key not a permutation", put("kf_by_key", 1, 0)),
           ("member keypoint beyond the points", put("kp_point", 0, 4)), ("member keypoint below -1", put("kp_point", 3, -2)),
           ("observer slot beyond the key frames", put("obs", 0, 4)),
           ("cur_kf out of range", dict(s, cur_kf=4)), ("cur_kf negative", dict(s, cur_kf=-1)),
           ("conn_kf out of range", put("conn", 0, 4)), ("conn_kf negative", put("conn", 1, -1)), ("conn_kf twice", put("conn", 1, 2)), ("conn_kf names the current key frame", put("conn", 0, 0)),
           ("pose not finite", put("pose12", 12 * 3 + 5, np.inf)), ("pose NaN", put("pose12", 9, np.nan)),
           ("Scw8 not finite", put("Scw8", 4, np.nan)), ("scale 0", put("Scw8", 7, 0.0)), ("scale negative", put("Scw8", 7, -1.0)),
           ("pt_ref out of range", put("pt_ref", 1, 4)), ("pt_ref negative on an observed point", put("pt_ref", 0, -1)), ("pt_ref not an observer", put("pt_ref", 2, 1))]
    return out


def large_scene():
    """The largest scene of the GPU tests: 80 key frames, 3000 points, up to 70 observers, points with exactly 63, 64, 65 and 70."""
    return random_scene(7, nk=80, n_pt=3000, n_kp=110, max_obs=70, n_members=45, exact_obs=(63, 64, 65, 70))


# ==== the map update after a global bundle adjustment ===========================================================================================
TBC_I = I9 + [0, 0, 0]                    # body = camera: the hand-built scenes
TBC = [0.0148655429818, -0.999880929698, 0.00414029679422, 0.999557249008, 0.0149672133247, 0.025715529948, -0.0257744366974, 0.00375618835797, 0.999660727178,
       -0.0216401454975, -0.064676986768, 0.00981073058949]          # a camera-to-body transform with a real rotation: the random scenes


def _ns(C, V=(0, 0, 0), q=(0, 0, 0, 1)):
    return [C[0], C[1], C[2], V[0], V[1], V[2]] + list(q) + [0.0] * 12


def _pose(C):
    return I9 + [0.0 - C[0], 0.0 - C[1], 0.0 - C[2]]


def gba_all_rules():
    """One hand-built map that holds every rule, with identity rotations, so that the adjustment is a shift of every centre:
    key frame 0 (in the adjustment, an origin, shifted by (1, 0, 0)) has the siblings 1 and 8 outside it; 1 -> 2 -> 3 is a chain of three
    outside; key frame 6 is a second origin and a root OUTSIDE the adjustment, whose given GBA pose (a shift by (0, 2, 0)) is used as it
    is and passed to its child 7; key frame 4 carries the flag but hangs under no origin (unreached); key frame 5 is outside and unreached.
    Points: 0 bad, 1 in the adjustment, 2 through key frame 2, 3 with the unflagged reference 5, 4 with the flagged, unreached reference 4,
    5 through the root 6, which the walk reaches but never flags: untouched."""
    C = [(0, 0, 0), (2, 0, 0), (4, 0, 0), (6, 0, 0), (0, 9, 0), (0, 0, 9), (0, 0, 20), (0, 1, 20), (0, 3, 0)]
    D = {0: (1, 0, 0), 4: (5, 5, 5), 6: (0, 2, 0)}
    gC = [tuple(c[i] + D.get(k, (0, 0, 0))[i] for i in range(3)) for k, c in enumerate(C)]
    V = [(0, 0, 0), (1, 2, 3), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (4, 5, 6), (0, 0, 0)]
    children = [[1, 8], [2], [3], [], [], [], [7], [], []]
    s = M.gba_scene(children, [0, 6], [1, 0, 0, 0, 1, 0, 0, 0, 0], [_pose(c) for c in C], [_pose(c) for c in gC], [_ns(c, v) for c, v in zip(C, V)],
                    [_ns(c, v) for c, v in zip(gC, V)], pt_bad=[1, 0, 0, 0, 0, 0], pt_in_gba=[0, 1, 0, 0, 0, 0],
                    Pw=[(1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4), (5, 5, 5), (6, 6, 6)], PosGBA=[(9, 9, 9), (7, 7, 7), (9, 9, 9), (9, 9, 9), (9, 9, 9), (9, 9, 9)],
                    pt_ref=[0, 0, 2, 5, 4, 6])
    new = [(1, 0, 0), (3, 0, 0), (5, 0, 0), (7, 0, 0), (0, 9, 0), (0, 0, 9), (0, 2, 20), (0, 3, 20), (1, 3, 0)]       # the centres afterwards
    want = dict(kf_reached=[1, 1, 1, 1, 0, 0, 1, 1, 1], kf_in_gba_out=[1, 1, 1, 1, 1, 0, 0, 1, 1], pose12_out=[_pose(c) for c in new],
                TcwBef_out=[_pose(c) for c in C], ns22_out=[_ns(c, v) for c, v in zip(new, V)], nsBef_out=[_ns(c, v) for c, v in zip(C, V)],
                pt_code=[0, 1, 2, 3, 4, 3], Pw_out=[(1, 1, 1), (7, 7, 7), (4, 3, 3), (4, 4, 4), (5, 5, 5), (6, 6, 6)])
    return s, want


def gba_random_scene(seed, nk=None, n_pt=None):
    """A random forest: every key frame but the roots hangs under an earlier one; a few roots are origins; key frames are in the adjustment
    with probability 0.6; general rotations, so that Set_Rot has something to normalise."""
    rng = np.random.default_rng(seed)
    nk = nk or int(rng.integers(1, 14))
    n_pt = int(rng.integers(0, 20)) if n_pt is None else n_pt
    order = rng.permutation(nk).tolist()
    children, roots = [[] for _ in range(nk)], []
    for j, k in enumerate(order):
        if j == 0 or rng.random() < 0.15:
            roots.append(k)
        else:
            children[order[int(rng.integers(max(0, j - 3), j))]].append(k)
    origins = [r for r in roots if rng.random() < 0.7] or roots[:1]
    in_gba = (rng.random(nk) < 0.6).astype(np.uint8)

    def pose():
        return list(random_rotation(rng, int(rng.integers(0, 4)) if rng.random() < 0.3 else 0)) + list((rng.normal(size=3) * 3).astype(np.float32))

    def ns():
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        return list(rng.normal(size=6)) + list(q) + list(rng.normal(size=12) * 0.01)
    return M.gba_scene(children, origins, in_gba, [pose() for _ in range(nk)], [pose() for _ in range(nk)], [ns() for _ in range(nk)], [ns() for _ in range(nk)],
                       pt_bad=rng.random(n_pt) < 0.15, pt_in_gba=rng.random(n_pt) < 0.4, Pw=rng.normal(size=(n_pt, 3)) * 4, PosGBA=rng.normal(size=(n_pt, 3)) * 4,
                       pt_ref=rng.integers(0, nk, n_pt))


_gba_random = {}


def gba_random_streams(n=300):
    if n not in _gba_random:
        events = {}
        scenes = [gba_random_scene(5000 + i) for i in range(n)]
        _gba_random[n] = (scenes, [T.apply_global_ba(s, TBC, events=events) for s in scenes], events)
    return _gba_random[n]


def gba_sized_scenes():
    """(name, scene) one below, at and one above the strides viorb_apply_global_ba_shape reports: key frames around the threads of the
    key-frame phase, points around the threads of the point phase and around what all of a stream's workgroups take in one pass."""
    thr_kf, thr_pt, wave, groups = M.gba_shape()
    out = []
    for d in (-1, 0, 1):
        out.append(("kf_%d" % (thr_kf + d), gba_random_scene(300 + d, nk=thr_kf + d, n_pt=40)))
        out.append(("pt_%d" % (thr_pt + d), gba_random_scene(310 + d, nk=9, n_pt=thr_pt + d)))
        out.append(("pt_%d" % (2 * thr_pt + d), gba_random_scene(320 + d, nk=9, n_pt=2 * thr_pt + d)))
    return out


def gba_broken(s):
    """[(what, scene)]: every kind of broken map of one stream (s = gba_all_rules()[0])."""
    def put(f, i, v):
        a = s[f].copy()
        a.reshape(-1)[i] = v
        return dict(s, **{f: a})
    return [("child_start descends", put("child_start", 2, 0)), ("child_start beyond", put("child_start", 3, 1 << 20)), ("child_kf out of range", put("child_kf", 0, 9)),
            ("child_kf negative", put("child_kf", 1, -1)), ("a child twice", put("child_kf", 3, 1)), ("a key frame its own child", put("child_kf", 2, 1)),
            ("a cycle", put("child_kf", 4, 6)), ("an origin that is a child", put("origins", 1, 2)), ("an origin twice", put("origins", 1, 0)),
            ("origin out of range", put("origins", 0, 9)), ("origin negative", put("origins", 0, -3)),
            ("pose not finite", put("pose12", 12 * 5 + 3, np.nan)), ("NavState not finite", put("ns22", 22 * 2 + 7, np.inf)),
            ("GBA pose of a key frame in the adjustment not finite", put("TcwGBA12", 9, np.nan)), ("GBA NavState of a key frame in the adjustment not finite", put("nsGBA22", 22 * 4, np.nan)),
            ("point not finite", put("Pw", 3 * 2, np.nan)), ("PosGBA of a point in the adjustment not finite", put("PosGBA", 3, np.inf)),
            ("pt_ref out of range", put("pt_ref", 2, 9)), ("pt_ref negative", put("pt_ref", 3, -1))]
