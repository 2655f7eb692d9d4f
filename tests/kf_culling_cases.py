"""Hand-built scenes for key-frame culling, shared by tests/test_kf_culling_ref.py (CPU) and tests/test_gpu_culling.py, and the random
batches of the GPU tests with the checker's (tests/kf_culling_ref.py) results on them, computed once. A case is (name, scene, monocular,
want) where `want` holds what the case is about, written out by hand: cand_reason, and where it matters cand_redundant, cand_mps and
parts of the final state."""
import functools
import numpy as np
from viorb_amd import culling as M
from viorb_amd.synth import make_culling_problem
import kf_culling_ref as T

F, G, BC, RC, KEPT, CULLED, DEF = range(7)


def chain(times, first=(), not_erase=()):
    """Key frames in a prev / next chain in list order."""
    n = len(times)
    return [dict(t=times[k], prev=k - 1, next=k + 1 if k + 1 < n else -1, first=k in first, not_erase=k in not_erase) for k in range(n)]


def pts_seen_by(n, slots, octave=0, stereo=(), nobs=None):
    """n points, each observed by every slot of `slots` (octave: one value or one per slot; stereo: the slots with mvuRight >= 0)."""
    oc = octave if isinstance(octave, (list, tuple)) else [octave] * len(slots)
    return [dict(obs=[(s, oc[i], s in stereo) for i, s in enumerate(slots)], nobs=nobs) for _ in range(n)]


def table(first, n, octave=0, depth=1.0):
    """Keypoints for the points first .. first + n - 1."""
    return [(first + i, octave, depth) for i in range(n)]


# key frames 0..5 at 0.1 s, the current one (6) two seconds later; GetVINSInited() so that no time gap matters
def _base(**kw):
    return chain([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 2.5], **kw)


def fewer_observers(order, not_erase=()):
    # A = 0, B = 1 share ten points that 2 and 3 also observe: the first of A and B is culled, the other is left with two observers
    pts = pts_seen_by(10, [0, 1, 2, 3])
    cands = [(k, table(0, 10)) for k in order]
    return M.scene_from_lists(_base(not_erase=not_erase), 6, cands, pts, vins_inited=True)


def bad_points_shrink_mps(order, b_observes=True):
    # B = 1: ten redundant points (10..19) and two points (0, 1) with nObs == 3 that A = 0 also observes: 10 > 10.8 fails until A is culled
    # and the two go bad. A: twenty redundant points of its own (20..39) and the two. b_observes=False: B holds 0 and 1 in its table only.
    pts = pts_seen_by(2, [0, 1, 2] if b_observes else [0, 2, 3]) + [dict(obs=[], nobs=0)] * 8 + pts_seen_by(10, [1, 2, 3, 4]) + pts_seen_by(20, [0, 2, 3, 4])
    tabs = {0: table(20, 20) + table(0, 2), 1: table(10, 10) + table(0, 2)}
    return M.scene_from_lists(_base(), 6, [(k, tabs[k]) for k in order], pts, vins_inited=True)


def link_changes(order):
    # times 0, 0.3, 0.45, 0.7: culling either of 1 and 2 stretches the other's prev-next span to 0.7 > 0.5
    kfs = chain([0.0, 0.3, 0.45, 0.7, 3.0, 3.1])
    pts = pts_seen_by(5, [1, 0, 3, 4]) + pts_seen_by(5, [2, 0, 3, 4])
    tabs = {1: table(0, 5), 2: table(5, 5)}
    return M.scene_from_lists(kfs, 5, [(k, tabs[k]) for k in order], pts, vins_inited=False)


def threshold(n_mps, n_red):
    # candidate 0 with n_red redundant points and n_mps - n_red points of nObs == 3
    pts = pts_seen_by(n_red, [0, 1, 2, 3]) + pts_seen_by(n_mps - n_red, [0, 1, 2])
    return M.scene_from_lists(_base(), 6, [(0, table(0, n_mps))], pts, vins_inited=True)


def one_point(slots, octaves, stereo=(), nobs=None, cand_octave=2, depth=1.0, th_depth=40.0, n=1):
    # candidate 0 holds n copies of one kind of point
    pts = pts_seen_by(n, slots, octaves, stereo, nobs)
    return M.scene_from_lists(_base(), 6, [(0, table(0, n, cand_octave, depth))], pts, vins_inited=True, th_depth=th_depth)


def recent(t_c):
    kfs = chain([0.0, t_c, 0.9, 1.0])
    return M.scene_from_lists(kfs, 3, [(1, table(0, 3))], pts_seen_by(3, [1, 0, 2, 3]), vins_inited=True)


def depths():
    # four redundant points at depths th, above, below, negative (not monocular): two are counted
    pts = pts_seen_by(4, [0, 1, 2, 3])
    tab = [(0, 0, 40.0), (1, 0, np.nextafter(np.float32(40), np.float32(50))), (2, 0, np.nextafter(np.float32(40), np.float32(0))), (3, 0, -0.5)]
    return M.scene_from_lists(_base(), 6, [(0, tab)], pts, vins_inited=True, th_depth=40.0)


def point_twice():
    # point 0 (stereo at the candidate, the others at octave 3) at two keypoints of candidate 0, octaves 0 and 5: counted twice, redundant
    # once, erased once (nObs 5 -> 3; a second erase would leave 1 and a bad point)
    pts = [dict(obs=[(0, 0, True), (1, 3, False), (2, 3, False), (3, 3, False)])] + pts_seen_by(18, [0, 1, 2, 3])
    tab = [(0, 0, 1.0), (0, 5, 1.0)] + table(1, 18)
    return M.scene_from_lists(_base(), 6, [(0, tab)], pts, vins_inited=True)


CASES = []


def case(name, scene, mono, **want):
    CASES.append((name, scene, mono, want))


case("fewer_observers_ab", fewer_observers([0, 1]), True, cand_reason=[CULLED, KEPT], cand_redundant=[10, 0], cand_mps=[10, 10], culled_order=[0],
     pt_nobs_out=[3] * 10, kf_prev_out=[-1, -1, 1, 2, 3, 4, 5], kf_next_out=[-1, 2, 3, 4, 5, 6, -1], kf_repreint=[0] * 7)
case("fewer_observers_ba", fewer_observers([1, 0]), True, cand_reason=[CULLED, KEPT], cand_redundant=[10, 0], cand_mps=[10, 10], culled_order=[0],
     kf_prev_out=[-1, -1, 0, 2, 3, 4, 5], kf_next_out=[2, -1, 3, 4, 5, 6, -1], kf_repreint=[0, 0, 1, 0, 0, 0, 0], kf_bad=[0, 1, 0, 0, 0, 0, 0])
case("shrinking_mps_ab", bad_points_shrink_mps([0, 1]), True, cand_reason=[CULLED, CULLED], cand_redundant=[20, 10], cand_mps=[22, 10], culled_order=[0, 1],
     pt_bad_out=[1, 1] + [0] * 38, pt_nobs_out=[2, 2] + [0] * 8 + [3] * 10 + [3] * 20)
case("shrinking_mps_ba", bad_points_shrink_mps([1, 0]), True, cand_reason=[KEPT, CULLED], cand_redundant=[10, 20], cand_mps=[12, 22], culled_order=[1],
     pt_bad_out=[1, 1] + [0] * 38)
case("link_changes_12", link_changes([1, 2]), True, cand_reason=[CULLED, G], cand_redundant=[5, 0], cand_mps=[5, 0], kf_prev_out=[-1, -1, 0, 2, 3, 4],
     kf_next_out=[2, -1, 3, 4, 5, -1], kf_repreint=[0, 0, 1, 0, 0, 0])
case("link_changes_21", link_changes([2, 1]), True, cand_reason=[CULLED, G], cand_redundant=[5, 0], cand_mps=[5, 0], kf_prev_out=[-1, 0, -1, 1, 3, 4],
     kf_next_out=[1, 3, -1, 4, 5, -1], kf_repreint=[0, 0, 0, 1, 0, 0])
case("threshold_10_9", threshold(10, 9), True, cand_reason=[KEPT], cand_redundant=[9], cand_mps=[10])
case("threshold_10_10", threshold(10, 10), True, cand_reason=[CULLED], cand_redundant=[10], cand_mps=[10])
case("threshold_11_10", threshold(11, 10), True, cand_reason=[CULLED], cand_redundant=[10], cand_mps=[11])
case("threshold_20_18", threshold(20, 18), True, cand_reason=[KEPT], cand_redundant=[18], cand_mps=[20])
case("octave_plus_1_counts", one_point([0, 1, 2, 3], [2, 3, 3, 3]), True, cand_reason=[CULLED], cand_redundant=[1], cand_mps=[1])
case("octave_plus_2_does_not", one_point([0, 1, 2, 3], [2, 3, 3, 4]), True, cand_reason=[KEPT], cand_redundant=[0], cand_mps=[1])
case("two_stereo_observers", one_point([0, 1, 2], [2, 2, 2], stereo=(1, 2)), True, cand_reason=[KEPT], cand_redundant=[0], cand_mps=[1], pt_nobs_out=[5])
case("nobs_exactly_3", one_point([0, 1, 2, 3], [2, 2, 2, 2], nobs=3), True, cand_reason=[KEPT], cand_redundant=[0], cand_mps=[1])
case("nobs_4_three_observers", one_point([0, 1, 2, 3], [2, 2, 2, 2], nobs=4), True, cand_reason=[CULLED], cand_redundant=[1], cand_mps=[1], pt_nobs_out=[3],
     obs_alive=[0, 1, 1, 1])
case("own_observation_excluded", one_point([0, 1, 2], [2, 2, 2], nobs=4), True, cand_reason=[KEPT], cand_redundant=[0], cand_mps=[1])
case("recent_exactly", recent(0.8), True, cand_reason=[RC], cand_mps=[0])
case("recent_just_before", recent(float(np.nextafter(0.8, 0.0))), True, cand_reason=[CULLED], cand_mps=[3])
case("first_key_frame", M.scene_from_lists(_base(first=(0,)), 6, [(0, table(0, 4))], pts_seen_by(4, [0, 1, 2, 3]), vins_inited=True), True,
     cand_reason=[F], cand_mps=[0], kf_bad=[0] * 7)
case("before_current", M.scene_from_lists(_base(), 6, [(5, table(0, 4))], pts_seen_by(4, [5, 1, 2, 3]), vins_inited=True), True, cand_reason=[BC])
case("not_erase_defers", fewer_observers([0, 1], not_erase=(0,)), True, cand_reason=[DEF, CULLED], cand_redundant=[10, 10], cand_mps=[10, 10],
     kf_to_be_erased=[1, 0, 0, 0, 0, 0, 0], kf_bad=[0, 1, 0, 0, 0, 0, 0], culled_order=[1])
case("depths", depths(), False, cand_reason=[CULLED], cand_redundant=[2], cand_mps=[2], pt_nobs_out=[3, 3, 3, 3])
case("depths_monocular", depths(), True, cand_reason=[CULLED], cand_redundant=[4], cand_mps=[4])
case("point_twice", point_twice(), True, cand_reason=[CULLED], cand_redundant=[19], cand_mps=[20], pt_nobs_out=[3] * 19, pt_bad_out=[0] * 19)
case("table_entry_without_observation", bad_points_shrink_mps([0, 1], b_observes=False), True, cand_reason=[CULLED, CULLED], cand_redundant=[20, 10],
     cand_mps=[22, 10], pt_bad_out=[1, 1] + [0] * 38)
case("table_entry_without_observation_ba", bad_points_shrink_mps([1, 0], b_observes=False), True, cand_reason=[KEPT, CULLED], cand_mps=[12, 22])


@functools.lru_cache(maxsize=None)
def expected(name):
    _, scene, mono, _ = next(c for c in CASES if c[0] == name)
    return T.key_frame_culling(scene, mono)


# ---- broken snapshots ---------------------------------------------------------------------------------------------------------------------
def breakable_scene():
    """4 key frames, 2 candidates of 2 keypoints each, 3 points of which point 1 is seen by both candidates."""
    pts = pts_seen_by(1, [0, 2, 3]) + pts_seen_by(1, [0, 1, 2, 3]) + pts_seen_by(1, [1, 2, 3])
    return M.scene_from_lists(chain([0.0, 0.1, 0.2, 2.5]), 3, [(0, table(0, 2)), (1, table(1, 2))], pts, vins_inited=True)


def broken(scene):
    """(what, scene) for every kind of broken snapshot the validator refuses (the list of tests/cpp/culling_core_host_test.cpp), made from
    a scene with at least 2 candidates, 2 points, a keypoint and an observation."""
    nk, n_pt, big = len(scene["kf_flags"]), len(scene["pt_nobs"]), 1 << 28
    c = int(scene["cand_kf"][0])
    out = []

    def brk(what, field, index, value):
        s = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
        if index is None:
            s[field] = value
        else:
            s[field][index] = value
        out.append((what, s))
    brk("a point index at the end of the stream", "kp_point", 0, n_pt)
    brk("a point index far past the end", "kp_point", 0, big)
    brk("a point index below -1", "kp_point", 0, -2)
    brk("an observation slot at the end", "obs", 0, (int(scene["obs"][0]) & ~0xffff) | nk)
    brk("an observation slot past the end", "obs", 0, int(scene["obs"][0]) | 0xffff)
    brk("descending keypoint offsets", "kp_start", 1, int(scene["kp_start"][2]) + 1)
    brk("a keypoint offset past the total", "kp_start", 1, big)
    brk("descending observation offsets", "obs_start", 1, int(scene["obs_start"][2]) + 1)
    brk("a negative observation offset", "obs_start", 1, -big)
    brk("a candidate whose prev lies outside the snapshot", "kf_prev", c, nk)
    brk("a candidate whose next is below -1", "kf_next", c, -2)
    brk("cur_kf out of range", "cur", None, nk)
    brk("a negative cur_kf", "cur", None, -1)
    brk("a candidate slot past the end", "cand_kf", 0, big)
    brk("an observation count of 2^30", "pt_nobs", 0, 1 << 30)
    brk("a candidate listed twice", "cand_kf", 1, c)
    return out


def untouched(scenes, b, o, fill=77):
    """Whether stream b's ranges of the flat result arrays o (every field but status and n_culled, which a refused stream gets) still
    hold the fill value. The ranges are cut by the sizes of the scenes, not through the offsets of the snapshot."""
    size = dict(n_kf="kf_flags", n_cand="cand_kf", n_pt="pt_nobs", n_obs="obs")
    ok = True
    for f, total in M._OUT_LEN.items():
        if total == "batch":
            continue
        lo = sum(len(s[size[total]]) for s in scenes[:b])
        ok = ok and bool((np.asarray(o[f])[lo:lo + len(scenes[b][size[total]])] == fill).all())
    return ok


# ---- random batches -----------------------------------------------------------------------------------------------------------------------
CHECKED = ("cand_reason", "cand_redundant", "cand_mps", "n_culled", "culled_order", "kf_bad", "kf_to_be_erased", "kf_prev_out", "kf_next_out",
           "kf_repreint", "pt_nobs_out", "pt_bad_out", "obs_alive")


def differences(got, want):
    """The fields of one stream's result that differ from the checker's."""
    if got.get("status", 0) != 0:
        return ["status"]
    bad = [f for f in CHECKED if not np.array_equal(np.asarray(got[f]), np.asarray(want[f]))]
    if "culled_tail" in got and not (np.asarray(got["culled_tail"]) == -1).all():
        bad.append("culled_tail")
    return bad


@functools.lru_cache(maxsize=None)
def random_batch(seed, n, monocular):
    """(scenes, the checker's results)."""
    scenes = [make_culling_problem(seed * 1000 + b) for b in range(n)]
    return scenes, [T.key_frame_culling(s, monocular) for s in scenes]


def shape_scene(n_kps, obs_len, seed=0):
    """Three candidates of n_kps keypoints whose points have obs_len observations (slots 3.. besides the candidates'), so that culls
    happen and change the later candidates."""
    rng = np.random.default_rng(seed)
    nk = max(obs_len + 4, 8)
    kfs = chain([0.05 * k for k in range(nk)] + [10.0])
    npts = max(n_kps, 1)
    pts = []
    for p in range(npts):
        others = list(rng.permutation(np.arange(3, nk))[:max(obs_len - 2, 0)])
        own = [0, 1, 2][:min(obs_len, 2)] if p % 3 else [1, 2, 0][:min(obs_len, 2)]
        pts.append(dict(obs=[(int(s), int(rng.integers(0, 2)), bool(rng.random() < 0.3)) for s in own + others]))
    cands = [(c, [(int(p), int(rng.integers(0, 3)), 1.0) for p in rng.permutation(npts)[:n_kps]] if n_kps else []) for c in (0, 1, 2)]
    return M.scene_from_lists(kfs, nk, cands, pts, vins_inited=True)
