"""CPU tests of relocalisation (no GPU): the exported symbols of include/viorb_relocalization.h, the host hooks viorb_debug_reloc_project /
_match / _decide (reloc_core.h compiled for the host) against the numpy checker tests/reloc_ref.py bit for bit, and the conditions the
fixtures of tests/test_gpu_relocalization.py have to meet, asserted on the checker alone, so that a green GPU run means something."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import relocalization as R
import reloc_ref as T
import reloc_cases as K

f32, f64 = np.float32, np.float64


def test_symbols_struct_sizes_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_relocalization.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_relocalization.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_RELOCALIZATION)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_RELOCALIZATION[name][1]) == n, name
    assert not set(capi.SIGNATURES_RELOCALIZATION) & set(capi.SIGNATURES)
    assert re.search(r"#define VIORB_S3M_ROTATION\s+9\b", text) and R.ROTATION == T.ROTATION == 9
    for code, name in enumerate(T.STAGE_NAMES):
        assert getattr(R, name) == getattr(T, name) == code
        if code:
            assert re.search(r"#define VIORB_RELOC_%s\s+%d\b" % (name, code), text), name
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(capi.RelocConfig) == 32 and C.sizeof(capi.RelocOutputs) == 8 * vp and C.sizeof(capi.RelocInputs) == 13 * vp
    for name in ("RelocBatch", "search_by_projection_reloc"):
        assert hasattr(viorb_amd, name)
    assert R.shape()[1] == 64 and R.shape()[0] % 64 == 0 and R.shape()[2] >= 1
    c = R.default_config()                                       # the reference's constants (src/Tracking.cc:2228-2269)
    assert (c.min_good, c.accept, c.narrow_above, c.th_coarse, c.orb_dist_coarse, c.th_narrow, c.orb_dist_narrow, c.check_orientation) == (10, 50, 30, 10.0, 100, 3.0, 64, 1)
    s = L.viorb_relocalization_workspace_bytes
    assert s(300, 400, 2) > 0 and s(R.MAX_FEATURES + 1, 400, 2) == 0 and s(300, 0, 2) == 0 and s(300, 400, 0) == 0


# ---- the host hooks against the checker, bit for bit --------------------------------------------------------------------------------------
def _same_projection(cam_ref, cam_lib, pose, X, th):
    g = R.debug_project(pose, X, cam_lib, K.BOUNDS, th)
    e = T.project(cam_ref, pose, X, th)
    assert g["reason"] == (e["reason"] if e["reason"] != T.MATCHED or T.cell_rect(cam_ref, e["u"], e["v"], e["radius"]) is not None else T.NO_FEATURE_IN_WINDOW)
    same = lambda a, b: (np.isnan(a) and np.isnan(b)) or a == b
    assert same(g["u"], e["u"]) and same(g["v"], e["v"])
    if e["reason"] not in (T.OUT_OF_IMAGE,):
        assert g["dist3D"] == e["dist3D"]
    if e["reason"] == T.MATCHED:
        assert g["level"] == e["level"] and g["radius"] == e["radius"]
        rect = T.cell_rect(cam_ref, e["u"], e["v"], e["radius"])
        if rect is not None:
            assert g["rect"] == rect
    return e


def test_project_hook_equals_the_checker_on_random_points_and_on_the_fixture():
    rng = np.random.default_rng(3)
    for nlevels in (8, 1, 3):
        sf = K.scale_factors(nlevels)
        cr, cl = K.ref_camera(sf), K.lib_camera(sf)
        seen = set()
        for _ in range(1500):
            pose, C0 = K.make_pose(rng)
            Rm, t = pose[:9].reshape(3, 3).astype(f64), pose[9:].astype(f64)
            Xc = np.array([rng.normal(0, 3), rng.normal(0, 2), rng.normal(0, 5)])
            Xw = (Rm.T @ (Xc - t)).astype(f32)
            d = np.linalg.norm(Xc)
            mx = d * rng.uniform(0.5, 4.0)
            X = np.concatenate([Xw, [0, 0, 0, mx / rng.uniform(1.0, 4.0), mx]]).astype(f32)
            seen.add(_same_projection(cr, cl, pose, X, rng.choice([3.0, 10.0]))["reason"])
        assert seen >= {T.MATCHED, T.OUT_OF_IMAGE, T.OUT_OF_RANGE}
    F = K.matcher_fixture()
    cl = K.lib_camera(F["sf"])
    for h in F["hyps"][:1]:
        for X in h["pts_f"]:
            _same_projection(F["cam"], cl, h["pose12"], X, K.TH_COARSE)


def _random_lists(rng, npts, nfeat, max_len, dist_hi):
    cands = []
    for _ in range(npts):
        n = int(rng.integers(0, max_len + 1))
        feats = rng.choice(nfeat, min(n, nfeat), replace=False) if nfeat else []
        cands.append([(int(rng.integers(0, dist_hi)), int(f)) for f in feats])
    return cands


def test_match_hook_equals_the_literal_loop_on_random_and_adversarial_lists():
    rng = np.random.default_rng(11)
    for trial in range(120):
        npts, nfeat = int(rng.integers(0, 60)), int(rng.integers(1, 25))
        cands = _random_lists(rng, npts, nfeat, 6, int(rng.choice([8, 40, 140])))
        taken = (rng.uniform(size=nfeat) < 0.15).astype(np.uint8)
        ak = np.where(rng.uniform(size=npts) < 0.7, 100.0, rng.uniform(0, 359.9, npts)).astype(f32)
        af = np.where(rng.uniform(size=nfeat) < 0.7, 40.0, rng.uniform(0, 359.9, nfeat)).astype(f32)
        for od, ori in ((100, True), (64, True), (int(rng.integers(0, 140)), False)):
            bi, rm, nm = R.debug_match(cands, taken, ak, af, od, ori)
            e = T.match_lists(cands, taken, ak, af, od, ori)
            assert np.array_equal(bi, e[0]) and np.array_equal(rm, e[1]) and nm == e[2], (trial, od, ori)
    # every point wants the same features, best first: point p ends with feature p
    n = 70
    cands = [[(f, f) for f in range(n)] for _ in range(n)]
    bi, rm, nm = R.debug_match(cands, np.zeros(n, np.uint8), np.zeros(n, f32), np.zeros(n, f32), 100, True)
    assert np.array_equal(bi, np.arange(n)) and nm == n and not rm.any()
    # a removed match keeps its feature during the loop: point 0 takes feature 0 and loses it to the histogram, point 1 still takes feature 1
    cands = [[(1, 0)], [(1, 0), (5, 1)]] + [[(2, 2 + k)] for k in range(20)]
    ak = np.array([200.0, 0.0] + [0.0] * 20, f32)
    bi, rm, nm = R.debug_match(cands, np.zeros(22, np.uint8), ak, np.zeros(22, f32), 100, True)
    e = T.match_lists(cands, np.zeros(22, np.uint8), ak, np.zeros(22, f32), 100, True)
    assert np.array_equal(bi, e[0]) and bi[0] == -1 and rm[0] == 1 and bi[1] == 1 and nm == e[2] == 21


def test_decide_hook_is_the_reference_thresholds():
    c = R.default_config()
    for g in range(0, 80):
        assert R.debug_decide(c, 1, g) == (T.FEW_INLIERS if g < 10 else (T.RUNNING if g < 50 else T.ACCEPTED_FIRST))
        assert R.debug_decide(c, 3, g) == (T.RUNNING if 30 < g < 50 else (T.ACCEPTED_SECOND if g >= 50 else T.SECOND_WEAK))
        assert R.debug_decide(c, 5, g) == (T.ACCEPTED_THIRD if g >= 50 else T.THIRD_REJECTED)
        for a in (0, 1, 49 - g, 50 - g, 51 - g):
            assert R.debug_decide(c, 2, g, a) == (T.RUNNING if a + g >= 50 else T.COARSE_SHORT)
            assert R.debug_decide(c, 4, g, a) == (T.RUNNING if a + g >= 50 else T.NARROW_SHORT)
    c2 = R.default_config(min_good=4, accept=20, narrow_above=12)
    assert R.debug_decide(c2, 1, 3) == T.FEW_INLIERS and R.debug_decide(c2, 1, 4) == T.RUNNING and R.debug_decide(c2, 1, 20) == T.ACCEPTED_FIRST
    assert R.debug_decide(c2, 3, 12) == T.SECOND_WEAK and R.debug_decide(c2, 3, 13) == T.RUNNING


# ---- the conditions the matcher fixture has to meet ---------------------------------------------------------------------------------------
def test_matcher_fixture_holds_every_condition_the_gpu_tests_rely_on():
    F = K.matcher_fixture()
    frame, tags, feat, hyp = K.matcher_frame(), F["tags"], F["feat"], F["hyps"][0]
    want, free, unordered = K.matcher_expected(0), K.matcher_expected(0, False), K.matcher_expected(0, False, False)
    bi, re = want["best_idx"], want["reason"]
    assert 250 <= frame.N <= 400 and len(F["sf"]) == 8
    # every reason this function can end with, the histogram removal included; the three it cannot end with never occur
    assert set(re.tolist()) == set(T.POSSIBLE_REASONS)
    proj = [T.project(F["cam"], hyp["pose12"], X, K.TH_COARSE) for X in hyp["pts_f"]]
    one = lambda name: tags[name][0]
    # z < 0 and matched
    i = one("behind")
    z = (T.S._mul3(hyp["pose12"][:9].reshape(3, 3), hyp["pts_f"][i][:3]) + hyp["pose12"][9:])[2]
    assert z < 0 and bi[i] == feat["behind"]
    # z = 0 with x = y = 0: NaN coordinates pass the bounds test and the window is empty
    i = one("nan")
    pc = T.S._mul3(hyp["pose12"][:9].reshape(3, 3), hyp["pts_f"][i][:3]) + hyp["pose12"][9:]
    assert (pc == 0).all() and np.isnan(proj[i]["u"]) and np.isnan(proj[i]["v"]) and proj[i]["reason"] == T.MATCHED and re[i] == T.NO_FEATURE_IN_WINDOW
    # exactly on each bound, and matched there
    for name, key, val in (("on_min_x", "u", 0.0), ("on_max_x", "u", 752.0), ("on_min_y", "v", 0.0), ("on_max_y", "v", 480.0)):
        i = one(name)
        assert proj[i][key] == f32(val) and bi[i] == feat[name], name
    # dist3D equal to each distance limit passes; one ulp beyond does not
    i = one("at_min_distance")
    assert proj[i]["dist3D"] == f32(0.8) * hyp["pts_f"][i][6] and bi[i] == feat["at_min_distance"]
    i = one("at_max_distance")
    assert proj[i]["dist3D"] == f32(1.2) * hyp["pts_f"][i][7] and bi[i] == feat["at_max_distance"]
    assert all(re[i] == T.OUT_OF_RANGE for i in tags["out_of_range"]) and len(tags["out_of_range"]) == 2
    # predicted levels 0 and top
    levels = {proj[i]["level"] for i in range(len(proj)) if re[i] in (T.MATCHED, T.ROTATION)}
    assert 0 in levels and 7 in levels and proj[one("top_level")]["level"] == 7 and bi[one("top_level")] == feat["top_level"]
    # a feature wanted by three points whose second choices differ; the first of them loses its match to the histogram, and the feature stays claimed
    a, b, c = tags["trio"]
    assert unordered["best_idx"][a] == unordered["best_idx"][b] == unordered["best_idx"][c] == feat["trio0"]
    assert free["best_idx"][a] == feat["trio0"] and bi[a] == -1 and re[a] == T.ROTATION
    assert bi[b] == feat["trio1"] and bi[c] == feat["trio2"]
    # the chain: without the order every point takes its own feature; in order each is pushed to the next, 64 deep
    ch = tags["chain"]
    assert len(ch) == 64 and free["best_idx"][one("chain_start")] == feat["chain0"]
    for k, i in enumerate(ch):
        assert unordered["best_idx"][i] == feat["chain%d" % k] and free["best_idx"][i] == feat["chain%d" % (k + 1)]
    # more than eight candidates under orb_dist (the lists of the kernel hold R.shape()[2])
    for k, i in enumerate(tags["cluster"]):
        g = proj[i]
        cand = [j for j in T.get_features_in_area(frame, g["u"], g["v"], g["radius"], g["level"] - 1, g["level"] + 1)
                if not hyp["feat_taken"][j] and T.hamming(hyp["pts_desc"][i], frame.desc[j]) <= K.ORB_COARSE]
        assert len(cand) >= 12 > R.shape()[2] and free["best_idx"][i] == feat["cluster%d" % k]
    # distance exactly orb_dist matches, orb_dist + 1 does not
    i, j = one("at_orb_dist"), one("above_orb_dist")
    assert T.hamming(hyp["pts_desc"][i], frame.desc[feat["at_orb_dist"]]) == K.ORB_COARSE and free["best_idx"][i] == feat["at_orb_dist"]
    assert T.hamming(hyp["pts_desc"][j], frame.desc[feat["above_orb_dist"]]) == K.ORB_COARSE + 1 and re[j] == T.ABOVE_THRESHOLD
    # a tie in distance goes to the first in visiting order, which is not the lower index
    i = one("tie")
    assert feat["tie_first_visited"] > feat["tie_lower_index"] and free["best_idx"][i] == feat["tie_first_visited"]
    # no feature in the window: an empty region, and a window whose only feature is two levels off; a window whose only feature is taken
    assert re[one("empty_window")] == re[one("level_off")] == T.NO_FEATURE_IN_WINDOW and re[one("taken_only")] == T.ABOVE_THRESHOLD
    assert all(re[i] == T.OUT_OF_IMAGE for i in tags["outside"])
    # the histograms: a tie between the third and the fourth bin (first hypothesis); the 0.1 * max rule drops the second and third (second)
    def histogram(h):
        fr = K.matcher_expected(h, False)["best_idx"]
        hist = [[] for _ in range(30)]
        for p in np.nonzero(fr >= 0)[0]:
            hist[T.rot_bin(F["hyps"][h]["kf_angle"][p], frame.kps["angle"][fr[p]])].append(p)
        return hist
    h0 = histogram(0)
    sizes = sorted((len(b) for b in h0), reverse=True)
    ind = T.compute_three_maxima(h0, 30)
    assert sizes[2] == sizes[3] > 0 and sizes[2] >= 0.1 * sizes[0] and -1 not in ind and ind[2] == 9 and len(h0[11]) == len(h0[9])
    assert (re == T.ROTATION).sum() == sum(len(b) for k, b in enumerate(h0) if k not in ind) >= sizes[3]
    h1 = histogram(1)
    sizes1 = sorted((len(b) for b in h1), reverse=True)
    assert T.compute_three_maxima(h1, 30)[1:] == (-1, -1) and sizes1[1] > 0 and sizes1[2] > 0
    assert (K.matcher_expected(1)["reason"] == T.ROTATION).sum() == sizes1[1] + sizes1[2]
    # the result differs from the unordered function and from the result without the orientation check
    assert (free["best_idx"] != unordered["best_idx"]).sum() >= 64 + 2 + 2                   # the chain, two of the trio, two of the cluster
    assert not np.array_equal(bi, K.matcher_expected(0, True, False)["best_idx"])
    assert (bi != free["best_idx"]).sum() >= 10 and want["nmatches"] < free["nmatches"]
    assert want["nmatches"] == (bi >= 0).sum() >= 100


def test_small_problems_match_and_contend():
    for npts in (63, 257, 513):
        P = K.small_problem(npts, npts, 300)
        e = K.small_expected(P)
        assert e["nmatches"] >= npts // 8
        u = K.ref_search(T.Frame(P["cam"], P["kps"], P["desc"]), P["hyp"], ordered=False)
        assert not np.array_equal(u["best_idx"], e["best_idx"])
    P = K.small_problem(7, 200, 300, 1)
    assert len(P["sf"]) == 1 and K.small_expected(P)["nmatches"] >= 20


# ---- the cascade fixtures -----------------------------------------------------------------------------------------------------------------
def _ulps(k):
    def move(pose):
        p = np.array(pose, f32)
        for _ in range(abs(k)):
            p = np.nextafter(p, f32(np.inf if k > 0 else -np.inf), dtype=f32)
        return p
    return move


def _alternate(pose):
    p = np.array(pose, f32)
    up, dn = _ulps(2)(p), _ulps(-2)(p)
    return np.where(np.arange(12) % 2 == 0, up, dn).astype(f32)


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_cascade_fixtures_leave_at_every_exit_and_stay_put_under_two_ulps(oracle, stereo):
    """One hypothesis per exit under the reference's constants; each keeps its stage, counts, map points and outlier flags when every pose
    a solve hands on is moved by two float ulps in every entry (up, down, alternating): a fixture-robustness condition, so that the
    device's solver, which agrees with the oracle's to 1e-5 in chi2 and not bit for bit, cannot flip a decision."""
    F = K.cascade_fixture(stereo)
    want = K.cascade_expected(oracle.pose_opt_se3, stereo)
    assert [w["stage"] for w in want] == list(K.CASCADE_EXITS) and len(set(K.CASCADE_EXITS)) == 8
    for k, w in enumerate(want):
        plan = K.CASCADE_PLANS[w["stage"]]
        assert w["accepted"] == (w["stage"] in (T.ACCEPTED_FIRST, T.ACCEPTED_SECOND, T.ACCEPTED_THIRD))
        assert w["counts"][0] == plan[0], (k, w["counts"])
    for key, cfg in K.CONFIGS.items():                           # the other configurations the GPU tests run stay put as well
        for k, w in enumerate(K.cascade_expected(oracle.pose_opt_se3, stereo, cfg_key=key)):
            for move in (_ulps(2), _ulps(-2), _alternate):
                g = K.ref_refine(F, k, oracle.pose_opt_se3, cfg, perturb=move)
                assert g["stage"] == w["stage"] and np.array_equal(g["counts"], w["counts"]), (key, k, g["counts"], w["counts"])
                assert np.array_equal(g["frame_match"], w["frame_match"]) and np.array_equal(g["outlier"], w["outlier"]) and g["n_good"] == w["n_good"]
    by = {w["stage"]: w for w in want}
    # what each exit leaves behind (:2228 nothing nulled; :2231-2233 outliers nulled; :2246-2252 the second solve's outliers stay)
    w = by[T.FEW_INLIERS]
    assert (w["counts"][1:5] == -1).all() and (w["frame_match"] >= 0).sum() == 8
    w = by[T.ACCEPTED_FIRST]
    assert w["outlier"].sum() == 5 and not (w["outlier"].astype(bool) & (w["frame_match"] >= 0)).any() and (w["frame_match"] >= 0).sum() == w["n_good"] == 70
    for st in (T.SECOND_WEAK, T.NARROW_SHORT):
        w = by[st]
        assert (w["outlier"].astype(bool) & (w["frame_match"] >= 0)).sum() >= 10                # outliers of the second solve that were not nulled
    w = by[T.NARROW_SHORT]
    assert 30 < w["counts"][2] < 50 and w["counts"][3] == 3 and w["counts"][4] == -1
    w = by[T.ACCEPTED_THIRD]
    assert w["counts"][3] == 9 and w["counts"][4] >= 50 and not (w["outlier"].astype(bool) & (w["frame_match"] >= 0)).any()
    w = by[T.THIRD_REJECTED]
    assert w["counts"][2] + w["counts"][3] >= 50 > w["counts"][4]
    # non-default thresholds move the exits: the configuration is read
    assert [o["stage"] for o in K.cascade_expected(oracle.pose_opt_se3, stereo, cfg_key="low")] != [w["stage"] for w in want]
    assert [o["counts"][1] for o in K.cascade_expected(oracle.pose_opt_se3, stereo, cfg_key="tight")] != [w["counts"][1] for w in want]
