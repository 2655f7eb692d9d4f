"""CPU tests of the Sim3 RANSAC solver (no GPU): the numpy checker tests/sim3_ref.py against ground truth, the measurement of every
tolerance the GPU tests use (mode "f32" against mode "f64"), the decision-band and skipped-set conditions, the exported symbols, the host
helpers viorb_sim3_draw_sets / viorb_sim3_ransac_iterations, and the host hooks viorb_debug_sim3_* (sim3_core.h compiled for the host)
against the checker."""
import ctypes as C
import functools
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi, sim3
from viorb_amd.synth import make_sim3_problem
import sim3_ref as T

f32, f64 = np.float32, np.float64
EPS32 = float(np.finfo(f32).eps)


@functools.lru_cache(maxsize=None)
def case(i):
    ps = T.PARAM_SETS[i]
    p = make_sim3_problem(*ps)
    return p, sim3.draw_sets(ps[2], T.ITERATIONS, ps[0]), ps[1] == "fix_scale"


@functools.lru_cache(maxsize=None)
def hyp(i, mode):
    p, sets, fix = case(i)
    return T.hypotheses(p, sets, fix, mode)


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(np.asarray(Ra, f64).T @ np.asarray(Rb, f64)) - 1) / 2, -1, 1)))


# ---- the checker against ground truth ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["general", "small_rotation"])
def test_noise_free_input_recovers_the_similarity(kind):
    p = make_sim3_problem(21, kind, 100, 0.0, 0.0, 0.0)
    sets = sim3.draw_sets(100, 50, 3)
    h = T.hypotheses(p, sets, False, "f64")
    good = h["gap"] >= T.GAP_MIN
    assert good.sum() >= 45
    for k in np.nonzero(good)[0]:
        assert rot_angle(h["R"][k], p["R12"]) < 2e-5
        assert np.linalg.norm(h["t"][k] - p["t12"]) < 2e-4 and abs(h["s"][k] - p["s12"]) < 2e-5 * p["s12"]
    r = T.ransac(p, sets, "f64", per_call=50)
    assert r["status"] == T.FOUND and r["best_iter"] == 0 and r["n_inliers"] == 100 and r["inliers"].all()


def test_fix_scale_returns_a_unit_scale():
    p = make_sim3_problem(22, "fix_scale", 100, 0.0, 0.0, 0.0)
    sets = sim3.draw_sets(100, 50, 4)
    for mode in ("f32", "f64"):
        h = T.hypotheses(p, sets, True, mode)
        assert (h["s"] == 1).all()
        k = int(np.argmax(h["gap"]))
        assert rot_angle(h["R"][k], p["R12"]) < 1e-3 and np.linalg.norm(h["t"][k] - p["t12"]) < 1e-3
    assert np.abs(T.hypotheses(p, sets, False, "f64")["s"] - 1).max() > 0           # the free scale is not exactly one


def test_with_outliers_the_inlier_set_is_the_true_one():
    p = make_sim3_problem(23, "general", 300, 0.3, 0.3, 0.0)
    sets = sim3.draw_sets(300, 300, 5)
    r = T.ransac(p, sets, "f64", per_call=300)
    assert r["status"] == T.FOUND
    k = int(np.argmax(r["counts"]))                                  # the best model of the whole run
    e1, e2 = T.errors(r["hyp"]["R"][k].astype(f32), r["hyp"]["t"][k].astype(f32), r["hyp"]["s"][k].astype(f32), p, "f64")
    fl, band = T.flags_of(e1, e2, p)[0], T.err_band(e1, e2, p, T.ERR_DEV_F32)[0]
    assert band.mean() <= T.MAX_BAND_SHARE_CPU
    assert (fl[~band] == (p["true_inlier"][~band] != 0)).all()
    assert fl.sum() == r["counts"][k] and abs(int(fl.sum()) - 210) <= band.sum()


# ---- measurement of the tolerances ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measured():
    dev = dict(R=0.0, T=0.0, S=0.0, ERR=0.0)
    info = dict(skipped=[], band=[], flips_outside_band=0, gap_c=0.0)
    for i in range(len(T.PARAM_SETS)):
        p, sets, fix = case(i)
        a, b = hyp(i, "f32"), hyp(i, "f64")
        keep = b["gap"] >= T.GAP_MIN
        dR = np.abs(a["R"].astype(f64) - b["R"]).max((1, 2))
        dev["R"] = max(dev["R"], float(dR[keep].max()))
        dev["T"] = max(dev["T"], float((np.linalg.norm(a["t"].astype(f64) - b["t"], axis=1) / b["O1n"])[keep].max()))
        dev["S"] = max(dev["S"], float((np.abs(a["s"].astype(f64) - b["s"]) / b["s"])[keep].max()))
        info["gap_c"] = max(info["gap_c"], float((dR * b["gap"]).max() / EPS32))
        info["skipped"].append(1 - keep.mean())
        e1, e2 = T.errors(a["R"], a["t"], a["s"], p, "f32")
        k = int(np.argmax(T.flags_of(e1, e2, p).sum(1)))              # the best model of the f32 mode, the same float32 model in both
        ea = (e1[k:k + 1], e2[k:k + 1]); eb = T.errors(a["R"][k], a["t"][k], a["s"][k], p, "f64")
        for x, y, m in zip(ea, eb, (T.max_error(p["sigma2_1"]).astype(f64), T.max_error(p["sigma2_2"]).astype(f64))):
            near = y[0] <= 2 * m
            dev["ERR"] = max(dev["ERR"], float((np.abs(x[0].astype(f64) - y[0]) / np.maximum(y[0], m))[near].max()))
        band = T.err_band(eb[0], eb[1], p, T.ERR_DEV_F32)
        info["flips_outside_band"] += int(((T.flags_of(*ea, p) != T.flags_of(*eb, p)) & ~band).sum())
        info["band"].append(band.mean())
    return dev, info


def test_float32_restatement_against_float64():
    """Every tolerance constant of sim3_ref.py is the rounded-up largest deviation of its f32 mode from its f64 mode on PARAM_SETS: a
    fresh measurement must not exceed it and must not be more than ten times below it."""
    dev, info = measured()
    print("measured deviations:", {k: "%.3g" % v for k, v in dev.items()})
    for k, v in dev.items():
        const = getattr(T, k + "_DEV_F32")
        assert v <= const, "%s_DEV_F32 = %g is below the measured %g" % (k, const, v)
        assert v >= const / 10, "%s_DEV_F32 = %g is more than ten times the measured %g" % (k, const, v)


def test_decision_bands_and_skipped_sets_of_the_checker_alone():
    dev, info = measured()
    print("skipped sets:", ["%.3f" % v for v in info["skipped"]], "bands:", ["%.4f" % v for v in info["band"]], "deviation x gap / eps32: %.2f" % info["gap_c"])
    assert info["flips_outside_band"] == 0
    assert max(info["band"]) <= T.MAX_BAND_SHARE_CPU
    assert max(info["skipped"]) <= T.MAX_SKIPPED_SETS
    assert info["gap_c"] <= T.GAP_C


def test_both_modes_take_the_same_decisions_on_the_parameter_sets():
    for i in range(len(T.PARAM_SETS)):
        p, sets, fix = case(i)
        a, b = T.ransac(p, sets, "f32", fix_scale=fix, per_call=T.ITERATIONS), T.ransac(p, sets, "f64", fix_scale=fix, per_call=T.ITERATIONS)
        assert (a["status"], a["best_iter"], a["iterations_done"]) == (b["status"], b["best_iter"], b["iterations_done"]) and a["status"] == T.FOUND
        e = T.errors(a["R12"], a["t12"], a["s12"], p, "f64")
        band = T.err_band(e[0], e[1], p, T.ERR_DEV_F32)[0]
        assert abs(a["n_inliers"] - b["n_inliers"]) <= band.sum()


# ---- the library, without a device ---------------------------------------------------------------------------------------------------------
def test_symbols_struct_sizes_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    assert C.sizeof(capi.Sim3Config) == 16 and C.sizeof(capi.Sim3Outputs) == 10 * C.sizeof(C.c_void_p) and C.sizeof(capi.Sim3Inputs) == 8 * C.sizeof(C.c_void_p)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_sim3.h"' in open(os.path.join(inc, "viorb.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "viorb_sim3.h")).read(), flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_SIM3)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_SIM3[name][1]) == n, name
    for struct, fields in (("outputs", capi.SIM3_OUTPUT_FIELDS), ("inputs", tuple(n for n, _ in capi.Sim3Inputs._fields_)),
                           ("config", tuple(n for n, _ in capi.Sim3Config._fields_))):
        m = re.search(r"typedef struct viorb_sim3_%s \{(.*?)\}" % struct, hdr, flags=re.S)
        assert tuple(re.findall(r"([A-Za-z0-9_]+)\s*;", m.group(1))) == fields
    assert not set(capi.SIGNATURES_SIM3) & set(capi.SIGNATURES)


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    p, sets, _ = case(5)
    if L.viorb_device_count() < 1:
        with pytest.raises(viorb_amd.ViorbError) as e:
            sim3.sim3_ransac(p, sets)
        assert e.value.code == capi.ERR_NO_DEVICE
    for j, v in ((1, sets[7, 0]), (0, 65), (2, -1)):                 # a repeated index, one past the end, a negative one
        bad = sets.copy(); bad[7, j] = v
        with pytest.raises(viorb_amd.ViorbError) as e:
            sim3.sim3_ransac(p, bad)
        assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(viorb_amd.ViorbError) as e:                   # no sets for iterations 300..399
        sim3.sim3_ransac(p, sets, max_its=400)
    assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(viorb_amd.ViorbError) as e:
        sim3.sim3_ransac(p, sets, iterations_per_call=0)
    assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(viorb_amd.ViorbError) as e:
        sim3.sim3_ransac(p, np.zeros((4097, 3), np.int32))
    assert e.value.code == capi.ERR_INVALID_ARG
    # the device forms: null arrays, sizes and the workspace are refused before any GPU call
    cfg, I, O = sim3.sim3_config(300), capi.Sim3Inputs(), capi.Sim3Outputs()
    one = C.c_void_p(256)
    assert L.viorb_sim3_ransac_device(C.byref(I), C.byref(cfg), one, one, one, one, 1, C.byref(O), one, 1 << 30, None) == capi.ERR_INVALID_ARG
    for f, _ in capi.Sim3Inputs._fields_[:7]:
        setattr(I, f, 256)
    I.cap = 0
    assert L.viorb_sim3_hypotheses_device(C.byref(I), C.byref(cfg), one, 1, one, one, one, one, one, 1 << 30, None) == capi.ERR_INVALID_ARG
    I.cap = 300
    assert L.viorb_sim3_hypotheses_device(C.byref(I), C.byref(cfg), one, 0, one, one, one, one, one, 1 << 30, None) == capi.ERR_INVALID_ARG
    assert L.viorb_sim3_hypotheses_device(C.byref(I), C.byref(cfg), one, 65536, one, one, one, one, one, 1 << 40, None) == capi.ERR_INVALID_ARG
    assert L.viorb_sim3_inliers_device(C.byref(I), C.byref(cfg), 1, one, one, one, one, None, one, 16, None) == capi.ERR_INVALID_ARG     # workspace too small
    assert L.viorb_sim3_inliers_device(C.byref(I), C.byref(cfg), 1, one, one, one, one, None, C.c_void_p(8), 1 << 30, None) == capi.ERR_INVALID_ARG
    assert L.viorb_sim3_select_device(C.byref(cfg), one, one, one, one, None, 1, one, one, one, one, None) == capi.ERR_INVALID_ARG
    assert L.viorb_sim3_workspace_bytes(0, 300, 1) == 0 and L.viorb_sim3_workspace_bytes(300, 4097, 1) == 0 and L.viorb_sim3_workspace_bytes(300, 300, 65536) == 0
    assert L.viorb_sim3_workspace_bytes(300, 300, 4) % 256 == 0 and L.viorb_sim3_workspace_bytes(300, 300, 4) > 0


def test_draw_sets():
    s = sim3.draw_sets(300, 300, 7)
    assert s.shape == (300, 3) and s.min() >= 0 and s.max() < 300
    assert all(len(set(r)) == 3 for r in s)
    assert (s == sim3.draw_sets(300, 300, 7)).all() and (s != sim3.draw_sets(300, 300, 8)).any()
    assert len(np.unique(s)) > 250                                   # the draws cover the list
    e = sim3.draw_sets(3, 50, 1)
    assert all(sorted(r) == [0, 1, 2] for r in e) and len({tuple(r) for r in e}) == 6
    with pytest.raises(viorb_amd.ViorbError) as err:
        sim3.draw_sets(2, 10, 0)
    assert err.value.code == capi.ERR_INVALID_ARG


def test_ransac_iterations_against_the_formula():
    for n, prob, mi, mx in ((300, 0.99, 20, 300), (40, 0.99, 20, 300), (25, 0.99, 20, 300), (21, 0.99, 20, 300), (100, 0.999, 20, 5000), (1000, 0.99, 20, 300),
                            (30, 0.5, 20, 300)):
        eps = float(f32(mi) / f32(n))
        want = max(1, min(int(np.ceil(np.log(1 - prob) / np.log(1 - eps ** 3))), mx))
        assert sim3.ransac_iterations(n, prob, mi, mx) == want == T.ransac_iterations(n, prob, mi, mx), (n, prob, mi, mx)
    assert sim3.ransac_iterations(40, 0.99, 20, 300) == 35 and sim3.ransac_iterations(300, 0.99, 20, 300) == 300
    assert sim3.ransac_iterations(20, 0.99, 20, 300) == 1                      # minInliers == N
    assert sim3.ransac_iterations(10, 0.99, 20, 300) == 300                    # N < minInliers: never read by iterate
    for bad in ((0, 0.99, 20, 300), (30, 1.0, 20, 300), (30, 0.0, 20, 300), (30, 0.99, 0, 300), (30, 0.99, 20, 0)):
        with pytest.raises(viorb_amd.ViorbError) as err:
            sim3.ransac_iterations(*bad)
        assert err.value.code == capi.ERR_INVALID_ARG


# ---- the host hooks against the checker ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 2, 3, 4])
def test_hook_horn_matches_the_checker(i):
    p, sets, fix = case(i)
    b = hyp(i, "f64")
    ks = range(0, len(sets), 3)
    skipped = 0
    for k in ks:
        reason, R, t, s = sim3.debug_horn(p["X1c"][sets[k]], p["X2c"][sets[k]], fix)
        assert reason == T.SET_OK
        if b["gap"][k] < T.GAP_MIN:
            skipped += 1
            continue
        assert np.abs(R - b["R"][k]).max() <= T.GPU_FACTOR * T.R_DEV_F32
        assert np.linalg.norm(t - b["t"][k]) <= T.GPU_FACTOR * T.T_DEV_F32 * b["O1n"][k]
        assert abs(s - b["s"][k]) <= T.GPU_FACTOR * T.S_DEV_F32 * b["s"][k] and (not fix or s == 1)
        assert abs(np.linalg.det(R.astype(f64)) - 1) < 1e-6
    assert skipped <= T.MAX_SKIPPED_SETS * len(ks)


def test_hook_horn_on_a_zero_rotation_and_on_a_collinear_set():
    P = np.array([[0.5, -0.25, 4.0], [-1.0, 0.75, 6.0], [1.5, 1.0, 3.0]], f32)
    reason, R, t, s = sim3.debug_horn(P, P)                           # identical points: the quaternion is (1, 0, 0, 0), 0 / 0 at :280
    assert reason == T.SET_ZERO_ROTATION and (R == 0).all() and (t == 0).all() and s == 0
    assert T.horn(P[None], P[None], False, "f64")["reason"][0] == T.SET_ZERO_ROTATION
    p, _, _ = case(0)
    inl, err, _ = sim3.debug_inlier(R, t, s, p["K1"], p["K2"], P[0], P[0], 1.0, 1.0)
    assert not inl and np.isnan(err).all()                             # every comparison fails, as with the reference's NaN matrices
    L = np.array([[0, 0, 4.0], [0.5, 0.25, 5.0], [1.0, 0.5, 6.0]], f32)  # collinear: the rotation about the line is free
    reason, R, t, s = sim3.debug_horn(L, (L * f32(0.5) + f32(0.25)).astype(f32))
    assert reason == T.SET_OK and np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s)
    assert abs(np.linalg.det(R.astype(f64)) - 1) < 1e-6 and abs(s - 2) < 1e-5
    assert T.horn(L[None], (L * f32(0.5) + f32(0.25))[None], False, "f64")["gap"][0] < T.GAP_MIN


def test_hook_thresholds_are_truncated_to_integers():
    p, _, _ = case(0)
    R, t = np.eye(3, dtype=f32), np.zeros(3, f32)
    X = np.array([0.5, -0.25, 4.0], f32)
    for sigma2, want in ((1.0, 9.0), (1.44, 13.0), (2.0736, 19.0), (f32(1.2) ** 2, 13.0)):
        _, _, mx = sim3.debug_inlier(R, t, 1.0, p["K1"], p["K2"], X, X, sigma2, sigma2)
        assert (mx == f32(want)).all() and (T.max_error([sigma2]) == f32(want)).all()
    # an error between the truncated and the untruncated threshold is an outlier: sigma2 = 1.44, 13 <= err < 13.26
    fx = float(p["K1"][0])
    for du, inlier in ((3.59, True), (3.62, False), (3.65, False)):      # du^2 = 12.9, 13.1, 13.3
        X2 = X.copy(); X2[0] += f32(du * 4.0 / fx)
        inl, err, mx = sim3.debug_inlier(R, t, 1.0, p["K1"], p["K2"], X, X2, 1.44, 1.44)
        assert inl == inlier and abs(err[0] - du * du) < 0.05, (du, err, mx)


@pytest.mark.parametrize("i", [1, 4])
def test_hook_inlier_errors_match_the_checker(i):
    p, sets, fix = case(i)
    a = hyp(i, "f32")
    e1, e2 = T.errors(a["R"], a["t"], a["s"], p, "f32")
    k = int(np.argmax(T.flags_of(e1, e2, p).sum(1)))
    R, t, s = a["R"][k], a["t"][k], a["s"][k]
    r1, r2 = T.errors(R, t, s, p, "f64")
    fl, band = T.flags_of(r1, r2, p)[0], T.err_band(r1, r2, p, T.GPU_FACTOR * T.ERR_DEV_F32)[0]
    m = (T.max_error(p["sigma2_1"]).astype(f64), T.max_error(p["sigma2_2"]).astype(f64))
    for j in range(len(fl)):
        inl, err, mx = sim3.debug_inlier(R, t, s, p["K1"], p["K2"], p["X1c"][j], p["X2c"][j], p["sigma2_1"][j], p["sigma2_2"][j])
        assert mx[0] == m[0][j] and mx[1] == m[1][j]
        for e, r, th in ((err[0], r1[0, j], m[0][j]), (err[1], r2[0, j], m[1][j])):
            if r <= 2 * th:
                assert abs(float(e) - r) <= T.GPU_FACTOR * T.ERR_DEV_F32 * max(r, th)
        if not band[j]:
            assert inl == bool(fl[j])
    assert band.mean() <= T.MAX_BAND_SHARE_GPU


def test_hook_select_rule():
    F, Cn, NM, FEW = T.FOUND, T.CONTINUE, T.NO_MORE, T.FEW
    sel = lambda c, n=300, mi=20, mx=None, first=0, best=0, per=5: sim3.debug_select(c, n, mi, len(c) if mx is None else mx, first, best, per)
    assert sel([25, 30, 40]) == (F, 1, 25, 0)                          # a first count above the minimum
    assert sel([3, 25, 40]) == (F, 2, 25, 1)
    assert sel([25, 30, 40], first=1, best=25) == (F, 2, 30, 1)        # a later larger one, after a resume
    assert sel([25, 24, 25, 30], first=1, best=25) == (F, 3, 25, 2)    # a tie updates and returns; the smaller count in between does not
    assert sel([20, 20, 20], mi=20) == (NM, 3, 20, 2)                  # == min_inliers is not enough; ties move the best to the last
    assert sel([5, 7, 7, 3, 1], mx=5) == (NM, 5, 7, 2)                 # nothing above the minimum: NO_MORE exactly at max_its
    assert sel([5, 7, 7, 3, 1, 0], mx=6) == (Cn, 5, 7, 2)              # ... and CONTINUE one before it
    assert sel([5, 7, 7, 3, 1, 0], mx=6, first=5, best=7) == (NM, 6, 7, -1)
    assert sel([30, 29, 28, 27, 26, 25, 24], first=1, best=30) == (Cn, 6, 30, -1)     # best_inliers_in above every later count
    assert sel([30, 29, 28, 27, 26, 25, 24], first=6, best=30) == (NM, 7, 30, -1)
    assert sel([30, 29, 28, 27, 26, 31], first=1, best=30) == (F, 6, 31, 5)          # FOUND at the last iteration: not NO_MORE
    assert sel([30] * 10, n=19) == (FEW, 0, 0, -1)
    assert sel([0, 0, 0], n=3, mi=2, mx=3) == (NM, 3, 0, 2)
    assert sel([1, 3], n=3, mi=2) == (F, 2, 3, 1)
    assert sel([9] * 8, first=8, best=3) == (NM, 8, 3, -1)             # already at max_its
    rng = np.random.default_rng(11)
    for _ in range(300):
        n_counts = int(rng.integers(1, 200))
        c = rng.integers(0, 40, n_counts)
        args = (int(rng.integers(15, 40)), int(rng.integers(1, 30)), int(rng.integers(1, n_counts + 20)), int(rng.integers(0, n_counts + 3)), int(rng.integers(0, 40)),
                int(rng.integers(1, 80)))
        assert sim3.debug_select(c, *args) == T.select(c, *args)
