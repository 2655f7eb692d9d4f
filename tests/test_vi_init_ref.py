"""CPU checks of the visual-inertial initialisation: the numpy restatement tests/vi_init_ref.py against the synthetic truth, its
float32 form against its float64 form (which fixes the tolerances the GPU tests grant the device), and the library's shared
arithmetic compiled for the host (viorb_debug_vi_init_*) against the restatement."""
import ctypes as C
import functools
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi
from viorb_amd.capi import ptr
from viorb_amd.synth import make_vi_init_problem
import vi_init_ref as vr

_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_f64 = lambda a: np.ascontiguousarray(a, np.float64)


@functools.lru_cache(maxsize=None)
def case(seed, N, kf_dt, noise):
    p = make_vi_init_problem(seed, N, kf_dt=kf_dt, noise=noise)
    return p, vr.vi_init(p, mode="f64"), vr.vi_init(p, mode="f32")


def test_entry_points_are_exported_and_refuse_without_a_device():
    L = viorb_amd.lib()
    names = ["viorb_preintegrate_intervals_device", "viorb_preintegrate_intervals", "viorb_optimize_initial_gyro_bias_device",
             "viorb_optimize_initial_gyro_bias", "viorb_vi_init_device", "viorb_vi_init", "viorb_vi_init_apply_device", "viorb_vi_init_apply",
             "viorb_scale_map_points_device", "viorb_debug_vi_init_gyro_edge", "viorb_debug_vi_init_gyro_solve", "viorb_debug_vi_init_rows",
             "viorb_debug_vi_init_solve", "viorb_debug_vi_init_rwi", "viorb_debug_vi_init_navstate"]
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viorb.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(viorb_(?:debug_)?(?:vi_init|preintegrate_intervals|optimize_initial_gyro_bias|scale_map_points)[a-z0-9_]*)\s*\(", hdr))
    assert declared == set(names), declared ^ set(names)       # every new symbol of the header is in the list
    for n in names:
        assert hasattr(L, n), n
        assert n in capi.SIGNATURES, n
    assert L.viorb_abi_version() == 2
    assert C.sizeof(capi.ViInitConfig) == 19 * 8
    if L.viorb_device_count() > 0:
        return
    p = make_vi_init_problem(0, 5)
    cfg = dict(Tbc=p["Tbc"], g=p["g"])
    pre = vr.preintegrations(p, 5)
    codes = []
    est_ok = np.zeros(48); est_ok[7] = 1.0
    for call in (lambda: viorb_amd.PreintegrateIntervals(p), lambda: viorb_amd.OptimizeInitialGyroBias(cfg, p["twc12"], pre),
                 lambda: viorb_amd.ViInitHost(cfg, p, pre), lambda: viorb_amd.ViInitApplyHost(cfg, p, np.zeros((5, 12), np.float32), est_ok, pre, 4, 5)):
        try:
            call()
        except viorb_amd.ViorbError as e:
            codes.append(e.code)
    # the device forms check for a device before they touch a pointer: host arrays stand in for device memory here
    c = viorb_amd.vi_config(cfg)
    z = np.zeros(4096, np.uint8); v = ptr(z)
    codes.append(L.viorb_preintegrate_intervals_device(v, v, v, v, 0, None, None, 0.0, 0.0, 0, 4, 1, v, None))
    codes.append(L.viorb_optimize_initial_gyro_bias_device(C.byref(c), v, v, v, 4, 1, v, v, None))
    codes.append(L.viorb_vi_init_device(C.byref(c), v, v, v, v, 0, v, v, 4, 1, v, v, v, None))
    f = np.zeros(64, np.float32); fv = ptr(f)
    apply_args = lambda preint_out, preint_v: (C.byref(c), v, v, v, v, v, 0, v, v, v, v, preint_v, 4, 1, v, v, preint_out, None)
    w = ptr(np.zeros(4096, np.uint8))
    codes.append(L.viorb_vi_init_apply_device(*apply_args(v, w)))
    codes.append(L.viorb_scale_map_points_device(fv, None, None, v, v, 4, 1, None))
    assert codes == [capi.ERR_NO_DEVICE] * 9, codes
    assert b"no HIP device" in L.viorb_last_error()
    # argument checks come first
    assert L.viorb_vi_init_apply_device(*apply_args(v, v)) == capi.ERR_INVALID_ARG          # preint (out) == preint_v
    assert L.viorb_vi_init_apply_device(*apply_args(None, w)) == capi.ERR_INVALID_ARG
    assert L.viorb_scale_map_points_device(None, None, None, v, v, 4, 1, None) == capi.ERR_INVALID_ARG
    assert L.viorb_scale_map_points_device(fv, None, None, v, v, -1, 1, None) == capi.ERR_INVALID_ARG
    assert L.viorb_vi_init_apply(C.byref(c), 3, 5, v, v, v, v, v, v, v, v, v, v) == capi.ERR_INVALID_ARG     # n_est < 4
    assert L.viorb_vi_init_device(C.byref(c), v, v, v, v, 0, v, v, 4, 1, v, v, None, None) == capi.ERR_INVALID_ARG
    assert L.viorb_preintegrate_intervals_device(v, v, v, v, 0, None, None, 0.0, 0.0, 8, 4, 1, v, None) == capi.ERR_INVALID_ARG


@pytest.mark.parametrize("noise", [0.0, 1.0])
def test_float64_restatement_recovers_the_synthetic_truth(noise):
    """What the METHOD can do on the committed parameter sets (a fresh measurement of the restatement, rounded up; not a bound on the
    device). Measured maxima, noise-free / with sample noise (0.01 rad/s, 0.1 m/s^2): scale 0.23 % / 0.24 %, gravity direction 0.19 /
    0.26 degrees, accelerometer bias 0.035 / 0.039 m/s^2, gyro bias 1.2e-6 / 9.3e-4 rad/s; cond(A) 1.7-2.9, cond(C) 40-92."""
    bound = dict(s=3e-3, gw=0.25, ba=0.04, bg=2e-6) if noise == 0 else dict(s=3e-3, gw=0.3, ba=0.05, bg=1.5e-3)
    seen = dict(s=0, gw=0, ba=0, bg=0)
    for ps in vr.PARAMETER_SETS:
        if ps[3] != noise:
            continue
        p, r, _ = case(*ps)
        t = p["truth"]
        assert r["status"] == vr.OK
        ang = np.degrees(np.arccos(np.clip(r["gw"] @ t["gw"] / np.linalg.norm(r["gw"]) / np.linalg.norm(t["gw"]), -1, 1)))
        got = dict(s=abs(r["s"] / t["s"] - 1), gw=ang, ba=np.abs(r["ba"] - t["ba"]).max(), bg=np.abs(r["bg"] - t["bg"]).max())
        for k in seen:
            seen[k] = max(seen[k], got[k])
        assert abs(np.linalg.norm(r["gw"]) - p["g"]) < 1e-9 and r["cond_a"] < 4 and r["cond_c"] < 120
    print("truth recovery, noise %g: %s" % (noise, seen))
    for k in seen:
        assert seen[k] <= bound[k], (k, seen[k], bound[k])


def test_float32_restatement_against_float64():
    """DEV_F32: the reference's own rounding band per output quantity; the constants in vi_init_ref.py are not exceeded and not more
    than ten times too loose."""
    seen = {k: 0.0 for k in vr.DEV_F32}
    for ps in vr.PARAMETER_SETS:
        _, r64, r32 = case(*ps)
        assert r32["status"] == vr.OK
        for k, v in vr.deviations(r32, r64).items():
            seen[k] = max(seen[k], v)
    print("DEV_F32 measured:", seen)
    for k, v in seen.items():
        assert v <= vr.DEV_F32[k], (k, v)
        assert vr.DEV_F32[k] <= 10 * v, (k, v, "constant more than ten times too loose")


def test_gyro_bias_double_against_longdouble():
    """DEV_F64_BG: the double gyro-bias step against the same step in longdouble with the edges summed in reverse order."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is not wider than double on this platform")
    seen = 0.0
    for ps in vr.PARAMETER_SETS:
        p, r64, _ = case(*ps)
        ref = vr.gyro_bias(p, vr.preintegrations(p, ps[1]), ps[1], np.longdouble, reverse=True)
        seen = max(seen, float(np.abs(r64["bg"] - ref).max()))
    print("DEV_F64_BG measured: %.3g" % seen)
    assert seen <= vr.DEV_F64_BG and vr.DEV_F64_BG <= 10 * seen


def test_degenerate_and_short_streams_return_a_status():
    p = make_vi_init_problem(1, 12)
    assert vr.vi_init(p, n_est=3)["status"] == vr.INVALID
    q = dict(p); q["imu_start"] = p["imu_start"].copy(); q["imu_start"][6:] -= (p["imu_start"][6] - p["imu_start"][5])      # interval 5 empty
    assert vr.vi_init(q)["status"] == vr.INVALID
    m = vr.motionless(12)
    assert vr.vi_init(m, mode="f64")["status"] == vr.DEGENERATE and vr.vi_init(m, mode="f32")["status"] == vr.DEGENERATE


# ---- the library's host hooks against the restatement -------------------------------------------------------------------------------
def test_hook_gyro_edge_and_solve_match_the_restatement():
    L = viorb_amd.lib()
    for ps in vr.PARAMETER_SETS[::7]:
        p, r64, _ = case(*ps)
        N = ps[1]
        pre = vr.preintegrations(p, N)
        Rcb, _ = vr.extrinsics(p["Tbc"])
        Hg = np.zeros(12)
        for i in range(1, N):
            e, J, hg = np.zeros(3), np.zeros(9), np.zeros(12)
            L.viorb_debug_vi_init_gyro_edge(ptr(_f64(p["Tbc"])), ptr(_f32(p["twc12"][i - 1])), ptr(_f32(p["twc12"][i])), ptr(_f64(pre[i])), ptr(e), ptr(J), ptr(hg))
            e_ref, J_ref = vr.gyro_edge(Rcb, p["twc12"][i - 1], p["twc12"][i], pre[i])
            # the product's SO3 functions against the oracle's: the 1e-12 double state is granted across the suite
            assert np.allclose(e, e_ref, rtol=0, atol=1e-12) and np.allclose(J.reshape(3, 3), J_ref, rtol=1e-12, atol=1e-12)
            Hg += hg
        bg = np.zeros(3)
        assert L.viorb_debug_vi_init_gyro_solve(ptr(Hg), ptr(bg)) == 0
        assert np.abs(bg - r64["bg"]).max() <= max(4 * vr.DEV_F64_BG, 1e-12)
    assert L.viorb_debug_vi_init_gyro_solve(ptr(np.zeros(12)), ptr(bg)) == capi.VI_DEGENERATE and not bg.any()


def test_hook_triplet_rows_match_the_restatement():
    """Rows of A|B and C|D for one triplet: double products in another association than numpy's, so a few ulps of the largest term of a row
    (|terms| < 1 here): 1e-14 absolute."""
    L = viorb_amd.lib()
    for ps in vr.PARAMETER_SETS[::5]:
        p, r64, _ = case(*ps)
        pre = r64["preint_bg"]
        for i in (0, ps[1] // 2, ps[1] - 3):
            ab, cd = np.zeros(15), np.zeros(21)
            L.viorb_debug_vi_init_rows(ptr(_f64(p["Tbc"])), ptr(_f32(p["twc12"][i:i + 3])), ptr(_f64(pre[i + 1])), ptr(_f64(pre[i + 2])), ptr(_f64(r64["Rwi"])),
                                       C.c_double(p["g"]), ptr(ab), ptr(cd))
            AB, CD = vr.triplet_rows(p, pre, i, r64["Rwi"], "f64")
            assert np.abs(ab.reshape(3, 5) - AB).max() <= 1e-14 and np.abs(cd.reshape(3, 7) - CD).max() <= 1e-14
        R = np.zeros(9)
        assert L.viorb_debug_vi_init_rwi(ptr(_f64(r64["gwstar"])), ptr(R)) == 0
        assert np.abs(R.reshape(3, 3) - r64["Rwi"]).max() <= 1e-14
    assert L.viorb_debug_vi_init_rwi(ptr(_f64([0, 0, 9.8])), ptr(R)) == capi.VI_DEGENERATE
    assert L.viorb_debug_vi_init_rwi(ptr(_f64([0, 0, 0])), ptr(R)) == capi.VI_DEGENERATE


@pytest.mark.parametrize("n", [4, 6])
@pytest.mark.parametrize("cond", [3.0, 1e2, 1e4])
def test_hook_small_solve_against_lapack(n, cond):
    """The Gram-matrix solve against numpy.linalg.lstsq / svd in double. Forming M^T M squares the condition number: the solution of the
    normal equations carries a relative error of about cond^2 eps (Higham, Accuracy and Stability of Numerical Algorithms, §20.4), the
    eigenvalues of the Gram matrix an absolute one of about eps |M|^2, i.e. each singular value one of eps |M|^2 / (2 w). The bounds below
    are those expressions with a factor 20 for the constants hidden in `about` (dimension, sums over 90 rows)."""
    L = viorb_amd.lib()
    eps = np.finfo(np.float64).eps
    rng = np.random.default_rng(int(n * 1000 + cond))
    for _ in range(5):
        m = 90
        U, _ = np.linalg.qr(rng.normal(size=(m, n))); V, _ = np.linalg.qr(rng.normal(size=(n, n)))
        w_true = np.geomspace(1.0, 1.0 / cond, n) * rng.uniform(0.5, 5)
        M = _f64(U * w_true @ V.T)
        x_true = rng.normal(size=n)
        v = _f64(M @ x_true + 1e-3 * rng.normal(size=m))
        x, w = np.zeros(n), np.zeros(n)
        assert L.viorb_debug_vi_init_solve(ptr(M), ptr(v), m, n, ptr(x), ptr(w)) == 0
        x_ref = np.linalg.lstsq(M, v, rcond=None)[0]
        w_ref = np.linalg.svd(M, compute_uv=False)
        assert np.linalg.norm(x - x_ref) <= 20 * cond ** 2 * eps * np.linalg.norm(x_ref), (np.linalg.norm(x - x_ref), cond)
        assert np.all(np.abs(w - w_ref) <= 20 * eps * w_ref[0] ** 2 / (2 * w_ref)), (w, w_ref)
        assert np.all(np.diff(w) <= 0)


@pytest.mark.parametrize("n", [4, 6])
def test_hook_small_solve_reports_rank_deficiency(n):
    L = viorb_amd.lib()
    rng = np.random.default_rng(n)
    M = rng.normal(size=(60, n))
    M[:, 0] = 0.0                                              # the motionless stream's shape: an exactly zero column
    x, w = np.ones(n), np.ones(n)
    assert L.viorb_debug_vi_init_solve(ptr(_f64(M)), ptr(_f64(rng.normal(size=60))), 60, n, ptr(x), ptr(w)) == capi.VI_DEGENERATE
    M = rng.normal(size=(60, n)); M[:, n - 1] = M[:, 0] * (1 + 1e-9)      # two columns parallel to 1e-9: under the 1e-7 the solve resolves
    assert L.viorb_debug_vi_init_solve(ptr(_f64(M)), ptr(_f64(rng.normal(size=60))), 60, n, ptr(x), ptr(w)) == capi.VI_DEGENERATE
    assert L.viorb_debug_vi_init_solve(ptr(_f64(M)), ptr(_f64(M[:, 0])), 60, 5, ptr(x), ptr(w)) == capi.ERR_INVALID_ARG


def test_interval_clamp_is_expressed_on_the_stamps():
    """vi_init_ref.interval: with no stamp out of order the clamped and the plain integration agree exactly."""
    p = make_vi_init_problem(2, 4)
    S = p["imu"][p["imu_start"][2]:p["imu_start"][3]]
    a = vr.interval(S, np.zeros(3), np.zeros(3), p["kf_time"][1], p["kf_time"][2], True)
    b = vr.interval(S, np.zeros(3), np.zeros(3), p["kf_time"][1], p["kf_time"][2], False)
    assert (a == b).all()


@pytest.mark.parametrize("n_est,n_kf", [(12, 12), (9, 12), (11, 12), (4, 5)])
def test_hook_navstate_matches_the_restatement(n_est, n_kf):
    """viorb_debug_vi_init_navstate (forward, newest-of-set and trailing velocities) against vi_init_ref.apply: atol 1e-11 on double
    state, what test_imu_predict_matches_oracle grants a predicted NavState."""
    L = viorb_amd.lib()
    p, _, _ = case(1, 12, 0.25, 0.0)
    r = vr.vi_init(p, n_est=n_est)
    assert r["status"] == vr.OK
    pv = np.zeros((n_kf, 142)); pv[:n_est] = r["preint_bg"]
    ns_ref, fin = vr.apply(p, r, n_est, n_kf, pv)
    est = np.zeros(48); est[0:3] = r["bg"]; est[7] = r["s"]; est[10:13] = r["ba"]; est[31:34] = r["gw"]
    for i in range(n_kf):
        ns = np.full(22, np.nan)
        L.viorb_debug_vi_init_navstate(ptr(_f64(p["Tbc"])), i, n_est, n_kf, ptr(_f32(p["twc12"][:n_kf])), ptr(est), ptr(_f64(pv)), ptr(_f64(fin)), ptr(ns))
        q = ns[6:10] if ns[6:10] @ ns_ref[i, 6:10] > 0 else -ns[6:10]
        np.testing.assert_allclose(np.concatenate([ns[:6], q, ns[10:]]), ns_ref[i], rtol=0, atol=1e-11, err_msg="key frame %d" % i)
    # the restatement's velocities against the true ones: measured 0.005, 0.034, 0.047 and 0.10 m/s on these four cases (the estimate's own error: the last uses 4 key frames; speeds reach 3.5 m/s); a sign
    # or index slip in the formulas would be metres per second off
    dv = np.abs(ns_ref[:, 3:6] - p["truth"]["kf_vel"][:n_kf]).max()
    print("velocity error against the truth: %.3g m/s" % dv)
    assert dv < 0.15


def test_shim_try_init_vio_throws_without_a_device(tmp_path):
    """tests/cpp/shim_vi_init_test.cpp compiles against viorb_amd/shim/LocalMapping_shim.h with its stand-in types and links the library;
    without a device viorb_shim::try_init_vio throws with the library's error text (on the GPU the program's output is compared with the
    Python path by tests/test_gpu_vi_init_shim.py)."""
    import test_gpu_vi_init_shim as sh
    have = viorb_amd.lib().viorb_device_count() > 0
    p = make_vi_init_problem(41, 8)
    own = vr.preintegrations(p, 8)
    fin, fout = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    sh.write_problem(fin, p, 6, 8, sh.tcw_of(p), own, np.ones((5, 3), np.float32), np.ones(5, np.float32), np.ones(5, np.float32))
    import subprocess
    out = subprocess.run([sh.build_vi_init_shim_test(tmp_path), fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK status 0" if have else "OK no device"), out.stdout + out.stderr
