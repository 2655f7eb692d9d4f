"""-m gpu: visual-inertial initialisation on the device (viorb_amd/csrc/vi_init.hip) against the numpy restatement tests/vi_init_ref.py
and the CPU oracle's pre-integration.

Tolerances (vi_init_ref.py holds the constants; tests/test_vi_init_ref.py re-measures them on every run):
  pre-integration      what tests/test_gpu_frontend.py::test_imu_predict_matches_oracle grants the same quantity: dP dV dR J* atol 1e-12,
                       covariance rtol 1e-9 / atol 1e-18, dt 1e-14.
  DEV_F32[q]           the largest |float32 restatement - float64 restatement| over the 36 parameter sets, i.e. the reference's own
                       rounding band: s* 2.5e-7, gw* 2.7e-7 (relative norm), s 2.4e-7, dtheta 3.0e-7 rad, ba 2.9e-6 m/s^2, singular values
                       9.3e-8 (A) and 2.0e-7 (C), written rounded up as 3e-7, 3e-7, 3e-7, 4e-7, 3e-6, 1e-7, 2.5e-7.
  device vs f64 mode   4 x DEV_F32[q], the margin the mapping tests use for another correct algorithm with the same order of backward
                       error (here: Gram matrix + Jacobi in double against LAPACK's SVD). Each test prints the deviation it saw.
  gyro bias            4 x DEV_F64_BG (double against longdouble with the edges summed in reverse: 1.85e-17, written 2e-17), with the
                       floor of 1e-12 the project grants double state.
  Rwi, Rwi_, gw        recomputed by the checker from the DEVICE's own gw* and dtheta (so the estimate's tolerance is not counted
                       twice): atol 1e-11, what test_imu_predict_matches_oracle grants a predicted NavState.
  NavStates            viorb_vi_init_apply_device against vi_init_ref.apply fed the DEVICE's own estimate: atol 1e-11 on double state (measured
                       1.8e-15 on the MI355X); scaled poses and map points bit-exact against numpy.float32 products by (float)s; the final
                       pre-integrations with the tolerances of the first line.
  status, counts       exactly.
Measured on the MI355X against the f64 restatement, largest over all tests: s* 1.7e-15, gw* 1.3e-15, s 2.2e-14, dtheta 1.9e-13 rad,
ba 1.6e-12 m/s^2, singular values 5.9e-16 / 3.3e-13, gyro bias 2.9e-16 rad/s."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi
from viorb_amd.synth import make_vi_init_problem
from viorb_amd.vi_init import unpack_est
import vi_init_ref as vr

pytestmark = pytest.mark.gpu

TOL = {k: 4 * v for k, v in vr.DEV_F32.items()}
TOL_BG = max(4 * vr.DEV_F64_BG, 1e-12)


def need_gpu():
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")


def cfg_of(p):
    return dict(Tbc=p["Tbc"], g=p["g"])


def check_preint(got, want, what=""):
    np.testing.assert_allclose(got[:60], want[:60], rtol=0, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(got[60:141], want[60:141], rtol=1e-9, atol=1e-18, err_msg=what)
    assert abs(got[141] - want[141]) < 1e-14, what


RESET = np.zeros(142); RESET[[6, 10, 14]] = 1.0


def check_est(est, ref, p, seen):
    """One OK stream of the device against the f64 restatement; `seen` collects the largest deviation per quantity."""
    e = unpack_est(est)
    d = vr.deviations(dict(sstar=e["sstar"], gwstar=e["gwstar"], s=e["s"], dtheta=e["dtheta"], ba=e["ba"], w=e["w"], w2=e["w2"]), ref)
    d["bg"] = float(np.abs(e["bg"] - ref["bg"]).max())
    for k, v in d.items():
        seen[k] = max(seen.get(k, 0.0), v)
        assert v <= (TOL_BG if k == "bg" else TOL[k]), (k, v)
    Rwi = vr.rwi_from_gravity(e["gwstar"], np.float64)
    Rwi_ = Rwi @ vr.ob.so3_matrix(vr.ob.so3_exp(np.array([e["dtheta"][0], e["dtheta"][1], 0.0])))
    np.testing.assert_allclose(e["Rwi"], Rwi, rtol=0, atol=1e-11)
    np.testing.assert_allclose(e["Rwi_"], Rwi_, rtol=0, atol=1e-11)
    np.testing.assert_allclose(e["gw"], Rwi_ @ np.array([0, 0, p["g"]]), rtol=0, atol=1e-11)
    assert (est[44:] == 0).all()


def ragged_interval_streams():
    """Three streams whose intervals hold 1, 2, 49, 50 and 200 samples, an empty one, and one whose first stamp precedes the previous key
    frame (the clamp case); unequal key-frame counts."""
    rng = np.random.default_rng(11)
    def stream(counts, early_first=()):
        t, imu, start = [0.0], [], [0, 0]
        for i, n in enumerate(counts, 1):
            T = 0.005 * max(n, 1) + 0.002
            ts = t[-1] + 0.001 + 0.005 * np.arange(n)
            if i in early_first:
                ts[0] = t[-1] - 0.003
            S = np.zeros((n, 7)); S[:, :3] = rng.normal(size=(n, 3)) * 0.3; S[:, 3:6] = rng.normal(size=(n, 3)) * 2 + [0.3, 9.7, -0.5]; S[:, 6] = ts
            imu.append(S); t.append(t[-1] + T); start.append(start[-1] + n)
        return dict(kf_time=np.array(t), imu=np.concatenate(imu), imu_start=np.array(start, np.int32))
    return [stream([1, 2, 49, 50, 200, 0, 7]), stream([50, 3, 50], early_first=(2,)), stream([9])]


@pytest.mark.parametrize("with_ba", [False, True])
def test_interval_preintegration_matches_oracle(with_ba):
    need_gpu()
    ss = ragged_interval_streams()
    rng = np.random.default_rng(5)
    bg = rng.normal(size=(3, 3)) * 0.02
    ba = rng.normal(size=(3, 3)) * 0.1 if with_ba else None
    for clamp in (True, False):
        got = viorb_amd.PreintegrateIntervalsBatch(ss, bg=bg, ba=ba, clamp=clamp)
        assert got.shape == (3, 8, 142)
        for b, s in enumerate(ss):
            n = len(s["kf_time"])
            for i in range(got.shape[1]):
                S = s["imu"][s["imu_start"][i]:s["imu_start"][i + 1]] if 1 <= i < n else np.zeros((0, 7))
                if len(S) == 0:
                    assert (got[b, i] == RESET).all(), (b, i)
                    continue
                if b == 1 and i == 2 and not clamp:
                    want = vr.ob.preintegrate(S, bg[b], ba[b] if with_ba else np.zeros(3), s["kf_time"][i - 1], s["kf_time"][i])     # a negative first dt, as KeyFrame::ComputePreInt takes it
                else:
                    want = vr.interval(S, bg[b], ba[b] if with_ba else np.zeros(3), s["kf_time"][i - 1], s["kf_time"][i], clamp)
                check_preint(got[b, i], want, "stream %d interval %d clamp %s" % (b, i, clamp))
    # the clamp case differs from the unclamped integration (the flag does something)
    a = viorb_amd.PreintegrateIntervalsBatch(ss[1:2], clamp=True)[0, 2]; c = viorb_amd.PreintegrateIntervalsBatch(ss[1:2], clamp=False)[0, 2]
    assert abs(a[141] - c[141]) > 2e-3
    # host form = device form, bit for bit
    h = viorb_amd.PreintegrateIntervals(ss[0], bg=bg[0], ba=ba[0] if with_ba else None)
    assert (h == viorb_amd.PreintegrateIntervalsBatch(ss[:1], bg=bg[:1], ba=ba[:1] if with_ba else None)[0]).all()
    # offsets that point outside the pool are treated as empty intervals, never read
    bad = dict(ss[2]); bad["imu_start"] = np.array([0, 0, 10 ** 6], np.int32)
    p = viorb_amd.vi_init.pack_streams([bad]); p["total_imu"] = 9
    assert (viorb_amd.PreintegrateIntervalsBatch(None, packed=p)[0, 1] == RESET).all()


def test_initial_gyro_bias_alone_20_frames():
    """viorb_optimize_initial_gyro_bias(_device) as Tracking.cc:67 uses it: 20 frames after a relocalisation."""
    need_gpu()
    seen = 0.0
    for seed in (0, 1, 2):
        p = make_vi_init_problem(seed, 20, kf_dt=0.05)
        pre = vr.preintegrations(p, 20)
        want = vr.gyro_bias(p, pre, 20)
        bg_d, st_d = viorb_amd.OptimizeInitialGyroBias(cfg_of(p), p["twc12"], pre, device=True)
        bg_h, st_h = viorb_amd.OptimizeInitialGyroBias(cfg_of(p), p["twc12"], pre)
        assert st_d == 0 and st_h == 0 and (bg_d == bg_h).all()
        seen = max(seen, np.abs(bg_d - want).max())
        assert np.abs(bg_d - want).max() <= TOL_BG
        assert np.abs(bg_d - p["truth"]["bg"]).max() < 1e-5
    print("gyro bias alone: largest deviation from the f64 restatement %.3g (granted %.3g)" % (seen, TOL_BG))
    _, st = viorb_amd.OptimizeInitialGyroBias(cfg_of(p), p["twc12"][:1], pre[:1], device=True)
    assert st == capi.VI_INVALID


def test_estimate_on_the_parameter_sets_batch_1():
    need_gpu()
    seen = {}
    for ps in vr.PARAMETER_SETS:
        p = make_vi_init_problem(ps[0], ps[1], kf_dt=ps[2], noise=ps[3])
        ref = vr.vi_init(p, mode="f64")
        est, st, pb = viorb_amd.ViInit(cfg_of(p), [p])().results()
        assert st[0] == 0 == ref["status"]
        check_est(est[0], ref, p, seen)
        want = vr.preintegrations(p, ps[1], unpack_est(est[0])["bg"])          # the re-integration, with the DEVICE's own gyro bias
        for i in range(ps[1]):
            check_preint(pb[0, i], want[i], "set %s key frame %d" % (ps, i))
    print("device against the f64 restatement, largest deviations:", {k: "%.2e" % v for k, v in seen.items()}, "granted:", TOL, TOL_BG)


def test_estimate_ragged_batch_of_7():
    need_gpu()
    spec = [(0, 12, 12), (1, 40, 30), (2, 20, 20), (3, 80, 64), (4, 5, 4), (5, 33, 33), (6, 96, 96)]      # (seed, key frames, n_est): n_est < n_kf twice
    Tbc = make_vi_init_problem(0, 4)["Tbc"]                   # one configuration per call
    ps = [make_vi_init_problem(s, n, kf_dt=0.25 if s % 2 else 0.4, Tbc=Tbc) for s, n, _ in spec]
    cfg = cfg_of(ps[0])
    n_est = [e for _, _, e in spec]
    est, st, pb = viorb_amd.ViInit(cfg, ps, n_est=n_est)().results()
    seen = {}
    for b, p in enumerate(ps):
        ref = vr.vi_init(p, n_est=n_est[b], mode="f64")
        assert st[b] == ref["status"] == 0, (b, st[b])
        check_est(est[b], ref, p, seen)
        assert (pb[b, n_est[b]:] == RESET).all()
        alone = viorb_amd.ViInit(cfg, [p], n_est=[n_est[b]])().results()
        assert (alone[0][0] == est[b]).all() and (alone[2][0] == pb[b, :n_est[b]]).all()
    print("ragged batch of 7, largest deviations:", {k: "%.2e" % v for k, v in seen.items()})


def test_status_paths_in_one_mixed_batch():
    """N = 3, an empty interval and a motionless stream between healthy streams: statuses exact, outputs of the failed streams zero, the
    healthy ones equal to the same streams run alone, bit for bit. The failing inputs are well-formed arrays."""
    need_gpu()
    base = make_vi_init_problem(4, 16)
    Tbc = base["Tbc"]
    h1, h2, h3 = [make_vi_init_problem(s, n, Tbc=Tbc) for s, n in ((7, 16), (8, 24), (9, 12))]
    short = make_vi_init_problem(10, 3, Tbc=Tbc)
    hole = make_vi_init_problem(11, 14, Tbc=Tbc)
    w = hole["imu_start"][6] - hole["imu_start"][5]
    hole["imu_start"] = hole["imu_start"].copy(); hole["imu_start"][6:] -= w; hole["imu"] = np.delete(hole["imu"], np.s_[hole["imu_start"][5]:hole["imu_start"][5] + w], axis=0)
    still = vr.motionless(16)
    batch = [h1, short, h2, hole, still, h3]
    est, st, pb = viorb_amd.ViInit(cfg_of(base), batch)().results()
    assert list(st) == [0, capi.VI_INVALID, 0, capi.VI_INVALID, capi.VI_DEGENERATE, 0], list(st)
    assert [vr.vi_init(p)["status"] for p in batch] == list(st)
    for b in (1, 3, 4):
        assert (est[b] == 0).all()
    for b in (0, 2, 5):
        a = viorb_amd.ViInit(cfg_of(base), [batch[b]])().results()
        assert a[1][0] == 0 and (a[0][0] == est[b]).all()
        check_est(est[b], vr.vi_init(batch[b]), batch[b], {})


def test_1024_streams_of_up_to_96_key_frames():
    need_gpu()
    Ns = [96, 60, 12, 80, 33, 20, 47, 64]
    base = make_vi_init_problem(0, 4)
    distinct = [make_vi_init_problem(20 + k, n, Tbc=base["Tbc"]) for k, n in enumerate(Ns)]
    run = viorb_amd.ViInit(cfg_of(base), distinct * 128, max_kf=96)
    est, st, pb = run().results()
    assert est.shape == (1024, 48) and (st == 0).all()
    for k in range(8):
        assert (est[k::8] == est[k]).all() and (pb[k::8] == pb[k]).all()
        check_est(est[k], vr.vi_init(distinct[k]), distinct[k], {})
    # determinism: the same call again gives identical bytes
    est2, st2, pb2 = run().results()
    assert est2.tobytes() == est.tobytes() and pb2.tobytes() == pb.tobytes() and (st2 == st).all()


def test_host_form_equals_device_form():
    need_gpu()
    p = make_vi_init_problem(3, 30)
    pre0 = viorb_amd.PreintegrateIntervals(p)
    est_h, st_h, pb_h = viorb_amd.ViInitHost(cfg_of(p), p, pre0)
    est_d, st_d, pb_d = viorb_amd.ViInit(cfg_of(p), [p], preint_in=pre0[None])().results()
    assert st_h == st_d[0] == 0 and est_h.tobytes() == est_d[0].tobytes() and pb_h.tobytes() == pb_d[0].tobytes()
    # n_est smaller than the stream
    est_h, st_h, pb_h = viorb_amd.ViInitHost(cfg_of(p), p, pre0, n_est=17)
    est_d, st_d, pb_d = viorb_amd.ViInit(cfg_of(p), [p], n_est=[17], preint_in=pre0[None, :17])().results()
    assert st_h == 0 and est_h.tobytes() == est_d[0].tobytes() and pb_h.tobytes() == pb_d[0].tobytes()


def tcw_of(p):
    """Tcw = Rcw(9) tcw(3) as float, from the float Twc the streams carry (inverted in double, rounded once)."""
    T = np.asarray(p["twc12"], np.float64)
    out = np.zeros((len(T), 12), np.float32)
    for i, t in enumerate(T):
        R = t[:9].reshape(3, 3)
        out[i, :9] = R.T.ravel(); out[i, 9:] = -R.T @ t[9:]
    return out


def test_apply_navstates_poses_points_and_final_preintegrations():
    """NavStates (forward, newest-of-set and trailing velocities) against the checker fed the DEVICE's own estimate: atol 1e-11; scaled poses
    and map points bit-exact against numpy.float32 arithmetic on the same (float)s; final pre-integrations with the tolerances of the
    interval test; a stream whose estimate failed is left untouched."""
    need_gpu()
    Tbc = make_vi_init_problem(0, 4)["Tbc"]
    spec = [(31, 20, 20), (32, 30, 24), (33, 16, 15), (34, 3, 3), (35, 40, 33)]       # (seed, n_kf, n_est); stream 3 is INVALID
    ps = [make_vi_init_problem(s, n, Tbc=Tbc) for s, n, _ in spec]
    n_kf, n_est = [n for _, n, _ in spec], [e for _, _, e in spec]
    cfg = cfg_of(ps[0])
    run = viorb_amd.ViInit(cfg, ps, n_est=n_est, max_kf=40)()
    rng = np.random.default_rng(3)
    npts = 1001                                                # rows of 3003 floats: not a multiple of four, rows start unaligned
    pts = rng.normal(size=(5, npts, 3)).astype(np.float32) * 5; dmin = rng.uniform(0.5, 2, (5, npts)).astype(np.float32); dmax = dmin * 7
    pose = np.zeros((5, 40, 12), np.float32)
    for b, p in enumerate(ps):
        pose[b, :n_kf[b]] = tcw_of(p)
    got = run.apply(ps, pose, n_kf=n_kf, points=pts, min_dist=dmin, max_dist=dmax)()
    est, st, pbg = run.results()
    assert list(st) == [0, 0, 0, capi.VI_INVALID, 0]
    worst = 0.0
    for b, p in enumerate(ps):
        if st[b] != 0:
            assert np.isnan(got["navstate"][b]).all() and np.isnan(got["preint"][b]).all() and np.isnan(got["pose12_scaled"][b]).all()
            assert (got["points"][b] == pts[b]).all() and (got["min_dist"][b] == dmin[b]).all() and (got["max_dist"][b] == dmax[b]).all()
            continue
        e = unpack_est(est[b])
        ns_ref, fin = vr.apply(p, e, n_est[b], n_kf[b], pbg[b])
        ns = got["navstate"][b, :n_kf[b]].copy()
        flip = np.sum(ns[:, 6:10] * ns_ref[:, 6:10], axis=1) < 0
        ns[flip, 6:10] *= -1
        worst = max(worst, np.abs(ns - ns_ref).max())
        np.testing.assert_allclose(ns, ns_ref, rtol=0, atol=1e-11, err_msg="stream %d" % b)
        assert np.isnan(got["navstate"][b, n_kf[b]:]).all()
        for i in range(n_kf[b]):
            check_preint(got["preint"][b, i], fin[i], "final, stream %d key frame %d" % (b, i))
        sf = np.float32(e["s"])
        assert (got["pose12_scaled"][b, :n_kf[b], :9] == pose[b, :n_kf[b], :9]).all()
        assert (got["pose12_scaled"][b, :n_kf[b], 9:] == pose[b, :n_kf[b], 9:] * sf).all()
        assert (got["points"][b] == pts[b] * sf).all() and (got["min_dist"][b] == dmin[b] * sf).all() and (got["max_dist"][b] == dmax[b] * sf).all()
        # host form = device form, bit for bit
        h = viorb_amd.ViInitApplyHost(cfg, p, pose[b], est[b], pbg[b], n_est[b], n_kf[b])
        assert h[0].tobytes() == got["navstate"][b, :n_kf[b]].tobytes() and h[1].tobytes() == got["pose12_scaled"][b, :n_kf[b]].tobytes()
        assert h[2].tobytes() == got["preint"][b, :n_kf[b]].tobytes()
    print("apply: largest NavState deviation from the checker %.3g (granted 1e-11)" % worst)
