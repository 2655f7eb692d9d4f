"""GPU parity of Optimizer::BundleAdjustment (viorb_global_ba_se3, csrc/global_ba_se3.hip) against the numpy checker
tests/global_ba_se3_ref.py, compared as tests/test_gpu_global_ba.py compares the NavState solve: the same accept / reject sequence and
iteration count, chi2 before and after within 1e-5 relative (the project's stated tolerance), final lambda within 1e-6, the same
point_included, key-frame rows and points within a band measured on the checker itself.

The band. The device sums a Schur block's terms in an order that is not fixed, so the yardstick is how far the CHECKER moves when its own
reduced solve is done two ways: Schur sums in edge order + Cholesky, and sums in reverse edge order + numpy.linalg.solve. The device is
granted four times that distance, but never less than the window tests' 1e-7 (key-frame rows) / 1e-6 (points). Every test prints the
band of the case it runs."""
import functools
import os
import sys
import threading
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ba_se3_ref as G
import global_ba_se3_cases as GC

pytestmark = pytest.mark.gpu
KF_FLOOR, PT_FLOOR = 1e-7, 1e-6


@functools.lru_cache(maxsize=None)
def _reference_of(name):
    q, robust, iterations = {n: (q, r, i) for n, q, r, i in GC.checked_variants()}[name]
    return (q, robust, iterations) + _band(q, robust, iterations, name)


def _band(p, robust, iterations, label):
    """the checker's result and the band of the case: (result, 4 x band of the key-frame rows floored, 4 x band of the points floored)"""
    a = G.global_ba_se3(*GC.args(p), iterations=iterations, robust=bool(robust))
    b = G.global_ba_se3(*GC.args(p), iterations=iterations, robust=bool(robust), linear="solve", reverse=True)
    assert [t[4] for t in a["trials"]] == [t[4] for t in b["trials"]]
    dk, dp = np.abs(a["kfs"] - b["kfs"]).max(), np.abs(a["points"] - b["points"]).max()
    print("checker band: %s: key frames %.3g points %.3g" % (label, dk, dp))
    return a, max(4 * dk, KF_FLOOR), max(4 * dp, PT_FLOOR)


@functools.lru_cache(maxsize=None)
def _reference(seed, N, robust, stereo, revisit):
    return _band(GC.problem(seed, N, stereo, revisit), robust, GC.ITERATIONS, "seed %d N %d robust %d stereo %.1f revisit %.1f" % (seed, N, robust, stereo, revisit))


def _solve(p, **kw):
    from viorb_amd import GlobalBundleAdjustmentSE3
    return GlobalBundleAdjustmentSE3(*GC.args(p), **kw)


def _compare(got, ref, kf_tol, pt_tol):
    print("device: chi2 %.10g -> %.10g, %d iterations, %d trials, %d failed | checker: %.10g -> %.10g, %d, %d" %
          (got["chi2_before"], got["chi2_after"], got["iterations"], got["trials"], got["failed_factorisations"], ref["info"][0], ref["info"][1], ref["its"], len(ref["trials"])))
    print("max |d key frames| %.3g (granted %.3g)  max |d points| %.3g (granted %.3g)" % (np.abs(got["kfs"] - ref["kfs"]).max(), kf_tol,
                                                                                      np.abs(got["points"] - ref["points"]).max() if len(ref["points"]) else 0.0, pt_tol))
    assert got["iterations"] == ref["its"] and got["trials"] == len(ref["trials"])
    assert got["failed_factorisations"] == sum(1 for t in ref["trials"] if not t[2])
    assert abs(got["chi2_before"] - ref["info"][0]) <= 1e-5 * ref["info"][0]
    assert abs(got["chi2_after"] - ref["info"][1]) <= 1e-5 * ref["info"][1]
    assert got["accepted"] == [bool(t[4]) for t in ref["trials"]]             # the accept / reject sequence, trial by trial (viorb_debug_gba_last_trials)
    assert abs(got["final_lambda"] - ref["info"][4]) <= 1e-6 * ref["info"][4]
    assert np.array_equal(got["point_included"], ref["point_included"])
    np.testing.assert_allclose(got["kfs"], ref["kfs"], rtol=0, atol=kf_tol)
    np.testing.assert_allclose(got["points"], ref["points"], rtol=0, atol=pt_tol)


@pytest.mark.parametrize("seed,N,robust,stereo,revisit", GC.CASES)
def test_global_ba_se3_matches_checker(seed, N, robust, stereo, revisit):
    p = GC.problem(seed, N, stereo, revisit)
    ref, kf_tol, pt_tol = _reference(seed, N, robust, stereo, revisit)
    _compare(_solve(p, iterations=GC.ITERATIONS, robust=robust), ref, kf_tol, pt_tol)


def test_ten_iterations_not_robust_as_the_loop_closer_calls_it():
    q, robust, iterations, ref, kf_tol, pt_tol = _reference_of("loop-closer")
    assert (robust, iterations) == (0, 10)
    _compare(_solve(q, iterations=iterations, robust=robust), ref, kf_tol, pt_tol)


def test_twenty_robust_iterations_as_the_monocular_initialiser_calls_it():
    q, robust, iterations, ref, kf_tol, pt_tol = _reference_of("initial-map")
    assert (robust, iterations) == (1, 20) and not (q["edge_obs"][:, 2] >= 0).any() and len(q["kfs"]) == 2
    _compare(_solve(q, iterations=iterations, robust=robust), ref, kf_tol, pt_tol)


# the device form on six cases of the cross (revisit 0.2): robust 0 / 1 with stereo 0 / 0.5 / 1, alternating between N = 43 and N = 12
DEVICE_FORM_CASES = {25: (43, 0, 0.0), 15: (12, 0, 0.5), 29: (43, 0, 1.0), 19: (12, 1, 0.0), 33: (43, 1, 0.5), 23: (12, 1, 1.0)}


@pytest.mark.parametrize("index", sorted(DEVICE_FORM_CASES))
def test_device_form_equals_host_form(index):
    from viorb_amd import GlobalBundleAdjustmentSE3Device
    seed, N, robust, stereo, revisit = GC.CASES[index]
    assert (N, robust, stereo) == DEVICE_FORM_CASES[index] and revisit == 0.2
    p = GC.problem(seed, N, stereo, revisit)
    ref, kf_tol, pt_tol = _reference(seed, N, robust, stereo, revisit)
    _compare(GlobalBundleAdjustmentSE3Device(*GC.args(p), iterations=GC.ITERATIONS, robust=robust), ref, kf_tol, pt_tol)


def test_run_to_run_agreement():
    seed, N, robust, stereo, revisit = GC.CASES[29]
    p = GC.problem(seed, N, stereo, revisit)
    _, kf_tol, pt_tol = _reference(seed, N, robust, stereo, revisit)
    a, b = _solve(p, robust=robust), _solve(p, robust=robust)
    assert (a["iterations"], a["trials"]) == (b["iterations"], b["trials"])
    print("run to run: key frames %.3g points %.3g" % (np.abs(a["kfs"] - b["kfs"]).max(), np.abs(a["points"] - b["points"]).max()))
    np.testing.assert_allclose(a["kfs"], b["kfs"], rtol=0, atol=kf_tol)
    np.testing.assert_allclose(a["points"], b["points"], rtol=0, atol=pt_tol)
    assert abs(a["chi2_after"] - b["chi2_after"]) <= 1e-9 * b["chi2_after"]


def test_four_threads_each_get_their_solo_result():
    probs = [GC.problem(seed, N) for seed, N in GC.THREAD_SEEDS]
    solo = [_solve(p, robust=True) for p in probs]
    out = [None] * 4

    def work(i):
        out[i] = _solve(probs[i], robust=True)
    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in th]; [t.join() for t in th]
    for g, r in zip(out, solo):
        assert g is not None and (g["iterations"], g["trials"], g["accepted"]) == (r["iterations"], r["trials"], r["accepted"])
        np.testing.assert_allclose(g["kfs"], r["kfs"], rtol=0, atol=KF_FLOOR)
        np.testing.assert_allclose(g["points"], r["points"], rtol=0, atol=PT_FLOOR)
        assert abs(g["chi2_after"] - r["chi2_after"]) <= 1e-9 * r["chi2_after"]


def test_stop_flag_raised_before_the_call():
    p = GC.problem(*GC.STOP_SEED)
    q = dict(p, points=np.vstack([p["points"], [[1.0, 2.0, 30.0]]]))
    from viorb_amd import GlobalBundleAdjustmentSE3Device
    for fn in (_solve, lambda q, **kw: GlobalBundleAdjustmentSE3Device(*GC.args(q), **kw)):
        g = fn(q, stop=np.ones(1, np.int32))
        assert g["iterations"] == 0 and np.array_equal(g["kfs"], q["kfs"]) and np.array_equal(g["points"], q["points"])
        assert g["point_included"][:-1].all() and g["point_included"][-1] == 0 and g["accepted"] == []


def test_stop_flag_raised_mid_solve():
    seed, N, robust, stereo, revisit = GC.CASES[36]
    assert N == 130
    p = GC.problem(seed, N, stereo, revisit)
    full = _solve(p, iterations=GC.ITERATIONS)
    stop = np.zeros(1, np.int32)
    t = threading.Timer(0.004, lambda: stop.__setitem__(0, 1))
    t.start()
    g = _solve(p, iterations=GC.ITERATIONS, stop=stop)
    t.join()
    print("stopped after %d of %d iterations" % (g["iterations"], full["iterations"]))
    assert g["iterations"] <= full["iterations"]
    assert np.isfinite(g["kfs"]).all() and np.isfinite(g["points"]).all() and np.isfinite(g["info"]).all()
    assert g["chi2_after"] <= g["chi2_before"]


@pytest.mark.parametrize("robust", [0, 1])
def test_degenerate_points(robust):
    """no edge, a single monocular edge, a single stereo edge, one monocular + one stereo edge, seen only by fixed key frames"""
    q, r, iterations, ref, kf_tol, pt_tol = _reference_of("degenerate-%d" % robust)
    ei, eo = q["edge_idx"], q["edge_obs"]
    assert [int((ei[:, 0] == pid).sum()) for pid in (5, 6, 7, 8, 9)] == [1, 1, 2, 2, 0]
    assert eo[ei[:, 0] == 5][0, 2] < 0 and eo[ei[:, 0] == 6][0, 2] >= 0 and sorted(eo[ei[:, 0] == 7][:, 2] >= 0) == [False, True]
    assert q["fixed"][ei[ei[:, 0] == 8][:, 1]].all()
    got = _solve(q, iterations=iterations, robust=r)
    _compare(got, ref, kf_tol, pt_tol)
    assert got["point_included"][9] == 0 and got["point_included"][-1] == 0 and got["point_included"][5:9].all()
    assert np.array_equal(got["points"][9], q["points"][9]) and np.array_equal(got["points"][-1], q["points"][-1])
    assert not np.array_equal(got["points"][8], q["points"][8])            # a vertex although only fixed key frames see it: it moves
    assert np.array_equal(got["kfs"][q["fixed"] != 0], q["kfs"][q["fixed"] != 0])


def test_fixed_key_frames_inside_the_graph():
    q, robust, iterations, ref, kf_tol, pt_tol = _reference_of("fixed-inside")
    got = _solve(q, iterations=iterations, robust=robust)
    _compare(got, ref, kf_tol, pt_tol)
    assert q["fixed"].sum() == 3 and np.array_equal(got["kfs"][q["fixed"] != 0], q["kfs"][q["fixed"] != 0])


def test_no_fixed_key_frame_at_all():
    q, robust, iterations, ref, kf_tol, pt_tol = _reference_of("no-fixed")
    assert not q["fixed"].any()
    _compare(_solve(q, iterations=iterations, robust=robust), ref, kf_tol, pt_tol)


def test_over_the_limit_is_refused():
    from viorb_amd import ViorbError, capi, GlobalBundleAdjustmentSE3
    p = GC.problem(*GC.STOP_SEED)
    nk = 4097
    with pytest.raises(ViorbError) as e:
        GlobalBundleAdjustmentSE3(np.tile(p["kfs"][:1], (nk, 1)), np.zeros(nk, np.uint8), np.zeros((0, 3)), np.zeros((0, 2), np.int32), np.zeros((0, 4)), p["intr5"])
    assert e.value.code == capi.ERR_CAPACITY


def test_a_stereo_edge_without_a_baseline_is_refused():
    from viorb_amd import ViorbError, capi, GlobalBundleAdjustmentSE3, GlobalBundleAdjustmentSE3Device
    p = GC.problem(*GC.STOP_SEED)
    assert (p["edge_obs"][:, 2] >= 0).any()
    intr = p["intr5"].copy(); intr[4] = 0.0
    for fn in (GlobalBundleAdjustmentSE3, GlobalBundleAdjustmentSE3Device):
        with pytest.raises(ViorbError) as e:
            fn(p["kfs"], p["fixed"], p["points"], p["edge_idx"], p["edge_obs"], intr)
        assert e.value.code == capi.ERR_INVALID_ARG
