"""GPU parity of Optimizer::GlobalBundleAdjustmentNavState (viorb_global_ba_navstate, csrc/global_ba.hip) against the numpy checker
tests/global_ba_ref.py: the same accept / reject sequence and iteration count, chi2 before and after within 1e-5 relative (the project's
stated tolerance), the same point_included, key-frame states and points within a band measured on the checker itself.

The band. The device sums a Schur block's terms in an order that is not fixed, so the yardstick is how far the CHECKER moves when its
own reduced solve is done two ways: Schur sums in edge order + Cholesky, and sums in reverse edge order + numpy.linalg.solve. The device
is granted four times that distance, but never less than the window tests' 1e-7 (key-frame states) / 1e-6 (points). Measured on the
checker for the 20 cases below (max over a case's key frames / points of the absolute difference):
    N = 3      states 3e-16 .. 2e-15    points 3e-12 .. 4e-11
    N = 21     states 2e-15 .. 2e-14    points 9e-12 .. 4e-10
    N = 60     states 6e-14 .. 4e-13    points 4e-11 .. 1e-10
    N = 128    states 1e-14 .. 4e-12    points 4e-11 .. 2e-10
    N = 256    states 4e-13 .. 4e-12    points 2e-11 .. 2e-10
Four times the largest of them is far below the floor, so 1e-7 / 1e-6 is what the assertions below apply at every size; the test still
measures the band of each case it runs and prints it, and would widen the grant by itself if a case's band outgrew the floor."""
import ctypes as C
import functools
import os
import sys
import threading
import time
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ba_ref as G
import global_ba_cases as GC
from viorb_amd.synth import make_global_ba_problem

pytestmark = pytest.mark.gpu
KF_FLOOR, PT_FLOOR = 1e-7, 1e-6


@functools.lru_cache(maxsize=None)
def _problem(seed, N, revisit=0.0):
    return make_global_ba_problem(seed, N, revisit_frac=revisit)           # pre-integrations from viorb_preintegrate_intervals


@functools.lru_cache(maxsize=None)
def _reference(seed, N, robust, revisit, iterations=GC.ITERATIONS):
    """the checker's result and the band of the case: (result, 4 x band of the states floored, 4 x band of the points floored)"""
    p = _problem(seed, N, revisit)
    a = G.global_ba(*GC.args(p), iterations=iterations, robust=bool(robust))
    b = G.global_ba(*GC.args(p), iterations=iterations, robust=bool(robust), linear="solve", reverse=True)
    assert [t[4] for t in a["trials"]] == [t[4] for t in b["trials"]]
    dk, dp = np.abs(a["kfs"] - b["kfs"]).max(), np.abs(a["points"] - b["points"]).max()
    print("checker band: seed %d N %d robust %d revisit %.1f: states %.3g points %.3g" % (seed, N, robust, revisit, dk, dp))
    return a, max(4 * dk, KF_FLOOR), max(4 * dp, PT_FLOOR)


def _solve(p, **kw):
    from viorb_amd import GlobalBundleAdjustmentNavState
    return GlobalBundleAdjustmentNavState(*GC.args(p), **kw)


def _compare(got, ref, kf_tol, pt_tol):
    print("device: chi2 %.10g -> %.10g, %d iterations, %d trials, %d failed | checker: %.10g -> %.10g, %d, %d" %
          (got["chi2_before"], got["chi2_after"], got["iterations"], got["trials"], got["failed_factorisations"], ref["info"][0], ref["info"][1], ref["its"], len(ref["trials"])))
    print("max |d states| %.3g (granted %.3g)  max |d points| %.3g (granted %.3g)" % (np.abs(got["kfs"] - ref["kfs"]).max(), kf_tol,
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


@pytest.mark.parametrize("seed,N,robust,revisit", GC.CASES)
def test_global_ba_matches_checker(seed, N, robust, revisit):
    p = _problem(seed, N, revisit)
    ref, kf_tol, pt_tol = _reference(seed, N, robust, revisit)
    _compare(_solve(p, iterations=GC.ITERATIONS, robust=robust), ref, kf_tol, pt_tol)


# the device form on four cases: every size up to N = 60, both robust flags, both revisit fractions
DEVICE_FORM_CASES = {1: (3, 0, 0.2), 7: (21, 1, 0.2), 8: (60, 0, 0.0), 11: (60, 1, 0.2)}


@pytest.mark.parametrize("index", sorted(DEVICE_FORM_CASES))
def test_device_form_equals_host_form(index):
    from viorb_amd import GlobalBundleAdjustmentNavStateDevice
    seed, N, robust, revisit = GC.CASES[index]
    assert (N, robust, revisit) == DEVICE_FORM_CASES[index]
    p = _problem(seed, N, revisit)
    ref, kf_tol, pt_tol = _reference(seed, N, robust, revisit)
    _compare(GlobalBundleAdjustmentNavStateDevice(*GC.args(p), iterations=GC.ITERATIONS, robust=robust), ref, kf_tol, pt_tol)


def test_run_to_run_agreement():
    seed, N, robust, revisit = GC.CASES[11]
    p = _problem(seed, N, revisit)
    _, kf_tol, pt_tol = _reference(seed, N, robust, revisit)
    a, b = _solve(p, robust=robust), _solve(p, robust=robust)
    assert (a["iterations"], a["trials"]) == (b["iterations"], b["trials"])
    print("run to run: states %.3g points %.3g" % (np.abs(a["kfs"] - b["kfs"]).max(), np.abs(a["points"] - b["points"]).max()))
    np.testing.assert_allclose(a["kfs"], b["kfs"], rtol=0, atol=kf_tol)
    np.testing.assert_allclose(a["points"], b["points"], rtol=0, atol=pt_tol)
    assert abs(a["chi2_after"] - b["chi2_after"]) <= 1e-9 * b["chi2_after"]


def test_four_threads_each_get_their_solo_result():
    probs = [_problem(seed, N) for seed, N in GC.THREAD_SEEDS]
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
    p = _problem(*GC.STOP_SEED)
    g = _solve(p, stop=np.ones(1, np.int32))
    assert g["iterations"] == 0 and np.array_equal(g["kfs"], p["kfs"]) and np.array_equal(g["points"], p["points"])


def test_stop_flag_raised_mid_solve():
    seed, N, robust, revisit = GC.CASES[12]
    p = _problem(seed, N, revisit)
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


def test_points_with_no_edge_and_with_a_single_edge():
    p = _problem(*GC.DEGENERATE_SEED)
    q = GC.degenerate_points_variant(p)
    for robust in (0, 1):
        ref = G.global_ba(*GC.args(q), iterations=GC.ITERATIONS, robust=bool(robust))
        got = _solve(q, iterations=GC.ITERATIONS, robust=robust)
        _compare(got, ref, KF_FLOOR, PT_FLOOR)
        assert got["point_included"][9] == 0 and got["point_included"][-1] == 0 and got["point_included"][5] == 1
        assert np.array_equal(got["points"][9], q["points"][9]) and np.array_equal(got["points"][-1], q["points"][-1])


def test_fixed_key_frames_inside_the_graph():
    """fixed[] is general: two fixed key frames, one of them in the middle; an IMU factor whose both ends are fixed only adds to chi2."""
    q = GC.fixed_inside_variant(_problem(*GC.FIXED_SEED))
    ref = G.global_ba(*GC.args(q), iterations=GC.FIXED_ITERATIONS, robust=True)
    _compare(_solve(q, iterations=GC.FIXED_ITERATIONS, robust=1), ref, KF_FLOOR, PT_FLOOR)


def test_over_the_limit_is_refused():
    from viorb_amd import ViorbError, capi
    p = _problem(311, 21)
    nk = 2050
    with pytest.raises(ViorbError) as e:
        from viorb_amd import GlobalBundleAdjustmentNavState
        GlobalBundleAdjustmentNavState(np.tile(p["kfs"][:1], (nk, 1)), np.full(nk, -1, np.int32), np.zeros(nk, np.uint8), np.zeros((nk, 142)),
                                       np.zeros((0, 3)), np.zeros((0, 2), np.int32), np.zeros((0, 3)), p["gw"], p["cam"])
    assert e.value.code == capi.ERR_CAPACITY


# ---- the blocked Cholesky alone -------------------------------------------------------------------------------------------------------
def _spd(n, seed):
    r = np.random.default_rng(seed)
    B = r.standard_normal((n, min(n, 512)))
    A = B @ B.T
    A += np.diag(r.uniform(0.5, 2.0, n)) * (np.trace(A) / n)
    return (A + A.T) / 2


@pytest.mark.parametrize("n", [12, 240, 252, 3060, 6144])
def test_cholesky_residual(n):
    """||L L^T - A|| / ||A|| (Frobenius) of the device factor against numpy's on the same matrix: numpy's own residual is measured and the
    device is granted 8 x it (a small multiple of n eps either way)."""
    from viorb_amd.global_ba import debug_cholesky
    A = _spd(n, 40 + n)
    Ln = np.linalg.cholesky(A)
    L, ok = debug_cholesky(A)
    assert ok
    nA = np.linalg.norm(A)
    r_np, r_dev = np.linalg.norm(Ln @ Ln.T - A) / nA, np.linalg.norm(L @ L.T - A) / nA
    print("n %d: residual numpy %.3g device %.3g (n eps = %.3g); max |L - L_numpy| / max |L| %.3g" % (n, r_np, r_dev, n * np.finfo(float).eps, np.abs(L - Ln).max() / np.abs(Ln).max()))
    assert np.all(np.triu(L, 1) == 0)
    assert r_dev <= 8 * r_np


@pytest.mark.parametrize("n,where", [(12, 7), (252, 100), (252, 251), (3060, 2000)])
def test_cholesky_reports_a_bad_pivot(n, where):
    from viorb_amd.global_ba import debug_cholesky
    A = _spd(n, 90 + n)
    A[where, where] = -abs(A[where, where])          # not positive definite: the pivot at `where` (or an earlier one) is not positive
    L, ok = debug_cholesky(A)
    assert not ok and np.isfinite(L).all()
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A)
