"""The global and the local bundle adjustment draw their stream contexts (stream, device arena, page-locked scalars) from one pool of
the process (csrc/viorb_common.hip): a solve of one running beside a solve of the other gets what it gets alone."""
import os
import sys
import threading
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ba_cases as GC
from viorb_amd.synth import make_global_ba_problem, make_local_ba_problem

pytestmark = pytest.mark.gpu


def _local_args(oracle, p):
    pre = []
    for i, (imu, t0, t1) in enumerate(p["imu"]):
        j = i - 1 if i > 0 else p["prev_kf"]
        pre.append(oracle.preintegrate(imu, p["kfs"][j][10:13], p["kfs"][j][13:16], t0, t1))
    return (p["kfs"], p["n_local"], p["prev_kf"], np.stack(pre), p["points"], p["edge_idx"], p["edge_obs"], p["gw"], p["cam"])


def test_global_and_local_ba_side_by_side(oracle):
    """Two threads start together, one makes three global solves in a row, the other three local window solves; every result is
    compared with the same call made alone beforehand in this process.

    Neither solver is bit-reproducible from one solo run to the next: both sum their Schur terms with floating-point atomics, in an
    order that is not fixed (tests/test_gpu_global_ba.py, test_local_ba_batch_equals_single_calls). So each result is held to what the
    solver's own solo-versus-concurrent test grants: the global solve to test_four_threads_each_get_their_solo_result (same
    iterations, trials and accept sequence, states 1e-7, points 1e-6, chi2 1e-9 relative), the window solve to
    test_local_ba_batch_equals_single_calls (same iteration counts and erase flags, states and points 1e-9, chi2 1e-9 relative)."""
    from viorb_amd import GlobalBundleAdjustmentNavState, LocalBundleAdjustmentNavState
    ga = GC.args(make_global_ba_problem(301, N=12))
    la = _local_args(oracle, make_local_ba_problem(21, W=4, n_points=60))
    solve_g = lambda: GlobalBundleAdjustmentNavState(*ga, robust=True)
    solve_l = lambda: LocalBundleAdjustmentNavState(*la)
    solo_g, solo_l = solve_g(), solve_l()
    start = threading.Barrier(2)
    out = {"g": [], "l": []}

    def work(key, solve):
        start.wait()
        for _ in range(3):
            out[key].append(solve())
    th = [threading.Thread(target=work, args=("g", solve_g)), threading.Thread(target=work, args=("l", solve_l))]
    [t.start() for t in th]; [t.join() for t in th]
    assert len(out["g"]) == 3 and len(out["l"]) == 3
    for g in out["g"]:
        print("global: max |d states| %.3g  max |d points| %.3g" % (np.abs(g["kfs"] - solo_g["kfs"]).max(), np.abs(g["points"] - solo_g["points"]).max()))
        assert (g["iterations"], g["trials"], g["accepted"]) == (solo_g["iterations"], solo_g["trials"], solo_g["accepted"])
        assert np.array_equal(g["point_included"], solo_g["point_included"])
        np.testing.assert_allclose(g["kfs"], solo_g["kfs"], rtol=0, atol=1e-7)
        np.testing.assert_allclose(g["points"], solo_g["points"], rtol=0, atol=1e-6)
        assert abs(g["chi2_after"] - solo_g["chi2_after"]) <= 1e-9 * solo_g["chi2_after"]
    for g in out["l"]:
        print("local: max |d states| %.3g  max |d points| %.3g" % (np.abs(g["kfs"] - solo_l["kfs"]).max(), np.abs(g["points"] - solo_l["points"]).max()))
        assert (g["its_first"], g["its_second"]) == (solo_l["its_first"], solo_l["its_second"])
        np.testing.assert_array_equal(g["erase"], solo_l["erase"])
        np.testing.assert_allclose(g["kfs"], solo_l["kfs"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(g["points"], solo_l["points"], rtol=0, atol=1e-9)
        assert abs(g["chi2_final"] - solo_l["chi2_final"]) <= 1e-9 * solo_l["chi2_final"]
