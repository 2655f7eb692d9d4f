"""CPU tests of OptimizeSim3 (no GPU): the numpy checker of tests/sim3_ref.py against ground truth, its numeric-Jacobian mode (g2o's own)
against its analytic mode with the measurement of the tolerances the GPU tests use, the agreement of both modes on iteration counts and
accept / reject sequences for every case used on the GPU, the argument checks of the entries, and the host hooks viorb_debug_sim3_exp /
viorb_debug_sim3_edges (sim3_core.h compiled for the host) against the checker."""
import ctypes as C
import functools
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi, sim3
import sim3_ref as T

f64 = np.float64
ALL = T.OPT_CASES + T.OPT_CASES_FLOOR


@functools.lru_cache(maxsize=None)
def solved(i, mode):
    p, S0, valid, fix, th2 = T.opt_case(ALL[i])
    return T.optimize_sim3(p, S0, th2, fix, valid, mode)


def test_optimiser_lowers_the_cost_and_keeps_the_inliers():
    for i, c in enumerate(ALL):
        if c[2] < 60:
            continue
        p, S0, valid, fix, th2 = T.opt_case(c)
        r = solved(i, "numeric")
        ncorr, nbad, its1, its2, chi1, chi2 = r["info"][:6]
        assert ncorr == c[2] and 1 <= its1 <= 5 and 1 <= its2 <= (10 if nbad else 5)
        truth = (T.mat2q(np.asarray(p["R12"], f64)), np.asarray(p["t12"], f64), float(p["s12"]))
        S = T.sim3_unpack(r["S12"])
        assert np.abs(S[1] - truth[1]).max() < np.abs(T.sim3_unpack(S0)[1] - truth[1]).max() and (fix or abs(S[2] - truth[2]) < 0.01)        # closer than it started (one per cent off)
        assert not fix or S[2] == 1.0
        good = (valid != 0) & (p["true_inlier"] != 0)
        assert r["keep"][good].mean() > 0.97 and not r["keep"][valid == 0].any()
        wrong = (valid != 0) & (p["true_inlier"] == 0)
        assert not wrong.any() or r["keep"][wrong].mean() < 0.2
        assert r["n_in"] == r["keep"].sum() and chi2 <= chi1 + 1e-9 * chi1


def test_early_return_leaves_the_estimate_and_keeps_the_first_removals():
    for i, c in enumerate(ALL):
        if c[2] != 9:
            continue
        p, S0, valid, fix, th2 = T.opt_case(c)
        r = solved(i, "numeric")
        assert r["n_in"] == 0 and np.array_equal(r["S12"], S0) and r["info"][3] == 0 and r["info"][0] == 9
        assert r["keep"].sum() == 9 - r["info"][1]


def test_optimiser_numeric_against_analytic():
    """Both modes agree on every count and on the accept / reject sequence of every case the GPU tests use; OPT_S_DEV, OPT_CHI_DEV and
    OPT_EDGE_DEV are the rounded-up largest deviations: a fresh measurement must not exceed them nor be ten times below them."""
    dev = dict(S=0.0, CHI=0.0, EDGE=0.0)
    for i, c in enumerate(ALL):
        a, b = solved(i, "numeric"), solved(i, "analytic")
        if c in T.OPT_CASES:
            assert a["trials"] == b["trials"] and (a["info"][:4] == b["info"][:4]).all() and (a["info"][6:] == b["info"][6:]).all(), c
            assert min(a["margin"], b["margin"]) >= 1e-11, c
        assert np.array_equal(a["keep"], b["keep"]) and a["n_in"] == b["n_in"] and a["info"][0] == b["info"][0] and a["info"][1] == b["info"][1]
        dev["S"] = max(dev["S"], float(np.abs(a["S12"] - b["S12"]).max()))
        if a["info"][5] > 0:
            dev["CHI"] = max(dev["CHI"], abs(a["info"][5] - b["info"][5]) / a["info"][5])
        for r in (0, 1):
            k = "chi_pairs_%d" % r
            if k in a:
                for x, y in ((a[k][1], b[k][1]), (a[k][2], b[k][2])):
                    m = y <= 2 * 10.0
                    if m.any():
                        dev["EDGE"] = max(dev["EDGE"], float((np.abs(x - y) / 10.0)[m].max()))
        assert T.chi_band(a, 10.0, T.GPU_FACTOR * T.OPT_EDGE_DEV).sum() <= T.MAX_BAND_SHARE_GPU * len(a["keep"]) + 1
    print("measured:", {k: "%.3g" % v for k, v in dev.items()})
    for k, v in dev.items():
        const = getattr(T, "OPT_%s_DEV" % k)
        assert v <= const and v >= const / 10, (k, v, const)
    assert any(any(solved(i, "numeric")["last_rejected"]) for i in range(len(ALL)))     # rounds that end on a rejected trial (floor cases)
    got = {(c[1], c[2], c[3]) for c in ALL}
    assert got == {(bool(f), n, o) for f in (0, 1) for n in T.OPT_SIZES for o in (0.0, 0.2)}


def test_optimiser_entries_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    p, S0, valid, fix, th2 = T.opt_case(T.OPT_CASES[0])
    if L.viorb_device_count() < 1:
        with pytest.raises(viorb_amd.ViorbError) as e:
            sim3.optimize_sim3(p, S0, th2, fix, valid)
        assert e.value.code == capi.ERR_NO_DEVICE
    with pytest.raises(viorb_amd.ViorbError) as e:
        sim3.optimize_sim3(p, S0, 0.0, fix, valid)
    assert e.value.code == capi.ERR_INVALID_ARG
    I, one = capi.Sim3OptInputs(), C.c_void_p(256)
    assert L.viorb_optimize_sim3_device(C.byref(I), 10.0, 0, 1, one, one, one, one, None) == capi.ERR_INVALID_ARG
    for f, _ in capi.Sim3OptInputs._fields_[:11]:
        setattr(I, f, 256)
    I.cap = 0
    assert L.viorb_optimize_sim3_device(C.byref(I), 10.0, 0, 1, one, one, one, one, None) == capi.ERR_INVALID_ARG
    I.cap = 10
    assert L.viorb_optimize_sim3_device(C.byref(I), 10.0, 0, 0, one, one, one, one, None) == capi.ERR_INVALID_ARG
    assert L.viorb_optimize_sim3_device(C.byref(I), 10.0, 0, 65536, one, one, one, one, None) == capi.ERR_INVALID_ARG
    assert L.viorb_optimize_sim3_device(C.byref(I), 10.0, 0, 1, one, None, one, one, None) == capi.ERR_INVALID_ARG
    assert C.sizeof(capi.Sim3OptInputs) == 12 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("sigma", [0.0, 0.9e-5, 1.1e-5, 0.3, -0.2])
@pytest.mark.parametrize("theta", [0.0, 0.9e-5, 1.1e-5, 0.4, 2.5])
def test_hook_exponential_on_both_sides_of_its_switches(sigma, theta):
    axis = np.array([0.6, -0.48, 0.64])
    u = np.concatenate([theta * axis, [0.3, -0.2, 0.5], [sigma]])
    est = np.array([0.1, -0.2, 0.05, 0.97, 0.4, -0.1, 0.2, 1.3]); est[:4] /= np.linalg.norm(est[:4])
    e, pr = sim3.debug_exp(u, est)
    want = T.sim3_exp(u)
    # the same formulas on both sides; sin, cos and exp of two libraries differ by an ulp, entries are of order one
    np.testing.assert_allclose(e, T.sim3_pack(want), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(pr, T.sim3_pack(T.sim3_mul(want, T.sim3_unpack(est))), rtol=2e-14, atol=2e-14)
    assert abs(e[7] - np.exp(sigma)) < 1e-15 and abs(np.linalg.norm(e[:4]) - 1) < (1e-9 if theta < 1e-4 else 1e-14)
    # across a switch the two branches agree to the order of the terms they drop. Not so for theta < 1e-5 <= |sigma|: the reference's B
    # of that branch, (sigma^2 / 2 - sigma + 1) s / sigma^3, is no limit of the general one (t is thousands of metres there), and it is
    # restated as it stands
    pairs = []
    if sigma in (0.9e-5, 1.1e-5) and theta >= 0.4:
        pairs.append(np.concatenate([u[:6], [2e-5 - sigma]]))
    if theta in (0.9e-5, 1.1e-5) and sigma == 0.0:
        pairs.append(np.concatenate([(2e-5 - theta) * axis, u[3:]]))
    for u2 in pairs:
        e2, _ = sim3.debug_exp(u2, est)
        assert np.abs(e2 - e).max() < 1e-5


@pytest.mark.parametrize("fix", [False, True])
def test_hook_edges_and_numeric_jacobians_match_the_checker(fix):
    p, S0, valid, _, _ = T.opt_case(T.OPT_CASES[4])
    S = T.sim3_unpack(S0)
    a = [np.asarray(p[k], np.float32).astype(f64) for k in ("X1c", "X2c", "K1", "K2", "obs1", "obs2")]
    J12, J21 = T.edge_jacobians(S, a[0], a[1], a[2], a[3], a[4], a[5], fix, "numeric")
    A12, A21 = T.edge_jacobians(S, a[0], a[1], a[2], a[3], a[4], a[5], fix, "analytic")
    e12, e21 = T.edge_errors(S, a[1], a[2], a[4]), T.edge_errors(T.sim3_inv(S), a[0], a[3], a[5])
    for j in range(0, len(a[0]), 7):
        h = sim3.debug_edges(S0, a[0][j], a[1][j], a[4][j], a[5][j], a[2], a[3], fix)
        np.testing.assert_allclose(h[0], e12[j], rtol=0, atol=1e-11); np.testing.assert_allclose(h[1], e21[j], rtol=0, atol=1e-11)
        # a difference of two errors rounded at 1e-13 over 2e-9: 1e-4 absolute on entries of a few hundred
        np.testing.assert_allclose(h[2], J12[j], rtol=0, atol=2e-3); np.testing.assert_allclose(h[3], J21[j], rtol=0, atol=2e-3)
        np.testing.assert_allclose(h[2], A12[j], rtol=0, atol=2e-3); np.testing.assert_allclose(h[3], A21[j], rtol=0, atol=2e-3)
        if fix:
            assert (h[2][:, 6] == 0).all() and (h[3][:, 6] == 0).all()          # oplusImpl zeroes update[6]: both perturbed estimates are equal
        else:
            assert np.abs(h[3][:, 6]).max() > 1e-2          # (the first edge's projection does not see a scaling about camera 1)
