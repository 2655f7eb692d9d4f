"""CPU checks of the global bundle adjustment (no GPU): the numpy checker tests/global_ba_ref.py is pinned against the oracle's window
solve (whose first optimize(5) is the same computation when key frame 0 is fixed and every other one is local), the oracle's edge
functions, central differences and a solve of the un-eliminated normal equations; the library exports the new entry points and refuses
malformed inputs before any GPU call; and every problem the GPU tests solve keeps its Levenberg decisions away from their thresholds and (up
to N = 60) its result within a quarter of the GPU tests' floors when its points move in their last bit."""
import ctypes as C
import functools
import os
import re
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi
from viorb_amd.capi import ptr
from viorb_amd.synth import make_global_ba_problem
import global_ba_ref as G
import global_ba_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _problem(seed, N, revisit=0.0, n_points=None):
    from oracle import binding
    return make_global_ba_problem(seed, N, n_points=n_points, revisit_frac=revisit, preint_fn=GC.oracle_preint(binding))


# ---- the checker against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 21, 60])
def test_checker_reproduces_the_oracles_first_phase(oracle, N):
    """Key frame 0 fixed, all others free = oracle.local_ba(n_local = N - 1, prev_kf = N - 1) up to its first optimize(5): robust, mono
    delta^2 5.991 as the oracle forms it, 5 iterations. Same iteration count, chi2 to 1e-9 relative."""
    p = _problem(3, N, 0.2)
    r = G.global_ba(*GC.args(p), iterations=5, robust=True, delta2_mono=5.991)
    order = list(range(1, N)) + [0]                                         # the oracle wants the local window first
    ei = p["edge_idx"].copy(); ei[:, 1] = np.where(ei[:, 1] == 0, N - 1, ei[:, 1] - 1)
    o = oracle.local_ba(p["kfs"][order], N - 1, N - 1, p["preint"][1:], p["points"], ei, p["edge_obs"], p["gw"], p["cam"])
    print("N", N, "its", r["its"], o["its_first"], "chi2", r["info"][1], o["chi2_first"])
    assert r["its"] == o["its_first"]
    assert abs(r["info"][1] - o["chi2_first"]) <= 1e-9 * o["chi2_first"]


def test_checker_edges_match_the_oracle_and_central_differences(oracle):
    p = _problem(5, 8, 0.0)
    kfs, pts = p["kfs"], p["points"]
    for i in (1, 4, 7):
        e, J = G.edge_pvr(kfs[i - 1], kfs[i], p["preint"][i], p["gw"])
        oe, Ji, Jj, Jb = oracle.edge_pvr(kfs[i - 1], kfs[i], kfs[i - 1], p["preint"][i], p["gw"])
        np.testing.assert_allclose(e, oe, rtol=0, atol=1e-12)
        np.testing.assert_allclose(J, np.hstack([Ji, Jj, Jb]), rtol=0, atol=1e-9)
    e, Jp, Jk, _ = G.edge_proj(kfs, pts, p["cam"], p["edge_idx"].astype(np.int64), p["edge_obs"])
    for k in range(0, len(e), 37):
        pi, ki = p["edge_idx"][k]
        oe, oJ = oracle.edge_proj(kfs[ki], p["cam"], np.concatenate([pts[pi], p["edge_obs"][k]]))
        np.testing.assert_allclose(e[k], oe, rtol=0, atol=1e-9)
        np.testing.assert_allclose(Jk[k], oJ[:, [0, 1, 2, 6, 7, 8]], rtol=0, atol=1e-9)
        assert np.all(oJ[:, 3:6] == 0)
        # the point Jacobian (the oracle's pose edge has none) against central differences
        h = 1e-6
        for c in range(3):
            d = np.zeros(3); d[c] = h
            ep = G.edge_proj(kfs, np.array([pts[pi] + d]), p["cam"], np.array([[0, ki]]), p["edge_obs"][k:k + 1], jac=False)[0][0]
            em = G.edge_proj(kfs, np.array([pts[pi] - d]), p["cam"], np.array([[0, ki]]), p["edge_obs"][k:k + 1], jac=False)[0][0]
            np.testing.assert_allclose(Jp[k][:, c], (ep - em) / (2 * h), rtol=1e-6, atol=1e-5)


@pytest.mark.parametrize("robust", [False, True])
def test_schur_solve_equals_the_full_normal_equations(robust):
    """Same Levenberg, solved without eliminating the points: guards the Schur algebra (and the back-substitution)."""
    p = _problem(7, 6, 0.0, n_points=60)
    a = G.global_ba(*GC.args(p), iterations=6, robust=robust)
    b = G.global_ba(*GC.args(p), iterations=6, robust=robust, linear="full")
    assert [t[4] for t in a["trials"]] == [t[4] for t in b["trials"]] and a["its"] == b["its"]
    assert abs(a["info"][1] - b["info"][1]) <= 1e-9 * b["info"][1]
    np.testing.assert_allclose(a["kfs"], b["kfs"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(a["points"], b["points"], rtol=0, atol=1e-8)


def test_checker_leaves_a_point_without_edges_alone():
    p = _problem(311, 21)
    pts = np.vstack([p["points"], [[1.0, 2.0, 3.0]]])
    r = G.global_ba(p["kfs"], p["prev"], p["fixed"], p["preint"], pts, p["edge_idx"], p["edge_obs"], p["gw"], p["cam"], iterations=3)
    assert r["point_included"][-1] == 0 and r["point_included"][:-1].all()
    assert np.array_equal(r["points"][-1], [1.0, 2.0, 3.0])


# ---- the library, without a device ----------------------------------------------------------------------------------------------------
def _call(p, **over):
    a = dict(kfs=p["kfs"], prev=p["prev"], fixed=p["fixed"], preint=p["preint"], points=p["points"], edge_idx=p["edge_idx"], edge_obs=p["edge_obs"])
    a.update(over)
    kfs = np.ascontiguousarray(a["kfs"], np.float64); pts = np.ascontiguousarray(a["points"], np.float64)
    ei = np.ascontiguousarray(a["edge_idx"], np.int32); eo = np.ascontiguousarray(a["edge_obs"], np.float64)
    prev = np.ascontiguousarray(a["prev"], np.int32); fixed = np.ascontiguousarray(a["fixed"], np.uint8); pre = np.ascontiguousarray(a["preint"], np.float64)
    ko, po, inc, info = np.zeros_like(kfs), np.zeros_like(pts), np.zeros(len(pts) + 1, np.uint8), np.zeros(6)
    cfg = capi.GbaConfig(over.get("iterations", 10), over.get("robust", 0))
    stop = over.get("stop")
    rc = viorb_amd.lib().viorb_global_ba_navstate(C.byref(cfg), ptr(kfs), len(kfs), ptr(prev), ptr(fixed), ptr(pre), ptr(pts), len(pts), ptr(ei), ptr(eo),
                                                  len(ei), ptr(p["gw"]), ptr(p["cam"]), ptr(stop) if stop is not None else None, ptr(ko), ptr(po), ptr(inc), ptr(info))
    return rc, ko, po, inc[:len(pts)], info


def test_entry_points_are_exported_and_check_their_arguments_without_a_device():
    L = viorb_amd.lib()
    names = {"viorb_global_ba_navstate", "viorb_global_ba_navstate_device", "viorb_global_ba_navstate_workspace_bytes", "viorb_debug_gba_cholesky",
             "viorb_debug_gba_last_trials"}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viorb.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(viorb_(?:debug_gba|global_ba)[a-z0-9_]*)\s*\(", hdr)) == names
    for n in names:
        assert hasattr(L, n) and n in capi.SIGNATURES, n
    assert L.viorb_abi_version() == 2 and C.sizeof(capi.GbaConfig) == 8
    p = _problem(311, 21)
    E = capi.ERR_INVALID_ARG
    ei = p["edge_idx"]
    bad = ei.copy(); bad[5, 0] = len(p["points"])
    assert _call(p, edge_idx=bad)[0] == E                                   # point index out of range
    bad = ei.copy(); bad[5, 1] = 21
    assert _call(p, edge_idx=bad)[0] == E                                   # key-frame index out of range
    bad = ei.copy(); bad[7, 1] = -1
    assert _call(p, edge_idx=bad)[0] == E
    assert _call(p, edge_idx=ei[::-1].copy(), edge_obs=p["edge_obs"][::-1].copy())[0] == E      # not sorted by point
    bad = p["prev"].copy(); bad[4] = 4
    assert _call(p, prev=bad)[0] == E                                       # prev[i] >= i
    bad = p["prev"].copy(); bad[4] = 9
    assert _call(p, prev=bad)[0] == E
    bad = p["edge_obs"].copy(); bad[3, 2] = -1.0                            # what a caller might try for a stereo observation
    assert _call(p, edge_obs=bad)[0] == E
    assert _call(p, iterations=-1)[0] == E
    assert b"invalid argument" in L.viorb_last_error()
    # over the documented limit: refused, not truncated (checked before anything is allocated)
    nk = 2050
    big = dict(kfs=np.tile(p["kfs"][:1], (nk, 1)), prev=np.full(nk, -1, np.int32), fixed=np.zeros(nk, np.uint8), preint=np.zeros((nk, 142)),
               points=np.zeros((0, 3)), edge_idx=np.zeros((0, 2), np.int32), edge_obs=np.zeros((0, 3)))
    assert _call(p, **big)[0] == capi.ERR_CAPACITY
    assert L.viorb_global_ba_navstate_workspace_bytes(1024, 40960, 300000) > 1024 * 12 * 1024 * 12 * 8
    assert L.viorb_global_ba_navstate_workspace_bytes(0, 0, 0) == 0
    # a stop flag raised before the call: the inputs come back, whether or not there is a device
    rc, ko, po, inc, info = _call(p, stop=np.ones(1, np.int32))
    assert rc == capi.VIORB_OK and np.array_equal(ko, p["kfs"]) and np.array_equal(po, p["points"]) and info[2] == 0 and inc.all()
    if L.viorb_device_count() > 0:
        return
    assert _call(p)[0] == capi.ERR_NO_DEVICE                                # a valid problem needs the GPU: no CPU fallback
    with pytest.raises(viorb_amd.ViorbError):
        viorb_amd.GlobalBundleAdjustmentNavState(*GC.args(p))
    z = np.zeros(8, np.float64)
    assert L.viorb_debug_gba_cholesky(ptr(np.eye(2)), 2, ptr(z), ptr(np.zeros(1, np.int32))) == capi.ERR_NO_DEVICE


def test_cpp_shim_compiles_links_and_refuses_without_a_device(tmp_path):
    """viorb_shim::global_bundle_adjustment_navstate compiles against stand-ins with the reference's member names and links the library; a
    stereo observation throws; without a device the call throws with the library's text and leaves the map untouched (with one, the tiny
    map is solved)."""
    import subprocess
    from test_gpu_global_ba_shim import build_global_ba_shim_test
    out = subprocess.run([build_global_ba_shim_test(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    if viorb_amd.lib().viorb_device_count() < 1:
        assert "no HIP device" in out.stdout


# ---- margins of the GPU cases -------------------------------------------------------------------------------------------------------
def _margins(r):
    rho = min(abs(t[3]) for t in r["trials"])
    term = min(abs((ini - cur) * 1e3 - ini) / ini for ini, cur in r["term"])
    return rho, term


PERTURBATION, PERTURBED_RUNS = 1e-15, 12


def _check_perturbation_margin(name, p, r, robust, iterations, rng_seed):
    """The checker on the problem with its points scaled by 1 + 1e-15 N(0, 1), 12 times (generator seed rng_seed, written by the caller),
    against its result r on the problem as it stands: the same accept / reject sequence every time, and no key-frame state further than
    a quarter of the 1e-7, no point further than a quarter of the 1e-6 that tests/test_gpu_global_ba.py holds the device to. A case that
    fails this sits on a discrete event of its own solve, and the device's unordered FP64 sums land on either side of it."""
    seq = [t[4] for t in r["trials"]]
    rng = np.random.default_rng(rng_seed)
    same, dk, dp = True, 0.0, 0.0
    for _ in range(PERTURBED_RUNS):
        q = dict(p, points=p["points"] * (1.0 + PERTURBATION * rng.standard_normal(p["points"].shape)))
        b = G.global_ba(*GC.args(q), iterations=iterations, robust=bool(robust))
        same = same and [t[4] for t in b["trials"]] == seq
        dk, dp = max(dk, np.abs(r["kfs"] - b["kfs"]).max()), max(dp, np.abs(r["points"] - b["points"]).max())
    print(name, "%d perturbations of %.0e (generator seed %d): same decisions %s, moves: states %.3g points %.3g" % (PERTURBED_RUNS, PERTURBATION, rng_seed, same, dk, dp))
    assert same, name
    assert 4 * dk <= 1e-7 and 4 * dp <= 1e-6, name


@pytest.mark.parametrize("seed,N,robust,revisit", [c for c in GC.CASES if c[1] <= 60])
def test_gpu_cases_do_not_move_with_the_last_bit_of_their_points(seed, N, robust, revisit):
    p = _problem(seed, N, revisit)
    r = G.global_ba(*GC.args(p), iterations=GC.ITERATIONS, robust=bool(robust))
    _check_perturbation_margin("seed %d N %d" % (seed, N), p, r, robust, GC.ITERATIONS, rng_seed=10000 + seed)


@pytest.mark.parametrize("seed,N,robust,revisit", GC.CASES)
def test_gpu_cases_keep_their_decisions_away_from_the_thresholds(seed, N, robust, revisit):
    """A device whose chi2 differs from the checker's in the 10th digit takes the same accept / reject and termination decisions only
    if no decision is that close: every trial's rho at least 1e-6 from 0, (iniChi - chi) * 1e3 at least 1e-6 relative from iniChi.
    (The pre-integrations come from the oracle here and from the device in the GPU tests; they agree to rounding.)"""
    p = _problem(seed, N, revisit)
    r = G.global_ba(*GC.args(p), iterations=GC.ITERATIONS, robust=bool(robust))
    rho, term = _margins(r)
    print("seed", seed, "N", N, "trials", "".join("A" if t[4] else "R" for t in r["trials"]), "min |rho| %.3g" % rho, "termination margin %.3g" % term)
    assert rho >= 1e-6 and term >= 1e-6
    assert len(r["trials"]) < 10 * GC.ITERATIONS


def test_the_other_checked_gpu_problems_keep_their_margins():
    """the exact variants the remaining GPU tests compare with the checker (global_ba_cases.checked_variants): same generator arguments,
    same edits, same robust flag and iteration count"""
    for i, (name, q, robust, iterations) in enumerate(GC.checked_variants(lambda seed, N: _problem(seed, N))):
        r = G.global_ba(*GC.args(q), iterations=iterations, robust=bool(robust))
        rho, term = _margins(r)
        print(name, "trials", "".join("A" if t[4] else "R" for t in r["trials"]), "min |rho| %.3g" % rho, "termination margin %.3g" % term)
        assert rho >= 1e-6 and term >= 1e-6, name
        _check_perturbation_margin(name, q, r, robust, iterations, rng_seed=20000 + i)
