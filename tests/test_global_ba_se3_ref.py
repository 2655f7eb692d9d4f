"""CPU checks of the vision-only global bundle adjustment (no GPU): the numpy checker tests/global_ba_se3_ref.py is pinned against the
oracle's vision-only window solve (whose first optimize(5) is the same computation when the local key frames are free and the rest
fixed), the library's host edge hook, central differences and a solve of the un-eliminated normal equations; the library exports the
new entry points and refuses malformed inputs before any GPU call; the C++ shim compiles and links; and every problem the GPU tests
solve keeps its Levenberg decisions away from their thresholds and its result within a quarter of the GPU tests' floors when its points move
in their last bit."""
import ctypes as C
import os
import re
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi
from viorb_amd.capi import ptr
from viorb_amd.global_ba import debug_se3_edge
from viorb_amd.synth import make_local_ba_se3_problem
import global_ba_se3_ref as G
import global_ba_se3_cases as GC


# ---- the checker against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [8, 20])
@pytest.mark.parametrize("stereo", [0.0, 0.5, 1.0])
def test_checker_reproduces_the_oracles_first_phase(oracle, W, stereo):
    """The local key frames free, the rest fixed = oracle.local_ba_se3 up to its first optimize(5): robust, deltas as the oracle forms them
    (fsq(5.991), fsq(7.815)), 5 iterations. Same iteration count, chi2 to 1e-9 relative."""
    p = make_local_ba_se3_problem(3, W=W, stereo_frac=stereo)
    fixed = np.arange(len(p["kfs"])) >= W
    r = G.global_ba_se3(p["kfs"], fixed, p["points"], p["edge_idx"], p["edge_obs"], p["intr5"], iterations=5, robust=True, delta2_mono=5.991, delta2_stereo=7.815)
    o = oracle.local_ba_se3(p["kfs"], W, p["points"], p["edge_idx"], p["edge_obs"], p["intr5"])
    print("W", W, "stereo", stereo, "its", r["its"], o["its_first"], "chi2", r["info"][1], o["chi2_first"])
    assert r["its"] == o["its_first"]
    assert abs(r["info"][1] - o["chi2_first"]) <= 1e-9 * o["chi2_first"]


@pytest.mark.parametrize("stereo", [0.0, 1.0])
def test_checker_edges_match_the_host_hook_and_central_differences(stereo):
    p = GC.problem(5, 8, stereo)
    kfs, pts, ei, eo, intr = p["kfs"], p["points"], p["edge_idx"].astype(np.int64), p["edge_obs"], p["intr5"]
    e, Jp, Jk = G.edges(kfs, pts, intr, ei, eo)
    seen = set()
    for k in range(0, len(e), 17):
        pi, ki = ei[k]
        dim, he, hJp, hJk = debug_se3_edge(kfs[ki], pts[pi], eo[k], intr)
        assert dim == (2 if eo[k, 2] < 0 else 3)
        seen.add(dim)
        np.testing.assert_allclose(e[k], he, rtol=0, atol=1e-10)
        np.testing.assert_allclose(Jp[k], hJp, rtol=1e-12, atol=1e-10)
        np.testing.assert_allclose(Jk[k], hJk, rtol=1e-12, atol=1e-9)
        if dim == 2:
            assert e[k, 2] == 0 and not Jp[k, 2].any() and not Jk[k, 2].any()
        one = lambda K, X: G.edges(np.array([K]), np.array([X]), intr, np.array([[0, 0]]), eo[k:k + 1], jac=False)[0][0]
        # the point Jacobian against central differences. A stereo edge projects with a float reciprocal depth: a projection of up to
        # 1300 px moves by up to 1300 * 2^-24 = 8e-5 px from that rounding alone, 0.08 per unit in a quotient over 2 h = 2e-3
        h = 1e-3 if dim == 3 else 1e-6
        for c in range(3):
            d = np.zeros(3); d[c] = h
            np.testing.assert_allclose(Jp[k][:, c], (one(kfs[ki], pts[pi] + d) - one(kfs[ki], pts[pi] - d)) / (2 * h), rtol=1e-4 if dim == 3 else 1e-5, atol=0.1 if dim == 3 else 1e-4)
        # the pose Jacobian: the increment is applied as exp(d) * T (VertexSE3Expmap::oplusImpl)
        for c in range(6):
            d = np.zeros(6); d[c] = h
            Kp = np.concatenate(G.se3_mul(*G.se3_exp(d), kfs[ki][:4], kfs[ki][4:]))
            Km = np.concatenate(G.se3_mul(*G.se3_exp(-d), kfs[ki][:4], kfs[ki][4:]))
            np.testing.assert_allclose(Jk[k][:, c], (one(Kp, pts[pi]) - one(Km, pts[pi])) / (2 * h), rtol=1e-4 if dim == 3 else 1e-5, atol=0.1 if dim == 3 else 1e-3)
    assert (3 in seen) == (stereo > 0) and (2 in seen or stereo > 0)


@pytest.mark.parametrize("robust", [False, True])
def test_schur_solve_equals_the_full_normal_equations(robust):
    """Same Levenberg, solved without eliminating the points: guards the Schur algebra (and the back-substitution)."""
    p = GC.problem(7, 6, 0.5)
    a = G.global_ba_se3(*GC.args(p), iterations=6, robust=robust)
    b = G.global_ba_se3(*GC.args(p), iterations=6, robust=robust, linear="full")
    assert [t[4] for t in a["trials"]] == [t[4] for t in b["trials"]] and a["its"] == b["its"]
    assert abs(a["info"][1] - b["info"][1]) <= 1e-9 * b["info"][1]
    np.testing.assert_allclose(a["kfs"], b["kfs"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(a["points"], b["points"], rtol=0, atol=1e-7)


def test_checker_leaves_a_point_without_edges_alone():
    p = GC.problem(311, 12)
    pts = np.vstack([p["points"], [[1.0, 2.0, 30.0]]])
    r = G.global_ba_se3(p["kfs"], p["fixed"], pts, p["edge_idx"], p["edge_obs"], p["intr5"], iterations=3)
    assert r["point_included"][-1] == 0 and r["point_included"][:-1].all()
    assert np.array_equal(r["points"][-1], [1.0, 2.0, 30.0])


# ---- the library, without a device ----------------------------------------------------------------------------------------------------
def _call(p, **over):
    a = dict(kfs=p["kfs"], fixed=p["fixed"], points=p["points"], edge_idx=p["edge_idx"], edge_obs=p["edge_obs"], intr5=p["intr5"])
    a.update(over)
    kfs = np.ascontiguousarray(a["kfs"], np.float64); pts = np.ascontiguousarray(a["points"], np.float64)
    ei = np.ascontiguousarray(a["edge_idx"], np.int32); eo = np.ascontiguousarray(a["edge_obs"], np.float64)
    fixed = np.ascontiguousarray(a["fixed"], np.uint8); intr = np.ascontiguousarray(a["intr5"], np.float64)
    ko, po, inc, info = np.zeros_like(kfs), np.zeros_like(pts), np.zeros(len(pts) + 1, np.uint8), np.zeros(6)
    cfg = capi.GbaConfig(over.get("iterations", 10), over.get("robust", 0))
    stop = over.get("stop")
    rc = viorb_amd.lib().viorb_global_ba_se3(C.byref(cfg), ptr(kfs), len(kfs), ptr(fixed), ptr(pts), len(pts), ptr(ei), ptr(eo), len(ei), ptr(intr),
                                             ptr(stop) if stop is not None else None, ptr(ko), ptr(po), ptr(inc), ptr(info))
    return rc, ko, po, inc[:len(pts)], info


def test_entry_points_are_exported_and_check_their_arguments_without_a_device():
    L = viorb_amd.lib()
    names = {"viorb_global_ba_se3", "viorb_global_ba_se3_device", "viorb_global_ba_se3_workspace_bytes", "viorb_debug_gba_se3_edge"}
    # the header of these entry points (viorb.h includes it) declares exactly them, with the argument counts of the ctypes mirror
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_global_ba_se3.h"' in open(os.path.join(inc, "viorb.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "viorb_global_ba_se3.h")).read(), flags=re.S)
    counts = {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == names == set(capi.SIGNATURES_GLOBAL_BA_SE3)
    for n in names:
        assert hasattr(L, n) and len(capi.SIGNATURES_GLOBAL_BA_SE3[n][1]) == counts[n], n
    assert L.viorb_abi_version() == 2 and C.sizeof(capi.GbaConfig) == 8
    p = GC.problem(311, 12)
    assert (p["edge_obs"][:, 2] >= 0).any() and (p["edge_obs"][:, 2] < 0).any()
    E = capi.ERR_INVALID_ARG
    ei = p["edge_idx"]
    bad = ei.copy(); bad[5, 0] = len(p["points"])
    assert _call(p, edge_idx=bad)[0] == E                                   # point index out of range
    bad = ei.copy(); bad[5, 1] = 12
    assert _call(p, edge_idx=bad)[0] == E                                   # key-frame index out of range
    bad = ei.copy(); bad[7, 1] = -1
    assert _call(p, edge_idx=bad)[0] == E
    assert _call(p, edge_idx=ei[::-1].copy(), edge_obs=p["edge_obs"][::-1].copy())[0] == E      # not sorted by point
    bad = p["edge_obs"].copy(); bad[3, 3] = 0.0
    assert _call(p, edge_obs=bad)[0] == E                                   # invSigma2 <= 0
    for bf in (0.0, -1.0):
        intr = p["intr5"].copy(); intr[4] = bf
        assert _call(p, intr5=intr)[0] == E                                 # a stereo edge without a baseline
    assert _call(p, iterations=-1)[0] == E
    assert b"invalid argument" in L.viorb_last_error()
    # over the documented limit: refused, not truncated (checked before anything is allocated); 4096 free key frames are not over it
    nk = 4097
    big = dict(kfs=np.tile(p["kfs"][:1], (nk, 1)), fixed=np.zeros(nk, np.uint8), points=np.zeros((0, 3)), edge_idx=np.zeros((0, 2), np.int32), edge_obs=np.zeros((0, 4)))
    assert _call(p, **big)[0] == capi.ERR_CAPACITY
    big["fixed"][0] = 1
    assert _call(p, **big)[0] in (capi.VIORB_OK, capi.ERR_NO_DEVICE, capi.ERR_HIP)
    assert L.viorb_global_ba_se3_workspace_bytes(2048, 40960, 300000) > 2048 * 6 * 2048 * 6 * 8
    assert L.viorb_global_ba_se3_workspace_bytes(0, 0, 0) == 0
    # a stop flag raised before the call: the inputs come back with point_included filled, whether or not there is a device
    q = dict(p, points=np.vstack([p["points"], [[1.0, 2.0, 30.0]]]))
    rc, ko, po, inc, info = _call(q, stop=np.ones(1, np.int32))
    assert rc == capi.VIORB_OK and np.array_equal(ko, q["kfs"]) and np.array_equal(po, q["points"]) and info[2] == 0 and inc[:-1].all() and inc[-1] == 0
    # the edge hook runs on the host
    dim, e, Jp, Jk = debug_se3_edge(p["kfs"][ei[0, 1]], p["points"][ei[0, 0]], p["edge_obs"][0], p["intr5"])
    assert dim in (2, 3) and np.isfinite(e).all() and np.abs(Jk).max() > 0
    if L.viorb_device_count() > 0:
        return
    intr = p["intr5"].copy(); intr[4] = 0.0
    mono = p["edge_obs"].copy(); mono[:, 2] = -1.0
    assert _call(p, edge_obs=mono, intr5=intr)[0] == capi.ERR_NO_DEVICE       # bf is not needed without a stereo edge
    assert _call(p)[0] == capi.ERR_NO_DEVICE                                # a valid problem needs the GPU: no CPU fallback
    with pytest.raises(viorb_amd.ViorbError):
        viorb_amd.GlobalBundleAdjustmentSE3(*GC.args(p))


def test_cpp_shim_compiles_links_and_refuses_without_a_device(tmp_path):
    """viorb_shim::global_bundle_adjustment / bundle_adjustment compile against stand-ins with the reference's member names and link the
    library; without a device the call throws with the library's text and leaves the map untouched (with one, the tiny map is solved)."""
    import subprocess
    from test_gpu_global_ba_se3_shim import build_global_ba_se3_shim_test
    out = subprocess.run([build_global_ba_se3_shim_test(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    if viorb_amd.lib().viorb_device_count() < 1:
        assert "no HIP device" in out.stdout


# ---- margins of the GPU cases -------------------------------------------------------------------------------------------------------
def _margins(p, robust, iterations):
    """(trials, min |rho|, termination margin, the checker's own spread of the final lambda) of one problem. The spread: the checker run
    with its sums in edge order + Cholesky and in reverse order + numpy.linalg.solve. Near convergence lambda's update 1 - (2 rho - 1)^3
    multiplies a rounding-level difference of chi2 by chi2 / (its last decrease), and the stereo edges' float reciprocal depth makes chi2
    itself jump by about 1e-10 relative when a depth crosses a float boundary; a problem whose two checker runs end further apart in
    lambda than a tenth of the 1e-6 the device is held to says nothing about the device. The same two runs give the band of the poses and
    points; four times it has to stay under the floors of 1e-7 / 1e-6, so that the floors are what the GPU tests apply."""
    a = G.global_ba_se3(*GC.args(p), iterations=iterations, robust=bool(robust))
    b = G.global_ba_se3(*GC.args(p), iterations=iterations, robust=bool(robust), linear="solve", reverse=True)
    rho = min(abs(t[3]) for t in a["trials"])
    term = min(abs((ini - cur) * 1e3 - ini) / ini for ini, cur in a["term"])
    return a["trials"], rho, term, abs(a["info"][4] - b["info"][4]) / a["info"][4], np.abs(a["kfs"] - b["kfs"]).max(), np.abs(a["points"] - b["points"]).max()


PERTURBATION = 1e-15


def _perturbation_moves(p, robust, iterations, runs, rng_seed):
    """(same accept / reject sequence in every run, worst move of a key-frame row, worst move of a point) of the checker when the points
    it starts from are scaled by 1 + 1e-15 N(0, 1), `runs` times, against the checker on the problem as it stands. Two summation orders
    are two samples; a solve that sits on a discrete event (a stereo edge's float reciprocal depth crossing a float boundary, a Huber
    switch) lands on the other side of it in a fraction of the samples only, and the device's unordered FP64 sums are such samples."""
    a = G.global_ba_se3(*GC.args(p), iterations=iterations, robust=bool(robust))
    seq = [t[4] for t in a["trials"]]
    rng = np.random.default_rng(rng_seed)
    same, dk, dp = True, 0.0, 0.0
    for _ in range(runs):
        q = dict(p, points=p["points"] * (1.0 + PERTURBATION * rng.standard_normal(p["points"].shape)))
        b = G.global_ba_se3(*GC.args(q), iterations=iterations, robust=bool(robust))
        same = same and [t[4] for t in b["trials"]] == seq
        dk = max(dk, np.abs(a["kfs"] - b["kfs"]).max())
        dp = max(dp, np.abs(a["points"] - b["points"]).max()) if len(a["points"]) else dp
    return same, dk, dp


def _check_margins(name, p, robust, iterations, runs=12, rng_seed=0):
    trials, rho, term, dlam, dk, dp = _margins(p, robust, iterations)
    print(name, "trials", "".join("A" if t[4] else "R" for t in trials), "min |rho| %.3g" % rho, "termination margin %.3g" % term, "lambda spread %.3g" % dlam,
          "band: key frames %.3g points %.3g" % (dk, dp))
    assert rho >= 1e-6 and term >= 1e-6, name
    assert len(trials) < 10 * iterations, name
    assert dlam <= 1e-7, name
    assert 4 * dk <= 1e-7 and 4 * dp <= 1e-6, name
    # the same quarter of the floors for the inputs moved in their last bit: generator seed rng_seed, written by the caller
    same, mk, mp = _perturbation_moves(p, robust, iterations, runs, rng_seed)
    print(name, "%d perturbations of %.0e (generator seed %d): same decisions %s, moves: key frames %.3g points %.3g" % (runs, PERTURBATION, rng_seed, same, mk, mp))
    assert same, name
    assert 4 * mk <= 1e-7 and 4 * mp <= 1e-6, name


@pytest.mark.parametrize("seed,N,robust,stereo,revisit", GC.CASES)
def test_gpu_cases_keep_their_decisions_away_from_the_thresholds(seed, N, robust, stereo, revisit):
    """A device whose chi2 differs from the checker's in the 10th digit takes the same accept / reject and termination decisions only
    if no decision is that close: every trial's rho at least 1e-6 from 0, (iniChi - chi) * 1e3 at least 1e-6 relative from iniChi."""
    _check_margins("seed %d N %d" % (seed, N), GC.problem(seed, N, stereo, revisit), robust, GC.ITERATIONS, runs=12 if N <= 43 else 6, rng_seed=10000 + seed)


def test_the_other_checked_gpu_problems_keep_their_margins():
    """the exact variants the remaining GPU tests compare with the checker (global_ba_se3_cases.checked_variants): same generator
    arguments, same edits, same robust flag and iteration count"""
    for i, (name, q, robust, iterations) in enumerate(GC.checked_variants()):
        _check_margins(name, q, robust, iterations, runs=12, rng_seed=20000 + i)
