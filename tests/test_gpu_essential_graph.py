"""GPU tests of the essential-graph solve (viorb_optimize_essential_graph and its device form) against the numpy checker
tests/essential_graph_ref.py in its "numeric" mode (g2o's Jacobians), over tests/essential_graph_cases.py. Poses, Tcw_out and points
agree within GPU_FACTOR times the deviation of the checker's two Jacobian modes (EG_*_DEV, measured by
tests/test_essential_graph_ref.py), the final chi2 within the project's 1e-5 relative. The accept / reject sequence is compared trial for
trial over the decidable prefix: up to, not including, the first trial whose relative chi2 change in the checker is below BAND_FACTOR x
EG_CHI_DEV; behind it the solve gains at the rounding floor of chi2 and its trials are decided by rounding, in g2o as here.

Run-to-run spread: the solve has three sums whose order the hardware picks (chi2 and the gain ratio's denominator over the workgroups
of k_eg_errors / k_eg_update, and the off-diagonal block of a pair joined by several edges). Each of them has at most two terms at the
sizes of these tests (up to 512 edges, 256 vertices, a pair joined twice), and a sum of two terms does not depend on their order: the
results are bit for bit reproducible here, which test_run_to_run_and_device_form_agree_bit_for_bit asserts."""
import os
import sys
import threading
import ctypes as C

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_graph_ref as ER
import essential_graph_cases as EC

pytestmark = pytest.mark.gpu


def _solve(p, device=False, iterations=ER.ITERATIONS):
    from viorb_amd import essential_graph as EG
    return EG.solve(p, device=device, iterations=iterations)


def _compare(got, ref, p, name):
    dev = ER.deviations(ref, dict(Scw_out=got["Scw_out"], Tcw_out=got["Tcw_out"], points_out=got["points_out"], info=got["info"]))
    floor = ER.BAND_FACTOR * ER.EG_CHI_DEV
    k = ER.decidable_prefix(ref, floor)
    print("%s: S %.2e T %.2e P %.2e (bounds %.1e %.1e %.1e) chi2 %.6e against %.6e, trials %s against %s, prefix %d" % (
        name, dev[0], dev[1], dev[2], ER.GPU_FACTOR * ER.EG_S_DEV, ER.GPU_FACTOR * ER.EG_T_DEV, ER.GPU_FACTOR * ER.EG_P_DEV, got["chi2_after"], ref["info"][1],
        "".join("1" if a else "0" for a in got["accepted"]), "".join("1" if a else "0" for a in ref["accepted"]), k))
    assert dev[0] <= ER.GPU_FACTOR * ER.EG_S_DEV and dev[1] <= ER.GPU_FACTOR * ER.EG_T_DEV and dev[2] <= ER.GPU_FACTOR * ER.EG_P_DEV
    if name in EC.ZERO_CHI2:
        assert got["chi2_before"] <= ER.EG_CHI_ABS and got["chi2_after"] <= ER.EG_CHI_ABS
    else:
        assert abs(got["chi2_before"] - ref["info"][0]) <= ER.CHI2_TOL * ref["info"][0]
        assert abs(got["chi2_after"] - ref["info"][1]) <= ER.CHI2_TOL * ref["info"][1]
    assert got["accepted"][:k] == ref["accepted"][:k]
    assert got["failed_factorisations"] == 0 and got["trials"] == len(got["accepted"]) and got["iterations"] <= ER.ITERATIONS
    fixed = p["fixed"].astype(bool)
    assert (got["Scw_out"][fixed].view(np.uint64) == np.ascontiguousarray(p["Scw"], np.float64)[fixed].view(np.uint64)).all()      # fixed rows bit for bit
    if p["fix_scale"]:
        assert (got["Scw_out"][:, 7].view(np.uint64) == np.ascontiguousarray(p["Scw"][:, 7], np.float64).view(np.uint64)).all()


@pytest.mark.parametrize("name", EC.NAMES)
def test_essential_graph_matches_checker(name):
    p = EC.problem(name)
    _compare(_solve(p), EC.reference(name), p, name)


def _same_bits(a, b):
    return all((np.ascontiguousarray(a[k]).view(np.uint8) == np.ascontiguousarray(b[k]).view(np.uint8)).all() for k in ("Scw_out", "Tcw_out", "points_out"))


def test_run_to_run_and_device_form_agree_bit_for_bit():
    for name in ("points", "n110_free", "duplicated_pair"):
        p = EC.problem(name)
        a, b, d = _solve(p), _solve(p), _solve(p, device=True)
        print("%s: run to run |dS| %.3g, device against host |dS| %.3g, chi2 %.17g %.17g %.17g" % (
            name, np.abs(a["Scw_out"] - b["Scw_out"]).max(), np.abs(a["Scw_out"] - d["Scw_out"]).max(), a["chi2_after"], b["chi2_after"], d["chi2_after"]))
        assert a["accepted"] == b["accepted"] == d["accepted"]
        assert _same_bits(a, b) and _same_bits(a, d)
        assert a["chi2_after"] == b["chi2_after"] == d["chi2_after"] and (a["info"] == d["info"]).all()


def test_four_threads_each_get_their_solo_result():
    names = ("n9_free", "n37_fix", "points", "three_fixed_inside")
    solo = [_solve(EC.problem(n)) for n in names]
    out = [None] * 4

    def work(i):
        out[i] = _solve(EC.problem(names[i]))
    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in th]; [t.join() for t in th]
    for g, r in zip(out, solo):
        assert g is not None and g["accepted"] == r["accepted"] and (g["info"] == r["info"]).all()
        assert _same_bits(g, r)


def test_a_free_vertex_without_an_edge_keeps_its_estimate():
    p = dict(EC.problem("n10_free"))
    lone = np.array([[0.1, -0.2, 0.3, 0.9, 1.0, 2.0, 3.0, 1.25]])
    p["Scw"], p["Smeas"] = np.concatenate([p["Scw"], lone]), np.concatenate([p["Smeas"], lone])
    p["fixed"] = np.concatenate([p["fixed"], [0]]).astype(np.uint8)
    got, ref = _solve(p), EC.reference("n10_free")
    assert (got["Scw_out"][-1].view(np.uint64) == lone[0].view(np.uint64)).all()
    assert np.abs(got["Scw_out"][:-1] - ref["Scw_out"]).max() <= ER.GPU_FACTOR * ER.EG_S_DEV * max(1.0, np.abs(ref["Scw_out"][:, 4:7]).max())
    assert abs(got["chi2_after"] - ref["info"][1]) <= ER.CHI2_TOL * ref["info"][1]


def test_zero_iterations_write_the_input_back():
    p = EC.problem("points")
    got = _solve(p, iterations=0)
    assert (got["Scw_out"] == p["Scw"]).all() and got["iterations"] == 0 and got["trials"] == 0 and got["chi2_before"] == got["chi2_after"] > 0
    T, P = ER.recover(p, np.asarray(p["Scw"], np.float64))
    assert np.abs(got["Tcw_out"] - T).max() <= 1e-12 * max(1.0, np.abs(T).max())
    skipped = p["point_ref"] < 0
    assert skipped.any() and (got["points_out"][skipped] == p["points"][skipped]).all()
    assert np.abs(got["points_out"] - P).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(P).max())


def _device_call(p, ws_bytes=None, **over):
    """The raw status of the device form (the argument checks run in k_eg_setup)."""
    import torch
    import viorb_amd
    from viorb_amd import capi
    from viorb_amd.capi import ptr, _torch_up as up
    q = dict(p); q.update(over)
    Scw, Smeas = up(np.ascontiguousarray(q["Scw"], np.float64)), up(np.ascontiguousarray(q["Smeas"], np.float64))
    fixed = up(np.ascontiguousarray(q["fixed"], np.uint8))
    ei, ec = up(np.ascontiguousarray(q["edge_idx"], np.int32)), up(np.ascontiguousarray(q["edge_corrected"], np.uint8))
    pts, ref = up(np.ascontiguousarray(q["points"], np.float32)), up(np.ascontiguousarray(q["point_ref"], np.int32))
    nk, ne, npt = len(q["Scw"]), len(q["edge_idx"]), len(q["points"])
    dev = torch.device("cuda", 0)
    So, To, Po = torch.zeros_like(Scw), torch.zeros((nk, 12), dtype=torch.float64, device=dev), torch.zeros_like(pts)
    nbytes = viorb_amd.essential_graph_workspace_bytes(nk, ne, npt) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    info = np.zeros(6)
    cfg = capi.EgConfig(20, int(q["fix_scale"]))
    torch.cuda.synchronize()
    return viorb_amd.lib().viorb_optimize_essential_graph_device(C.byref(cfg), ptr(Scw), ptr(Smeas), ptr(fixed), nk, ptr(ei), ptr(ec), ne, ptr(pts), ptr(ref), npt,
                                                                 ptr(So), ptr(To), ptr(Po), ptr(info), ptr(ws), nbytes, None)


def test_device_form_refuses_what_its_setup_kernel_flags():
    import viorb_amd
    from viorb_amd import capi
    p = EC.problem("points")
    E, nk = capi.ERR_INVALID_ARG, len(p["Scw"])
    assert _device_call(p) == capi.VIORB_OK
    bad = p["edge_idx"].copy(); bad[3, 1] = nk
    assert _device_call(p, edge_idx=bad) == E and b"Sim3 edge index" in viorb_amd.lib().viorb_last_error()
    bad = p["edge_idx"].copy(); bad[5, 1] = bad[5, 0]
    assert _device_call(p, edge_idx=bad) == E
    bad = p["Scw"].copy(); bad[4, 7] = 0.0
    assert _device_call(p, Scw=bad) == E and b"Sim3 pose" in viorb_amd.lib().viorb_last_error()
    bad = p["Smeas"].copy(); bad[2, 5] = np.nan
    assert _device_call(p, Smeas=bad) == E
    bad = p["point_ref"].copy(); bad[7] = nk
    assert _device_call(p, point_ref=bad) == E and b"point_ref" in viorb_amd.lib().viorb_last_error()
    assert _device_call(p, fixed=np.zeros(nk, np.uint8)) == E and b"no fixed vertex" in viorb_amd.lib().viorb_last_error()
    assert _device_call(p, ws_bytes=1024) == capi.ERR_CAPACITY               # a workspace that is too small, never a truncated solve
    assert _device_call(p) == capi.VIORB_OK                                  # and the library is usable after every refusal


def test_3511_free_vertices_are_refused_without_an_allocation_of_that_size():
    import torch
    import viorb_amd
    from viorb_amd import capi, ViorbError
    n = 3512
    S = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1.0]), (n, 1)); S[:, 4] = np.arange(n) * 0.1
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    ei = np.stack([np.arange(1, n), np.arange(0, n - 1)], 1).astype(np.int32)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(ViorbError) as e:
        viorb_amd.OptimizeEssentialGraph(S, S, fixed, ei, np.zeros(n - 1, np.uint8))
    assert e.value.code == capi.ERR_CAPACITY
    assert free0 - torch.cuda.mem_get_info()[0] < (1 << 30)                  # the system of 3511 vertices would take 4.8 GB
