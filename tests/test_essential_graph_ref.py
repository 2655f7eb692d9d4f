"""CPU tests of the essential-graph solve (no GPU): the host hooks viorb_debug_sim3_log / viorb_debug_essential_graph_edge
(essential_graph_core.h compiled for the host) against the numpy checker tests/essential_graph_ref.py; the measurement run that fixes
the tolerances of tests/test_gpu_essential_graph.py (the checker's two Jacobian modes over tests/essential_graph_cases.py); the
conditions the accept / reject comparison of the GPU test rests on, asserted on the checker alone; the refusals of the host form that
need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import viorb_amd
from viorb_amd import capi, synth
from viorb_amd import essential_graph as EG
from viorb_amd.capi import ptr

import essential_graph_ref as ER
import essential_graph_cases as EC
from sim3_ref import sim3_exp, sim3_pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def _S(angle, sigma, axis=(0.3, -0.5, 0.8), t=(0.7, -1.3, 2.1)):
    return np.concatenate([_quat(axis, angle), t, [np.exp(sigma)]])


def test_entry_points_are_declared_exported_and_mirrored():
    L = viorb_amd.lib()
    names = {"viorb_essential_graph_workspace_bytes", "viorb_optimize_essential_graph", "viorb_optimize_essential_graph_device", "viorb_debug_sim3_log",
             "viorb_debug_essential_graph_edge"}
    inc = os.path.join(ROOT, "include")
    assert '#include "viorb_essential_graph.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_essential_graph.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == names == set(capi.SIGNATURES_ESSENTIAL_GRAPH)
    for n in names:
        assert hasattr(L, n) and len(capi.SIGNATURES_ESSENTIAL_GRAPH[n][1]) == counts[n], n
    assert not set(capi.SIGNATURES_ESSENTIAL_GRAPH) & set(capi.SIGNATURES)
    assert C.sizeof(capi.EgConfig) == 8
    assert viorb_amd.OptimizeEssentialGraph is EG.OptimizeEssentialGraph
    assert L.viorb_essential_graph_workspace_bytes(0, 0, 0) == 0 and L.viorb_essential_graph_workspace_bytes(10, 30, 5) > 0


# d = cos(angle) of a unit quaternion: 1 - 1e-5 lies at angle 4.4721e-3; sigma's threshold is 1e-5 itself
ANGLES = (0.0, 1e-4, 4.46e-3, 4.48e-3, 0.8, 2.5)
SIGMAS = (0.0, 0.9e-5, -0.9e-5, 1.1e-5, -1.1e-5, 0.35, -0.6)


def test_sim3_log_equals_the_checker_in_all_four_branches_and_at_both_sides_of_both_thresholds():
    seen = set()
    for a in ANGLES:
        for sg in SIGMAS:
            S = _S(a, sg)
            seen.add(ER.log_branch(S))
            got, ref = EG.debug_sim3_log(S), ER.sim3_log(S)
            # In the branch |sigma| >= eps, d > 1 - eps g2o's B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 is about 1 / sigma^3 (restated as it
            # stands), so W = ... + B Omega^2 + C I carries entries of size theta^2 / |sigma|^3 next to C = 1: the solve loses that factor
            # of its sixteen digits, in g2o as here, and a last bit in log or acos moves the result by as much.
            cond = a * a / abs(sg) ** 3 if ER.log_branch(S) == (False, True) else 0.0
            assert np.abs(got - ref).max() <= (1e-12 + 1e-14 * cond) * max(1.0, np.abs(ref).max()), (a, sg, got, ref)
            assert got[6] == np.log(S[7])
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    # both sides of both thresholds were really taken
    assert ER.log_branch(_S(4.46e-3, 0.9e-5)) == (True, True) and ER.log_branch(_S(4.48e-3, 1.1e-5)) == (False, False)


def test_exp_of_log_is_the_identity_to_rounding_also_near_pi():
    rng = np.random.default_rng(5)
    for k in range(40):
        u = np.concatenate([rng.normal(size=3) * 0.6, rng.normal(size=3) * 2, [rng.normal() * 0.4]])
        if k % 4 == 1:
            u[6] = 0.5e-5 * rng.normal()
        if k % 4 == 2:
            u[:3] *= 1e-6
        S = sim3_pack(sim3_exp(u))
        back = sim3_pack(sim3_exp(EG.debug_sim3_log(S)))
        if back[3] * S[3] < 0:
            back[:4] = -back[:4]
        assert np.abs(back - S).max() <= 1e-12 * max(1.0, np.abs(S).max()), (u, back - S)
    # a rotation near pi: deltaR is small and divided by sqrt(1 - d^2), which costs (pi - theta)^-2 in relative accuracy
    for gap in (1e-2, 1e-3):
        S = _S(np.pi - gap, 0.2)
        got, ref = EG.debug_sim3_log(S), ER.sim3_log(S)
        assert np.isfinite(got).all() and abs(np.linalg.norm(got[:3]) - (np.pi - gap)) < 1e-9 / gap ** 2 * 1e-3
        assert np.abs(got - ref).max() <= 1e-9
        back = sim3_pack(sim3_exp(got))
        if back[3] * S[3] < 0:
            back[:4] = -back[:4]
        assert np.abs(back - S).max() <= 1e-8


def test_edge_hook_equals_the_checkers_numeric_jacobians():
    p = EC.problem("n10_free")
    Cm = ER.measurements(p)
    rng = np.random.default_rng(7)
    for k in rng.permutation(len(Cm))[:6]:
        i, j = p["edge_idx"][k]
        for fs in (False, True):
            for fi, fj in ((False, False), (True, False), (False, True), (True, True)):
                e, Ji, Jj = EG.debug_edge(p["Scw"][i], p["Scw"][j], Cm[k], fs, fi, fj)
                e2, Ji2, Jj2 = ER.one_edge(p["Scw"][i], p["Scw"][j], Cm[k], fs, fi, fj)
                assert np.abs(e - e2).max() <= 1e-13 * max(1.0, np.abs(e2).max())
                # one differing last bit in an error is 1e-16 / (2 delta) = 5e-8 in a column
                assert np.abs(Ji - Ji2).max() <= 1e-6 * max(1.0, np.abs(Ji2).max()) and np.abs(Jj - Jj2).max() <= 1e-6 * max(1.0, np.abs(Jj2).max())
                assert (Ji == 0).all() if fi else np.abs(Ji).max() > 0.1          # a fixed side gets no Jacobian
                assert (Jj == 0).all() if fj else np.abs(Jj).max() > 0.1
                if fs:
                    assert (Ji[:, 6] == 0).all() and (Jj[:, 6] == 0).all()         # exactly zero, not small
                elif not fi:
                    assert np.abs(Ji[:, 6]).max() > 1e-3


def test_measurement_run_fixes_the_tolerances_and_the_decidable_prefix_conditions_hold():
    """Re-measures EG_S_DEV, EG_T_DEV, EG_P_DEV, EG_CHI_DEV (the deviation of the checker's two Jacobian modes) on every run, and asserts
    on the checker alone what the accept / reject comparison of the GPU test needs: in every case with a non-zero chi2 the decidable
    prefix covers at least the first three iterations, and at least one case has a rejected trial inside it."""
    floor = ER.BAND_FACTOR * ER.EG_CHI_DEV
    worst = np.zeros(4)
    rejected_inside = []
    for name in EC.NAMES:
        a, b = EC.reference(name), EC.reference(name, "numeric2")
        dev = np.array(ER.deviations(a, b))
        worst = np.maximum(worst, dev)
        k = ER.decidable_prefix(a, floor)
        its_in = a["iteration_of"][k - 1] + 1 if k else 0
        print("%-20s chi2 %.4e -> %.4e its %d trials %d prefix %d trials / %d its  dev S %.2e T %.2e P %.2e chi %.2e  %s" % (
            name, a["info"][0], a["info"][1], a["info"][2], a["info"][3], k, its_in, dev[0], dev[1], dev[2], dev[3], "".join("1" if x else "0" for x in a["accepted"])))
        assert a["accepted"][:k] == b["accepted"][:k], name                      # the other evaluation order decides the prefix alike
        if name in EC.ZERO_CHI2:
            assert a["info"][0] < ER.EG_CHI_ABS and a["info"][1] < ER.EG_CHI_ABS and k == 0
            continue
        assert its_in >= 3, (name, its_in, a["rel_change"])
        if not all(a["accepted"][:k]):
            rejected_inside.append(name)
    print("measured  EG_S_DEV %.2e  EG_T_DEV %.2e  EG_P_DEV %.2e  EG_CHI_DEV %.2e" % tuple(worst))
    assert rejected_inside, "no case has a rejected trial inside its decidable prefix"
    const = np.array([ER.EG_S_DEV, ER.EG_T_DEV, ER.EG_P_DEV, ER.EG_CHI_DEV])
    assert (worst < const).all(), (worst, const)
    assert (const <= 4 * worst).all(), ("a constant is far above what is measured", worst, const)
    assert any(len(EC.problem(n)["points"]) == 200 and (EC.problem(n)["point_ref"] < 0).any() for n in EC.NAMES)


def _call(p, **over):
    q = dict(p); q.update(over)
    Scw, Smeas = np.ascontiguousarray(q["Scw"], np.float64), np.ascontiguousarray(q["Smeas"], np.float64)
    fixed = np.ascontiguousarray(q["fixed"], np.uint8)
    ei, ec = np.ascontiguousarray(q["edge_idx"], np.int32), np.ascontiguousarray(q["edge_corrected"], np.uint8)
    pts, ref = np.ascontiguousarray(q["points"], np.float32), np.ascontiguousarray(q["point_ref"], np.int32)
    So, To, Po, info = np.zeros_like(Scw), np.zeros((len(Scw), 12)), np.zeros((max(len(pts), 1), 3), np.float32), np.zeros(6)
    cfg = capi.EgConfig(int(q.get("iterations", 20)), int(q["fix_scale"]))
    return viorb_amd.lib().viorb_optimize_essential_graph(C.byref(cfg), ptr(Scw), ptr(Smeas), ptr(fixed), len(Scw), ptr(ei), ptr(ec), len(ei), ptr(pts), ptr(ref),
                                                          len(pts), ptr(So), ptr(To), ptr(Po), ptr(info))


def test_host_form_refuses_bad_arguments_before_any_device_call():
    p = EC.problem("points")
    E = capi.ERR_INVALID_ARG
    nk = len(p["Scw"])
    bad = p["edge_idx"].copy(); bad[3, 1] = nk
    assert _call(p, edge_idx=bad) == E                                      # edge index out of range
    bad = p["edge_idx"].copy(); bad[3, 0] = -1
    assert _call(p, edge_idx=bad) == E
    bad = p["edge_idx"].copy(); bad[5, 1] = bad[5, 0]
    assert _call(p, edge_idx=bad) == E                                      # i == j
    for arr in ("Scw", "Smeas"):
        bad = p[arr].copy(); bad[4, 7] = 0.0
        assert _call(p, **{arr: bad}) == E                                  # scale <= 0
        bad = p[arr].copy(); bad[4, 7] = -1.0
        assert _call(p, **{arr: bad}) == E
        bad = p[arr].copy(); bad[2, 5] = np.nan
        assert _call(p, **{arr: bad}) == E                                  # a pose that is not finite
        bad = p[arr].copy(); bad[2, 1] = np.inf
        assert _call(p, **{arr: bad}) == E
    bad = p["point_ref"].copy(); bad[7] = nk
    assert _call(p, point_ref=bad) == E                                     # point_ref outside -1 .. nk - 1
    bad = p["point_ref"].copy(); bad[7] = -2
    assert _call(p, point_ref=bad) == E
    assert _call(p, fixed=np.zeros(nk, np.uint8)) == E                      # no fixed vertex: the gauge is not held
    assert b"no fixed vertex" in viorb_amd.lib().viorb_last_error()
    assert _call(p, iterations=-1) == E and _call(p, fix_scale=2) == E


def test_3511_free_vertices_are_refused_by_the_size_check_alone():
    """More than 3510 free key frames (order 24577) is VIORB_ERR_CAPACITY from the host form's count, before a device is looked for and
    with nothing of that size allocated; 3510 passes that check (and then needs a device)."""
    n = 3512
    S = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1.0]), (n, 1))
    S[:, 4] = np.arange(n) * 0.1
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    ei = np.stack([np.arange(1, n), np.arange(0, n - 1)], 1).astype(np.int32)
    p = dict(Scw=S, Smeas=S, fixed=fixed, edge_idx=ei, edge_corrected=np.zeros(n - 1, np.uint8), points=np.zeros((0, 3), np.float32), point_ref=np.zeros(0, np.int32),
             fix_scale=False)
    assert _call(p) == capi.ERR_CAPACITY
    assert b"3511 free key frames" in viorb_amd.lib().viorb_last_error()


@pytest.mark.parametrize("N", [2, 12])
def test_synthetic_problem_has_the_edges_the_reference_builds(N):
    p = synth.make_essential_graph_problem(3, N=N, duplicate_pair=N > 2, n_points=20)
    ei, ec = p["edge_idx"], p["edge_corrected"]
    assert p["fixed"][0] == 1 and p["fixed"].sum() == 1 and (ei[:, 0] != ei[:, 1]).all()
    assert {(k, k - 1) for k in range(1, N)} <= {tuple(e) for e, c in zip(ei, ec) if c == 0}          # the spanning tree
    assert ec.sum() >= 1 and (p["Scw"][N - 1] != p["Smeas"][N - 1]).any() and (p["Scw"][0] == p["Smeas"][0]).all()
    pairs = [tuple(sorted(e)) for e in ei]
    assert len(pairs) > len(set(pairs))                                                                 # a pair joined twice
