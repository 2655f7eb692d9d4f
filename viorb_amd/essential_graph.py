"""The essential-graph optimisation of loop closing (Optimizer::OptimizeEssentialGraph) through the C ABI of include/viorb_essential_graph.h.
A problem is what synth.make_essential_graph_problem returns: Scw, Smeas [N,8] = r(x y z w) t s, fixed [N], edge_idx [E,2] = (vertex 0 =
i, vertex 1 = j), edge_corrected [E], points [P,3] float32, point_ref [P], fix_scale."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as up
from .global_ba import last_trials, INFO, _workspace  # noqa: F401

_f64 = lambda a: np.ascontiguousarray(a, np.float64)
_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)
_u8 = lambda a: np.ascontiguousarray(a, np.uint8)


def essential_graph_workspace_bytes(nk, n_edges, n_points):
    return int(lib().viorb_essential_graph_workspace_bytes(nk, n_edges, n_points))


def _arrays(Scw, Smeas, fixed, edge_idx, edge_corrected, points, point_ref):
    Scw, Smeas = _f64(Scw).reshape(-1, 8), _f64(Smeas).reshape(-1, 8)
    ei, ec = _i32(edge_idx).reshape(-1, 2), _u8(edge_corrected).reshape(-1)
    pts = _f32(points if points is not None else np.zeros((0, 3))).reshape(-1, 3)
    ref = _i32(point_ref if point_ref is not None else np.zeros(0)).reshape(-1)
    fixed = _u8(fixed)
    assert len(Scw) == len(Smeas) == len(fixed) and len(ei) == len(ec) and len(pts) == len(ref)
    return Scw, Smeas, fixed, ei, ec, pts, ref


def _result(So, To, Po, info):
    return dict(accepted=last_trials(), Scw_out=So, Tcw_out=To, points_out=Po, info=info, chi2_before=info[0], chi2_after=info[1], iterations=int(info[2]),
                trials=int(info[3]), final_lambda=info[4], failed_factorisations=int(info[5]))


def OptimizeEssentialGraph(Scw, Smeas, fixed, edge_idx, edge_corrected, points=None, point_ref=None, fix_scale=False, iterations=20):
    """viorb_optimize_essential_graph: host buffers in and out. Raises ViorbError on a status other than VIORB_OK."""
    Scw, Smeas, fixed, ei, ec, pts, ref = _arrays(Scw, Smeas, fixed, edge_idx, edge_corrected, points, point_ref)
    So, To, Po, info = np.zeros_like(Scw), np.zeros((len(Scw), 12)), np.zeros_like(pts), np.zeros(6)
    cfg = capi.EgConfig(int(iterations), int(bool(fix_scale)))
    check(lib().viorb_optimize_essential_graph(C.byref(cfg), ptr(Scw), ptr(Smeas), ptr(fixed), len(Scw), ptr(ei), ptr(ec), len(ei), ptr(pts), ptr(ref),
                                               len(pts), ptr(So), ptr(To), ptr(Po), ptr(info)))
    return _result(So, To, Po, info)


def OptimizeEssentialGraphDevice(Scw, Smeas, fixed, edge_idx, edge_corrected, points=None, point_ref=None, fix_scale=False, iterations=20, workspace=None):
    """viorb_optimize_essential_graph_device: the arrays are uploaded here as torch tensors on cuda:0 (a map that lives on the device);
    the results come back as numpy arrays. workspace: a capi.Workspace at least as large as the problem needs, used as it is; default: a
    fresh one, not cleared."""
    import torch
    dev = torch.device("cuda", 0)
    Scw, Smeas, fixed, ei, ec, pts, ref = _arrays(Scw, Smeas, fixed, edge_idx, edge_corrected, points, point_ref)
    t = dict(Scw=up(Scw), Smeas=up(Smeas), fixed=up(fixed), ei=up(ei if len(ei) else np.zeros((1, 2), np.int32)), ec=up(ec if len(ei) else np.zeros(1, np.uint8)),
             pts=up(pts if len(pts) else np.zeros((1, 3), np.float32)), ref=up(ref if len(pts) else np.zeros(1, np.int32)))
    So = torch.zeros_like(t["Scw"]); To = torch.zeros((len(Scw), 12), dtype=torch.float64, device=dev); Po = torch.zeros_like(t["pts"])
    nbytes = essential_graph_workspace_bytes(len(Scw), len(ei), len(pts))
    ws = _workspace(torch, dev, nbytes, workspace)
    info = np.zeros(6)
    cfg = capi.EgConfig(int(iterations), int(bool(fix_scale)))
    torch.cuda.synchronize()
    check(lib().viorb_optimize_essential_graph_device(C.byref(cfg), ptr(t["Scw"]), ptr(t["Smeas"]), ptr(t["fixed"]), len(Scw), ptr(t["ei"]), ptr(t["ec"]), len(ei),
                                                      ptr(t["pts"]), ptr(t["ref"]), len(pts), ptr(So), ptr(To), ptr(Po), ptr(info), ws.ptr, nbytes, None))
    return _result(So.cpu().numpy(), To.cpu().numpy(), Po.cpu().numpy()[:len(pts)], info)


def solve(prob, device=False, iterations=20, **kw):
    """A problem dictionary through the host or the device form (kw: workspace, device form only)."""
    f = OptimizeEssentialGraphDevice if device else OptimizeEssentialGraph
    return f(prob["Scw"], prob["Smeas"], prob["fixed"], prob["edge_idx"], prob["edge_corrected"], prob.get("points"), prob.get("point_ref"),
             fix_scale=prob["fix_scale"], iterations=iterations, **kw)


def debug_sim3_log(S8):
    """viorb_debug_sim3_log (no device): g2o's Sim3::log of r(x y z w) t s as omega, upsilon, sigma [7]."""
    out = np.zeros(7)
    check(lib().viorb_debug_sim3_log(ptr(_f64(S8)), ptr(out)))
    return out


def debug_edge(Si8, Sj8, C8, fix_scale=False, fixed_i=False, fixed_j=False):
    """viorb_debug_essential_graph_edge (no device): (e [7], Ji [7,7], Jj [7,7]) of one EdgeSim3 with g2o's numeric Jacobians."""
    e, Ji, Jj = np.zeros(7), np.zeros((7, 7)), np.zeros((7, 7))
    check(lib().viorb_debug_essential_graph_edge(ptr(_f64(Si8)), ptr(_f64(Sj8)), ptr(_f64(C8)), int(bool(fix_scale)), int(bool(fixed_i)), int(bool(fixed_j)),
                                                 ptr(e), ptr(Ji), ptr(Jj)))
    return e, Ji, Jj
