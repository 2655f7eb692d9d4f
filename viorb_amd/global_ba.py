"""Global bundle adjustment with NavState IMU edges (Optimizer::GlobalBundleAdjustmentNavState) and the vision-only one over SE3 poses
(Optimizer::BundleAdjustment, GlobalBundleAdjustmentSE3 below) through the C ABI of include/viorb.h.
A problem is what synth.make_global_ba_problem returns: kfs [N,22] in an order with prev[i] < i, prev [N], fixed [N], preint [N,142]
(row i = the interval ending at key frame i), points [P,3], edge_idx [E,2] = (point, key frame) sorted by point, edge_obs [E,3] = u v
invSigma2, gw [3], cam [16]."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as up

_f64 = lambda a: np.ascontiguousarray(a, np.float64)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)
INFO = ("chi2_before", "chi2_after", "iterations", "trials", "lambda", "failed_factorisations")


def last_trials():
    """viorb_debug_gba_last_trials: accept (True) / reject (False) of every trial of this thread's last solve."""
    a, n = np.zeros(256, np.uint8), C.c_int(0)
    check(lib().viorb_debug_gba_last_trials(ptr(a), len(a), C.byref(n)))
    return [bool(v) for v in a[:min(n.value, len(a))]]


def _result(ko, po, inc, info):
    return dict(accepted=last_trials(), kfs=ko, points=po, point_included=inc, info=info, chi2_before=info[0], chi2_after=info[1], iterations=int(info[2]),
                trials=int(info[3]), final_lambda=info[4], failed_factorisations=int(info[5]))


def _workspace(torch, dev, nbytes, given):
    """The caller's capi.Workspace when it gave one, else a fresh one of nbytes; its contents stay as they are either way."""
    if given is None:
        return capi.Workspace(torch, dev, nbytes, fill=None)
    assert given.fits(nbytes)
    return given


def gba_workspace_bytes(nk, n_points, n_edges):
    return int(lib().viorb_global_ba_navstate_workspace_bytes(nk, n_points, n_edges))


def GlobalBundleAdjustmentNavState(kfs, prev, fixed, preint, points, edge_idx, edge_obs, gw, cam, iterations=10, robust=False, stop=None):
    """viorb_global_ba_navstate: host buffers in and out. stop: None or an int32 array of one element (pbStopFlag; another thread may
    raise it while the call runs). Raises ViorbError on a status other than VIORB_OK."""
    kfs = _f64(kfs).reshape(-1, 22); preint = _f64(preint).reshape(-1, 142); points = _f64(points).reshape(-1, 3)
    ei = _i32(edge_idx).reshape(-1, 2); eo = _f64(edge_obs).reshape(-1, 3)
    prev = _i32(prev); fixed = np.ascontiguousarray(fixed, np.uint8)
    assert len(prev) == len(fixed) == len(preint) == len(kfs) and len(ei) == len(eo)
    ko, po, inc, info = np.zeros_like(kfs), np.zeros_like(points), np.zeros(max(len(points), 1), np.uint8), np.zeros(6)
    cfg = capi.GbaConfig(int(iterations), int(bool(robust)))
    check(lib().viorb_global_ba_navstate(C.byref(cfg), ptr(kfs), len(kfs), ptr(prev), ptr(fixed), ptr(preint), ptr(points), len(points),
                                         ptr(ei), ptr(eo), len(ei), ptr(_f64(gw)), ptr(_f64(cam)), ptr(stop) if stop is not None else None,
                                         ptr(ko), ptr(po), ptr(inc), ptr(info)))
    return _result(ko, po, inc[:len(points)], info)


def GlobalBundleAdjustmentNavStateDevice(kfs, prev, fixed, preint, points, edge_idx, edge_obs, gw, cam, iterations=10, robust=False, stop=None, workspace=None):
    """viorb_global_ba_navstate_device: the arrays are uploaded here as torch tensors on cuda:0 (the mapping thread's device-resident
    form); the results come back as numpy arrays. workspace: a capi.Workspace at least as large as the problem needs, used as it is (a
    caller that keeps one allocation across solves); default: a fresh one, not cleared."""
    import torch
    dev = torch.device("cuda", 0)
    kfs = _f64(kfs).reshape(-1, 22); points = _f64(points).reshape(-1, 3); ei = _i32(edge_idx).reshape(-1, 2)
    t = dict(kfs=up(kfs), prev=up(_i32(prev)), fixed=up(np.ascontiguousarray(fixed, np.uint8)), preint=up(_f64(preint).reshape(-1, 142)),
             points=up(points if len(points) else np.zeros((1, 3))), ei=up(ei if len(ei) else np.zeros((1, 2), np.int32)),
             eo=up(_f64(edge_obs).reshape(-1, 3) if len(ei) else np.zeros((1, 3))))
    ko, po = torch.zeros_like(t["kfs"]), torch.zeros_like(t["points"])
    inc = torch.zeros(max(len(points), 1), dtype=torch.uint8, device=dev)
    nbytes = gba_workspace_bytes(len(kfs), len(points), len(ei))
    ws = _workspace(torch, dev, nbytes, workspace)
    info = np.zeros(6)
    cfg = capi.GbaConfig(int(iterations), int(bool(robust)))
    torch.cuda.synchronize()
    check(lib().viorb_global_ba_navstate_device(C.byref(cfg), ptr(t["kfs"]), len(kfs), ptr(t["prev"]), ptr(t["fixed"]), ptr(t["preint"]), ptr(t["points"]),
                                                len(points), ptr(t["ei"]), ptr(t["eo"]), len(ei), ptr(_f64(gw)), ptr(_f64(cam)),
                                                ptr(stop) if stop is not None else None, ptr(ko), ptr(po), ptr(inc), ptr(info), ws.ptr, nbytes, None))
    return _result(ko.cpu().numpy(), po.cpu().numpy()[:len(points)], inc.cpu().numpy()[:len(points)], info)


def gba_se3_workspace_bytes(nk, n_points, n_edges):
    return int(lib().viorb_global_ba_se3_workspace_bytes(nk, n_points, n_edges))


def GlobalBundleAdjustmentSE3(kfs, fixed, points, edge_idx, edge_obs, intr5, iterations=10, robust=False, stop=None):
    """viorb_global_ba_se3 (Optimizer::BundleAdjustment): host buffers in and out. kfs [N,7] = qx qy qz qw tx ty tz of Tcw, fixed [N],
    points [P,3], edge_idx [E,2] = (point, key frame) sorted by point, edge_obs [E,4] = u v uRight (< 0: monocular) invSigma2, intr5 = fx
    fy cx cy bf. stop as GlobalBundleAdjustmentNavState. Returns the same result dictionary."""
    kfs = _f64(kfs).reshape(-1, 7); points = _f64(points).reshape(-1, 3)
    ei = _i32(edge_idx).reshape(-1, 2); eo = _f64(edge_obs).reshape(-1, 4)
    fixed = np.ascontiguousarray(fixed, np.uint8)
    assert len(fixed) == len(kfs) and len(ei) == len(eo)
    ko, po, inc, info = np.zeros_like(kfs), np.zeros_like(points), np.zeros(max(len(points), 1), np.uint8), np.zeros(6)
    cfg = capi.GbaConfig(int(iterations), int(bool(robust)))
    check(lib().viorb_global_ba_se3(C.byref(cfg), ptr(kfs), len(kfs), ptr(fixed), ptr(points), len(points), ptr(ei), ptr(eo), len(ei),
                                    ptr(_f64(intr5)), ptr(stop) if stop is not None else None, ptr(ko), ptr(po), ptr(inc), ptr(info)))
    return _result(ko, po, inc[:len(points)], info)


def GlobalBundleAdjustmentSE3Device(kfs, fixed, points, edge_idx, edge_obs, intr5, iterations=10, robust=False, stop=None, workspace=None):
    """viorb_global_ba_se3_device: the arrays are uploaded here as torch tensors on cuda:0; the results come back as numpy arrays.
    workspace as GlobalBundleAdjustmentNavStateDevice."""
    import torch
    dev = torch.device("cuda", 0)
    kfs = _f64(kfs).reshape(-1, 7); points = _f64(points).reshape(-1, 3); ei = _i32(edge_idx).reshape(-1, 2)
    t = dict(kfs=up(kfs), fixed=up(np.ascontiguousarray(fixed, np.uint8)), points=up(points if len(points) else np.zeros((1, 3))),
             ei=up(ei if len(ei) else np.zeros((1, 2), np.int32)), eo=up(_f64(edge_obs).reshape(-1, 4) if len(ei) else np.zeros((1, 4))))
    ko, po = torch.zeros_like(t["kfs"]), torch.zeros_like(t["points"])
    inc = torch.zeros(max(len(points), 1), dtype=torch.uint8, device=dev)
    nbytes = gba_se3_workspace_bytes(len(kfs), len(points), len(ei))
    ws = _workspace(torch, dev, nbytes, workspace)
    info = np.zeros(6)
    cfg = capi.GbaConfig(int(iterations), int(bool(robust)))
    torch.cuda.synchronize()
    check(lib().viorb_global_ba_se3_device(C.byref(cfg), ptr(t["kfs"]), len(kfs), ptr(t["fixed"]), ptr(t["points"]), len(points), ptr(t["ei"]), ptr(t["eo"]),
                                           len(ei), ptr(_f64(intr5)), ptr(stop) if stop is not None else None, ptr(ko), ptr(po), ptr(inc), ptr(info),
                                           ws.ptr, nbytes, None))
    return _result(ko.cpu().numpy(), po.cpu().numpy()[:len(points)], inc.cpu().numpy()[:len(points)], info)


def debug_se3_edge(kf7, pt3, obs4, intr5):
    """viorb_debug_gba_se3_edge (no device): (dimension, e [3], Jp [3,3], Jk [3,6]) of one edge."""
    e, Jp, Jk = np.zeros(3), np.zeros((3, 3)), np.zeros((3, 6))
    dim = lib().viorb_debug_gba_se3_edge(ptr(_f64(kf7)), ptr(_f64(pt3)), ptr(_f64(obs4)), ptr(_f64(intr5)), ptr(e), ptr(Jp), ptr(Jk))
    return dim, e, Jp, Jk


def debug_cholesky(A):
    """viorb_debug_gba_cholesky: (L, ok) of the blocked device Cholesky of the symmetric matrix A (its lower triangle is read)."""
    A = _f64(A); n = len(A)
    L, ok = np.zeros((n, n)), C.c_int32(0)
    check(lib().viorb_debug_gba_cholesky(ptr(A), n, ptr(L), C.byref(ok)))
    return L, bool(ok.value)
