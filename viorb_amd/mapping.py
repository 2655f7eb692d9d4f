"""Map-point creation (LocalMapping::CreateNewMapPoints, MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth) through
the C ABI of include/viorb.h. A key frame is a dict of flat arrays: kps (KP_DTYPE, undistorted), desc [n,32], hp (has map point),
ur (mvuRight), depth (mvDepth), xy_dist [n,2] (the distorted mvKeys), node [n], pose12 (Rcw tcw), Ow [3]; a neighbour adds F12 [3,3],
median_depth and kf2_first. The camera is a dict(intr4, mb, mbf, scale_factor, sf, level_sigma2)."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as _up

_u8 = lambda a: np.ascontiguousarray(a, np.uint8)
_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)


def mapping_camera(cam):
    """viorb_mapping_camera from dict(intr4, mb, mbf, scale_factor, sf, level_sigma2)."""
    c = capi.MappingCamera()
    c.fx, c.fy, c.cx, c.cy = [float(v) for v in cam["intr4"]]
    c.mb, c.mbf, c.scale_factor = float(cam["mb"]), float(cam["mbf"]), float(cam["scale_factor"])
    sf, s2 = _f32(cam["sf"]), _f32(cam["level_sigma2"])
    c.nlevels = len(sf)
    for i in range(len(sf)):
        c.scale_factors[i] = sf[i]; c.level_sigma2[i] = s2[i]
    return c


def TriangulatePairs(cam, kf1, kf2, match12):
    """The per-pair loop of CreateNewMapPoints (reference src/LocalMapping.cc:1312-1464), host buffers: (accept [n1] u8, Pw [n1,3],
    reason [n1] u8)."""
    c = mapping_camera(cam)
    k1, k2 = np.ascontiguousarray(kf1["kps"], capi.KP_DTYPE), np.ascontiguousarray(kf2["kps"], capi.KP_DTYPE)
    n1 = len(k1)
    acc, rea, Pw = np.zeros(max(n1, 1), np.uint8), np.full(max(n1, 1), 255, np.uint8), np.zeros((max(n1, 1), 3), np.float32)
    check(lib().viorb_triangulate_pairs(C.byref(c), ptr(k1), ptr(_f32(kf1["xy_dist"])), ptr(_f32(kf1["ur"])), ptr(_f32(kf1["depth"])), n1, ptr(_f32(kf1["pose12"])),
                                        ptr(_f32(kf1["Ow"])), ptr(k2), ptr(_f32(kf2["xy_dist"])), ptr(_f32(kf2["ur"])), ptr(_f32(kf2["depth"])), len(k2),
                                        ptr(_f32(kf2["pose12"])), ptr(_f32(kf2["Ow"])), ptr(_i32(match12)), ptr(acc), ptr(Pw), ptr(rea)))
    return acc[:n1], Pw[:n1], rea[:n1]


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _stack(arrs, cap, dtype, tail=()):
    out = np.zeros((len(arrs), cap) + tuple(tail), dtype)
    for b, a in enumerate(arrs):
        out[b, :len(a)] = a
    return out


def TriangulatePairsBatch(cam, kf1s, kf2s, match12s):
    """viorb_triangulate_pairs_device for a batch of key-frame pairs (uploaded here, one launch): list of (accept, Pw, reason)."""
    torch, dev = _dev()
    c = mapping_camera(cam)
    B = len(kf1s)
    cap = max(max(len(k["kps"]) for k in kf1s), max(len(k["kps"]) for k in kf2s), 1)
    def side(kfs):
        return [_up(_stack([k["kps"] for k in kfs], cap, capi.KP_DTYPE)), _up(_stack([k["xy_dist"] for k in kfs], cap, np.float32, (2,))),
                _up(_stack([k["ur"] for k in kfs], cap, np.float32)), _up(_stack([k["depth"] for k in kfs], cap, np.float32)),
                _up(np.stack([_f32(k["pose12"]) for k in kfs])), _up(np.stack([_f32(k["Ow"]) for k in kfs]))]
    a, b = side(kf1s), side(kf2s)
    n1 = _up(np.array([len(k["kps"]) for k in kf1s], np.int32))
    m = _up(_stack([_i32(x) for x in match12s], cap, np.int32))              # entries beyond n1[b] are not read
    acc = torch.zeros((B, cap), dtype=torch.uint8, device=dev); rea = torch.zeros((B, cap), dtype=torch.uint8, device=dev)
    Pw = torch.zeros((B, cap, 3), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lib().viorb_triangulate_pairs_device(C.byref(c), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(n1), ptr(a[4]), ptr(a[5]), ptr(b[0]), ptr(b[1]), ptr(b[2]),
                                               ptr(b[3]), ptr(b[4]), ptr(b[5]), ptr(m), cap, B, ptr(acc), ptr(Pw), ptr(rea), C.c_void_p(st)))
    torch.cuda.synchronize(dev)
    acc, rea, Pw = acc.cpu().numpy(), rea.cpu().numpy(), Pw.cpu().numpy()
    return [(acc[i, :len(k["kps"])], Pw[i, :len(k["kps"])], rea[i, :len(k["kps"])]) for i, k in enumerate(kf1s)]


def _csr(obs):
    start = np.zeros(len(obs) + 1, np.int32)
    for p, o in enumerate(obs):
        start[p + 1] = start[p] + len(o)
    flat = np.array([e for o in obs for e in o], np.int32).reshape(-1, 2)
    return start, np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])


def _kf_pool(kf_desc, kf_octave):
    base = np.zeros(len(kf_desc), np.int64)
    for k in range(1, len(kf_desc)):
        base[k] = base[k - 1] + len(kf_desc[k - 1])
    return base, _u8(np.concatenate([_u8(d).reshape(-1, 32) for d in kf_desc])), _i32(np.concatenate([_i32(o) for o in kf_octave]))


def MapPointUpdate(cam, obs, ref_obs, Pw, kf_desc, kf_octave, kf_Ow, device=False):
    """MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (reference src/MapPoint.cc:249-314, :337-378) for len(obs) points:
    obs[p] = [(key frame, feature), ...] in the order mObservations is iterated, ref_obs[p] = which of them is mpRefKF's.
    Returns (pts_desc [np,32], best_obs [np], pts_f [np,8]). device=True goes through the device form with torch tensors."""
    c = mapping_camera(cam)
    start, okf, ofe = _csr(obs)
    base, drows, orows = _kf_pool(kf_desc, kf_octave)
    npts = len(obs)
    Pw = _f32(Pw).reshape(-1, 3); Ow = _f32(np.stack([_f32(o) for o in kf_Ow])); ro = _i32(ref_obs)
    if not device:
        pd, bo, pf = np.zeros((max(npts, 1), 32), np.uint8), np.zeros(max(npts, 1), np.int32), np.zeros((max(npts, 1), 8), np.float32)
        check(lib().viorb_map_points_update(ptr(start), ptr(okf), ptr(ofe), ptr(ro), ptr(Pw), npts, ptr(base), ptr(Ow), len(base), ptr(drows), ptr(orows),
                                            len(orows), C.byref(c), ptr(pd), ptr(bo), ptr(pf)))
        return pd[:npts], bo[:npts], pf[:npts]
    torch, dev = _dev()
    t = [_up(x) for x in (start, okf if len(okf) else np.zeros(1, np.int32), ofe if len(ofe) else np.zeros(1, np.int32), ro, Pw, base, Ow, drows, orows)]
    pd = torch.zeros((npts, 32), dtype=torch.uint8, device=dev); bo = torch.zeros(npts, dtype=torch.int32, device=dev)
    pf = torch.zeros((npts, 8), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lib().viorb_map_points_update_device(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(t[4]), npts, ptr(t[5]), ptr(t[6]), len(base), ptr(t[7]), ptr(t[8]),
                                               len(orows), C.byref(c), ptr(pd), ptr(bo), ptr(pf), C.c_void_p(st)))
    torch.cuda.synchronize(dev)
    return pd.cpu().numpy(), bo.cpu().numpy(), pf.cpu().numpy()


class CreateNewMapPoints:
    """viorb_create_new_map_points_device for a batch of streams: problems[b] = dict(kf1, neigh[<= J]). The key frames are uploaded
    once; __call__(j_begin, j_end) enqueues that range of neighbours on the current torch stream (has_point1, n_new and status carry
    over between calls); results() downloads. No host synchronisation happens inside __call__."""

    def __init__(self, cam, problems, J, pcap, monocular=True, cap=None):
        torch, dev = _dev()
        self.cam, self.J, self.pcap, self.monocular, self.B = mapping_camera(cam), J, pcap, int(monocular), len(problems)
        kf1s = [p["kf1"] for p in problems]
        cap = cap or max([len(k["kps"]) for k in kf1s] + [len(n["kps"]) for p in problems for n in p["neigh"]] + [1])
        self.cap = cap
        B = self.B
        self.n1s = [len(k["kps"]) for k in kf1s]
        g = lambda key, dt, tail=(): _up(_stack([k[key] for k in kf1s], cap, dt, tail))
        self.k1, self.d1, self.hp1, self.ur1 = g("kps", capi.KP_DTYPE), g("desc", np.uint8, (32,)), g("hp", np.uint8), g("ur", np.float32)
        self.dep1, self.xy1, self.node1 = g("depth", np.float32), g("xy_dist", np.float32, (2,)), g("node", np.int32)
        self.n1 = _up(np.array(self.n1s, np.int32))
        self.T1 = _up(np.stack([_f32(k["pose12"]) for k in kf1s])); self.O1 = _up(np.stack([_f32(k["Ow"]) for k in kf1s]))
        def g2(key, dt, tail=()):
            out = np.zeros((B, J, cap) + tuple(tail), dt)
            for b, p in enumerate(problems):
                for j, n in enumerate(p["neigh"][:J]):
                    out[b, j, :len(n[key])] = n[key]
            return _up(out)
        self.k2, self.d2, self.hp2, self.ur2 = g2("kps", capi.KP_DTYPE), g2("desc", np.uint8, (32,)), g2("hp", np.uint8), g2("ur", np.float32)
        self.dep2, self.xy2, self.node2 = g2("depth", np.float32), g2("xy_dist", np.float32, (2,)), g2("node", np.int32)
        def s2(get, dt, tail=(), fill=0):
            out = np.full((B, J) + tuple(tail), fill, dt)
            for b, p in enumerate(problems):
                for j, n in enumerate(p["neigh"][:J]):
                    out[b, j] = get(n)
            return _up(out)
        self.n2 = s2(lambda n: len(n["kps"]), np.int32)
        self.T2, self.O2 = s2(lambda n: _f32(n["pose12"]), np.float32, (12,)), s2(lambda n: _f32(n["Ow"]), np.float32, (3,))
        self.F12 = s2(lambda n: _f32(n["F12"]).ravel(), np.float32, (9,))
        self.md2, self.kf2_first = s2(lambda n: n["median_depth"], np.float32, (), 1), s2(lambda n: n["kf2_first"], np.uint8)
        self.n_neigh = _up(np.array([min(len(p["neigh"]), J) for p in problems], np.int32))
        self.new_idx = torch.full((B, pcap, 3), -1, dtype=torch.int32, device=dev)
        self.new_pts_f = torch.zeros((B, pcap, 8), dtype=torch.float32, device=dev)
        self.new_desc = torch.zeros((B, pcap, 32), dtype=torch.uint8, device=dev)
        self.n_new = torch.zeros(B, dtype=torch.int32, device=dev); self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.ws_bytes = lib().viorb_create_new_map_points_workspace_bytes(cap, B)
        self.ws = capi.Workspace(torch, dev, self.ws_bytes)         # may be re-filled or replaced by a larger one between calls

    def __call__(self, j_begin=0, j_end=None):
        torch, dev = _dev()
        j_end = self.J if j_end is None else j_end
        st = torch.cuda.current_stream(dev).cuda_stream
        check(lib().viorb_create_new_map_points_device(
            C.byref(self.cam), self.monocular, ptr(self.k1), ptr(self.d1), ptr(self.hp1), ptr(self.ur1), ptr(self.dep1), ptr(self.xy1), ptr(self.node1), ptr(self.n1),
            ptr(self.T1), ptr(self.O1), ptr(self.k2), ptr(self.d2), ptr(self.hp2), ptr(self.ur2), ptr(self.dep2), ptr(self.xy2), ptr(self.node2), ptr(self.n2),
            ptr(self.T2), ptr(self.O2), ptr(self.F12), ptr(self.md2), ptr(self.kf2_first), ptr(self.n_neigh), self.J, j_begin, j_end, self.cap, self.B, self.pcap,
            ptr(self.new_idx), ptr(self.new_pts_f), ptr(self.new_desc), ptr(self.n_new), ptr(self.status), self.ws.ptr, self.ws_bytes, C.c_void_p(st)))
        return self

    def results(self):
        torch, dev = _dev()
        torch.cuda.synchronize(dev)
        n = self.n_new.cpu().numpy(); hp = self.hp1.cpu().numpy()
        idx, pf, de = self.new_idx.cpu().numpy(), self.new_pts_f.cpu().numpy(), self.new_desc.cpu().numpy()
        return [dict(n_new=int(n[b]), status=int(self.status[b].item()), new_idx=idx[b, :n[b]], new_pts_f=pf[b, :n[b]], new_desc=de[b, :n[b]],
                     has_point1=hp[b, :self.n1s[b]], new_idx_all=idx[b]) for b in range(self.B)]


def CreateNewMapPointsHost(cam, problem, pcap, monocular=True):
    """viorb_create_new_map_points: the host-buffer drop-in for one key frame and its neighbours.
    Returns dict(status, n_new, new_idx, new_pts_f, new_desc, has_point1); status is VIORB_ERR_CAPACITY (with the first pcap points)
    when more than pcap points are created, every other error raises."""
    c = mapping_camera(cam)
    kf1, ng = problem["kf1"], problem["neigh"]
    J = len(ng)
    k1 = np.ascontiguousarray(kf1["kps"], capi.KP_DTYPE)
    n1 = len(k1)
    cap = max([n1] + [len(n["kps"]) for n in ng] + [1])
    st = lambda key, dt, tail=(): _stack([n[key] for n in ng], cap, dt, tail) if J else np.zeros((1, cap) + tuple(tail), dt)
    hp1 = _u8(kf1["hp"]).copy()
    n2 = np.array([len(n["kps"]) for n in ng] or [0], np.int32)
    T2 = _f32(np.stack([_f32(n["pose12"]) for n in ng])) if J else np.zeros((1, 12), np.float32)
    O2 = _f32(np.stack([_f32(n["Ow"]) for n in ng])) if J else np.zeros((1, 3), np.float32)
    F = _f32(np.stack([_f32(n["F12"]).ravel() for n in ng])) if J else np.zeros((1, 9), np.float32)
    md = _f32([n["median_depth"] for n in ng] or [1]); kf = _u8([n["kf2_first"] for n in ng] or [0])
    idx, pf, de = np.zeros((pcap, 3), np.int32), np.zeros((pcap, 8), np.float32), np.zeros((pcap, 32), np.uint8)
    n = C.c_int(0)
    arrs = [st("kps", capi.KP_DTYPE), st("desc", np.uint8, (32,)), st("hp", np.uint8), st("ur", np.float32), st("depth", np.float32), st("xy_dist", np.float32, (2,)),
            st("node", np.int32)]
    rc = lib().viorb_create_new_map_points(C.byref(c), int(monocular), ptr(k1), ptr(_u8(kf1["desc"])), ptr(hp1), ptr(_f32(kf1["ur"])), ptr(_f32(kf1["depth"])),
                                           ptr(_f32(kf1["xy_dist"])), ptr(_i32(kf1["node"])), n1, ptr(_f32(kf1["pose12"])), ptr(_f32(kf1["Ow"])), ptr(arrs[0]),
                                           ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]), ptr(arrs[4]), ptr(arrs[5]), ptr(arrs[6]), ptr(n2), ptr(T2), ptr(O2), ptr(F),
                                           ptr(md), ptr(kf), J, cap, pcap, ptr(idx), ptr(pf), ptr(de), C.byref(n))
    if rc != capi.VIORB_OK and rc != capi.ERR_CAPACITY:
        check(rc)
    return dict(status=rc, n_new=n.value, new_idx=idx[:n.value], new_pts_f=pf[:n.value], new_desc=de[:n.value], has_point1=hp1)
