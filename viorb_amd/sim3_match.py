"""The loop-closing matchers that project through a similarity (ORBmatcher::SearchBySim3, SearchByProjection(KF, Scw) and Fuse(KF, Scw),
reference src/ORBmatcher.cc:290-403, :977-1100, :1102-1326) and the handle-free key-frame grid, through the C ABI of
include/viorb_sim3_match.h. A key frame is (kps [n] of capi.KP_DTYPE, desc [n,32] uint8); a map point list is (pts_f [p,8] = Pw3 normal3
minDist maxDist, pts_desc [p,32]); the camera is (intr4 = fx fy cx cy, scale_factors [nlevels], bounds4 = minX maxX minY maxY). The host
hooks (no device) are the debug_* functions at the end."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as _up

MATCHED, NOT_CANDIDATE, BEHIND, OUT_OF_IMAGE, OUT_OF_RANGE, VIEW_ANGLE, NO_FEATURE_IN_WINDOW, ABOVE_THRESHOLD, NOT_MUTUAL = range(9)
SEARCH_BY_SIM3, SEARCH_BY_PROJECTION, FUSE = 0, 1, 2
GRID_CELLS = 64 * 48
MAX_FEATURES = 16384

_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)
_u8 = lambda a: np.ascontiguousarray(a, np.uint8)
_kp = lambda a: np.ascontiguousarray(a, capi.KP_DTYPE)


def camera(intr4, scale_factors, nlevels=None):
    """capi.MappingCamera with the fields the matchers read: fx fy cx cy, nlevels, scale_factors."""
    c = capi.MappingCamera()
    c.fx, c.fy, c.cx, c.cy = [float(v) for v in intr4]
    sf = np.asarray(scale_factors, np.float32)
    c.nlevels = int(len(sf) if nlevels is None else nlevels)
    for i in range(16):
        c.scale_factors[i] = float(sf[min(i, len(sf) - 1)])
        c.level_sigma2[i] = float(sf[min(i, len(sf) - 1)] ** 2)
    c.scale_factor = float(sf[min(1, len(sf) - 1)])
    return c


def shape():
    """(points per workgroup, wavefront size, candidates per list) of the built kernels."""
    o = np.zeros(3, np.int32)
    check(lib().viorb_sim3_match_shape(ptr(o)))
    return tuple(int(v) for v in o)


def keyframe_grid(kps, bounds4):
    """viorb_keyframe_grid (host buffers): (cell_start [64*48+1], cell_idx [number of features inside the grid])."""
    k = _kp(kps)
    cs, ci = np.zeros(GRID_CELLS + 1, np.int32), np.zeros(max(len(k), 1), np.int32)
    check(lib().viorb_keyframe_grid(ptr(k), len(k), ptr(_f32(bounds4)), ptr(cs), ptr(ci)))
    return cs, ci[:cs[GRID_CELLS]]


def search_by_sim3(side1, side2, R12, t12, s12, cam, bounds4, th=7.5):
    """viorb_search_by_sim3 (host buffers, one pair). A side is a dict(kps, desc, pose12, has_point, pts_f, pts_desc, already).
    dict(match12, nfound, match1, match2, reason1, reason2)."""
    a, n = [], []
    for s in (side1, side2):
        k = _kp(s["kps"])
        n.append(len(k))
        a.append([k, _u8(s["desc"]), _f32(s["pose12"]), _u8(s["has_point"]), _f32(s["pts_f"]), _u8(s["pts_desc"]), _u8(s["already"])])
    o = dict(match12=np.full(n[0], -1, np.int32), match1=np.full(n[0], -1, np.int32), match2=np.full(n[1], -1, np.int32),
             reason1=np.zeros(n[0], np.int32), reason2=np.zeros(n[1], np.int32))
    nf = C.c_int32(0)
    args = []
    for k in range(2):
        x = a[k]
        args += [ptr(x[0]), ptr(x[1]), n[k], ptr(x[2]), ptr(x[3]), ptr(x[4]), ptr(x[5]), ptr(x[6])]
    check(lib().viorb_search_by_sim3(*args, ptr(_f32(R12)), ptr(_f32(t12)), float(np.float32(s12)), C.byref(cam), ptr(_f32(bounds4)), float(th),
                                     ptr(o["match12"]), C.byref(nf), ptr(o["match1"]), ptr(o["match2"]), ptr(o["reason1"]), ptr(o["reason2"])))
    o["nfound"] = nf.value
    return o


def search_by_projection_sim3(kps, desc, Scw, pts_f, pts_desc, pts_valid, feat_taken, cam, bounds4, th=10.0):
    """viorb_search_by_projection_sim3 (host buffers, one key frame): dict(best_idx [npts], nmatches, reason [npts])."""
    k, pf = _kp(kps), _f32(pts_f).reshape(-1, 8)
    bi, re, nm = np.full(len(pf), -1, np.int32), np.zeros(len(pf), np.int32), C.c_int32(0)
    check(lib().viorb_search_by_projection_sim3(ptr(k), ptr(_u8(desc)), len(k), ptr(_f32(Scw)), ptr(pf), ptr(_u8(pts_desc)), ptr(_u8(pts_valid)), len(pf),
                                                ptr(_u8(feat_taken)), C.byref(cam), ptr(_f32(bounds4)), float(th), ptr(bi), C.byref(nm), ptr(re)))
    return dict(best_idx=bi, nmatches=nm.value, reason=re)


def fuse_sim3(kps, desc, Scw, pts_f, pts_desc, pts_valid, cam, bounds4, th=4.0):
    """viorb_fuse_sim3 (host buffers, one key frame): dict(best_idx [npts], nfused, reason [npts])."""
    k, pf = _kp(kps), _f32(pts_f).reshape(-1, 8)
    bi, re, nf = np.full(len(pf), -1, np.int32), np.zeros(len(pf), np.int32), C.c_int32(0)
    check(lib().viorb_fuse_sim3(ptr(k), ptr(_u8(desc)), len(k), ptr(_f32(Scw)), ptr(pf), ptr(_u8(pts_desc)), ptr(_u8(pts_valid)), len(pf), C.byref(cam),
                                ptr(_f32(bounds4)), float(th), ptr(bi), C.byref(nf), ptr(re)))
    return dict(best_idx=bi, nfused=nf.value, reason=re)


class Sim3MatchBatch:
    """A batch of key frames on the device (uploaded once, grids built by viorb_keyframe_grid_device): the device entries on torch
    tensors. frames: a list of (kps, desc); cap: the capacity of the per-key-frame arrays (default: the largest count)."""

    def __init__(self, frames, cam, bounds4, cap=None, device=0):
        import torch
        self.torch, self.dev, self.device = torch, torch.device("cuda", device), device
        self.cam, self.bounds = cam, _f32(bounds4)
        self.B = len(frames)
        self.n = [len(k) for k, _ in frames]
        self.cap = int(cap or max(max(self.n), 1))
        kps, desc = np.zeros((self.B, self.cap), capi.KP_DTYPE), np.zeros((self.B, self.cap, 32), np.uint8)
        for b, (k, d) in enumerate(frames):
            kps[b, :self.n[b]], desc[b, :self.n[b]] = _kp(k), _u8(d).reshape(-1, 32)
        self.kps, self.desc, self.count = _up(kps, device), _up(desc, device), _up(np.array(self.n, np.int32), device)
        self.cell_start = torch.zeros((self.B, GRID_CELLS + 1), dtype=torch.int32, device=self.dev)
        self.cell_idx = torch.zeros((self.B, self.cap), dtype=torch.int32, device=self.dev)
        check(lib().viorb_keyframe_grid_device(ptr(self.kps), ptr(self.count), self.cap, self.B, ptr(self.bounds), ptr(self.cell_start), ptr(self.cell_idx),
                                               self._stream()))
        self.kf = capi.S3mKeyframes(ptr(self.kps), ptr(self.desc), ptr(self.count), ptr(self.cell_start), ptr(self.cell_idx), self.cap)
        self.ws = None                                              # a capi.Workspace once a call needed one; a test may put its own here

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _workspace(self, cap, pcap):
        wb = lib().viorb_sim3_match_workspace_bytes(int(cap), int(pcap), self.B)
        self.ws_bytes = wb                                          # what the last call was handed
        if self.ws is None or not self.ws.fits(wb):
            self.ws = capi.Workspace(self.torch, self.dev, wb)
        return self.ws.ptr, wb

    def _pad(self, rows, cap, tail, dtype):
        """rows: one array per key frame -> [B, cap, *tail] on the device."""
        a = np.zeros((self.B, cap) + tail, dtype)
        for b, r in enumerate(rows):
            r = np.asarray(r, dtype).reshape((-1,) + tail)
            a[b, :len(r)] = r
        return _up(a, self.device)

    def grid(self):
        """(cell_start [B, 64*48+1], cell_idx [B, cap]) as numpy arrays."""
        self.torch.cuda.synchronize(self.dev)
        return self.cell_start.cpu().numpy(), self.cell_idx.cpu().numpy()

    def side(self, pose12, has_point, pts_f, pts_desc, already):
        """The per-feature map points of the batch's key frames as one side of SearchBySim3 (lists with one array per key frame)."""
        t = [_up(_f32(np.stack([_f32(p) for p in pose12])), self.device), self._pad(has_point, self.cap, (), np.uint8),
             self._pad(pts_f, self.cap, (8,), np.float32), self._pad(pts_desc, self.cap, (32,), np.uint8), self._pad(already, self.cap, (), np.uint8)]
        s = capi.S3mSide(self.kf, *[ptr(x) for x in t])
        s._keep = t
        return s

    def search_by_sim3(self, side1, other, side2, R12, t12, s12, th=7.5, raw=True):
        """viorb_search_by_sim3_device: this batch's key frames are side 1, `other` (a Sim3MatchBatch) holds side 2. R12 [B,3,3], t12 [B,3],
        s12 [B]: device tensors (used where they lie) or arrays. One dict per pair."""
        t = self.torch
        dv = lambda a: a if isinstance(a, t.Tensor) else _up(_f32(a), self.device)
        R12, t12, s12 = dv(R12), dv(t12), dv(s12)
        z = lambda cap: t.zeros((self.B, cap), dtype=t.int32, device=self.dev)
        m12, nf = z(self.cap), t.zeros(self.B, dtype=t.int32, device=self.dev)
        m1, m2, r1, r2 = (z(self.cap), z(other.cap), z(self.cap), z(other.cap)) if raw else (None,) * 4
        ws, wb = self._workspace(max(self.cap, other.cap), 1)
        check(lib().viorb_search_by_sim3_device(C.byref(side1), C.byref(side2), ptr(R12), ptr(t12), ptr(s12), C.byref(self.cam), ptr(self.bounds), float(th),
                                                self.B, ptr(m12), ptr(nf), ptr(m1), ptr(m2), ptr(r1), ptr(r2), ws, wb, self._stream()))
        t.cuda.synchronize(self.dev)
        h = lambda x: None if x is None else x.cpu().numpy()
        m12, nf, m1, m2, r1, r2 = [h(x) for x in (m12, nf, m1, m2, r1, r2)]
        cut = lambda x, b, n: None if x is None else x[b, :n]
        return [dict(match12=m12[b, :self.n[b]], nfound=int(nf[b]), match1=cut(m1, b, self.n[b]), match2=cut(m2, b, other.n[b]),
                     reason1=cut(r1, b, self.n[b]), reason2=cut(r2, b, other.n[b])) for b in range(self.B)]

    def search_by_projection(self, Scw, pts_f, pts_desc, pts_valid, feat_taken, th=10.0, pcap=None):
        """viorb_search_by_projection_sim3_device: Scw [B,12]; pts_f / pts_desc / pts_valid / feat_taken: one array per key frame."""
        t = self.torch
        npts = [len(_f32(p).reshape(-1, 8)) for p in pts_f]
        pcap = int(pcap or max(max(npts), 1))
        d = [_up(_f32(Scw).reshape(self.B, 12), self.device), self._pad(pts_f, pcap, (8,), np.float32), self._pad(pts_desc, pcap, (32,), np.uint8),
             self._pad(pts_valid, pcap, (), np.uint8), _up(np.array(npts, np.int32), self.device), self._pad(feat_taken, self.cap, (), np.uint8)]
        bi, re = [t.zeros((self.B, pcap), dtype=t.int32, device=self.dev) for _ in range(2)]
        nm = t.zeros(self.B, dtype=t.int32, device=self.dev)
        ws, wb = self._workspace(self.cap, pcap)
        check(lib().viorb_search_by_projection_sim3_device(C.byref(self.kf), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), pcap, ptr(d[5]),
                                                           C.byref(self.cam), ptr(self.bounds), float(th), self.B, ptr(bi), ptr(nm), ptr(re), ws, wb,
                                                           self._stream()))
        t.cuda.synchronize(self.dev)
        bi, re, nm = bi.cpu().numpy(), re.cpu().numpy(), nm.cpu().numpy()
        return [dict(best_idx=bi[b, :npts[b]], nmatches=int(nm[b]), reason=re[b, :npts[b]], tail=bi[b, npts[b]:]) for b in range(self.B)]

    def fuse(self, Scw, pts_f, pts_desc, pts_valid, th=4.0, pcap=None):
        """viorb_fuse_sim3_device: Scw [B,12]; ONE point list pts_f [p,8], pts_desc [p,32]; pts_valid [B,p]."""
        t = self.torch
        pf = _f32(pts_f).reshape(-1, 8)
        npts = len(pf)
        pcap = int(pcap or max(npts, 1))
        one = lambda a, tail, dt: _up(np.concatenate([np.asarray(a, dt).reshape((-1,) + tail), np.zeros((pcap - npts,) + tail, dt)]), self.device)
        d = [_up(_f32(Scw).reshape(self.B, 12), self.device), one(pf, (8,), np.float32), one(pts_desc, (32,), np.uint8),
             self._pad(list(np.asarray(pts_valid, np.uint8).reshape(self.B, npts)), pcap, (), np.uint8)]
        bi, re = [t.zeros((self.B, pcap), dtype=t.int32, device=self.dev) for _ in range(2)]
        nf = t.zeros(self.B, dtype=t.int32, device=self.dev)
        ws, wb = self._workspace(self.cap, pcap)
        check(lib().viorb_fuse_sim3_device(C.byref(self.kf), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), npts, pcap, C.byref(self.cam), ptr(self.bounds),
                                           float(th), self.B, ptr(bi), ptr(nf), ptr(re), ws, wb, self._stream()))
        t.cuda.synchronize(self.dev)
        bi, re, nf = bi.cpu().numpy(), re.cpu().numpy(), nf.cpu().numpy()
        return [dict(best_idx=bi[b, :npts], nfused=int(nf[b]), reason=re[b, :npts], tail=bi[b, npts:]) for b in range(self.B)]


# ---- host hooks (sim3_match_core.h compiled for the host) ------------------------------------------------------------------------------
def debug_decompose(Scw):
    """(scw, Rcw [3,3], tcw [3], Ow [3]) of Scw [12]."""
    o = np.zeros(16, np.float32)
    check(lib().viorb_debug_sim3_decompose(ptr(_f32(Scw)), ptr(o)))
    return o[0], o[1:10].reshape(3, 3), o[10:13], o[13:16]


def debug_pair(R12, t12, s12):
    """(sR12 [3,3], sR21 [3,3], t21 [3])."""
    o = np.zeros(21, np.float32)
    check(lib().viorb_debug_sim3_pair(ptr(_f32(R12)), ptr(_f32(t12)), float(np.float32(s12)), ptr(o)))
    return o[:9].reshape(3, 3), o[9:18].reshape(3, 3), o[18:21]


def debug_project(which, T12, pt8, cam, bounds4, th, sR=None, t=None):
    """One point through the gates of function `which`: dict(u, v, dist3D, radius, level, rect, reason)."""
    o4, o6 = np.zeros(4, np.float32), np.zeros(6, np.int32)
    check(lib().viorb_debug_sim3_project(int(which), ptr(_f32(T12)), ptr(None if sR is None else _f32(sR)), ptr(None if t is None else _f32(t)),
                                         ptr(_f32(pt8)), C.byref(cam), ptr(_f32(bounds4)), float(th), ptr(o4), ptr(o6)))
    return dict(u=o4[0], v=o4[1], dist3D=o4[2], radius=o4[3], level=int(o6[0]), rect=tuple(int(v) for v in o6[1:5]), reason=int(o6[5]))


def debug_claim_in_order(cands, taken_in):
    """The ordered phase over candidate lists cands[p] = [(distance, feature), ...]: (best_idx [npts], nmatches, sweeps)."""
    npts, lcap = len(cands), max([len(c) for c in cands] + [1])
    cand, cn = np.zeros((max(npts, 1), lcap), np.uint32), np.zeros(max(npts, 1), np.int32)
    for p, lst in enumerate(cands):
        cn[p] = len(lst)
        for k, (d, idx) in enumerate(lst):
            cand[p, k] = (int(d) << 16) | int(idx)
    tk = _u8(taken_in)
    bi, nm = np.full(max(npts, 1), -1, np.int32), C.c_int32(0)
    sweeps = lib().viorb_debug_claim_in_order(ptr(cand), ptr(cn), npts, lcap, ptr(tk), len(tk), ptr(bi), C.byref(nm))
    if sweeps < 0:
        check(sweeps)
    return bi[:npts], nm.value, sweeps
