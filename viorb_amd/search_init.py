"""The monocular matcher ORBmatcher::SearchForInitialization (reference src/ORBmatcher.cc:405-520) and KeyFrame::ComputeSceneMedianDepth
(src/KeyFrame.cc:970-1000) through the C ABI of include/viorb_search_init.h. A frame is (kps [n] of capi.KP_DTYPE, desc [n,32] uint8);
prev_matched is [n1,2] float32 (vbPrevMatched); bounds4 = minX maxX minY maxY. The host hooks (no device) are the debug_* functions at
the end."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as _up

MATCHED, NOT_CANDIDATE, NO_FEATURE_IN_WINDOW, ABOVE_THRESHOLD, RATIO, DISPLACED, ROTATION = range(7)
GRID_CELLS = 64 * 48
MAX_FEATURES = 16384
INT_MAX = 2 ** 31 - 1
NONE = 0xffffffff

_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)
_u8 = lambda a: np.ascontiguousarray(a, np.uint8)
_kp = lambda a: np.ascontiguousarray(a, capi.KP_DTYPE)


def shape():
    """(points per workgroup of the candidate pass, wavefront size, candidates per list, threads of the ordered phase)."""
    o = np.zeros(4, np.int32)
    check(lib().viorb_search_init_shape(ptr(o)))
    return tuple(int(v) for v in o)


def search_for_initialization(kps1, desc1, kps2, desc2, prev_matched, bounds4, window_size=100, nnratio=0.9, check_orientation=True):
    """viorb_search_for_initialization (host buffers, one stream): dict(matches12, nmatches, prev_matched, matches21, matched_distance,
    rot_hist, reason, xy1, xy2, sweeps). prev_matched is not modified; the updated copy is in the result."""
    k1, k2 = _kp(kps1), _kp(kps2)
    n1, n2 = len(k1), len(k2)
    pm = np.array(prev_matched, np.float32, copy=True).reshape(-1, 2)
    assert len(pm) == n1
    o = dict(matches12=np.full(n1, -1, np.int32), matches21=np.full(n2, -1, np.int32), matched_distance=np.full(n2, INT_MAX, np.int32),
             rot_hist=np.zeros(30, np.int32), reason=np.zeros(n1, np.int32), xy1=np.zeros((n1, 2), np.float32), xy2=np.zeros((n2, 2), np.float32),
             sweeps=np.zeros(1, np.int32))
    out = capi.SearchInitOutputs(*[ptr(o[f]) for f in capi.SEARCH_INIT_OUTPUT_FIELDS])
    nm = C.c_int32(0)
    check(lib().viorb_search_for_initialization(ptr(k1), ptr(_u8(desc1)), n1, ptr(k2), ptr(_u8(desc2)), n2, ptr(pm), ptr(_f32(bounds4)), int(window_size),
                                                float(np.float32(nnratio)), int(bool(check_orientation)), ptr(o["matches12"]), C.byref(nm), C.byref(out)))
    o["nmatches"], o["prev_matched"], o["sweeps"] = nm.value, pm, int(o["sweeps"][0])
    return o


def scene_median_depth(pose12, points, has_point, q=2):
    """viorb_scene_median_depth (host buffers, one key frame): (median, n_depths)."""
    X, hp = _f32(points).reshape(-1, 3), _u8(has_point)
    med, n = C.c_float(0), C.c_int32(0)
    check(lib().viorb_scene_median_depth(ptr(_f32(pose12)), ptr(X), ptr(hp), len(X), int(q), C.byref(med), C.byref(n)))
    return np.float32(med.value), n.value


class SearchInitBatch:
    """A batch of streams on the device: frame 1 (the initial frame) is uploaded once with prev_matched, which stays on the device from
    call to call as mvbPrevMatched does; every search() uploads a frame 2, builds its grid and runs the device entry on torch tensors.
    frames1: a list of (kps, desc); prev_matched: a list of [n1,2]; cap: the capacity of every per-stream array."""

    def __init__(self, frames1, prev_matched, bounds4, cap, device=0):
        import torch
        self.torch, self.dev, self.device = torch, torch.device("cuda", device), device
        self.bounds, self.B, self.cap = _f32(bounds4), len(frames1), int(cap)
        self.n1 = [len(k) for k, _ in frames1]
        self.kps1, self.desc1, self.count1 = self._frames(frames1)
        pm = np.zeros((self.B, self.cap, 2), np.float32)
        for b, p in enumerate(prev_matched):
            pm[b, :self.n1[b]] = _f32(p).reshape(-1, 2)
        self.prev = _up(pm, device)
        wb = lib().viorb_search_init_workspace_bytes(self.cap, self.B)
        self.ws, self.ws_bytes = capi.Workspace(torch, self.dev, wb), wb          # ws may be re-filled or replaced by a larger one between calls

    def _frames(self, frames, garbage=None):
        kps, desc = np.zeros((self.B, self.cap), capi.KP_DTYPE), np.zeros((self.B, self.cap, 32), np.uint8)
        if garbage is not None:                   # entries beyond the counts that must never be read as valid
            kps[:], desc[:] = garbage
        n = [len(k) for k, _ in frames]
        for b, (k, d) in enumerate(frames):
            kps[b, :n[b]], desc[b, :n[b]] = _kp(k), _u8(d).reshape(-1, 32)
        return _up(kps, self.device), _up(desc, self.device), _up(np.array(n, np.int32), self.device)

    def set_frame1(self, frames1, garbage):
        """Replaces frame 1's arrays (same counts), with `garbage` = (key point, descriptor row) beyond the counts."""
        self.kps1, self.desc1, self.count1 = self._frames(frames1, garbage)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def search(self, frames2, window_size=100, nnratio=0.9, check_orientation=True, garbage=None, raw=False):
        """viorb_search_for_initialization_device against frames2 (a list of (kps, desc)). One dict per stream, arrays cut to the counts
        (`tail12`: matches12 from n1 on). raw=True: dict(matches12, xy1, xy2, n1, n2) of device tensors as well, nothing copied."""
        t = self.torch
        n2 = [len(k) for k, _ in frames2]
        kps2, desc2, count2 = self._frames(frames2, garbage)
        cs = t.zeros((self.B, GRID_CELLS + 1), dtype=t.int32, device=self.dev)
        ci = t.zeros((self.B, self.cap), dtype=t.int32, device=self.dev)
        check(lib().viorb_keyframe_grid_device(ptr(kps2), ptr(count2), self.cap, self.B, ptr(self.bounds), ptr(cs), ptr(ci), self._stream()))
        kf = capi.S3mKeyframes(ptr(kps2), ptr(desc2), ptr(count2), ptr(cs), ptr(ci), self.cap)
        zi = lambda *s: t.zeros(s, dtype=t.int32, device=self.dev)
        d = dict(matches12=zi(self.B, self.cap), nmatches=zi(self.B), matches21=zi(self.B, self.cap), matched_distance=zi(self.B, self.cap),
                 rot_hist=zi(self.B, 30), reason=zi(self.B, self.cap), xy1=t.zeros((self.B, self.cap, 2), dtype=t.float32, device=self.dev),
                 xy2=t.zeros((self.B, self.cap, 2), dtype=t.float32, device=self.dev), sweeps=zi(self.B))
        out = capi.SearchInitOutputs(*[ptr(d[f]) for f in capi.SEARCH_INIT_OUTPUT_FIELDS])
        check(lib().viorb_search_for_initialization_device(ptr(self.kps1), ptr(self.desc1), ptr(self.count1), C.byref(kf), ptr(self.prev), self.cap, self.B,
                                                           ptr(self.bounds), int(window_size), float(np.float32(nnratio)), int(bool(check_orientation)),
                                                           ptr(d["matches12"]), ptr(d["nmatches"]), C.byref(out), self.ws.ptr, self.ws_bytes, self._stream()))
        if raw:
            self._keep = (kps2, desc2, count2, cs, ci)
            return dict(matches12=d["matches12"], xy1=d["xy1"], xy2=d["xy2"], n1=self.count1, n2=count2)
        t.cuda.synchronize(self.dev)
        h = {k: v.cpu().numpy() for k, v in d.items()}
        pm = self.prev.cpu().numpy()
        res = []
        for b in range(self.B):
            a, c = self.n1[b], n2[b]
            res.append(dict(matches12=h["matches12"][b, :a], tail12=h["matches12"][b, a:], nmatches=int(h["nmatches"][b]), prev_matched=pm[b, :a],
                            prev_tail=pm[b, a:], matches21=h["matches21"][b, :c], matched_distance=h["matched_distance"][b, :c], rot_hist=h["rot_hist"][b],
                            reason=h["reason"][b, :a], xy1=h["xy1"][b, :a], xy2=h["xy2"][b, :c], sweeps=int(h["sweeps"][b])))
        return res


def scene_median_depth_batch(pose12, points, has_point, q=2, cap=None, device=0):
    """viorb_scene_median_depth_device: one (pose12, points [n,3], has_point [n]) per key frame. (median [B], n_depths [B])."""
    import torch
    B = len(points)
    n = [len(_f32(p).reshape(-1, 3)) for p in points]
    cap = int(cap or max(max(n), 1))
    X, hp = np.zeros((B, cap, 3), np.float32), np.zeros((B, cap), np.uint8)
    X[:], hp[:] = 7.0, 1                                 # beyond the counts: points that must not be read
    for b in range(B):
        X[b, :n[b]], hp[b, :n[b]] = _f32(points[b]).reshape(-1, 3), _u8(has_point[b])
    dev = torch.device("cuda", device)
    d = [_up(_f32(np.stack([_f32(p) for p in pose12])), device), _up(X, device), _up(hp, device), _up(np.array(n, np.int32), device)]
    med, cnt = torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    check(lib().viorb_scene_median_depth_device(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), cap, B, int(q), ptr(med), ptr(cnt),
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    return med.cpu().numpy(), cnt.cpu().numpy()


# ---- host hooks (search_init_core.h compiled for the host) -----------------------------------------------------------------------------
def debug_ordered(cands, nfeat, nnratio=0.9):
    """The ordered phase over candidate lists cands[p] = [(distance, feature), ...] (None or [] for a point without candidates):
    dict(state, why, matches12, matches21, matched_distance, nmatches, sweeps)."""
    npts, lcap = len(cands), max([len(c) for c in cands if c] + [1])
    m = max(npts, 1)
    cand, cn = np.zeros((m, lcap), np.uint32), np.zeros(m, np.int32)
    for p, lst in enumerate(cands):
        for k, (d, idx) in enumerate(lst or []):
            cand[p, k] = (int(d) << 16) | int(idx)
        cn[p] = len(lst or [])
    st, why, m12 = np.zeros(m, np.uint32), np.zeros(m, np.int32), np.zeros(m, np.int32)
    m21, md = np.zeros(max(nfeat, 1), np.int32), np.zeros(max(nfeat, 1), np.int32)
    nm = C.c_int32(0)
    sweeps = lib().viorb_debug_search_init_ordered(ptr(cand), ptr(cn), npts, lcap, int(nfeat), float(np.float32(nnratio)), ptr(st), ptr(why), ptr(m12),
                                                   ptr(m21), ptr(md), C.byref(nm))
    if sweeps < 0:
        check(sweeps)
    return dict(state=st[:npts], why=why[:npts], matches12=m12[:npts], matches21=m21[:nfeat], matched_distance=md[:nfeat], nmatches=nm.value, sweeps=sweeps)


def debug_window(kps2, cell_start, cell_idx, bounds4, x, y, r, level1=0):
    """One window through GetFeaturesInArea over a host grid: (rect4, the features in visiting order)."""
    k = _kp(kps2)
    rect, idx = np.zeros(4, np.int32), np.zeros(max(len(k), 1), np.int32)
    ci = _i32(cell_idx) if len(cell_idx) else np.zeros(1, np.int32)
    n = lib().viorb_debug_search_init_window(ptr(k), len(k), ptr(_i32(cell_start)), ptr(ci), ptr(_f32(bounds4)), float(np.float32(x)), float(np.float32(y)),
                                             float(np.float32(r)), int(level1), ptr(rect), ptr(idx))
    if n < 0:
        check(n)
    return tuple(int(v) for v in rect), idx[:n]


def debug_scene_depth(pose12, point3):
    return np.float32(lib().viorb_debug_scene_depth(ptr(_f32(pose12)), ptr(_f32(point3))))
