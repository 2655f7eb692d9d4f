"""The two-view (monocular) initialiser (Initializer::Initialize, reference src/Initializer.cc:44-929) through the C ABI of
include/viorb_two_view.h. A problem is a dict(xy1 [n1,2], xy2 [n2,2] undistorted key points, matches12 [n1] (index in frame 2 or -1),
K4 = fx fy cx cy); the RANSAC sets [iterations,8] index the compacted match list and come from draw_sets(n_matches, iterations, seed).
The host hooks (no device) are the debug_* functions at the end."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as _up

FAILED, FROM_H, FROM_F = 0, 1, 2
REASON_OK, REASON_FEW_MATCHES, REASON_BAD_SET, REASON_NO_MODEL, REASON_H_DEGENERATE, REASON_NO_WINNER, REASON_FEW_GOOD, REASON_PARALLAX = range(8)

_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)


def two_view_config(K4, sigma=1.0, iterations=200, min_parallax_deg=1.0, min_triangulated=50):
    c = capi.TwoViewConfig()
    c.sigma, c.iterations, c.min_parallax_deg, c.min_triangulated = float(sigma), int(iterations), float(min_parallax_deg), int(min_triangulated)
    c.fx, c.fy, c.cx, c.cy = [float(v) for v in K4]
    return c


def draw_sets(n_matches, iterations=200, seed=0):
    """viorb_two_view_draw_sets: [iterations, 8] int32, eight distinct indices of 0..n_matches-1 per row."""
    sets = np.zeros((iterations, 8), np.int32)
    check(lib().viorb_two_view_draw_sets(int(n_matches), int(iterations), C.c_uint64(int(seed)), ptr(sets)))
    return sets


# field -> (dtype, shape per stream with `cap` standing for the capacity)
_OUT = dict(status=("i4", ()), reason=("i4", ()), n_matches=("i4", ()), scores=("f4", (2,)), best_iter=("i4", (2,)), H21=("f4", (3, 3)),
            F21=("f4", (3, 3)), inliers_h=("u1", ("cap",)), inliers_f=("u1", ("cap",)), R21=("f4", (3, 3)), t21=("f4", (3,)),
            P3D=("f4", ("cap", 3)), triangulated=("u1", ("cap",)), n_hyp=("i4", ()), hyp_n_good=("i4", (8,)), hyp_parallax=("f4", (8,)),
            hyp_R=("f4", (8, 3, 3)), hyp_t=("f4", (8, 3)))


def _shape(field, cap, batch=None):
    s = tuple(cap if d == "cap" else d for d in _OUT[field][1])
    return s if batch is None else (batch,) + s


def _trim(out, n1, N):
    """One stream's outputs cut to their lengths: per key point of frame 1 (P3D, triangulated), per match (inlier flags)."""
    r = dict(out)
    r["P3D"], r["triangulated"] = out["P3D"][:n1], out["triangulated"][:n1]
    r["inliers_h"], r["inliers_f"] = out["inliers_h"][:N], out["inliers_f"][:N]
    for k in ("status", "reason", "n_matches", "n_hyp"):
        r[k] = int(out[k])
    return r


def TwoViewInit(prob, sets, sigma=1.0, min_parallax_deg=1.0, min_triangulated=50):
    """viorb_two_view_init (host buffers, one stream): dict of the outputs of include/viorb_two_view.h."""
    xy1, xy2, m = _f32(prob["xy1"]).reshape(-1, 2), _f32(prob["xy2"]).reshape(-1, 2), _i32(prob["matches12"])
    sets = _i32(sets).reshape(-1, 8)
    cfg = two_view_config(prob["K4"], sigma, len(sets), min_parallax_deg, min_triangulated)
    cap = max(len(xy1), len(xy2), 1)
    out = {f: np.zeros(_shape(f, cap), _OUT[f][0]) for f in capi.TWO_VIEW_OUTPUT_FIELDS}
    O = capi.TwoViewOutputs(**{f: ptr(out[f]) for f in out})
    check(lib().viorb_two_view_init(C.byref(cfg), ptr(xy1), len(xy1), ptr(xy2), len(xy2), ptr(m), ptr(sets), C.byref(O)))
    return _trim(out, len(xy1), int(out["n_matches"]))


class TwoViewBatch:
    """A batch of problems on the device (uploaded once): the end-to-end entry and the three stage entries on the same inputs.
    sets: one [iterations, 8] array per problem (rows of a stream with fewer than 8 matches are not read)."""

    def __init__(self, probs, sets, sigma=1.0, min_parallax_deg=1.0, min_triangulated=50, device=0):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.B = len(probs)
        self.n1 = [len(_f32(p["xy1"]).reshape(-1, 2)) for p in probs]
        self.n2 = [len(_f32(p["xy2"]).reshape(-1, 2)) for p in probs]
        self.cap = max(max(self.n1), max(self.n2), 1)
        self.iters = len(np.asarray(sets[0]).reshape(-1, 8))
        self.cfg = two_view_config(probs[0]["K4"], sigma, self.iters, min_parallax_deg, min_triangulated)
        xy1, xy2 = np.zeros((self.B, self.cap, 2), np.float32), np.zeros((self.B, self.cap, 2), np.float32)
        m = np.full((self.B, self.cap), -1, np.int32)
        for b, p in enumerate(probs):
            xy1[b, :self.n1[b]] = _f32(p["xy1"]).reshape(-1, 2); xy2[b, :self.n2[b]] = _f32(p["xy2"]).reshape(-1, 2)
            m[b, :self.n1[b]] = _i32(p["matches12"])
        self.d = [_up(xy1, device), _up(np.array(self.n1, np.int32), device), _up(xy2, device), _up(np.array(self.n2, np.int32), device), _up(m, device)]
        self.sets = _up(np.stack([_i32(s).reshape(-1, 8) for s in sets]), device)
        self.N = [int((np.asarray(p["matches12"]) >= 0).sum()) for p in probs]
        wb = lib().viorb_two_view_workspace_bytes(self.cap, self.iters, self.B)
        self.ws, self.ws_bytes = capi.Workspace(torch, self.dev, wb), wb          # ws may be re-filled or replaced by a larger one between calls

    @property
    def ws_ptr(self):
        return self.ws.ptr

    def _in(self):
        d = self.d
        return [C.byref(self.cfg), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), self.cap, ptr(d[4])]

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _outputs(self):
        t = self.torch
        dt = {"i4": t.int32, "f4": t.float32, "u1": t.uint8}
        out = {f: t.zeros(_shape(f, self.cap, self.B), dtype=dt[_OUT[f][0]], device=self.dev) for f in capi.TWO_VIEW_OUTPUT_FIELDS}
        return out, capi.TwoViewOutputs(**{f: ptr(out[f]) for f in out})

    def _down(self, out):
        self.torch.cuda.synchronize(self.dev)
        host = {f: v.cpu().numpy() for f, v in out.items()}
        return [_trim({f: host[f][b] for f in host}, self.n1[b], int(host["n_matches"][b])) for b in range(self.B)]

    def init(self):
        """viorb_two_view_init_device: one dict per stream."""
        out, O = self._outputs()
        check(lib().viorb_two_view_init_device(*self._in(), ptr(self.sets), self.B, C.byref(O), self.ws_ptr, self.ws_bytes, self._stream()))
        return self._down(out)

    def hypotheses(self):
        """viorb_two_view_hypotheses_device: (H21i, H12i, F21i) [B, iterations, 3, 3] device tensors and reason [B] (host)."""
        t = self.torch
        H21, H12, F21 = [t.zeros((self.B, self.iters, 3, 3), dtype=t.float32, device=self.dev) for _ in range(3)]
        reason = t.zeros(self.B, dtype=t.int32, device=self.dev)
        check(lib().viorb_two_view_hypotheses_device(*self._in(), ptr(self.sets), self.B, ptr(H21), ptr(H12), ptr(F21), ptr(reason), self.ws_ptr,
                                                     self.ws_bytes, self._stream()))
        t.cuda.synchronize(self.dev)
        return H21, H12, F21, reason.cpu().numpy()

    def score(self, H21, H12, F21, flags=False):
        """viorb_two_view_score_device on device matrices: scores [B, iterations, 2] and, on request, flags [B, iterations, 2, cap] (host)."""
        t = self.torch
        sc = t.zeros((self.B, self.iters, 2), dtype=t.float32, device=self.dev)
        fl = t.zeros((self.B, self.iters, 2, self.cap), dtype=t.uint8, device=self.dev) if flags else None
        check(lib().viorb_two_view_score_device(*self._in(), self.B, ptr(H21), ptr(H12), ptr(F21), ptr(sc), ptr(fl), self.ws_ptr, self.ws_bytes, self._stream()))
        t.cuda.synchronize(self.dev)
        return sc.cpu().numpy(), (fl.cpu().numpy() if flags else None)

    def reconstruct(self, model, M, inliers):
        """viorb_two_view_reconstruct_device: model [B], M [B,3,3], inliers [B, <= cap] over the compacted list (host arrays)."""
        inl = np.zeros((self.B, self.cap), np.uint8)
        for b, v in enumerate(inliers):
            inl[b, :len(v)] = v
        dm, dM, di = _up(_i32(model)), _up(_f32(M).reshape(self.B, 9)), _up(inl)
        out, O = self._outputs()
        check(lib().viorb_two_view_reconstruct_device(*self._in(), self.B, ptr(dm), ptr(dM), ptr(di), C.byref(O), self.ws_ptr, self.ws_bytes, self._stream()))
        return self._down(out)


# ---- host hooks (two_view_core.h compiled for the host) -------------------------------------------------------------------------------
def debug_hypothesis(model, pn1, pn2):
    """(M [3,3], vt.row(8) [3,3]) from eight pairs of normalised points."""
    M, pre = np.zeros(9, np.float32), np.zeros(9, np.float32)
    check(lib().viorb_debug_two_view_hypothesis(model, ptr(_f32(pn1)), ptr(_f32(pn2)), ptr(M), ptr(pre)))
    return M.reshape(3, 3), pre.reshape(3, 3)


def debug_normalise(xy):
    nrm = np.zeros(4, np.float32)
    xy = _f32(xy).reshape(-1, 2)
    check(lib().viorb_debug_two_view_normalise(ptr(xy), len(xy), ptr(nrm)))
    return nrm


def debug_denormalise(model, Mn, nrm1, nrm2):
    M21, M12 = np.zeros(9, np.float32), np.zeros(9, np.float32)
    check(lib().viorb_debug_two_view_denormalise(model, ptr(_f32(Mn)), ptr(_f32(nrm1)), ptr(_f32(nrm2)), ptr(M21), ptr(M12)))
    return M21.reshape(3, 3), M12.reshape(3, 3)


def debug_chi2(model, M21, M12, uv4, sigma=1.0):
    """(inlier, chi2 [2], score) of one match (u1 v1 u2 v2)."""
    chi2, score = np.zeros(2, np.float32), C.c_float(0)
    M12 = _f32(M12 if M12 is not None else np.zeros(9))
    inl = lib().viorb_debug_two_view_chi2(model, ptr(_f32(M21)), ptr(M12), ptr(_f32(uv4)), float(sigma), ptr(chi2), C.byref(score))
    return bool(inl), chi2, float(score.value)


def debug_decompose(model, M21, K4):
    """(n, R [8,3,3], t [8,3], d [3])."""
    R, t, d = np.zeros((8, 3, 3), np.float32), np.zeros((8, 3), np.float32), np.zeros(3, np.float32)
    n = lib().viorb_debug_two_view_decompose(model, ptr(_f32(M21)), ptr(_f32(K4)), ptr(R), ptr(t), ptr(d))
    return n, R, t, d


def debug_check_rt(K4, R, t, uv4, sigma=1.0):
    """(code, X [3], q6 = cosParallax z1 z2 squareError1 squareError2 dist2) of one match."""
    X, q = np.zeros(3, np.float32), np.zeros(6, np.float32)
    c = lib().viorb_debug_two_view_check_rt(ptr(_f32(K4)), ptr(_f32(R)), ptr(_f32(t)), ptr(_f32(uv4)), float(sigma), ptr(X), ptr(q))
    return c, X, q


def debug_parallax(cosines):
    c = _f32(cosines)
    return float(lib().viorb_debug_two_view_parallax(ptr(c), len(c)))


def debug_accept(model, n_good, parallax, n_inliers, min_parallax_deg=1.0, min_triangulated=50):
    r = C.c_int32(0)
    w = lib().viorb_debug_two_view_accept(model, ptr(_i32(n_good)), ptr(_f32(parallax)), int(n_inliers), float(min_parallax_deg), int(min_triangulated), C.byref(r))
    return w, r.value
