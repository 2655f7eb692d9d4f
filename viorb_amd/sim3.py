"""The Sim3 RANSAC solver (Sim3Solver::iterate, reference src/Sim3Solver.cc:37-423) through the C ABI of include/viorb_sim3.h. A problem
is a dict(X1c [n,3], X2c [n,3] the matched points in the frame of their own camera, sigma2_1 [n], sigma2_2 [n] = mvLevelSigma2[octave]
of the two key points, K1, K2 = fx fy cx cy); the RANSAC sets [iterations,3] index the correspondences and come from
draw_sets(n, iterations, seed). The host hooks (no device) are the debug_* functions at the end."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as _up

FOUND, CONTINUE, NO_MORE, FEW = range(4)
SET_OK, SET_FEW, SET_BAD, SET_ZERO_ROTATION = range(4)

_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)


def sim3_config(iterations, min_inliers=20, fix_scale=False, iterations_per_call=5):
    c = capi.Sim3Config()
    c.iterations, c.min_inliers, c.fix_scale, c.iterations_per_call = int(iterations), int(min_inliers), int(bool(fix_scale)), int(iterations_per_call)
    return c


def draw_sets(n, iterations=300, seed=0):
    """viorb_sim3_draw_sets: [iterations, 3] int32, three distinct indices of 0..n-1 per row."""
    sets = np.zeros((iterations, 3), np.int32)
    check(lib().viorb_sim3_draw_sets(int(n), int(iterations), C.c_uint64(int(seed)), ptr(sets)))
    return sets


def ransac_iterations(n, probability=0.99, min_inliers=20, max_iterations=300):
    """viorb_sim3_ransac_iterations: mRansacMaxIts of SetRansacParameters."""
    r = lib().viorb_sim3_ransac_iterations(int(n), float(probability), int(min_inliers), int(max_iterations))
    if r < 0:
        check(r)
    return r


# field -> (dtype, shape per pair with `cap` standing for the capacity)
_OUT = dict(status=("i4", ()), iterations_done=("i4", ()), best_inliers=("i4", ()), best_iter=("i4", ()), R12=("f4", (3, 3)), t12=("f4", (3,)),
            s12=("f4", ()), T12=("f4", (4, 4)), n_inliers=("i4", ()), inliers=("u1", ("cap",)))


def _shape(field, cap, batch=None):
    s = tuple(cap if d == "cap" else d for d in _OUT[field][1])
    return s if batch is None else (batch,) + s


def _trim(out, n):
    r = dict(out)
    r["inliers"] = out["inliers"][:n]
    for k in ("status", "iterations_done", "best_inliers", "best_iter", "n_inliers"):
        r[k] = int(out[k])
    r["s12"] = np.float32(out["s12"])
    return r


def sim3_ransac(prob, sets, max_its=None, first_iteration=0, best_inliers_in=0, min_inliers=20, fix_scale=False, iterations_per_call=5):
    """viorb_sim3_ransac (host buffers, one pair): dict of the outputs of include/viorb_sim3.h. max_its defaults to len(sets)."""
    X1, X2 = _f32(prob["X1c"]).reshape(-1, 3), _f32(prob["X2c"]).reshape(-1, 3)
    s1, s2 = _f32(prob["sigma2_1"]).ravel(), _f32(prob["sigma2_2"]).ravel()
    sets = _i32(sets).reshape(-1, 3)
    cfg = sim3_config(len(sets), min_inliers, fix_scale, iterations_per_call)
    n = len(X1)
    out = {f: np.zeros(_shape(f, max(n, 1)), _OUT[f][0]) for f in capi.SIM3_OUTPUT_FIELDS}
    O = capi.Sim3Outputs(**{f: ptr(out[f]) for f in out})
    check(lib().viorb_sim3_ransac(C.byref(cfg), ptr(X1), ptr(X2), ptr(s1), ptr(s2), ptr(_f32(prob["K1"])), ptr(_f32(prob["K2"])), n, ptr(sets),
                                  int(len(sets) if max_its is None else max_its), int(first_iteration), int(best_inliers_in), C.byref(O)))
    return _trim(out, n)


class Sim3Batch:
    """A batch of problems on the device (uploaded once): the end-to-end entry and the three stage entries on the same inputs.
    sets: one [iterations, 3] array per problem."""

    def __init__(self, probs, sets, min_inliers=20, fix_scale=False, device=0):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.B = len(probs)
        self.n = [len(_f32(p["X1c"]).reshape(-1, 3)) for p in probs]
        self.cap = max(max(self.n), 1)
        self.iters = len(np.asarray(sets[0]).reshape(-1, 3))
        self.min_inliers, self.fix_scale = int(min_inliers), bool(fix_scale)
        X1, X2 = np.zeros((self.B, self.cap, 3), np.float32), np.zeros((self.B, self.cap, 3), np.float32)
        s1, s2 = np.ones((self.B, self.cap), np.float32), np.ones((self.B, self.cap), np.float32)
        for b, p in enumerate(probs):
            n = self.n[b]
            X1[b, :n], X2[b, :n] = _f32(p["X1c"]).reshape(-1, 3), _f32(p["X2c"]).reshape(-1, 3)
            s1[b, :n], s2[b, :n] = _f32(p["sigma2_1"]).ravel(), _f32(p["sigma2_2"]).ravel()
        K1, K2 = np.stack([_f32(p["K1"]) for p in probs]), np.stack([_f32(p["K2"]) for p in probs])
        self.d = [_up(a, device) for a in (X1, X2, s1, s2, K1, K2, np.array(self.n, np.int32))]
        self.inputs = capi.Sim3Inputs(*[ptr(a) for a in self.d], self.cap)
        self.sets = _up(np.stack([_i32(s).reshape(-1, 3) for s in sets]), device)
        wb = lib().viorb_sim3_workspace_bytes(self.cap, self.iters, self.B)
        self.ws, self.ws_bytes = capi.Workspace(torch, self.dev, wb), wb          # ws may be re-filled or replaced by a larger one between calls

    @property
    def ws_ptr(self):
        return self.ws.ptr

    def _cfg(self, iterations_per_call=5):
        return sim3_config(self.iters, self.min_inliers, self.fix_scale, iterations_per_call)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _state(self, v, default):
        v = np.full(self.B, default, np.int32) if v is None else np.array(np.broadcast_to(_i32(v), (self.B,)))
        return _up(v)

    def hypotheses(self):
        """viorb_sim3_hypotheses_device: (R12 [B,it,3,3], t12 [B,it,3], s12 [B,it]) device tensors and reason [B,it] (host)."""
        t = self.torch
        R = t.zeros((self.B, self.iters, 3, 3), dtype=t.float32, device=self.dev)
        tt = t.zeros((self.B, self.iters, 3), dtype=t.float32, device=self.dev)
        s = t.zeros((self.B, self.iters), dtype=t.float32, device=self.dev)
        reason = t.zeros((self.B, self.iters), dtype=t.int32, device=self.dev)
        cfg = self._cfg()
        check(lib().viorb_sim3_hypotheses_device(C.byref(self.inputs), C.byref(cfg), ptr(self.sets), self.B, ptr(R), ptr(tt), ptr(s), ptr(reason),
                                                 self.ws_ptr, self.ws_bytes, self._stream()))
        t.cuda.synchronize(self.dev)
        return R, tt, s, reason.cpu().numpy()

    def inliers(self, R, tt, s, flags=False):
        """viorb_sim3_inliers_device on device models: counts [B,it] and, on request, flags [B,it,cap] (host)."""
        t = self.torch
        cnt = t.zeros((self.B, self.iters), dtype=t.int32, device=self.dev)
        fl = t.zeros((self.B, self.iters, self.cap), dtype=t.uint8, device=self.dev) if flags else None
        cfg = self._cfg()
        check(lib().viorb_sim3_inliers_device(C.byref(self.inputs), C.byref(cfg), self.B, ptr(R), ptr(tt), ptr(s), ptr(cnt), ptr(fl), self.ws_ptr,
                                              self.ws_bytes, self._stream()))
        t.cuda.synchronize(self.dev)
        return cnt.cpu().numpy(), (fl.cpu().numpy() if flags else None)

    def select(self, counts, max_its=None, first_iteration=None, best_inliers_in=None, iterations_per_call=5):
        """viorb_sim3_select_device on counts [B,it] (host array): dict of status, iterations_done, best_inliers, best_iter [B]."""
        t = self.torch
        dc = _up(_i32(counts).reshape(self.B, self.iters))
        o = [t.zeros(self.B, dtype=t.int32, device=self.dev) for _ in range(4)]
        cfg = self._cfg(iterations_per_call)
        mx, fi, bi = self._state(max_its, self.iters), self._state(first_iteration, 0), self._state(best_inliers_in, 0)      # alive until the synchronise
        check(lib().viorb_sim3_select_device(C.byref(cfg), ptr(dc), ptr(self.d[6]), ptr(mx), ptr(fi), ptr(bi), self.B, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), self._stream()))
        t.cuda.synchronize(self.dev)
        return dict(zip(("status", "iterations_done", "best_inliers", "best_iter"), [v.cpu().numpy() for v in o]))

    def ransac(self, max_its=None, first_iteration=None, best_inliers_in=None, iterations_per_call=5):
        """viorb_sim3_ransac_device: one dict per pair."""
        t = self.torch
        dt = {"i4": t.int32, "f4": t.float32, "u1": t.uint8}
        out = {f: t.zeros(_shape(f, self.cap, self.B), dtype=dt[_OUT[f][0]], device=self.dev) for f in capi.SIM3_OUTPUT_FIELDS}
        O = capi.Sim3Outputs(**{f: ptr(out[f]) for f in out})
        cfg = self._cfg(iterations_per_call)
        mx, fi, bi = self._state(max_its, self.iters), self._state(first_iteration, 0), self._state(best_inliers_in, 0)      # alive until the synchronise
        check(lib().viorb_sim3_ransac_device(C.byref(self.inputs), C.byref(cfg), ptr(self.sets), ptr(mx), ptr(fi), ptr(bi), self.B, C.byref(O),
                                             self.ws_ptr, self.ws_bytes, self._stream()))
        t.cuda.synchronize(self.dev)
        host = {f: v.cpu().numpy() for f, v in out.items()}
        return [_trim({f: host[f][b] for f in host}, self.n[b]) for b in range(self.B)]


# ---- host hooks (sim3_core.h compiled for the host) ------------------------------------------------------------------------------------
def debug_horn(P1, P2, fix_scale=False):
    """(reason, R [3,3], t [3], s) from three correspondences P1, P2 [3,3] (one point per row)."""
    R, t, s = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(1, np.float32)
    reason = lib().viorb_debug_sim3_horn(ptr(_f32(P1)), ptr(_f32(P2)), int(bool(fix_scale)), ptr(R), ptr(t), ptr(s))
    return reason, R.reshape(3, 3), t, s[0]


def debug_inlier(R, t, s, K1, K2, X1c, X2c, sigma2_1, sigma2_2):
    """(inlier, err [2], max [2]) of one correspondence."""
    err, mx = np.zeros(2, np.float32), np.zeros(2, np.float32)
    inl = lib().viorb_debug_sim3_inlier(ptr(_f32(R)), ptr(_f32(t)), float(np.float32(s)), ptr(_f32(K1)), ptr(_f32(K2)), ptr(_f32(X1c)), ptr(_f32(X2c)),
                                        float(np.float32(sigma2_1)), float(np.float32(sigma2_2)), ptr(err), ptr(mx))
    return bool(inl), err, mx


def debug_select(counts, n, min_inliers, max_its, first_iteration=0, best_inliers_in=0, iterations_per_call=5):
    """(status, iterations_done, best_inliers, best_iter) of the acceptance rule over a list of counts."""
    c, o = _i32(counts), np.zeros(4, np.int32)
    check(lib().viorb_debug_sim3_select(ptr(c), len(c), int(n), int(min_inliers), int(max_its), int(first_iteration), int(best_inliers_in),
                                        int(iterations_per_call), ptr(o)))
    return tuple(int(v) for v in o)


# ---- Optimizer::OptimizeSim3 -------------------------------------------------------------------------------------------------------------
_f64 = lambda a: np.ascontiguousarray(a, np.float64)
_u8 = lambda a: np.ascontiguousarray(a, np.uint8)


def _opt_arrays(prob, valid):
    X1, X2 = _f32(prob["X1c"]).reshape(-1, 3), _f32(prob["X2c"]).reshape(-1, 3)
    n = len(X1)
    w1 = _f32(prob["inv_sigma2_1"]) if "inv_sigma2_1" in prob else np.float32(1) / _f32(prob["sigma2_1"])
    w2 = _f32(prob["inv_sigma2_2"]) if "inv_sigma2_2" in prob else np.float32(1) / _f32(prob["sigma2_2"])
    v = np.ones(n, np.uint8) if valid is None else _u8(valid)
    return [X1, X2, _f32(prob["obs1"]).reshape(-1, 2), _f32(prob["obs2"]).reshape(-1, 2), _f32(w1), _f32(w2), v, _f32(prob["K1"]), _f32(prob["K2"])], n


def _opt_result(S, keep, n_in, info):
    return dict(S12=S, keep=keep, n_in=int(n_in), info=info)


def optimize_sim3(prob, S12, th2=10.0, fix_scale=False, valid=None):
    """viorb_optimize_sim3 (host buffers, one pair): dict(S12 [8] = r(xyzw) t s, keep [n], n_in, info [8]). prob as for sim3_ransac plus
    obs1, obs2 [n,2]; the information of an edge is 1 / sigma2 (or prob["inv_sigma2_1/2"])."""
    a, n = _opt_arrays(prob, valid)
    S, keep, n_in, info = np.zeros(8), np.zeros(max(n, 1), np.uint8), C.c_int32(0), np.zeros(8)
    check(lib().viorb_optimize_sim3(ptr(_f64(S12)), float(th2), int(bool(fix_scale)), *[ptr(x) for x in a], n, ptr(S), ptr(keep), C.byref(n_in), ptr(info)))
    return _opt_result(S, keep[:n], n_in.value, info)


def optimize_sim3_batch(probs, S12s, th2=10.0, fix_scale=False, valids=None, device=0):
    """viorb_optimize_sim3_device for a list of problems (uploaded here): one dict per pair."""
    import torch
    B = len(probs)
    arrs = [_opt_arrays(p, None if valids is None else valids[b]) for b, p in enumerate(probs)]
    ns = [n for _, n in arrs]
    cap = max(max(ns), 1)
    shapes = [(cap, 3), (cap, 3), (cap, 2), (cap, 2), (cap,), (cap,), (cap,), (4,), (4,)]
    host = [np.zeros((B,) + sh, arrs[0][0][k].dtype) for k, sh in enumerate(shapes)]
    for b, (a, n) in enumerate(arrs):
        for k in range(9):
            if k < 7:
                host[k][b, :n] = a[k]
            else:
                host[k][b] = a[k]
    d = [_up(_f64(np.stack([_f64(s) for s in S12s])), device)] + [_up(h, device) for h in host] + [_up(np.array(ns, np.int32), device)]
    I = capi.Sim3OptInputs(*[ptr(x) for x in d], cap)
    dev = torch.device("cuda", device)
    S = torch.zeros((B, 8), dtype=torch.float64, device=dev); keep = torch.zeros((B, cap), dtype=torch.uint8, device=dev)
    n_in = torch.zeros(B, dtype=torch.int32, device=dev); info = torch.zeros((B, 8), dtype=torch.float64, device=dev)
    check(lib().viorb_optimize_sim3_device(C.byref(I), float(th2), int(bool(fix_scale)), B, ptr(S), ptr(keep), ptr(n_in), ptr(info),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    S, keep, n_in, info = S.cpu().numpy(), keep.cpu().numpy(), n_in.cpu().numpy(), info.cpu().numpy()
    return [_opt_result(S[b], keep[b, :ns[b]], n_in[b], info[b]) for b in range(B)]


def debug_exp(u7, est8=(0, 0, 0, 1, 0, 0, 0, 1)):
    """(exp(u) [8], exp(u) * estimate [8]) as r(xyzw) t s."""
    e, p = np.zeros(8), np.zeros(8)
    check(lib().viorb_debug_sim3_exp(ptr(_f64(u7)), ptr(_f64(est8)), ptr(e), ptr(p)))
    return e, p


def debug_edges(S8, X1c, X2c, obs1, obs2, K1, K2, fix_scale=False):
    """(e12 [2], e21 [2], J12 [2,7], J21 [2,7]) of one correspondence, with g2o's numeric Jacobians."""
    e, J = np.zeros(4), np.zeros(28)
    check(lib().viorb_debug_sim3_edges(ptr(_f64(S8)), ptr(_f64(X1c)), ptr(_f64(X2c)), ptr(_f64(obs1)), ptr(_f64(obs2)), ptr(_f64(K1)), ptr(_f64(K2)),
                                       int(bool(fix_scale)), ptr(e), ptr(J)))
    return e[:2], e[2:], J[:14].reshape(2, 7), J[14:].reshape(2, 7)
