"""Visual-inertial initialisation (LocalMapping::TryInitVIO: gyro bias, scale, gravity, accelerometer bias) through the C ABI of
include/viorb.h. A stream is a dict(twc12 [N,12] f32 = Rwc(9) twc(3) of KeyFrame::GetPoseInverse(), kf_time [N], imu [n,7] =
gyro3 acc3 t, imu_start [N+1] offsets of the interval before each key frame) as synth.make_vi_init_problem returns it; the config is
dict(Tbc [4,4], g) with optional gyr_meas_cov / acc_meas_cov."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as _up

EST = dict(bg=slice(0, 3), sstar=3, gwstar=slice(4, 7), s=7, dtheta=slice(8, 10), ba=slice(10, 13), Rwi=slice(13, 22), Rwi_=slice(22, 31),
           gw=slice(31, 34), w=slice(34, 38), w2=slice(38, 44))

_f64 = lambda a: np.ascontiguousarray(a, np.float64)
_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)


def vi_config(cfg):
    """viorb_vi_init_config from dict(Tbc, g[, gyr_meas_cov, acc_meas_cov])."""
    c = capi.ViInitConfig()
    for i, v in enumerate(_f64(cfg["Tbc"]).ravel()):
        c.Tbc[i] = v
    c.g = float(cfg["g"]); c.gyr_meas_cov = float(cfg.get("gyr_meas_cov", 0.0)); c.acc_meas_cov = float(cfg.get("acc_meas_cov", 0.0))
    return c


def unpack_est(est):
    """est[48] -> dict of named views (bg, sstar, gwstar, s, dtheta, ba, Rwi, Rwi_, gw, w, w2)."""
    e = _f64(est)
    return {k: (e[v].reshape(3, 3) if k in ("Rwi", "Rwi_") else e[v]) for k, v in EST.items()}


def pack_streams(streams, n_kf=None, max_kf=None):
    """Ragged streams -> the batch arrays of the device forms: n_kf [B], kf_time [B,max_kf], imu_start [B,max_kf+1] into one pooled imu,
    twc12 [B,max_kf,12]. n_kf[b] key frames of stream b are used (default: all it has)."""
    B = len(streams)
    n_kf = [len(s["kf_time"]) for s in streams] if n_kf is None else list(n_kf)
    max_kf = max_kf or max(n_kf + [1])
    t, st, T = np.zeros((B, max_kf)), np.zeros((B, max_kf + 1), np.int32), np.zeros((B, max_kf, 12), np.float32)
    pool, base = [], 0
    for b, s in enumerate(streams):
        n = n_kf[b]
        t[b, :n] = _f64(s["kf_time"])[:n]
        if "twc12" in s:
            T[b, :n] = _f32(s["twc12"])[:n]
        off = _i32(s["imu_start"])
        st[b, :n + 1] = off[:n + 1] + base
        st[b, n + 1:] = st[b, n]
        pool.append(_f64(s["imu"]).reshape(-1, 7)); base += len(pool[-1])
    imu = np.concatenate(pool) if base else np.zeros((1, 7))
    return dict(n_kf=_i32(n_kf), kf_time=t, imu_start=st, imu=_f64(imu), total_imu=base, twc12=T, max_kf=max_kf, B=B)


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def PreintegrateIntervals(stream, bg=None, ba=None, clamp=True, gyr_meas_cov=0.0, acc_meas_cov=0.0):
    """viorb_preintegrate_intervals: host buffers, one stream. Returns preint [N,142]."""
    n = len(stream["kf_time"])
    out = np.zeros((n, 142))
    check(lib().viorb_preintegrate_intervals(n, ptr(_f64(stream["kf_time"])), ptr(_i32(stream["imu_start"])), ptr(_f64(stream["imu"])),
                                             ptr(_f64(bg)) if bg is not None else None, ptr(_f64(ba)) if ba is not None else None,
                                             gyr_meas_cov, acc_meas_cov, 0 if clamp else capi.PREINT_NO_CLAMP, ptr(out)))
    return out


def PreintegrateIntervalsBatch(streams, bg=None, ba=None, clamp=True, max_kf=None, packed=None):
    """viorb_preintegrate_intervals_device for a ragged batch (uploaded here, one launch): preint [B,max_kf,142]. bg / ba: [B,3] or None.
    packed: the arrays of pack_streams, when the caller has laid them out itself."""
    torch, dev = _dev()
    p = packed or pack_streams(streams, max_kf=max_kf)
    d = {k: _up(p[k]) for k in ("n_kf", "kf_time", "imu_start", "imu")}
    dbg = _up(_f64(bg).reshape(p["B"], 3)) if bg is not None else None
    dba = _up(_f64(ba).reshape(p["B"], 3)) if ba is not None else None
    out = torch.full((p["B"], p["max_kf"], 142), float("nan"), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lib().viorb_preintegrate_intervals_device(ptr(d["n_kf"]), ptr(d["kf_time"]), ptr(d["imu_start"]), ptr(d["imu"]), p["total_imu"], ptr(dbg), ptr(dba),
                                                    0.0, 0.0, 0 if clamp else capi.PREINT_NO_CLAMP, p["max_kf"], p["B"], ptr(out), C.c_void_p(st)))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def OptimizeInitialGyroBias(cfg, twc12, preint_in, device=False):
    """Optimizer::OptimizeInitialGyroBias(vTwc, vImuPreInt) for one stream: (bg [3], status). device=True: through the device form."""
    c = vi_config(cfg)
    T, P = _f32(twc12).reshape(-1, 12), _f64(preint_in).reshape(-1, 142)
    n = len(T)
    if not device:
        bg, st = np.zeros(3), np.zeros(1, np.int32)
        check(lib().viorb_optimize_initial_gyro_bias(C.byref(c), n, ptr(T), ptr(P), ptr(bg), ptr(st)))
        return bg, int(st[0])
    torch, dev = _dev()
    dn, dT, dP = _up(np.array([n], np.int32)), _up(T), _up(P)
    bg = torch.zeros((1, 3), dtype=torch.float64, device=dev); st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    check(lib().viorb_optimize_initial_gyro_bias_device(C.byref(c), ptr(dn), ptr(dT), ptr(dP), n, 1, ptr(bg), ptr(st), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    return bg.cpu().numpy()[0], int(st.item())


class ViInit:
    """viorb_vi_init_device for a ragged batch of streams: the arrays are uploaded once, __call__() enqueues the three kernels on the
    current torch stream without a host synchronisation, results() downloads (est [B,48], status [B], preint_bg [B,max_kf,142]).
    n_est[b] = how many of stream b's key frames enter the estimate (default: all); preint_in: [B,max_kf,142] or None = computed here
    with zero biases by viorb_preintegrate_intervals_device (what the key frames hold before initialisation)."""

    def __init__(self, cfg, streams, n_est=None, max_kf=None, preint_in=None):
        torch, dev = _dev()
        self.cfg = vi_config(cfg)
        p = self.p = pack_streams(streams, n_kf=n_est, max_kf=max_kf)
        self.d = {k: _up(p[k]) for k in ("n_kf", "kf_time", "imu_start", "imu", "twc12")}
        B, K = p["B"], p["max_kf"]
        self.est = torch.full((B, 48), float("nan"), dtype=torch.float64, device=dev)
        self.status = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.preint_bg = torch.full((B, K, 142), float("nan"), dtype=torch.float64, device=dev)
        if preint_in is None:
            self.preint_in = torch.zeros((B, K, 142), dtype=torch.float64, device=dev)
            d = self.d
            check(lib().viorb_preintegrate_intervals_device(ptr(d["n_kf"]), ptr(d["kf_time"]), ptr(d["imu_start"]), ptr(d["imu"]), p["total_imu"], None, None,
                                                            self.cfg.gyr_meas_cov, self.cfg.acc_meas_cov, 0, K, B, ptr(self.preint_in),
                                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        else:
            self.preint_in = _up(_f64(preint_in).reshape(B, K, 142))

    def __call__(self):
        torch, dev = _dev()
        d, p = self.d, self.p
        check(lib().viorb_vi_init_device(C.byref(self.cfg), ptr(d["n_kf"]), ptr(d["kf_time"]), ptr(d["imu_start"]), ptr(d["imu"]), p["total_imu"], ptr(d["twc12"]),
                                         ptr(self.preint_in), p["max_kf"], p["B"], ptr(self.est), ptr(self.status), ptr(self.preint_bg),
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return self

    def results(self):
        torch, dev = _dev()
        torch.cuda.synchronize(dev)
        return self.est.cpu().numpy(), self.status.cpu().numpy(), self.preint_bg.cpu().numpy()


    def apply(self, streams, pose12, n_kf=None, preint_v=None, points=None, min_dist=None, max_dist=None):
        """viorb_vi_init_apply_device (and viorb_scale_map_points_device when points [B,np,3] are given) on the estimate this object
        holds, still without a host synchronisation: `streams` are the same streams with all the key frames they have by now
        (n_kf[b] >= n_est[b]; uploaded here), pose12 [B,max_kf,12] their Tcw. preint_v: None = the re-integration preint_bg.
        Returns a function that synchronises and downloads dict(navstate, pose12_scaled, preint[, points, min_dist, max_dist])."""
        torch, dev = _dev()
        q = pack_streams(streams, n_kf=n_kf, max_kf=self.p["max_kf"])
        d = {k: _up(q[k]) for k in ("n_kf", "kf_time", "imu_start", "imu", "twc12")}
        B, K = q["B"], q["max_kf"]
        ns = torch.full((B, K, 22), float("nan"), dtype=torch.float64, device=dev)
        pre = torch.full((B, K, 142), float("nan"), dtype=torch.float64, device=dev)
        dpose = _up(_f32(pose12).reshape(B, K, 12)); out_pose = torch.full((B, K, 12), float("nan"), dtype=torch.float32, device=dev)
        pv = self.preint_bg if preint_v is None else _up(_f64(preint_v).reshape(B, K, 142))
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib().viorb_vi_init_apply_device(C.byref(self.cfg), ptr(self.d["n_kf"]), ptr(d["n_kf"]), ptr(d["kf_time"]), ptr(d["imu_start"]), ptr(d["imu"]),
                                               q["total_imu"], ptr(d["twc12"]), ptr(dpose), ptr(self.est), ptr(self.status), ptr(pv), K, B, ptr(ns), ptr(out_pose),
                                               ptr(pre), st))
        dev_pts = None
        if points is not None:
            dev_pts = [_up(_f32(points)), _up(_f32(min_dist)) if min_dist is not None else None, _up(_f32(max_dist)) if max_dist is not None else None]
            check(lib().viorb_scale_map_points_device(ptr(dev_pts[0]), ptr(dev_pts[1]), ptr(dev_pts[2]), ptr(self.est), ptr(self.status),
                                                      dev_pts[0].shape[1], B, st))

        def results():
            torch.cuda.synchronize(dev)
            r = dict(navstate=ns.cpu().numpy(), pose12_scaled=out_pose.cpu().numpy(), preint=pre.cpu().numpy())
            if dev_pts is not None:
                r.update(points=dev_pts[0].cpu().numpy(), min_dist=None if dev_pts[1] is None else dev_pts[1].cpu().numpy(),
                         max_dist=None if dev_pts[2] is None else dev_pts[2].cpu().numpy())
            return r
        return results


def ViInitApplyHost(cfg, stream, pose12, est, preint_v, n_est, n_kf=None):
    """viorb_vi_init_apply: the host-buffer form for one stream whose estimate is OK. Returns (navstate [n_kf,22], pose12_scaled, preint)."""
    c = vi_config(cfg)
    K = n_kf or len(stream["kf_time"])
    ns, po, pre = np.zeros((K, 22)), np.zeros((K, 12), np.float32), np.zeros((K, 142))
    check(lib().viorb_vi_init_apply(C.byref(c), n_est, K, ptr(_f64(_f64(stream["kf_time"])[:K])), ptr(_i32(_i32(stream["imu_start"])[:K + 1])), ptr(_f64(stream["imu"])),
                                    ptr(_f32(_f32(stream["twc12"])[:K])), ptr(_f32(_f32(pose12).reshape(-1, 12)[:K])), ptr(_f64(est)),
                                    ptr(_f64(_f64(preint_v).reshape(-1, 142)[:K])), ptr(ns), ptr(po), ptr(pre)))
    return ns, po, pre


def ViInitHost(cfg, stream, preint_in, n_est=None):
    """viorb_vi_init: the host-buffer form for one stream. Returns (est [48], status, preint_bg [n_est,142])."""
    c = vi_config(cfg)
    n = n_est or len(stream["kf_time"])
    est, st, pb = np.full(48, np.nan), np.full(1, -1, np.int32), np.zeros((n, 142))
    off = _i32(_i32(stream["imu_start"])[:n + 1])
    check(lib().viorb_vi_init(C.byref(c), n, ptr(_f64(_f64(stream["kf_time"])[:n])), ptr(off), ptr(_f64(stream["imu"])), ptr(_f32(_f32(stream["twc12"])[:n])),
                              ptr(_f64(_f64(preint_in).reshape(-1, 142)[:n])), ptr(est), ptr(st), ptr(pb)))
    return est, int(st[0]), pb
