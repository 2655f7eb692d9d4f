"""Time of the visual-inertial initialisation for streams of N = 60 key frames with 50 IMU samples per interval, for 1 and 1024 streams:
  vi_init    one viorb_vi_init_device call (gyro bias, re-integration of all intervals, both solves), device events around it;
  preint     viorb_preintegrate_intervals_device alone over the same intervals;
  apply      viorb_vi_init_apply_device (final pre-integration + NavStates + scaled poses);
  predict    the same N - 1 intervals through viorb_frontend_imu_predict_device, one call per interval over all streams: the only
             device path the library had for this work before (it also predicts a NavState and a pose per row);
  cpu        tests/vi_init_ref.py's float64 restatement of one stream (oracle pre-integration + numpy), host clock, one warm-up run
             and the median of three.
Device figures: warm-up calls first, then the median of --reps timed calls, HIP events around the call. For `predict` the events
bracket 59 asynchronous launches issued one by one through the Python wrapper: at one stream that figure is mostly launch and wrapper
time on the host (each launch is one workgroup), at 1024 streams the kernels outlast their launches. Prints one JSON line per stream count. Needs a HIP device (no fallback)."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viorb_amd
from viorb_amd import capi
from viorb_amd.capi import lib, check, ptr
from viorb_amd.synth import make_vi_init_problem, euroc_cam


def timed(torch, fn, reps, warm=3):
    ms = []
    for rep in range(reps + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        if rep >= warm:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 1024])
    ap.add_argument("--keyframes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic streams, repeated over the batch")
    a = ap.parse_args()
    if lib().viorb_device_count() < 1:
        raise SystemExit("vi_init_time.py needs a HIP device")
    import ctypes as C
    import torch
    import vi_init_ref as vr
    N = a.keyframes
    Tbc = make_vi_init_problem(0, 4)["Tbc"]
    base = [make_vi_init_problem(200 + k, N, kf_dt=0.25, imu_dt=0.005, Tbc=Tbc) for k in range(a.distinct)]
    cfg = dict(Tbc=Tbc, g=base[0]["g"])
    cpu = []
    for rep in range(4):
        t0 = time.perf_counter(); ref = vr.vi_init(base[0]); cpu.append((time.perf_counter() - t0) * 1e3)
    cpu_ms = float(np.median(cpu[1:]))
    dev = torch.device("cuda", 0)
    for B in a.streams:
        ss = [base[b % len(base)] for b in range(B)]
        run = viorb_amd.ViInit(cfg, ss)
        d, p = run.d, run.p
        st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        out = torch.zeros((B, N, 142), dtype=torch.float64, device=dev)
        vi = timed(torch, lambda: run(), a.reps)
        pre = timed(torch, lambda: check(lib().viorb_preintegrate_intervals_device(ptr(d["n_kf"]), ptr(d["kf_time"]), ptr(d["imu_start"]), ptr(d["imu"]), p["total_imu"],
                                                                                   None, None, 0.0, 0.0, 0, N, B, ptr(out), st())), a.reps)
        pose = torch.zeros((B, N, 12), dtype=torch.float32, device=dev)
        ns_out = torch.zeros((B, N, 22), dtype=torch.float64, device=dev); pose_out = torch.zeros_like(pose)
        ap_ms = timed(torch, lambda: check(lib().viorb_vi_init_apply_device(C.byref(run.cfg), ptr(d["n_kf"]), ptr(d["n_kf"]), ptr(d["kf_time"]), ptr(d["imu_start"]),
                                                                            ptr(d["imu"]), p["total_imu"], ptr(d["twc12"]), ptr(pose), ptr(run.est), ptr(run.status),
                                                                            ptr(run.preint_bg), N, B, ptr(ns_out), ptr(pose_out), ptr(out), st())), a.reps)
        est, status, _ = run.results()
        # the parent's path: one k_imu_predict launch per interval, rows = streams
        fe = viorb_amd.Frontend(euroc_cam(), np.array([0, 0, -9.8]), np.ones(8, np.float32), np.ones(8, np.float32), max_batch=B, cap=64)
        imu = torch.from_numpy(np.stack([np.stack([s["imu"][s["imu_start"][i]:s["imu_start"][i + 1]] for s in ss]) for i in range(1, N)])).to(dev)   # [N-1,B,50,7]
        kt = torch.from_numpy(np.stack([s["kf_time"] for s in ss]).T.copy()).to(dev)                                                                  # [N,B]
        ns = torch.zeros((B, 22), dtype=torch.float64, device=dev); ns[:, 9] = 1
        o1 = torch.zeros((B, 142), dtype=torch.float64, device=dev); o2 = torch.zeros((B, 22), dtype=torch.float64, device=dev); o3 = torch.zeros((B, 12), dtype=torch.float32, device=dev)
        def predict():
            for i in range(N - 1):
                fe.imu_predict(imu[i], kt[i], kt[i + 1], ns, o1, o2, o3)
        pr = timed(torch, predict, a.reps)
        print(json.dumps({"streams": B, "keyframes": N, "samples_per_interval": int(imu.shape[2]), "vi_init_ms_median": vi[0], "vi_init_ms_min": vi[1],
                          "preint_intervals_ms_median": pre[0], "apply_ms_median": ap_ms[0], "imu_predict_per_interval_ms_median": pr[0],
                          "cpu_restatement_one_stream_ms": cpu_ms, "status_nonzero": int((status != 0).sum()),
                          "s_first_stream": float(est[0, 7]), "s_restatement": float(ref["s"])}), flush=True)


if __name__ == "__main__":
    main()
