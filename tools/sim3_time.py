"""Time of the Sim3 RANSAC solver (viorb_sim3_ransac_device) at 300 correspondences and 300 sets for 1, 8 and 64 key-frame pairs: device
events around the call, then the library's per-kernel profiler over the same calls. Two forms of the call are timed: all 300 iterations
in one call (Sim3Solver::find) and the five iterations per call of LoopClosing::ComputeSim3, for which the kernels skip the iterations no
pair can reach. For context only, the wall time of the numpy checker (tests/sim3_ref.py, mode "f32") on one of the problems. Prints one
JSON line per batch size and form, then the same sizes through viorb_optimize_sim3_device (the kernel's time from the profiler; the wall
time includes the upload). Needs a HIP device (no fallback)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viorb_amd
from viorb_amd import capi, sim3
from viorb_amd.synth import make_sim3_problem


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--correspondences", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic problems, repeated over the pairs")
    a = ap.parse_args()
    L = viorb_amd.lib()
    if L.viorb_device_count() < 1:
        raise SystemExit("sim3_time.py needs a HIP device")
    import torch
    base = [make_sim3_problem(70 + k, "general", a.correspondences, 0.3, 0.5, 0.002) for k in range(a.distinct)]
    sets = [sim3.draw_sets(a.correspondences, a.iterations, k) for k in range(a.distinct)]
    for B in a.pairs:
        run = sim3.Sim3Batch([base[b % len(base)] for b in range(B)], [sets[b % len(base)] for b in range(B)])
        dt = {"i4": torch.int32, "f4": torch.float32, "u1": torch.uint8}
        out = {f: torch.zeros(sim3._shape(f, run.cap, B), dtype=dt[sim3._OUT[f][0]], device=run.dev) for f in capi.SIM3_OUTPUT_FIELDS}
        O = capi.Sim3Outputs(**{f: sim3.ptr(out[f]) for f in out})
        mx, fi, bi = run._state(None, a.iterations), run._state(None, 0), run._state(None, 0)
        for per_call in (a.iterations, 5):
            cfg = run._cfg(per_call)
            call = lambda: sim3.check(L.viorb_sim3_ransac_device(C.byref(run.inputs), C.byref(cfg), sim3.ptr(run.sets), sim3.ptr(mx), sim3.ptr(fi), sim3.ptr(bi), B,
                                                                 C.byref(O), run.ws_ptr, run.ws_bytes, run._stream()))
            ms = []
            for rep in range(a.reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record(); torch.cuda.synchronize()
                if rep >= 3:
                    ms.append(e0.elapsed_time(e1))
            torch.cuda.synchronize(); L.viorb_profile_select(None); L.viorb_profile_reset(); L.viorb_profile_enable(1)
            for _ in range(a.reps):
                call()
            torch.cuda.synchronize(); L.viorb_profile_enable(0)
            prof = {k: round(v[0] / a.reps, 4) for k, v in profile().items() if k.startswith("k_sim3_")}
            print(json.dumps({"pairs": B, "correspondences": a.correspondences, "iterations": a.iterations, "iterations_per_call": per_call,
                              "call_ms_median": float(np.median(ms)), "call_ms_min": float(np.min(ms)), "call_ms_per_pair": float(np.median(ms)) / B,
                              "kernel_ms_per_call": prof, "status_first_pairs": [int(s) for s in out["status"].cpu().numpy()[:4]],
                              "n_inliers_first_pairs": [int(s) for s in out["n_inliers"].cpu().numpy()[:4]]}), flush=True)
    import sim3_ref as T
    # OptimizeSim3 at the same sizes: the truth moved a little as the initial Sim3, every correspondence valid
    for B in a.pairs:
        probs = [base[b % len(base)] for b in range(B)]
        S0 = [T.sim3_pack(T.sim3_mul(T.sim3_exp([0.004, -0.003, 0.002, 0.02, -0.01, 0.02, 0.01]),
                                     (T.mat2q(np.asarray(p["R12"], float)), np.asarray(p["t12"], float), float(p["s12"])))) for p in probs]
        ms = []
        for rep in range(a.reps + 3):
            t0 = time.perf_counter()
            out = sim3.optimize_sim3_batch(probs, S0, 10.0, False)
            ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize(); L.viorb_profile_select(None); L.viorb_profile_reset(); L.viorb_profile_enable(1)
        for _ in range(a.reps):
            sim3.optimize_sim3_batch(probs, S0, 10.0, False)
        torch.cuda.synchronize(); L.viorb_profile_enable(0)
        prof = {k: round(v[0] / a.reps, 4) for k, v in profile().items() if k == "k_sim3_optimize"}
        print(json.dumps({"what": "viorb_optimize_sim3_device", "pairs": B, "correspondences": a.correspondences, "kernel_ms_per_call": prof,
                          "wall_ms_with_upload_median": float(np.median(ms[3:])), "n_in_first_pairs": [o["n_in"] for o in out[:4]],
                          "iterations_first_pair": [int(out[0]["info"][2]), int(out[0]["info"][3])]}), flush=True)
    t0 = time.perf_counter()
    r = T.optimize_sim3(base[0], S0[0], 10.0, False)
    print(json.dumps({"numpy_checker_optimiser_one_pair_ms": (time.perf_counter() - t0) * 1e3, "n_in": int(r["n_in"])}), flush=True)
    t0 = time.perf_counter()
    r = T.ransac(base[0], sets[0], "f32", per_call=a.iterations)
    print(json.dumps({"numpy_checker_f32_one_pair_ms": (time.perf_counter() - t0) * 1e3, "status": int(r["status"])}), flush=True)


if __name__ == "__main__":
    main()
