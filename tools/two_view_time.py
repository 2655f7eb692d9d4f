"""Time of the two-view initialiser (viorb_two_view_init_device) at 1000 key points per frame, about 300 matches and 200 iterations,
for 1, 16 and 256 streams: device events around the call, then the library's per-kernel profiler over the same calls. For context
only, the wall time of the numpy checker (tests/two_view_ref.py, mode "f32") on one of the problems. Prints one JSON line per stream
count. Needs a HIP device (no fallback)."""
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
from viorb_amd import two_view as tv
from viorb_amd.synth import make_two_view_init_problem


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic problems, repeated over the streams")
    a = ap.parse_args()
    L = viorb_amd.lib()
    if L.viorb_device_count() < 1:
        raise SystemExit("two_view_time.py needs a HIP device")
    import torch
    kinds = ("general", "planar", "forward", "general")
    base = [make_two_view_init_problem(50 + k, kinds[k % 4], a.features, a.features + 40, a.matches, 0.1, 0.5) for k in range(a.distinct)]
    sets = [tv.draw_sets(a.matches, a.iterations, k) for k in range(a.distinct)]
    for B in a.streams:
        run = tv.TwoViewBatch([base[b % len(base)] for b in range(B)], [sets[b % len(base)] for b in range(B)])
        out, O = run._outputs()
        call = lambda: tv.check(L.viorb_two_view_init_device(*run._in(), tv.ptr(run.sets), run.B, C.byref(O), run.ws_ptr, run.ws_bytes, run._stream()))
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
        prof = {k: round(v[0] / a.reps, 4) for k, v in profile().items() if k.startswith("k_tv_")}
        status = out["status"].cpu().numpy()
        print(json.dumps({"streams": B, "features": a.features, "matches": a.matches, "iterations": a.iterations, "call_ms_median": float(np.median(ms)),
                          "call_ms_min": float(np.min(ms)), "call_ms_per_stream": float(np.median(ms)) / B, "kernel_ms_per_call": prof,
                          "status_first_streams": [int(s) for s in status[:4]]}), flush=True)
    import two_view_ref as T
    t0 = time.perf_counter()
    r = T.initialise(base[0], sets[0], "f32")
    print(json.dumps({"numpy_checker_f32_one_stream_ms": (time.perf_counter() - t0) * 1e3, "status": int(r["status"])}), flush=True)


if __name__ == "__main__":
    main()
