"""Time of the monocular matcher (include/viorb_search_init.h) at the shapes Tracking::MonocularInitialization calls it with:
viorb_search_for_initialization_device for 1 and 64 streams of about 2000 and 4000 features per frame, window 100, nnratio 0.9, with the
orientation check, and viorb_scene_median_depth_device beside it. Device events around the call (inputs uploaded before, prev_matched
restored before every call), then the library's per-kernel profiler over the same calls with each kernel's share and the sweeps of the
ordered phase; one JSON line per shape. For context only, the wall time of the numpy checker (tests/search_init_ref.py) on the first
shape. Needs a HIP device (no fallback)."""
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
from viorb_amd import capi
from viorb_amd import search_init as M
from viorb_amd.capi import check, ptr, _torch_up as up
from viorb_amd.synth import make_search_init_problem


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def measure(call, before, reps, prefixes):
    import torch
    L = viorb_amd.lib()
    ms = []
    for rep in range(reps + 3):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        if rep >= 3:
            ms.append(e0.elapsed_time(e1))
    torch.cuda.synchronize(); L.viorb_profile_select(None); L.viorb_profile_reset(); L.viorb_profile_enable(1)
    for _ in range(reps):
        before(); call()
    torch.cuda.synchronize(); L.viorb_profile_enable(0)
    prof = {k: v[0] / reps for k, v in profile().items() if k.startswith(prefixes)}
    total = sum(prof.values()) or 1.0
    return {"call_ms_median": float(np.median(ms)), "call_ms_min": float(np.min(ms)), "kernel_ms_per_call": {k: round(v, 4) for k, v in prof.items()},
            "kernel_share": {k: round(v / total, 3) for k, v in prof.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--features", type=int, nargs="*", default=[2000, 4000])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
    a = ap.parse_args()
    L = viorb_amd.lib()
    if L.viorb_device_count() < 1:
        raise SystemExit("search_init_time.py needs a HIP device")
    import torch
    import search_init_ref as T
    dev = torch.device("cuda", 0)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    first = True
    for n in a.features:
        P = make_search_init_problem(1, n_scene=n, siblings=n // 10, twins=n // 13)
        n1, n2 = len(P["kps1"]), len(P["kps2"])
        cap = max(n1, n2)
        for B in a.batches:
            bt = M.SearchInitBatch([(P["kps1"], P["desc1"])] * B, [P["prev_matched"]] * B, P["bounds4"], cap)
            kps2, desc2, count2 = bt._frames([(P["kps2"], P["desc2"])] * B)
            cs = torch.zeros((B, M.GRID_CELLS + 1), dtype=torch.int32, device=dev)
            ci = torch.zeros((B, cap), dtype=torch.int32, device=dev)
            check(L.viorb_keyframe_grid_device(ptr(kps2), ptr(count2), cap, B, ptr(bt.bounds), ptr(cs), ptr(ci), stream()))
            kf = capi.S3mKeyframes(ptr(kps2), ptr(desc2), ptr(count2), ptr(cs), ptr(ci), cap)
            m12 = torch.zeros((B, cap), dtype=torch.int32, device=dev)
            nm, sw = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            out = capi.SearchInitOutputs(None, None, None, None, None, None, ptr(sw))
            prev0 = bt.prev.clone()
            call = lambda: check(L.viorb_search_for_initialization_device(ptr(bt.kps1), ptr(bt.desc1), ptr(bt.count1), C.byref(kf), ptr(bt.prev), cap, B,
                                                                          ptr(bt.bounds), 100, 0.9, 1, ptr(m12), ptr(nm), C.byref(out), bt.ws.ptr, bt.ws_bytes, stream()))
            r = measure(call, lambda: bt.prev.copy_(prev0), a.reps, "k_si_")
            print(json.dumps(dict(what="viorb_search_for_initialization_device", streams=B, n1=n1, n2=n2, nmatches=int(nm.cpu()[0]), sweeps=int(sw.cpu()[0]), **r)),
                  flush=True)
            X = up(np.random.default_rng(2).normal(0, 5, (B, cap, 3)).astype(np.float32))
            pose = up(np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 9], np.float32), (B, 1)))
            hp = up(np.ones((B, cap), np.uint8))
            med, cnt = torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            call = lambda: check(L.viorb_scene_median_depth_device(ptr(pose), ptr(X), ptr(hp), ptr(count2), cap, B, 2, ptr(med), ptr(cnt), stream()))
            r = measure(call, lambda: None, a.reps, "k_si_median")
            print(json.dumps(dict(what="viorb_scene_median_depth_device", key_frames=B, points=n2, **r)), flush=True)
        if first:
            first = False
            t0 = time.perf_counter()
            T.search_for_initialization(T.Frame(P["kps1"], P["desc1"], P["bounds4"]), T.Frame(P["kps2"], P["desc2"], P["bounds4"]), P["prev_matched"], 100, 0.9)
            print(json.dumps({"numpy_checker_one_stream_n%d_ms" % n: (time.perf_counter() - t0) * 1e3}), flush=True)


if __name__ == "__main__":
    main()
