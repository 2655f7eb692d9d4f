"""Time of key-frame removal (include/viorb_kf_removal.h) at the shape LocalMapping::KeyFrameCulling leaves it with: the 30 covisibles of
the current key frame, 400 keypoints each, a point seen from a run of consecutive key frames by about 6 of them, maps and full ordered
lists from the shared-point counts, every key frame's parent its heaviest older neighbour, one chain, and three SetBadFlag operations per
stream on distinct key frames. Three cases: 1, 64 and 1024 streams (eight different streams, repeated). HIP events around
viorb_remove_key_frames_device, inputs uploaded before, the median of --reps runs (default 3) after three warm-up runs, then the
library's per-kernel profiler over the same calls. Beside it, as context, the host build of kf_removal_core.h
(viorb_debug_remove_key_frames_host, one CPU thread on the same machine, at most 64 streams of the batch; it is linear in the streams).
The time is recorded, not gated. One JSON line per measurement, written to --out (default profiles/kf_removal_time.txt) as well as
printed. Needs a HIP device (no fallback)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import viorb_amd
from viorb_amd import capi, snapshot as S
from viorb_amd import kf_removal as M


def culling_sized_scene(seed, n_kf=30, n_kp=400, step=50, window=400, n_ops=3):
    rng = np.random.default_rng(seed)
    n_pt = (n_kf - 1) * step + window
    kp = np.stack([k * step + rng.choice(window, n_kp, replace=False) for k in range(n_kf)]).astype(np.int32)
    kp[rng.random(kp.shape) < 0.25] = -1
    held = np.zeros((n_kf, n_pt), bool)
    for k in range(n_kf):
        held[k, kp[k][kp[k] >= 0]] = True
    shared = held.astype(np.int32) @ held.astype(np.int32).T
    by_key = rng.permutation(n_kf)
    rank = np.empty(n_kf, np.int64)
    rank[by_key] = np.arange(n_kf)
    kfs = []
    for k in range(n_kf):
        conn = {int(o): int(shared[k, o]) for o in range(n_kf) if o != k and shared[k, o] > 0}
        full = sorted(conn.items(), key=lambda kv: (kv[1], rank[kv[0]]), reverse=True)
        older = [o for o, _ in full if o < k]
        kfs.append(dict(pts=kp[k].tolist(), conn=conn, ord=full, id0=(k == 0), parent=-1 if k == 0 else older[0] if older else k - 1, prev=k - 1,
                        next=k + 1 if k + 1 < n_kf else -1, pose=[1, 0, 0, 0, 1, 0, 0, 0, 1] + rng.normal(size=3).tolist()))
    pts = [dict(obs=[(int(k), bool(rng.random() < 0.3)) for k in np.where(held[:, p])[0]]) for p in range(n_pt)]
    ops = [int(x) for x in rng.choice(np.arange(1, n_kf - 1), size=n_ops, replace=False)]
    return M.scene_from_lists(kfs, pts, ops, by_key=by_key.tolist())


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def measure(call, reps):
    import torch
    L = viorb_amd.lib()
    ms = []
    for rep in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        if rep >= 3:
            ms.append(e0.elapsed_time(e1))
    torch.cuda.synchronize(); L.viorb_profile_select(None); L.viorb_profile_reset(); L.viorb_profile_enable(1)
    for _ in range(reps):
        call()
    torch.cuda.synchronize(); L.viorb_profile_enable(0)
    prof = {k: v[0] / reps for k, v in profile().items() if k.startswith("k_kfr_")}
    return {"call_ms_median": round(float(np.median(ms)), 4), "call_ms_min": round(float(np.min(ms)), 4), "call_ms_max": round(float(np.max(ms)), 4),
            "kernel_ms_per_call": {k: round(v, 4) for k, v in prof.items()}}


def host_core_ms(P, reps):
    o = S.outputs(capi.KFR_RESULT_FIELDS, lambda f: M.out_len(P, f), M.out_dtype)
    m, r = M._map_struct(P), S.struct(capi.KfrResult, (), capi.KFR_RESULT_FIELDS, o)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        M.check(viorb_amd.lib().viorb_debug_remove_key_frames_host(C.byref(m), C.byref(r), P["ccap"]))
        ms.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ms)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kf_removal_time.txt"))
    a = ap.parse_args()
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("kf_removal_time.py needs a HIP device")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    base = [culling_sized_scene(100 + i) for i in range(a.distinct)]
    for B in a.streams:
        scenes = [base[b % a.distinct] for b in range(B)]
        P = M.pack(scenes)
        bt = M.KfRemovalBatch(scenes, packed=P)
        shape = dict(streams=B, operations_per_stream=P["n_op"] // B, key_frames=P["n_kf"] // B, keypoints_per_key_frame=P["n_kp"] // P["n_kf"], points=P["n_pt"] // B,
                     observations_per_point=round(P["n_obs"] / P["n_pt"], 2), map_entries_per_key_frame=round(P["n_conn"] / P["n_kf"], 1), ccap=P["ccap"])
        r = measure(bt.run, a.reps)
        res = bt.results()
        assert all(g["status"] == M.OK and (g["op_reason"] == M.REMOVED).all() for g in res)
        mean = lambda f: round(float(np.mean([g[f].mean() for g in res])), 1)
        emit(dict(what="viorb_remove_key_frames_device", neighbours_rebuilt_per_operation=mean("op_rebuilt"), children_per_operation=mean("op_children"),
                  points_bad_per_operation=mean("op_points_bad"), **shape, **r))
        nb = min(B, 64)
        emit(dict(what="kf_removal_core.h on one CPU thread", for_streams=B, streams=nb, host_core_ms=host_core_ms(P if nb == B else M.pack(scenes[:nb]), a.reps)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
