"""Time of map fusion (include/viorb_map_fusion.h) at two shapes. "search_and_fuse": LoopClosing::SearchAndFuse, 10 corrected key
frames of 800 keypoints, one shared list of 500 loop points, 10 SIM3 calls whose best_idx rows hit a feature for about a third of the
entries. "search_in_neighbors": LocalMapping::SearchInNeighbors, 20 neighbours and the current key frame of 600 keypoints, 20 POSE calls
with the current key frame's points and one with the neighbours' points on the current key frame, about a quarter of the entries
hitting. A point is seen by 3 to 5 key frames. Three cases each: 1, 64 and 1024 streams (eight different streams, repeated). HIP events
around viorb_apply_fuse_device, inputs uploaded before, the median of --reps runs (default 3) after three warm-up runs, then the
library's per-kernel profiler over the same calls. Beside it the host build of map_fusion_core.h (viorb_debug_apply_fuse_host, one CPU
thread on the same machine, at most 64 streams of the batch; it is linear in the streams) on the same scenes. The time is recorded, not
gated. One JSON line per measurement, written to --out (default profiles/map_fusion_time.txt) as well as printed. Needs a HIP device
(no fallback)."""
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
from viorb_amd import map_fusion as M


def _map(rng, n_kf, n_kp, n_pt):
    table = np.full((n_kf, n_kp), -1, np.int64)
    pts = []
    for p in range(n_pt):
        obs = []
        for k in rng.choice(n_kf, int(rng.integers(3, 6)), replace=False):
            f = int(rng.integers(n_kp))
            if table[k, f] < 0:
                table[k, f] = p
                obs.append((int(k), f))
        pts.append(dict(obs=obs, bad=bool(rng.random() < 0.02), found=int(rng.integers(0, 40)), visible=int(rng.integers(0, 80))))
    kfs = [dict(pts=table[k].tolist(), stereo=rng.integers(0, 2, n_kp).tolist(), octave=rng.integers(0, 8, n_kp).tolist()) for k in range(n_kf)]
    return kfs, pts, table


def _row(rng, n, n_kp, hit):
    return [int(rng.integers(n_kp)) if rng.random() < hit else -1 for _ in range(n)]


def search_and_fuse_scene(seed, n_kf=10, n_kp=800, n_pt=2500, n_loop=500):
    rng = np.random.default_rng(seed)
    kfs, pts, _ = _map(rng, n_kf, n_kp, n_pt)
    loop = [int(p) for p in rng.choice(n_pt, n_loop, replace=False)]
    return M.scene_from_lists(kfs, pts, [(k, M.SIM3, _row(rng, n_loop, n_kp, 0.33)) for k in range(n_kf)], shared_list=loop, by_key=rng.permutation(n_kf).tolist())


def search_in_neighbors_scene(seed, n_kf=21, n_kp=600, n_pt=3000):
    rng = np.random.default_rng(seed)
    kfs, pts, table = _map(rng, n_kf, n_kp, n_pt)
    own = [int(p) for p in table[0] if p >= 0]
    calls = [(k, M.POSE, own, _row(rng, len(own), n_kp, 0.25)) for k in range(1, n_kf)]
    theirs = [int(p) for p in rng.choice(n_pt, 1500, replace=False)]
    calls.append((0, M.POSE, theirs, _row(rng, len(theirs), n_kp, 0.25)))
    return M.scene_from_lists(kfs, pts, calls, by_key=rng.permutation(n_kf).tolist())


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
    prof = {k: v[0] / reps for k, v in profile().items() if k.startswith("k_fuse_")}
    return {"call_ms_median": round(float(np.median(ms)), 4), "call_ms_min": round(float(np.min(ms)), 4), "call_ms_max": round(float(np.max(ms)), 4),
            "kernel_ms_per_call": {k: round(v, 4) for k, v in prof.items()}}


def host_core_ms(P, reps):
    o = S.outputs(capi.FUSE_RESULT_FIELDS, lambda f: M.out_len(P, f), M.out_dtype)
    m, r = M._map_struct(P), M._result_struct(o, capi.FUSE_RESULT_FIELDS)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        M.check(viorb_amd.lib().viorb_debug_apply_fuse_host(C.byref(m), C.byref(r)))
        ms.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ms)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_fusion_time.txt"))
    a = ap.parse_args()
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("map_fusion_time.py needs a HIP device")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    for load, make in (("search_and_fuse", search_and_fuse_scene), ("search_in_neighbors", search_in_neighbors_scene)):
        base = [make(300 + i) for i in range(a.distinct)]
        packed = [M.pack([s]) for s in base]
        for B in a.streams:
            scenes = [base[b % a.distinct] for b in range(B)]
            P = M.pack(scenes)
            bt = M.FuseBatch(scenes, packed=P)
            r = measure(bt.run, a.reps)
            bt.torch.cuda.synchronize()
            status, reason = bt.o["status"].cpu().numpy(), bt.o["op_reason"].cpu().numpy()[:P["n_op"]]
            assert (status == M.OK).all()
            share = lambda code: round(float((reason == code).mean()), 3)
            emit(dict(what="viorb_apply_fuse_device", load=load, streams=B, calls_per_stream=P["n_call"] // B, entries_per_stream=P["n_op"] // B, key_frames=P["n_kf"] // B,
                      keypoints_per_key_frame=P["n_kp"] // P["n_kf"], points=P["n_pt"] // B, observations_per_point=round(P["n_obs"] / P["n_pt"], 2),
                      added=share(M.ADDED), replaced=round(share(M.REPLACED_KF_POINT) + share(M.REPLACED_CANDIDATE), 3), **r))
            nb = min(B, 64)
            emit(dict(what="map_fusion_core.h on one CPU thread", load=load, for_streams=B, streams=nb,
                      host_core_ms=host_core_ms(P if nb == B else (packed[0] if nb == 1 else M.pack(scenes[:nb])), a.reps)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
