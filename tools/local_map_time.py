"""Time of Tracking::UpdateLocalMap (include/viorb_local_map.h) at the shape Tracking::TrackLocalMap calls it with on EuRoC: 60 key frames of
1000 keypoints per stream, a frame with 1000 matched points of about 8 observations each (7.1 over all points of the map: those of the first and last windows have fewer), about 40 voted key frames; for 1, 64 and 1024
streams (eight different streams, repeated). HIP events around viorb_update_local_map_device, inputs uploaded before, the median of --reps
runs (default 3) after three warm-up runs, then the library's per-kernel profiler over the same calls, and the same for
viorb_local_points_gather_device. Beside it the literal loop of tests/cpp/local_map_core_host_test.cpp (`time` mode, compiled -O2, one
CPU thread; the two routines alone, the objects built before) and the flat host form of local_map_core.h on the same snapshots (at most 64
streams of them; both are linear in the streams). One JSON line per measurement, written to --out (default profiles/local_map_time.txt) as
well as printed. Needs a HIP device (no fallback)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import viorb_amd
from viorb_amd import capi, snapshot as S
from viorb_amd import local_map as M


def euroc_like_scene(seed, n_kf=60, n_kp=1000, step=110, window=1100, n_frame=1000):
    """Key frame k sees points of the window [k step, k step + window): a point lies in window / step = 10 windows and is held by about 8 of
    those key frames (a key frame holds 900 of the 1100 points of its window). The frame holds points of the last 30 key frames' windows,
    so about 40 key frames are voted."""
    rng = np.random.default_rng(seed)
    n_pt = (n_kf - 1) * step + window
    kp = np.stack([k * step + rng.choice(window, n_kp, replace=False) for k in range(n_kf)]).astype(np.int32)
    kp[rng.random(kp.shape) < 0.1] = -1
    s = dict(prev_ref=-1, prev_lkf=np.zeros(0, np.int32))
    s["kf_bad"] = np.zeros(n_kf, np.uint8)
    idx = np.arange(n_kf, dtype=np.int32)
    s["kf_parent"], s["kf_prev"] = idx - 1, idx - 1
    s["kf_next"] = np.where(idx + 1 < n_kf, idx + 1, -1).astype(np.int32)
    near = np.array([sorted((j for j in range(n_kf) if j != k), key=lambda j: (abs(j - k), j))[:10] for k in range(n_kf)], np.int32)
    s["covis10"] = near
    s["child_start"] = np.minimum(np.arange(n_kf + 1), n_kf - 1).astype(np.int32)           # key frame k has the child k + 1
    s["child_kf"] = np.arange(1, n_kf, dtype=np.int32)
    s["kf_by_key"] = rng.permutation(n_kf).astype(np.int32)
    s["kp_start"] = (np.arange(n_kf + 1) * n_kp).astype(np.int32)
    s["kp_point"] = kp.reshape(-1)
    s["pt_bad"] = (rng.random(n_pt) < 0.05).astype(np.uint8)
    held = kp.reshape(-1) >= 0
    order = np.argsort(kp.reshape(-1)[held], kind="stable")                                  # observations: the key frames whose table holds the point
    s["obs"] = np.repeat(idx, n_kp)[held][order].astype(np.uint32)
    s["obs_start"] = np.concatenate([[0], np.cumsum(np.bincount(kp.reshape(-1)[held], minlength=n_pt))]).astype(np.int32)
    lo = (n_kf - 30) * step
    s["frame_point"] = rng.integers(lo, n_pt, n_frame).astype(np.int32)
    return s


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
    prof = {k: v[0] / reps for k, v in profile().items() if k.startswith("k_ulm_")}
    return {"call_ms_median": round(float(np.median(ms)), 4), "call_ms_min": round(float(np.min(ms)), 4), "call_ms_max": round(float(np.max(ms)), 4),
            "kernel_ms_per_call": {k: round(v, 4) for k, v in prof.items()}}


def literal_exe(given):
    if given:
        return given
    exe = os.path.join(tempfile.mkdtemp(), "local_map_literal")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "viorb_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "local_map_core_host_test.cpp"), "-o", exe])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map_time.txt"))
    ap.add_argument("--literal-exe", default=None, help="tests/cpp/local_map_core_host_test.cpp compiled -O2 (built when not given)")
    a = ap.parse_args()
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("local_map_time.py needs a HIP device")
    import torch
    exe = literal_exe(a.literal_exe)
    base = [euroc_like_scene(100 + i) for i in range(a.distinct)]
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    for B in a.streams:
        scenes = [base[b % len(base)] for b in range(B)]
        P = M.pack(scenes)
        bt = M.LocalMapBatch(scenes, packed=P)
        shape = dict(streams=B, key_frames=P["n_kf"] // B, keypoints_per_key_frame=P["n_kp"] // P["n_kf"], points=P["n_pt"] // B, frame_keypoints=int(P["frame_count"][0]),
                     observations_per_point=round(P["n_obs"] / P["n_pt"], 2))
        r = measure(bt.run, a.reps)
        res = bt.results()
        assert all(g["status"] == M.OK for g in res)
        emit(dict(what="viorb_update_local_map_device", voted=round(float(np.mean([g["n_voted"] for g in res])), 1), local_key_frames=round(float(np.mean([g["n_lkf"] for g in res])), 1),
                  local_points=round(float(np.mean([g["n_lpt"] for g in res])), 1), **shape, **r))
        n = max(P["n_pt"], 1)
        store = (torch.zeros((n, 8), dtype=torch.float32, device=bt.dev), torch.zeros((n, 32), dtype=torch.uint8, device=bt.dev), torch.ones(n, dtype=torch.int32, device=bt.dev))
        out = bt.gather(*store)
        emit(dict(what="viorb_local_points_gather_device", streams=B, pcap=P["pcap"], **measure(lambda: bt.gather(*store, out=out), a.reps)))
        del store, out
        nb = min(B, 64)
        Pc = P if nb == B else M.pack(scenes[:nb])
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "snapshot.bin")
            S.write_snapshot(path, [Pc[k] for k in capi.LOCAL_MAP_INTS] + [Pc["cap"], Pc["lcap"], Pc["pcap"]], Pc, capi.LOCAL_MAP_ARRAYS)
            out = subprocess.run([exe, "time", path, "3"], capture_output=True, text=True, check=True).stdout
        emit(dict(what="one CPU thread, -O2", for_streams=B, **json.loads(out)))           # "streams": how many of them were timed
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
