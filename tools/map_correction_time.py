"""Time of the two routines of include/viorb_map_correction.h. First the propagation of LoopClosing::CorrectLoop at its shape on EuRoC:
a map of --key-frames key frames (default 60 and 240) of 1000 keypoints per stream, a point seen by about 8 of them, the current key
frame's covisibles the 30 key frames before it, so about a third of a 60-key-frame map is corrected. Batches of 1, 16 and 256 streams
(eight different streams, repeated). HIP events around viorb_correct_loop_device, inputs uploaded before, the median of --reps runs
(default 3) after three warm-up runs, then the library's per-kernel profiler over the same calls. Beside it the host build of
map_correct_core.h (viorb_debug_correct_loop_host, one CPU thread, at most 16 streams of the batch; it is linear in the streams). There is
no parent-commit time to compare with: the routines are new. Then viorb_apply_global_ba_device on maps of the same key-frame counts (see
gba_map) in the same batches. One JSON line per measurement, written to --out (default
profiles/map_correction_time.txt) as well as printed. Needs a HIP device (no fallback)."""
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
from viorb_amd import map_correction as M


def euroc_like_scene(seed, n_kf=60, n_kp=1000, step=110, window=1100, n_members=30):
    """Key frame k sees points of the window [k step, k step + window): a point lies in window / step = 10 windows and is held by about 8 of
    those key frames. The current key frame is the last one, its covisibles the n_members before it, nearest first. Poses: a slow arc."""
    rng = np.random.default_rng(seed)
    n_pt = (n_kf - 1) * step + window
    kp = np.stack([k * step + rng.choice(window, n_kp, replace=False) for k in range(n_kf)]).astype(np.int32)
    kp[rng.random(kp.shape) < 0.1] = -1
    idx = np.arange(n_kf, dtype=np.int32)
    s = dict(kf_by_key=rng.permutation(n_kf).astype(np.int32), cur_kf=n_kf - 1, cur_id=n_kf - 1, conn=idx[n_kf - 1 - n_members:n_kf - 1][::-1].copy())
    s["kp_start"] = (np.arange(n_kf + 1) * n_kp).astype(np.int32)
    s["kp_point"] = kp.reshape(-1)
    s["pt_bad"] = (rng.random(n_pt) < 0.05).astype(np.uint8)
    held = kp.reshape(-1) >= 0
    order = np.argsort(kp.reshape(-1)[held], kind="stable")
    obs_kf = np.repeat(idx, n_kp)[held][order]
    s["obs"] = (obs_kf.astype(np.uint32) | (rng.integers(0, 8, len(obs_kf)).astype(np.uint32) << 16))
    s["obs_start"] = np.concatenate([[0], np.cumsum(np.bincount(kp.reshape(-1)[held], minlength=n_pt))]).astype(np.int32)
    first = np.minimum(s["obs_start"][:-1], max(len(obs_kf) - 1, 0))
    s["pt_ref"] = np.where(np.diff(s["obs_start"]) > 0, obs_kf[first], -1).astype(np.int32)
    s["pt_corrected_by"] = np.zeros(n_pt, np.int32)
    ang = 0.02 * np.arange(n_kf)
    R = np.zeros((n_kf, 3, 3)); R[:, 0, 0] = np.cos(ang); R[:, 0, 2] = np.sin(ang); R[:, 1, 1] = 1; R[:, 2, 0] = -np.sin(ang); R[:, 2, 2] = np.cos(ang)
    t = np.stack([0.3 * np.arange(n_kf), 0.05 * rng.normal(size=n_kf), 0.1 * rng.normal(size=n_kf)], 1)
    s["pose12"] = np.concatenate([R.reshape(n_kf, 9), t], 1).astype(np.float32)
    s["pts_f"] = (rng.normal(size=(n_pt, 8)) * 5).astype(np.float32)
    q = np.array([0.01, 0.02, -0.01, 1.0]); q /= np.linalg.norm(q)
    s["Scw8"] = np.concatenate([q, t[-1] + 0.2, [1.03]])
    return s


def gba_map(seed, n_kf, pts_per_kf=127):
    """A map after a global adjustment that ran while mapping went on: key frame k hangs under k - 1 (every fifth under k - 3), the newest
    tenth of the key frames and of the points were not in the adjustment."""
    rng = np.random.default_rng(seed)
    children = [[] for _ in range(n_kf)]
    for k in range(1, n_kf):
        children[k - 3 if k % 5 == 0 and k >= 3 else k - 1].append(k)
    in_gba = (np.arange(n_kf) < n_kf - max(n_kf // 10, 1)).astype(np.uint8)
    ang = 0.02 * np.arange(n_kf)
    R = np.zeros((n_kf, 3, 3)); R[:, 0, 0] = np.cos(ang); R[:, 0, 2] = np.sin(ang); R[:, 1, 1] = 1; R[:, 2, 0] = -np.sin(ang); R[:, 2, 2] = np.cos(ang)
    pose = np.concatenate([R.reshape(n_kf, 9), np.stack([0.3 * np.arange(n_kf), 0.05 * rng.normal(size=n_kf), 0.1 * rng.normal(size=n_kf)], 1)], 1)
    ns = np.concatenate([rng.normal(size=(n_kf, 6)), np.tile([0, 0, 0, 1.0], (n_kf, 1)), 0.01 * rng.normal(size=(n_kf, 12))], 1)
    n_pt = n_kf * pts_per_kf
    ref = np.repeat(np.arange(n_kf), pts_per_kf)
    return M.gba_scene(children, [0], in_gba, pose, pose + 0.01 * rng.normal(size=pose.shape), ns, ns + 0.01, pt_bad=rng.random(n_pt) < 0.05, pt_in_gba=in_gba[ref],
                       Pw=rng.normal(size=(n_pt, 3)) * 5, PosGBA=rng.normal(size=(n_pt, 3)) * 5, pt_ref=ref)


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def measure(call, reps, prefix="k_correct_loop_"):
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
    prof = {k: v[0] / reps for k, v in profile().items() if k.startswith(prefix)}
    return {"call_ms_median": round(float(np.median(ms)), 4), "call_ms_min": round(float(np.min(ms)), 4), "call_ms_max": round(float(np.max(ms)), 4),
            "kernel_ms_per_call": {k: round(v, 4) for k, v in prof.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--key-frames", type=int, nargs="*", default=[60, 240])
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_correction_time.txt"))
    a = ap.parse_args()
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("map_correction_time.py needs a HIP device")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    for n_kf in a.key_frames:
        base = [euroc_like_scene(100 + i, n_kf=n_kf) for i in range(a.distinct)]
        for B in a.streams:
            if B * n_kf > 256 * 60:                                     # the largest batch only at the smaller map
                continue
            scenes =[base[b % a.distinct] for b in range(B)]
            P = M.pack(scenes)
            bt = M.CorrectLoopBatch(scenes, packed=P)
            shape = dict(streams=B, key_frames=P["n_kf"] // B, members=P["n_conn"] // B + 1, keypoints_per_key_frame=P["n_kp"] // P["n_kf"], points=P["n_pt"] // B,
                         observations_per_point=round(P["n_obs"] / P["n_pt"], 2))
            r = measure(bt.run, a.reps)
            res = bt.results()
            assert all(g["status"] == M.OK for g in res)
            emit(dict(what="viorb_correct_loop_device", single_run_measurement=True, points_corrected=round(float(np.mean([g["pt_touched"].sum() for g in res])), 1), **shape, **r))
            nb = min(B, 16)
            Pc = P if nb == B else M.pack(scenes[:nb])
            t0 = time.perf_counter()
            M.correct_loop_host_core(None, packed=Pc)
            emit(dict(what="viorb_debug_correct_loop_host, one CPU thread", for_streams=B, streams_timed=nb, ms_per_stream=round((time.perf_counter() - t0) * 1e3 / nb, 3)))
    # the map update after a global bundle adjustment: a spanning chain with side branches, the newest tenth of the key frames outside the
    # adjustment, 127 points per key frame of which the newest tenth are moved through their reference key frame
    Tbc = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1, -0.02, -0.06, 0.01], np.float32)
    for n_kf in a.key_frames:
        base = [gba_map(200 + i, n_kf) for i in range(a.distinct)]
        for B in a.streams:
            scenes = [base[b % a.distinct] for b in range(B)]
            P = M.gba_pack(scenes)
            bt = M.ApplyGbaBatch(scenes, Tbc, packed=P)
            r = measure(bt.run, a.reps, "k_apply_gba_")
            res = bt.results()
            assert all(g["status"] == M.OK for g in res)
            emit(dict(what="viorb_apply_global_ba_device", single_run_measurement=True, streams=B, key_frames=P["n_kf"] // B, points=P["n_pt"] // B,
                      key_frames_derived=round(float(np.mean([(g["kf_in_gba_out"] != s["kf_in_gba"]).sum() for g, s in zip(res, scenes)])), 1),
                      points_by_reference=round(float(np.mean([(g["pt_code"] == M.AG_BY_REF).sum() for g in res])), 1), **r))
            nb = min(B, 16)
            t0 = time.perf_counter()
            M.apply_global_ba_host_core(scenes[:nb], Tbc)
            emit(dict(what="viorb_debug_apply_global_ba_host, one CPU thread (with packing)", for_streams=B, streams_timed=nb, ms_per_stream=round((time.perf_counter() - t0) * 1e3 / nb, 3)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
