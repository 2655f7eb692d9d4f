"""Time of KeyFrame::UpdateConnections (include/viorb_covisibility.h) at the shape the mapping and loop-closing threads call it with on
EuRoC: 60 key frames of 1000 keypoints per stream, a point seen by about 8 of them, so a target has about 20 observers of which about
ten pass the threshold. Three cases: one stream with one target (LocalMapping::ProcessNewKeyFrame), one stream with a loop-sized group of
30 targets in order with LoopConnections (LoopClosing::CorrectLoop), and batches of both (256 streams; eight different streams, repeated).
The maps and ordered lists a call starts from are what UpdateConnections of every key frame left behind (computed by the host form of
covis_core.h); the targets' keypoint tables then lose another tenth of their points, so weights change and lists are rebuilt. HIP events
around viorb_update_connections_device, inputs uploaded before, the median of --reps runs (default 3) after three warm-up runs, then the
library's per-kernel profiler over the same calls. Beside it the literal loop of tests/cpp/covis_core_host_test.cpp (`time` mode, compiled
-O2, one CPU thread; the routine alone, the objects built before) and the flat host form of covis_core.h on the same snapshots (at most
64 streams of them; both are linear in the streams). One JSON line per measurement, written to --out (default profiles/covis_time.txt)
as well as printed. Needs a HIP device (no fallback)."""
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
from viorb_amd import covisibility as M


def euroc_like_scene(seed, n_targets, n_kf=60, n_kp=1000, step=110, window=1100):
    """Key frame k sees points of the window [k step, k step + window): a point lies in window / step = 10 windows and is held by about 8
    of those key frames. The targets are the last n_targets key frames, oldest first; a group of several has 60 keypoints each on points of the
    first key frame's window, the other side of a loop."""
    rng = np.random.default_rng(seed)
    n_pt = (n_kf - 1) * step + window
    kp = np.stack([k * step + rng.choice(window, n_kp, replace=False) for k in range(n_kf)]).astype(np.int32)
    kp[rng.random(kp.shape) < 0.1] = -1
    idx = np.arange(n_kf, dtype=np.int32)
    s = dict(kf_by_key=rng.permutation(n_kf).astype(np.int32), kf_flags=np.full(n_kf, M.KF_FIRST, np.uint8), kf_parent=np.full(n_kf, -1, np.int32))
    s["kf_flags"][0] |= M.KF_ID0
    s["kp_start"] = (np.arange(n_kf + 1) * n_kp).astype(np.int32)
    s["kp_point"] = kp.reshape(-1)
    s["pt_bad"] = (rng.random(n_pt) < 0.05).astype(np.uint8)
    held = kp.reshape(-1) >= 0
    order = np.argsort(kp.reshape(-1)[held], kind="stable")                                  # observations: the key frames whose table holds the point
    s["obs"] = np.repeat(idx, n_kp)[held][order].astype(np.uint32)
    s["obs_start"] = np.concatenate([[0], np.cumsum(np.bincount(kp.reshape(-1)[held], minlength=n_pt))]).astype(np.int32)
    empty = dict(conn_start=np.zeros(n_kf + 1, np.int32), conn_kf=np.zeros(0, np.int32), conn_w=np.zeros(0, np.int32))
    empty.update(ord_start=empty["conn_start"], ord_kf=empty["conn_kf"], ord_w=empty["conn_w"])
    # the graph every key frame's own UpdateConnections left, in insertion order
    h = M.update_connections_host_core([dict(s, targets=idx, **empty)])[0]
    assert h["status"] == M.OK
    for what in ("conn", "ord"):
        n = h[what + "_n_out"]
        keep = np.arange(h[what + "_kf_out"].shape[1])[None, :] < n[:, None]
        s[what + "_start"] = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        s[what + "_kf"], s[what + "_w"] = h[what + "_kf_out"][keep].astype(np.int32), h[what + "_w_out"][keep].astype(np.int32)
    s["kf_flags"], s["kf_parent"] = h["kf_flags_out"].copy(), h["kf_parent_out"].copy()
    s["targets"] = idx[n_kf - n_targets:].copy()
    kp2 = kp.copy()
    rows = kp2[n_kf - n_targets:]
    rows[rng.random(rows.shape) < 0.1] = -1                                                  # the targets have lost points since
    if n_targets > 1:                                                                        # and, as after SearchAndFuse, hold points of the other side of the loop
        for r in rows:
            r[rng.choice(n_kp, 60, replace=False)] = rng.choice(window, 60, replace=False)
    s["kp_point"] = kp2.reshape(-1)
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
    prof = {k: v[0] / reps for k, v in profile().items() if k.startswith("k_covis_")}
    return {"call_ms_median": round(float(np.median(ms)), 4), "call_ms_min": round(float(np.min(ms)), 4), "call_ms_max": round(float(np.max(ms)), 4),
            "kernel_ms_per_call": {k: round(v, 4) for k, v in prof.items()}}


def literal_exe(given):
    if given:
        return given
    exe = os.path.join(tempfile.mkdtemp(), "covis_literal")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "viorb_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "covis_core_host_test.cpp"), "-o", exe])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", type=int, nargs="*", default=[1, 1, 1, 30, 256, 1, 256, 30], help="pairs: streams, targets per stream")
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_time.txt"))
    ap.add_argument("--literal-exe", default=None, help="tests/cpp/covis_core_host_test.cpp compiled -O2 (built when not given)")
    a = ap.parse_args()
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("covis_time.py needs a HIP device")
    exe = literal_exe(a.literal_exe)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    base = {}
    for B, n_targets in zip(a.cases[0::2], a.cases[1::2]):
        if n_targets not in base:
            base[n_targets] = [euroc_like_scene(100 + i, n_targets) for i in range(a.distinct)]
        scenes = [base[n_targets][b % a.distinct] for b in range(B)]
        P = M.pack(scenes)
        bt = M.CovisBatch(scenes, packed=P, erase_targets=1)
        shape = dict(streams=B, targets_per_stream=n_targets, key_frames=P["n_kf"] // B, keypoints_per_key_frame=P["n_kp"] // P["n_kf"], points=P["n_pt"] // B,
                     observations_per_point=round(P["n_obs"] / P["n_pt"], 2), ccap=P["ccap"])
        r = measure(bt.run, a.reps)
        res = bt.results()
        assert all(g["status"] == M.OK for g in res)
        touched = float(np.mean([(g["kf_touched"] != 0).sum() for g in res]))
        emit(dict(what="viorb_update_connections_device", observers_per_target=round(float(np.mean([g["t_observers"].mean() for g in res])), 1),
                  added_per_target=round(float(np.mean([g["t_added"].mean() for g in res])), 1), key_frames_touched=round(touched, 1),
                  loop_connections_per_target=round(float(np.mean([g["n_loop_conn"].mean() for g in res])), 1), **shape, **r))
        nb = min(B, 64)
        Pc = P if nb == B else M.pack(scenes[:nb])
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "snapshot.bin")
            S.write_snapshot(path, [Pc[k] for k in capi.COVIS_INTS] + [Pc["ccap"], 1], Pc, capi.COVIS_ARRAYS)
            out = subprocess.run([exe, "time", path, "3"], capture_output=True, text=True, check=True).stdout
        emit(dict(what="one CPU thread, -O2", for_streams=B, **json.loads(out)))           # "streams": how many of them were timed
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
