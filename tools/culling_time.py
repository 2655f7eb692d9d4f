"""Time of key-frame culling (include/viorb_culling.h) at the shape LocalMapping::Run calls it with: 40 candidates of about 1000 keypoints
each per stream, for 1, 64 and 1024 streams (eight different streams of synth.make_culling_problem, repeated), on a map in which most
candidates are culled and on one with few culls. HIP events around viorb_key_frame_culling_device, inputs uploaded before, the median of
--reps runs after three warm-up runs, then the library's per-kernel profiler over the same calls. Beside it the literal loop of
tests/cpp/culling_core_host_test.cpp (`time` mode, compiled -O2, one CPU thread; the candidate loop alone, the objects built before) and
the flat host form of culling_core.h on the same snapshots (at most 64 streams of them; both are linear in the streams). One JSON line
per measurement, written to --out (default profiles/culling_time.txt) as well as printed. Needs a HIP device (no fallback)."""
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
from viorb_amd import culling as M
from viorb_amd.synth import make_culling_problem


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
    prof = {k: v[0] / reps for k, v in profile().items() if k.startswith("k_cull_")}
    return {"call_ms_median": round(float(np.median(ms)), 4), "call_ms_min": round(float(np.min(ms)), 4), "call_ms_max": round(float(np.max(ms)), 4),
            "kernel_ms_per_call": {k: round(v, 4) for k, v in prof.items()}}


def literal_exe(given):
    if given:
        return given
    exe = os.path.join(tempfile.mkdtemp(), "culling_literal")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "viorb_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "culling_core_host_test.cpp"), "-o", exe])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "culling_time.txt"))
    ap.add_argument("--literal-exe", default=None, help="tests/cpp/culling_core_host_test.cpp compiled -O2 (built when not given)")
    a = ap.parse_args()
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("culling_time.py needs a HIP device")
    exe = literal_exe(a.literal_exe)
    # two maps: one in which most candidates are redundant (some twenty culls per stream), and one as the mapping thread usually finds
    # it (a few culls, none in some streams)
    maps = {"many culls": [make_culling_problem(100 + i, n_kf=60, n_cand=40, min_kps=900, max_kps=1100, n_pts=9000, obs_range=(4, 12)) for i in range(a.distinct)],
            "few culls": [make_culling_problem(100 + i, n_kf=60, n_cand=40, min_kps=900, max_kps=1100, n_pts=9000, obs_range=(3, 8)) for i in range(a.distinct)]}
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    for name, B in [(n, B) for n in maps for B in a.streams]:
        base = maps[name]
        scenes = [base[b % len(base)] for b in range(B)]
        P = M.pack(scenes)
        bt = M.CullBatch(scenes, True, packed=P)
        shape = dict(map=name, streams=B, candidates=P["n_cand"] // B, keypoints_per_candidate=P["n_kp"] // max(P["n_cand"], 1), points=P["n_pt"] // B, observations=P["n_obs"] // B)
        r = measure(bt.run, a.reps)
        res = bt.results()
        emit(dict(what="viorb_key_frame_culling_device", culled=sum(g["n_culled"] for g in res), counted=int(sum(g["cand_recounted"].sum() for g in res)), **shape, **r))
        nb = min(B, 64)
        Pc = P if nb == B else M.pack(scenes[:nb])
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "snapshot.bin")
            S.write_snapshot(path, [Pc[k] for k in capi.CULL_MAP_INTS] + [1, 0], Pc, capi.CULL_MAP_ARRAYS)          # monocular
            out = subprocess.run([exe, "time", path, "3"], capture_output=True, text=True, check=True).stdout
        emit(dict(what="one CPU thread, -O2", map=name, **json.loads(out)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
