"""Time of the Sim3 matchers (include/viorb_sim3_match.h) at the shapes loop closing calls them with: viorb_search_by_sim3_device for 1 and 4
key-frame pairs of 1000 features, viorb_search_by_projection_sim3_device for one key frame and 2000 / 8000 loop points,
viorb_fuse_sim3_device for 1, 16 and 48 key frames over 4000 shared points and, beside it for context, viorb_frontend_fuse_device (the
SE3 Fuse, one workgroup per key frame) at the same shape. Device events around the call (inputs uploaded before), then the library's
per-kernel profiler over the same calls; one JSON line per shape. For context only, the wall time of the numpy checker
(tests/sim3_match_ref.py) on the first shape of each entry. Needs a HIP device (no fallback)."""
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
from viorb_amd import sim3_match as M
from viorb_amd.capi import check, ptr, _torch_up as up
from viorb_amd.synth import make_sim3_match_problem


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def measure(call, reps, prefixes):
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
    prof = {k: round(v[0] / reps, 4) for k, v in profile().items() if k.startswith(prefixes)}
    return {"call_ms_median": float(np.median(ms)), "call_ms_min": float(np.min(ms)), "kernel_ms_per_call": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--features", type=int, default=1000)
    a = ap.parse_args()
    L = viorb_amd.lib()
    if L.viorb_device_count() < 1:
        raise SystemExit("sim3_match_time.py needs a HIP device")
    import torch
    import sim3_match_ref as T
    n = a.features
    dev = torch.device("cuda", 0)
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    # ---- (1) SearchBySim3
    P = make_sim3_match_problem(1, n1=n, n2=n, n_common=n // 2)
    cam, bounds = M.camera(P["intr4"], P["sf"]), np.asarray(P["bounds4"], np.float32)
    keys = ("pose12", "has_point", "pts_f", "pts_desc", "already")
    for B in (1, 4):
        b1 = M.Sim3MatchBatch([(P["kf1"]["kps"], P["kf1"]["desc"])] * B, cam, bounds)
        b2 = M.Sim3MatchBatch([(P["kf2"]["kps"], P["kf2"]["desc"])] * B, cam, bounds)
        s1, s2 = b1.side(*[[P["kf1"][k]] * B for k in keys]), b2.side(*[[P["kf2"][k]] * B for k in keys])
        R, t, s = up(np.stack([P["R12"]] * B)), up(np.stack([P["t12"]] * B)), up(np.full(B, P["s12"], np.float32))
        m12, nf = z(B, b1.cap), z(B)
        ws, wb = b1._workspace(max(b1.cap, b2.cap), 1)
        call = lambda: check(L.viorb_search_by_sim3_device(C.byref(s1), C.byref(s2), ptr(R), ptr(t), ptr(s), C.byref(cam), ptr(bounds), 7.5, B, ptr(m12), ptr(nf),
                                                           None, None, None, None, ws, wb, stream()))
        r = measure(call, a.reps, "k_s3m_")
        print(json.dumps(dict(what="viorb_search_by_sim3_device", pairs=B, features=n, nfound=[int(v) for v in nf.cpu().numpy()], **r)), flush=True)
    t0 = time.perf_counter()
    cam_ref = T.Camera(P["intr4"], P["bounds4"], P["sf"])
    x, y = P["kf1"], P["kf2"]
    T.search_by_sim3(T.KeyFrame(cam_ref, x["kps"], x["desc"]), x["pose12"], x["has_point"], x["pts_f"], x["pts_desc"], x["already"],
                     T.KeyFrame(cam_ref, y["kps"], y["desc"]), y["pose12"], y["has_point"], y["pts_f"], y["pts_desc"], y["already"], P["R12"], P["t12"], P["s12"], 7.5)
    print(json.dumps({"numpy_checker_search_by_sim3_one_pair_ms": (time.perf_counter() - t0) * 1e3}), flush=True)

    # ---- (2) SearchByProjection(KF, Scw): one key frame, the loop points of a neighbourhood
    for npts in (2000, 8000):
        P = make_sim3_match_problem(2, n1=n, n2=n, n_common=n // 2, duplicates=npts // 20, n_extra=npts - n // 2 - npts // 20 - 330)
        Lp = P["loop"]
        bt = M.Sim3MatchBatch([(P["kf1"]["kps"], P["kf1"]["desc"])], cam, bounds)
        pcap = len(Lp["pts_f"])
        d = [up(Lp["Scw"][None]), bt._pad([Lp["pts_f"]], pcap, (8,), np.float32), bt._pad([Lp["pts_desc"]], pcap, (32,), np.uint8),
             bt._pad([Lp["valid"]], pcap, (), np.uint8), up(np.array([pcap], np.int32)), bt._pad([Lp["feat_taken"]], bt.cap, (), np.uint8)]
        bi, nm = z(1, pcap), z(1)
        ws, wb = bt._workspace(bt.cap, pcap)
        call = lambda: check(L.viorb_search_by_projection_sim3_device(C.byref(bt.kf), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), pcap, ptr(d[5]),
                                                                      C.byref(cam), ptr(bounds), 10.0, 1, ptr(bi), ptr(nm), None, ws, wb, stream()))
        r = measure(call, a.reps, "k_s3m_")
        print(json.dumps(dict(what="viorb_search_by_projection_sim3_device", key_frames=1, features=n, points=pcap, nmatches=int(nm.cpu()[0]), **r)), flush=True)
        if npts == 2000:
            t0 = time.perf_counter()
            T.search_by_projection(T.KeyFrame(cam_ref, P["kf1"]["kps"], P["kf1"]["desc"]), Lp["Scw"], Lp["pts_f"], Lp["pts_desc"], Lp["valid"], Lp["feat_taken"], 10.0)
            print(json.dumps({"numpy_checker_search_by_projection_%d_points_ms" % pcap: (time.perf_counter() - t0) * 1e3}), flush=True)

    # ---- (3) Fuse(KF, Scw) over one shared list, and the SE3 Fuse at the same shape
    from viorb_amd.frontend import Frontend
    for B in (1, 16, 48):
        P = make_sim3_match_problem(3, n1=n, n2=n, n_common=n // 2, n_kf=B, n_extra=4000 - n // 2 - 330)
        Lp, F = P["loop"], P["fuse"]
        bt = M.Sim3MatchBatch(F["frames"], cam, bounds)
        npts = len(Lp["pts_f"])
        d = [up(F["Scw"]), up(Lp["pts_f"]), up(Lp["pts_desc"]), up(F["valid"])]
        bi, nf = z(B, npts), z(B)
        ws, wb = bt._workspace(bt.cap, npts)
        call = lambda: check(L.viorb_fuse_sim3_device(C.byref(bt.kf), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), npts, npts, C.byref(cam), ptr(bounds), 4.0, B,
                                                      ptr(bi), ptr(nf), None, ws, wb, stream()))
        r = measure(call, a.reps, "k_s3m_")
        print(json.dumps(dict(what="viorb_fuse_sim3_device", key_frames=B, features=n, points=npts, nfused_first=[int(v) for v in nf.cpu().numpy()[:4]], **r)), flush=True)
        # the SE3 sibling: the same key frames and points, each key frame with its own copy of the list and the pose Scw decomposes to
        cam16 = np.zeros(16); cam16[:4] = P["intr4"]
        fe = Frontend(cam16, [0, 0, -9.81], P["sf"], 1 / P["sf"] ** 2, bounds=tuple(bounds), max_batch=B, cap=bt.cap)
        pose = np.stack([np.concatenate([T.decompose(S)[1].ravel(), T.decompose(S)[2]]) for S in F["Scw"]]).astype(np.float32)
        e = [up(pose), up(np.stack([Lp["pts_f"]] * B)), up(np.stack([Lp["pts_desc"]] * B)), up(np.full((B, bt.cap), -1, np.float32)), up(np.full(B, npts, np.int32))]
        call = lambda: check(L.viorb_frontend_fuse_device(fe.h, ptr(bt.kps), ptr(bt.desc), ptr(e[3]), ptr(bt.count), ptr(bt.cell_start), ptr(bt.cell_idx), ptr(e[0]),
                                                          ptr(e[1]), ptr(d[3]), ptr(e[2]), ptr(e[4]), npts, 4.0, 0.0, B, ptr(bi), ptr(nf), stream()))
        r = measure(call, a.reps, "k_fuse")
        print(json.dumps(dict(what="viorb_frontend_fuse_device (SE3, for context)", key_frames=B, features=n, points=npts,
                              nfused_first=[int(v) for v in nf.cpu().numpy()[:4]], **r)), flush=True)
        if B == 1:
            t0 = time.perf_counter()
            T.fuse(T.KeyFrame(cam_ref, *F["frames"][0]), F["Scw"][0], Lp["pts_f"], Lp["pts_desc"], F["valid"][0], 4.0)
            print(json.dumps({"numpy_checker_fuse_one_key_frame_%d_points_ms" % npts: (time.perf_counter() - t0) * 1e3}), flush=True)


if __name__ == "__main__":
    main()
