"""Time of map-point creation for one key frame and J = 20 neighbours at 1000 key points, for 1, 64 and 1024 streams:
  chained  one viorb_create_new_map_points_device call (baseline test, 20 searches, vetting, ordered append), device events around it;
  search   the 20 host-form viorb_search_for_triangulation calls alone, host clock (each ends in a device synchronise): the part of
           this work the library could do before the chained call existed, per stream, with none of the triangulation.
Prints one JSON line per stream count. Needs a HIP device (no fallback)."""
import argparse
import json
import sys
import time
import os
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viorb_amd
from viorb_amd.synth import make_mapping_problem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic problems, repeated over the streams")
    a = ap.parse_args()
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("mapping_time.py needs a HIP device")
    import torch
    J, n = a.neighbours, a.features
    base = [make_mapping_problem(100 + k, J=J, n1=n, n2=n) for k in range(a.distinct)]
    cam = base[0]["cam"]
    for B in a.streams:
        probs = [base[b % len(base)] for b in range(B)]
        hp0 = None
        ms = []
        run = viorb_amd.CreateNewMapPoints(cam, probs, J, pcap=n, monocular=True)
        hp0 = run.hp1.clone()
        for rep in range(a.reps + 2):
            run.hp1.copy_(hp0); run.n_new.zero_(); run.status.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record(); torch.cuda.synchronize()
            if rep >= 2:
                ms.append(e0.elapsed_time(e1))
        res = run.results()
        n_new = [r["n_new"] for r in res]
        # the 20 host-form searches of one stream (has_point1 as the caller would have it before any point is created)
        p = base[0]; k1 = p["kf1"]
        hs = []
        for rep in range(min(a.reps, 5) + 1):
            t0 = time.perf_counter()
            for kf2 in p["neigh"]:
                viorb_amd.SearchForTriangulation(k1["kps"], k1["desc"], k1["hp"], k1["ur"], k1["node"], kf2["kps"], kf2["desc"], kf2["hp"], kf2["ur"], kf2["node"],
                                                 kf2["F12"], k1["Ow"], kf2["pose12"], cam["intr4"], cam["sf"], cam["level_sigma2"], False, False)
            if rep >= 1:
                hs.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"streams": B, "features": n, "neighbours": J, "chained_call_ms_median": float(np.median(ms)), "chained_call_ms_min": float(np.min(ms)),
                          "chained_call_ms_per_stream": float(np.median(ms)) / B, "host_form_20_searches_one_stream_ms_median": float(np.median(hs)),
                          "new_points_first_streams": n_new[:4], "status_nonzero": int(sum(r["status"] != 0 for r in res))}), flush=True)


if __name__ == "__main__":
    main()
