"""Time of relocalisation after the PnP hypothesis (include/viorb_relocalization.h) at the shape Tracking::Relocalization meets: one lost
frame of 1000 features against 1, 5 and 10 candidate key frames of 1000 map points, the candidates sharing one copy of the frame.
viorb_search_by_projection_reloc_device alone at th 10 / ORBdist 100 and at th 3 / ORBdist 64, and viorb_relocalization_refine_device (three
solves and two searches in lock step). Warm: the inputs are uploaded before, the call is repeated, device events around each call, the
median and the minimum over the repetitions, then the library's per-kernel profiler over the same calls; one JSON line per shape. For
context only, the wall time of the numpy checker (tests/reloc_ref.py) on one candidate. Needs a HIP device (no fallback)."""
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
from viorb_amd import relocalization as R
from viorb_amd.synth import make_reloc_problem
from sim3_match_time import measure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--points", type=int, default=1000)
    a = ap.parse_args()
    L = viorb_amd.lib()
    if L.viorb_device_count() < 1:
        raise SystemExit("reloc_time.py needs a HIP device")
    from viorb_amd.frontend import Frontend
    for B in (1, 5, 10):
        P = make_reloc_problem(7, a.features, a.points, B)
        cam = R.camera(P["intr4"], P["sf"])
        bt = R.RelocBatch([(P["kps"], P["desc"])], cam, P["bounds4"])
        for th, od in ((10.0, 100), (3.0, 64)):
            call, fetch = bt.search_call(P["hyps"], th=th, orb_dist=od, with_reason=False)
            r = measure(call, a.reps, "k_reloc_")
            print(json.dumps(dict(what="viorb_search_by_projection_reloc_device", candidates=B, features=a.features, points=a.points, th=th, orb_dist=od,
                                  nmatches=[g["nmatches"] for g in fetch()], **r)), flush=True)
        cam16 = np.zeros(16); cam16[:4] = P["intr4"]
        fe = Frontend(cam16, [0, 0, -9.81], P["sf"], 1 / P["sf"] ** 2, bounds=tuple(P["bounds4"]), max_batch=B, cap=bt.cap)
        call, fetch = bt.refine_call(fe, P["hyps"])
        r = measure(call, a.reps, ("k_reloc_", "k_pose_opt_se3"))
        got = fetch()
        print(json.dumps(dict(what="viorb_relocalization_refine_device", candidates=B, features=a.features, points=a.points,
                              stage=[R.STAGE_NAMES[g["stage"]] for g in got], counts=[[int(v) for v in g["counts"][:5]] for g in got], **r)), flush=True)
    import reloc_ref as T
    import reloc_cases as K
    h = P["hyps"][0]
    frame = T.Frame(T.Camera(P["intr4"], P["bounds4"], P["sf"]), P["kps"], P["desc"])
    t0 = time.perf_counter()
    K.ref_search(frame, h)
    print(json.dumps({"numpy_checker_search_one_candidate_ms": (time.perf_counter() - t0) * 1e3}), flush=True)


if __name__ == "__main__":
    main()
