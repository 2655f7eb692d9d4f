"""Time of viorb_optimize_essential_graph_device by map size, free and fixed scale: milliseconds per solve (HIP events around the
device-form call, inputs resident, median of --reps runs, profiling off), then one solve with the library's per-kernel events on:
milliseconds per kernel family, split into the shared factorisation and the essential graph's own kernels, and the FP64 rate of the
factorisation (n^3 / 3 per trial, n = 7 x free key frames). There is no g2o to run beside it: the yardstick is viorb_global_ba_se3_device
at the nearest equal reduced order (6 x free key frames), timed in the same session.
usage: python tools/essential_graph_time.py [--reps R] [--no-yardstick] [N ...]   (default 64 256 1024 2048)"""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import viorb_amd
from viorb_amd import capi
from viorb_amd.capi import ptr, check, _torch_up as up
from viorb_amd.synth import make_essential_graph_problem, make_global_ba_se3_problem

FAMILIES = {"graph set-up": ("k_eg_setup", "k_eg_csr_offsets", "k_eg_csr_fill", "k_eg_csr_sort"),
            "linearisation": ("k_eg_linearise", "k_eg_hpp", "k_gba_max_diag"),
            "chi2": ("k_eg_errors",),
            "system assembly": ("k_eg_init_reduced",),
            "factorisation": ("k_gba_potrf", "k_gba_trsm", "k_gba_syrk"),
            "backward solve": ("k_gba_bwd",),
            "increments": ("k_eg_update",),
            "write-back": ("k_eg_recover",)}
OWN = ("graph set-up", "linearisation", "chi2", "system assembly", "increments", "write-back")
PEAK_FP64_MATRIX = 78.6e12          # MI355X FP64 matrix peak (vendor figure)


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def timed(call, reps):
    import torch
    call(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def essential_graph_call(p):
    import torch
    L = viorb_amd.lib()
    nk, ne, npt = len(p["Scw"]), len(p["edge_idx"]), len(p["points"])
    t = dict(Scw=up(np.ascontiguousarray(p["Scw"], np.float64)), Smeas=up(np.ascontiguousarray(p["Smeas"], np.float64)), fixed=up(np.ascontiguousarray(p["fixed"], np.uint8)),
             ei=up(np.ascontiguousarray(p["edge_idx"], np.int32)), ec=up(np.ascontiguousarray(p["edge_corrected"], np.uint8)),
             pts=up(np.ascontiguousarray(p["points"], np.float32)), ref=up(np.ascontiguousarray(p["point_ref"], np.int32)))
    So, To, Po = torch.zeros_like(t["Scw"]), torch.zeros((nk, 12), dtype=torch.float64, device="cuda"), torch.zeros_like(t["pts"])
    nbytes = int(L.viorb_essential_graph_workspace_bytes(nk, ne, npt)); ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    info, cfg = np.zeros(6), capi.EgConfig(20, int(p["fix_scale"]))
    call = lambda: check(L.viorb_optimize_essential_graph_device(C.byref(cfg), ptr(t["Scw"]), ptr(t["Smeas"]), ptr(t["fixed"]), nk, ptr(t["ei"]), ptr(t["ec"]), ne,
                                                                 ptr(t["pts"]), ptr(t["ref"]), npt, ptr(So), ptr(To), ptr(Po), ptr(info), ptr(ws), nbytes, None))
    return call, info, (t, So, To, Po, ws, cfg)


def se3_call(p):
    import torch
    L = viorb_amd.lib()
    nk, npt, ne = len(p["kfs"]), len(p["points"]), len(p["edge_idx"])
    t = dict(kfs=up(np.ascontiguousarray(p["kfs"], np.float64).reshape(-1, 7)), fixed=up(np.ascontiguousarray(p["fixed"], np.uint8)),
             points=up(np.ascontiguousarray(p["points"], np.float64)), ei=up(np.ascontiguousarray(p["edge_idx"], np.int32)), eo=up(np.ascontiguousarray(p["edge_obs"], np.float64)))
    ko, po, inc = torch.zeros_like(t["kfs"]), torch.zeros_like(t["points"]), torch.zeros(npt, dtype=torch.uint8, device="cuda")
    nbytes = int(L.viorb_global_ba_se3_workspace_bytes(nk, npt, ne)); ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    info, cfg, intr = np.zeros(6), capi.GbaConfig(10, 1), np.ascontiguousarray(p["intr5"], np.float64)
    call = lambda: check(L.viorb_global_ba_se3_device(C.byref(cfg), ptr(t["kfs"]), nk, ptr(t["fixed"]), ptr(t["points"]), npt, ptr(t["ei"]), ptr(t["eo"]), ne, ptr(intr), None,
                                                      ptr(ko), ptr(po), ptr(inc), ptr(info), ptr(ws), nbytes, None))
    return call, info, (t, ko, po, inc, ws, cfg)


def report(label, call, info, n, reps, families):
    L = viorb_amd.lib()
    med, lo, hi = timed(call, reps)
    trials = int(info[3])
    print("%s n %5d: median of %d %9.2f ms per solve (min %.2f max %.2f), %d iterations, %d trials, %8.3f ms per trial, chi2 %.6g -> %.6g" %
          (label, n, reps, med, lo, hi, int(info[2]), trials, med / max(trials, 1), info[0], info[1]), flush=True)
    if families is None:
        return
    L.viorb_profile_select(None); L.viorb_profile_reset(); L.viorb_profile_enable(1)
    call()
    prof = profile()
    L.viorb_profile_enable(0)
    trials = int(info[3])
    total = sum(v[0] for v in prof.values())
    print("   with per-kernel events: %.2f ms in kernels, %d launches" % (total, sum(v[1] for v in prof.values())))
    fam_ms = {}
    for fam, ks in families.items():
        ks = [k for k in ks if k in prof]
        fam_ms[fam] = sum(prof[k][0] for k in ks)
        print("   %-16s %9.3f ms  %6d launches   (%s)" % (fam, fam_ms[fam], sum(prof[k][1] for k in ks), ", ".join("%s %.3f" % (k[2:], prof[k][0]) for k in ks)))
    own = sum(fam_ms[f] for f in OWN)
    print("   the essential graph's own kernels: %.3f ms = %.1f %% of the time in kernels (%.3f ms per trial)" % (own, 100 * own / max(total, 1e-9), own / max(trials, 1)))
    fac = fam_ms["factorisation"] * 1e-3
    flops = trials * float(n) ** 3 / 3.0
    if fac > 0:
        print("   factorisation: %d trials x n^3 / 3 = %.3g FLOP in %.3f ms = %.3f TFLOP/s; floor at the FP64 matrix peak %.3f ms: %.1f x the floor" %
              (trials, flops, fac * 1e3, flops / fac / 1e12, flops / PEAK_FP64_MATRIX * 1e3, fac / (flops / PEAK_FP64_MATRIX)), flush=True)


def main():
    args = sys.argv[1:]
    reps = 5
    if "--reps" in args:
        i = args.index("--reps"); reps = int(args[i + 1]); del args[i:i + 2]
    yard = "--no-yardstick" not in args
    sizes = [int(a) for a in args if not a.startswith("--")] or [64, 256, 1024, 2048]
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("essential_graph_time.py needs a HIP device")
    for N in sizes:
        for fs in (False, True):
            # a drift per step that shrinks with the length of the loop: the accumulated error stays that of a real loop closure
            p = make_essential_graph_problem(950 + N, N=N, fix_scale=fs, rot_drift=0.5 / N, scale_drift=0.5 / N, trans_drift=0.01, n_points=20 * N, loop_edges=N // 50)
            call, info, keep = essential_graph_call(p)
            report("essential graph N %4d %s edges %6d points %6d" % (N, "fixed scale" if fs else "free scale ", len(p["edge_idx"]), len(p["points"])), call, info, 7 * (N - 1), reps, FAMILIES)
            del keep
        if yard:
            M = int(round(7 * (N - 1) / 6.0)) + 1
            q = make_global_ba_se3_problem(900 + M, M, stereo_frac=0.0, revisit_frac=0.2)
            call, info, keep = se3_call(q)
            report("yardstick: global BA SE3 N %4d                              " % M, call, info, 6 * (M - 1), reps, None)
            del keep


if __name__ == "__main__":
    main()
