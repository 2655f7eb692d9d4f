"""Time of viorb_global_ba_se3 by map size, all monocular and half stereo: milliseconds per solve (HIP events around the device-form
call, inputs resident, median of --reps runs, profiling off), then one solve with the library's per-kernel events on: milliseconds per
kernel family, the FP64 rate of the factorisation (n^3 / 3 per trial, n = 6 x free key frames), and how far k_gse3_schur and the
factorisation are from their floors: the bytes of S the Schur atomics must touch (8 x 36 per pair of observers) over the HBM rate, and
n^3 / 3 over the FP64 matrix peak. With --navstate the NavState solve (twice the reduced order at the same N) is timed the same way in
the same session, as the only existing yardstick.
usage: python tools/global_ba_se3_time.py [--reps R] [--navstate] [N ...]   (default 64 256 1024 2048)"""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import viorb_amd
from viorb_amd import capi
from viorb_amd.capi import ptr, check, _torch_up as up
from viorb_amd.synth import make_global_ba_se3_problem, make_global_ba_problem

FAMILIES = {"graph set-up": ("k_gse3_setup", "k_gba_setup", "k_gba_edges_scan", "k_gba_kf_offsets", "k_gba_kf_fill", "k_gba_kf_sort"),
            "linearisation": ("k_gse3_lin_edges", "k_gse3_hll", "k_gse3_hpp", "k_gba_lin_edges", "k_gba_hll", "k_gba_hpp", "k_gba_imu", "k_gba_max_diag"),
            "chi2": ("k_gse3_errors", "k_gba_errors", "k_gba_imu_errors"),
            "reduced system": ("k_gba_dinv", "k_gse3_init_reduced", "k_gse3_schur", "k_gba_init_reduced", "k_gba_schur"),
            "factorisation": ("k_gba_potrf", "k_gba_trsm", "k_gba_syrk"),
            "backward solve": ("k_gba_bwd",),
            "increments": ("k_gse3_backsub", "k_gse3_update", "k_gba_backsub", "k_gba_update")}
PEAK_FP64_MATRIX = 78.6e12          # MI355X FP64 matrix peak (vendor figure)
HBM_BYTES_PER_S = 8e12              # MI355X HBM3E peak (vendor figure)


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


class Solve:
    """one problem resident on the device + a callable that runs the device form once and returns info[6]"""
    def __init__(self, kind, p, robust):
        import torch
        L = viorb_amd.lib()
        self.kind, self.p = kind, p
        nk, npt, ne = len(p["kfs"]), len(p["points"]), len(p["edge_idx"])
        w = 7 if kind == "se3" else 22
        t = dict(kfs=up(np.ascontiguousarray(p["kfs"], np.float64).reshape(-1, w)), fixed=up(np.ascontiguousarray(p["fixed"], np.uint8)),
                 points=up(np.ascontiguousarray(p["points"], np.float64)), ei=up(np.ascontiguousarray(p["edge_idx"], np.int32)),
                 eo=up(np.ascontiguousarray(p["edge_obs"], np.float64)))
        ko, po = torch.zeros_like(t["kfs"]), torch.zeros_like(t["points"])
        inc = torch.zeros(npt, dtype=torch.uint8, device="cuda")
        self.info = np.zeros(6)
        cfg = capi.GbaConfig(10, robust)
        if kind == "se3":
            nbytes = int(L.viorb_global_ba_se3_workspace_bytes(nk, npt, ne)); ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            intr = np.ascontiguousarray(p["intr5"], np.float64)
            self.call = lambda: check(L.viorb_global_ba_se3_device(C.byref(cfg), ptr(t["kfs"]), nk, ptr(t["fixed"]), ptr(t["points"]), npt, ptr(t["ei"]), ptr(t["eo"]), ne,
                                                                   ptr(intr), None, ptr(ko), ptr(po), ptr(inc), ptr(self.info), ptr(ws), nbytes, None))
        else:
            t["prev"] = up(np.ascontiguousarray(p["prev"], np.int32)); t["preint"] = up(np.ascontiguousarray(p["preint"], np.float64))
            nbytes = int(L.viorb_global_ba_navstate_workspace_bytes(nk, npt, ne)); ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            gw, cam = np.ascontiguousarray(p["gw"], np.float64), np.ascontiguousarray(p["cam"], np.float64)
            self.call = lambda: check(L.viorb_global_ba_navstate_device(C.byref(cfg), ptr(t["kfs"]), nk, ptr(t["prev"]), ptr(t["fixed"]), ptr(t["preint"]), ptr(t["points"]), npt,
                                                                        ptr(t["ei"]), ptr(t["eo"]), ne, ptr(gw), ptr(cam), None, ptr(ko), ptr(po), ptr(inc), ptr(self.info), ptr(ws), nbytes, None))
        self.keep = (t, ko, po, inc, ws, cfg)

    def timed(self, reps):
        import torch
        self.call(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); self.call(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), min(ms), max(ms)


def report(label, s, n, reps):
    L = viorb_amd.lib()
    p = s.p
    med, lo, hi = s.timed(reps)
    trials = int(s.info[3])
    print("%s n %5d points %6d edges %7d: median of %d %9.2f ms per solve (min %.2f max %.2f), %d iterations, %d trials, %8.3f ms per trial, chi2 %.6g -> %.6g" %
          (label, n, len(p["points"]), len(p["edge_idx"]), reps, med, lo, hi, int(s.info[2]), trials, med / max(trials, 1), s.info[0], s.info[1]), flush=True)
    L.viorb_profile_select(None); L.viorb_profile_reset(); L.viorb_profile_enable(1)
    s.call()
    prof = profile()
    L.viorb_profile_enable(0)
    trials = int(s.info[3])
    print("   with per-kernel events: %.2f ms in kernels, %d launches" % (sum(v[0] for v in prof.values()), sum(v[1] for v in prof.values())))
    for fam, ks in FAMILIES.items():
        ks = [k for k in ks if k in prof]
        print("   %-16s %9.3f ms  %6d launches   (%s)" % (fam, sum(prof[k][0] for k in ks), sum(prof[k][1] for k in ks), ", ".join("%s %.3f" % (k[2:], prof[k][0]) for k in ks)))
    fac = sum(prof.get(k, (0, 0))[0] for k in FAMILIES["factorisation"]) * 1e-3
    flops = trials * float(n) ** 3 / 3.0
    if fac > 0:
        print("   factorisation: %d trials x n^3 / 3 = %.3g FLOP in %.3f ms = %.3f TFLOP/s; floor at the FP64 matrix peak %.3f ms: %.1f x the floor" %
              (trials, flops, fac * 1e3, flops / fac / 1e12, flops / PEAK_FP64_MATRIX * 1e3, fac / (flops / PEAK_FP64_MATRIX)))
    # the Schur kernel: every ordered pair of free observers of a point with rank(a) >= rank(b) adds a 6 x 6 block: an atomic read-modify-write of 288 bytes
    ei = p["edge_idx"]; free = np.asarray(p["fixed"])[ei[:, 1]] == 0
    m = np.bincount(ei[free, 0], minlength=len(p["points"])).astype(np.float64)
    pairs = float((m * (m + 1) / 2).sum())
    name = "k_gse3_schur" if s.kind == "se3" else "k_gba_schur"
    if name in prof and prof[name][0] > 0:
        byts = trials * pairs * 36 * 8 * 2 + trials * len(ei) * 18 * 8
        print("   %s: %d trials x %.0f blocks: %.3g bytes (S read + written by the atomics, W read once) in %.3f ms = %.1f GB/s; floor at the HBM rate %.4f ms: %.0f x the floor" %
              (name, trials, pairs, byts, prof[name][0], byts / (prof[name][0] * 1e-3) / 1e9, byts / HBM_BYTES_PER_S * 1e3, prof[name][0] * 1e-3 / (byts / HBM_BYTES_PER_S)), flush=True)


def main():
    args = sys.argv[1:]
    reps = 10
    if "--reps" in args:
        i = args.index("--reps"); reps = int(args[i + 1]); del args[i:i + 2]
    nav = "--navstate" in args
    sizes = [int(a) for a in args if not a.startswith("--")] or [64, 256, 1024, 2048]
    if viorb_amd.lib().viorb_device_count() < 1:
        raise SystemExit("global_ba_se3_time.py needs a HIP device")
    for N in sizes:
        for stereo in (0.0, 0.5):
            p = make_global_ba_se3_problem(900 + N, N, stereo_frac=stereo, revisit_frac=0.2)
            report("SE3      N %4d stereo %.1f" % (N, stereo), Solve("se3", p, 1), 6 * (N - 1), reps)
        if nav:
            p = make_global_ba_problem(500 + N, N, revisit_frac=0.2)
            report("NavState N %4d           " % N, Solve("navstate", p, 1), 12 * (N - 1), reps)


if __name__ == "__main__":
    main()
