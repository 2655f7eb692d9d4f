"""Time of viorb_global_ba_navstate by map size: milliseconds per solve and per Levenberg trial (wall clock around the host-buffer
call, profiling off), then the same solve with the library's per-kernel events on: milliseconds per kernel family and the FP64 rate of
the factorisation (n^3 / 3 per trial, n = 12 x free key frames, over the time of k_gba_potrf + k_gba_trsm + k_gba_syrk together), the rate
of k_gba_syrk by the FLOP it executes itself, and the time of the memset that clears the reduced matrix before every trial. At N = 21
the same problem also goes through viorb_local_ba_navstate, whose first phase is the same computation inside one workgroup.
usage: python tools/global_ba_time.py [N ...]   (default 21 60 128 256 512 1024)"""
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import viorb_amd
from viorb_amd import GlobalBundleAdjustmentNavState, LocalBundleAdjustmentNavState
from viorb_amd.synth import make_global_ba_problem

FAMILIES = {"graph set-up": ("k_gba_setup", "k_gba_edges_scan", "k_gba_kf_offsets", "k_gba_kf_fill", "k_gba_kf_sort"),
            "linearisation": ("k_gba_lin_edges", "k_gba_hll", "k_gba_hpp", "k_gba_imu", "k_gba_max_diag"),
            "chi2": ("k_gba_errors", "k_gba_imu_errors"),
            "reduced system": ("k_gba_dinv", "k_gba_init_reduced", "k_gba_schur"),
            "factorisation": ("k_gba_potrf", "k_gba_trsm", "k_gba_syrk"),
            "backward solve": ("k_gba_bwd",),
            "increments": ("k_gba_backsub", "k_gba_update")}
PEAK_FP64_MATRIX = 78.6e12          # MI355X FP64 matrix peak (vendor figure)
WINDOW_CHOL = 2.07e12               # k_bab_chol_solve


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [21, 60, 128, 256, 512, 1024]
    L = viorb_amd.lib()
    if L.viorb_device_count() < 1:
        raise SystemExit("global_ba_time.py needs a HIP device")
    import torch
    # what one small readback costs by itself: 32 bytes device -> page-locked host on an idle stream, copy + synchronise
    d = torch.zeros(4, dtype=torch.float64, device="cuda"); h = torch.zeros(4, dtype=torch.float64).pin_memory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        h.copy_(d, non_blocking=True); torch.cuda.synchronize()
    print("one 32-byte readback (copy + synchronise, idle stream): %.1f us" % ((time.perf_counter() - t0) / 200 * 1e6), flush=True)
    for N in sizes:
        p = make_global_ba_problem(500 + N, N, revisit_frac=0.2)
        a = (p["kfs"], p["prev"], p["fixed"], p["preint"], p["points"], p["edge_idx"], p["edge_obs"], p["gw"], p["cam"])
        n = 12 * (N - 1)
        for robust in (0, 1):
            GlobalBundleAdjustmentNavState(*a, iterations=10, robust=robust)
            reps = 3 if N <= 256 else 1
            t0 = time.perf_counter()
            for _ in range(reps):
                r = GlobalBundleAdjustmentNavState(*a, iterations=10, robust=robust)
            wall = (time.perf_counter() - t0) / reps * 1e3
            print("N %4d n %5d points %6d edges %7d robust %d: %9.2f ms per solve, %d iterations, %d trials, %8.3f ms per trial, chi2 %.6g -> %.6g" %
                  (N, n, len(p["points"]), len(p["edge_idx"]), robust, wall, r["iterations"], r["trials"], wall / max(r["trials"], 1), r["chi2_before"], r["chi2_after"]), flush=True)
        L.viorb_profile_select(None); L.viorb_profile_reset(); L.viorb_profile_enable(1)
        t0 = time.perf_counter()
        r = GlobalBundleAdjustmentNavState(*a, iterations=10, robust=1)
        wall_prof = (time.perf_counter() - t0) * 1e3
        prof = profile()
        L.viorb_profile_enable(0)
        tot = sum(v[0] for v in prof.values())
        print("   with per-kernel events (every launch pays an event pair): %.2f ms wall, %.2f ms in kernels, %d launches" % (wall_prof, tot, sum(v[1] for v in prof.values())))
        for fam, ks in FAMILIES.items():
            ms = sum(prof.get(k, (0, 0))[0] for k in ks); nl = sum(prof.get(k, (0, 0))[1] for k in ks)
            print("   %-16s %9.3f ms  %6d launches   (%s)" % (fam, ms, nl, ", ".join("%s %.3f" % (k[6:], prof.get(k, (0, 0))[0]) for k in ks)))
        fac = sum(prof.get(k, (0, 0))[0] for k in FAMILIES["factorisation"]) * 1e-3
        flops = r["trials"] * float(n) ** 3 / 3.0
        print("   factorisation: %d trials x n^3 / 3 (n = %d: the useful work of a Cholesky of this order) = %.3g FLOP over the time of all three kernels, %.3f ms = %.3f TFLOP/s"
              "  (window solve's k_bab_chol_solve: %.2f; FP64 matrix peak: %.1f)" % (r["trials"], n, flops, fac * 1e3, flops / fac / 1e12, WINDOW_CHOL / 1e12, PEAK_FP64_MATRIX / 1e12))
        # what k_gba_syrk itself executes: every 64 x 64 tile of the trailing lower block triangle (diagonal tiles three quadrants of four), 2 * 64^3 each
        T = (n + 63) // 64
        tiles = sum(t * (t + 1) / 2 - t / 4.0 for t in range(1, T))
        syrk_ms = prof.get("k_gba_syrk", (0, 0))[0]
        if syrk_ms > 0:
            print("   k_gba_syrk alone: %d trials x %.0f tile updates x 2 * 64^3 = %.3g executed MFMA FLOP in %.3f ms = %.3f TFLOP/s" %
                  (r["trials"], tiles, r["trials"] * tiles * 2 * 64 ** 3, syrk_ms, r["trials"] * tiles * 2 * 64 ** 3 / (syrk_ms * 1e-3) / 1e12))
        # the reduced matrix is cleared by a memset before every trial: no kernel family above shows it
        ld = T * 64
        S = torch.empty(ld * ld, dtype=torch.float64, device="cuda")
        S.zero_(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            S.zero_()
        torch.cuda.synchronize()
        print("   clearing the reduced matrix (%d x %d doubles, %.1f MB, once per trial): %.3f ms" % (ld, ld, ld * ld * 8 / 1e6, (time.perf_counter() - t0) / 5 * 1e3), flush=True)
        del S
        if N == 21:
            # the same problem as a window: key frame 0 fixed and last in the table, the others local
            order = list(range(1, N)) + [0]
            ei = p["edge_idx"].copy(); ei[:, 1] = np.where(ei[:, 1] == 0, N - 1, ei[:, 1] - 1)
            w = (p["kfs"][order], N - 1, N - 1, p["preint"][1:], p["points"], ei, p["edge_obs"], p["gw"], p["cam"])
            LocalBundleAdjustmentNavState(*w)
            t0 = time.perf_counter()
            for _ in range(5):
                lw = LocalBundleAdjustmentNavState(*w)
            wl = (time.perf_counter() - t0) / 5 * 1e3
            its = lw["its_first"] + lw["its_second"]
            print("   viorb_local_ba_navstate on the same problem: %.2f ms per solve, %d + %d iterations (at least as many trials): at most %.3f ms per trial" %
                  (wl, lw["its_first"], lw["its_second"], wl / max(its, 1)), flush=True)


if __name__ == "__main__":
    main()
