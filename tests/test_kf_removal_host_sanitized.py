"""kf_removal_core.h compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/cpp/kf_removal_core_host_test.cpp) run as a child process on packed snapshots with exactly sized arrays: the seeded random set,
the hand-built scenes as one batch, the scenes sized around the kernels' strides, and every kind of broken snapshot in the middle of
three streams, each of which the validator must refuse without reading through it and without writing anything but its status. The
program prints a checksum over every result array, which must equal the one computed here from the checker tests/kf_removal_ref.py. A
clean exit is required. The sanitizer runtimes are linked statically into the program; nothing sanitised is loaded into this process."""
import os
import subprocess
import numpy as np
from viorb_amd import capi, snapshot as S
from viorb_amd import kf_removal as M
import kf_removal_ref as T
import kf_removal_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = capi.KFR_RESULT_FIELDS[:6] + capi.KFR_RESULT_FIELDS[7:] + ("status",)      # the order the program mixes the arrays in


def checksum(P, results):
    """The program's checksum from the checker's per-stream results (None: a refused stream, whose ranges keep the fill)."""
    o = S.outputs(capi.KFR_RESULT_FIELDS, lambda f: M.out_len(P, f), M.out_dtype)
    cc = P["ccap"]
    for b, r in enumerate(results):
        o["status"][b] = T.INVALID if r is None else T.OK
        if r is None:
            continue
        k0, k1, p0, p1, j0, j1, i0, i1, o0, o1 = M._ranges(P, b)
        for f in capi.KFR_RESULT_FIELDS:
            if f in M.KF_ROWS:
                o[f][k0 * cc:k1 * cc] = r[f].ravel()
            elif f == "kf_Tcp_out":
                for k, Tcp in enumerate(r["kf_Tcp"]):
                    if Tcp is not None:
                        o[f][(k0 + k) * 12:(k0 + k + 1) * 12] = Tcp
            elif f != "status":
                a, e = {"kp_point_out": (i0, i1), "obs_alive": (o0, o1)}.get(f, (k0, k1) if f in M.KF_FIELDS else (p0, p1) if f in M.PT_FIELDS else (j0, j1))
                o[f][a:e] = r[f]
    n = dict(n_kf=P["n_kf"], n_pt=P["n_pt"], n_op=P["n_op"], n_kp=P["n_kp"], n_obs=P["n_obs"])
    h = 0
    for f in ORDER:
        a = o[f][:{"status": P["batch"], "kf_Tcp_out": 12 * n["n_kf"], "kp_point_out": n["n_kp"], "obs_alive": n["n_obs"]}.get(
            f, n["n_kf"] * cc if f in M.KF_ROWS else n["n_kf"] if f in M.KF_FIELDS else n["n_pt"] if f in M.PT_FIELDS else n["n_op"])]
        vals = a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int64) & 0xffffffff
        for v in vals.tolist():
            h = (h * 1000003 + v) & 0xffffffffffffffff
    return h


def test_kf_removal_core_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "kf_removal_core_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "viorb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "kf_removal_core_host_test.cpp"), "-o", exe])
    scenes, exp, events = K.random_streams()
    assert all(events.get(what, 0) >= 1 for what in T.EVENTS), events
    batches = [(scenes, exp, K.RANDOM_CCAP), ([c[1] for c in K.CASES], [T.remove_key_frames(c[1], ccap=5) for c in K.CASES], 5)]
    batches += [([s], [T.remove_key_frames(s, ccap=cc)], cc or max(1, len(s["kf_flags"]) - 1)) for _, s, cc in K.sized_scenes()]
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "points")
    e_good, e_other = T.remove_key_frames(good, ccap=4), T.remove_key_frames(other, ccap=4)
    batches += [([other, bad, good], [e_other, None, e_good], 4) for _, bad in K.broken(good)]
    files, want = [], []
    for i, (ss, results, cc) in enumerate(batches):
        P = M.pack(ss, ccap=cc)
        path = str(tmp_path / ("snapshot_%d.bin" % i))
        S.write_snapshot(path, [P[f] for f in capi.KFR_INTS] + [P["ccap"]], P, capi.KFR_ARRAYS)
        clean = P if None not in results else M.pack([other, good, good], ccap=cc)      # a broken stream's own offsets are not used
        files.append(path)
        want.append("checksum %016x status %s" % (checksum(clean, results), " ".join(str(T.INVALID if r is None else T.OK) for r in results)))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = r.stdout.strip().split("\n")
    assert len(got) == len(want) == 2 + 14 + 28
    assert [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w] == []
