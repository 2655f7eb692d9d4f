"""map_fusion_core.h compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/cpp/map_fusion_core_host_test.cpp) run as a child process on packed snapshots with exactly sized arrays: the seeded random set,
the hand-built scenes as one batch, the scenes sized around the kernels' strides, and every kind of broken snapshot in the middle of
three streams, each of which the validator must refuse without reading through it and without writing anything but its status. The
program prints a checksum over every result array, which must equal the one computed here from the checker tests/map_fusion_ref.py. A
clean exit is required. The sanitizer runtimes are linked statically into the program; nothing sanitised is loaded into this process."""
import os
import subprocess
import numpy as np
from viorb_amd import capi, snapshot as S
from viorb_amd import map_fusion as M
import map_fusion_ref as T
import map_fusion_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = capi.FUSE_RESULT_FIELDS[1:] + ("status",)      # the order the program mixes the arrays in


def flat_expected(P, results):
    """The result arrays of a packed batch as the library leaves them, from the checker's per-stream results (None: a refused stream,
    whose ranges keep the fill), each exactly as long as its total."""
    n = dict(kp_point_out=P["n_kp"], obs_touched=P["n_obs"], call_nfused=P["n_call"], status=P["batch"], need=P["batch"])
    length = lambda f: n.get(f, P["n_pt"] if f in M.PT_FIELDS else P["n_pt"] + 1 if f in M.PT_STARTS else P["n_obs_out"] if f in M.OUT_FIELDS else P["n_op"])
    o = {f: np.full(length(f), S.FILL, M.out_dtype(f)) for f in capi.FUSE_RESULT_FIELDS}
    dat = 0
    for b, r in enumerate(results):
        o["status"][b] = T.INVALID if r is None else r["status"]
        if r is None:
            continue
        g = M._ranges(P, b)
        o["kp_point_out"][g["i0"]:g["i1"]] = r["kp_point_out"]
        for f in M.PT_FIELDS:
            o[f][g["p0"]:g["p1"]] = r[f]
        for f in M.OP_FIELDS:
            o[f][g["j0"]:g["j1"]] = r[f]
        o["call_nfused"][g["c0"]:g["c1"]], o["obs_touched"][g["o0"]:g["o1"]], o["need"][b] = r["call_nfused"], r["obs_touched"], r["need"]
        at = g["q0"]
        for p in range(g["p1"] - g["p0"]):
            if r["status"] == T.OK:
                o["obs_start_out"][g["p0"] + p] = at
                for k, octave, stereo, f in r["obs"][p]:
                    o["obs_out"][at], o["obs_feat_out"][at] = k | (octave << 16) | (stereo << 24), f
                    at += 1
            o["dirty_obs_start"][g["p0"] + p] = dat
            for k, f in r["dirty"][p]:
                o["dirty_obs_kf"][dat], o["dirty_obs_feat"][dat] = g["k0"] + k, f
                dat += 1
        if r["status"] == T.OK and (b + 1 == len(results) or results[b + 1] is None):
            o["obs_start_out"][g["p1"]] = at
        o["dirty_obs_start"][g["p1"]] = dat
    return o


def checksum(o):
    h = 0
    for f in ORDER:
        for v in (o[f].astype(np.int64) & 0xffffffff).tolist():
            h = (h * 1000003 + v) & 0xffffffffffffffff
    return h


def test_map_fusion_core_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "map_fusion_core_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "viorb_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "map_fusion_core_host_test.cpp"), "-o", exe])
    scenes, exp, events = K.random_streams()
    assert all(events.get(what, 0) >= 1 for what in T.EVENTS), events
    batches = [(M.pack(scenes), exp), (M.pack([c[1] for c in K.CASES]), [T.apply_fuse(c[1]) for c in K.CASES])]
    batches += [(M.pack([s]), [T.apply_fuse(s)]) for _, s in K.sized_scenes()]
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "shared_observer")
    e_good, e_other = T.apply_fuse(good), T.apply_fuse(other)
    batches += [(P, [r if st == T.OK else None for r, st in zip((e_other, e_good, e_good), statuses)]) for _, P, statuses in K.broken(other, good)]
    clean = M.pack([other, good, good])                                # a broken stream's own offsets are not used
    files, want = [], []
    for i, (P, results) in enumerate(batches):
        path = str(tmp_path / ("snapshot_%d.bin" % i))
        S.write_snapshot(path, [P[f] for f in capi.FUSE_INTS], P, capi.FUSE_ARRAYS)
        files.append(path)
        o = flat_expected(clean if None in results else P, results)
        want.append("checksum %016x status %s" % (checksum(o), " ".join(str(T.INVALID if r is None else r["status"]) for r in results)))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = r.stdout.strip().split("\n")
    assert len(got) == len(want) == 2 + 12 + 27
    assert [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w] == []
