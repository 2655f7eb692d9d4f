"""CPU checks of place recognition: the new C ABI is exported, checks its arguments and refuses without a device; the checker
tests/place_ref.py agrees with independent definitions (dense L1 distance, the oracle's BowVector, the sort key the device orders by);
the library's scalar pieces compiled for the host (viorb_debug_place_score / viorb_debug_place_select) equal the checker bit for bit;
and the synthetic problems exercise every branch the GPU tests rely on."""
import ctypes as C
import functools
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi, place
from viorb_amd.capi import ptr
from viorb_amd.synth import make_place_problem, make_vocabulary, descriptors_near_words
import place_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(N, per, seed, mode) for (N, per) in ((48, 120), (130, 300)) for seed in range(4) for mode in (pr.LOOP, pr.RELOC)]
NEW_SYMBOLS = ["viorb_bow_vector_device", "viorb_bow_vector", "viorb_bow_score_device", "viorb_bow_score", "viorb_kfdb_create", "viorb_kfdb_destroy",
               "viorb_kfdb_add_device", "viorb_kfdb_add", "viorb_kfdb_erase", "viorb_kfdb_clear", "viorb_kfdb_size", "viorb_kfdb_query_workspace_bytes",
               "viorb_kfdb_query_device", "viorb_kfdb_query", "viorb_debug_place_score", "viorb_debug_place_select"]


@functools.lru_cache(maxsize=None)
def solved(N, per, seed, mode):
    p = make_place_problem(seed, N, per, 4096)
    ms = pr.loop_min_score(p)
    return p, ms, pr.build(p).detect(mode, p["bows"][-1], p["covis10"], ms, p["connected"])


def test_new_symbols_are_exported_with_signatures_and_the_abi_version_is_2():
    L = viorb_amd.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n in capi.SIGNATURES, n
    assert L.viorb_abi_version() == 2
    for n in ("BowVector", "BowScore", "KeyFrameDatabase"):
        assert hasattr(viorb_amd, n)


def test_argument_errors_come_before_the_device_and_compute_refuses_without_one():
    L = viorb_amd.lib()
    i32, f64 = lambda a: np.array(a, np.int32), lambda a: np.array(a, np.float64)
    h = C.c_void_p()
    assert L.viorb_kfdb_create(0, 0, 0, C.byref(h)) == capi.ERR_INVALID_ARG
    assert L.viorb_kfdb_create(100, 4, 16, C.byref(h)) == capi.VIORB_OK
    slot, out, cnt = C.c_int(-7), np.zeros(4), C.c_int(0)
    ok_w, ok_v = i32([3, 9, 50]), f64([0.5, 0.25, 0.25])
    bad = [(i32([9, 3, 50]), ok_v, 3), (i32([3, 3, 50]), ok_v, 3), (i32([3, 9, 100]), ok_v, 3), (ok_w, f64([0.5, -0.25, 0.25]), 3),
           (ok_w, f64([0.5, np.nan, 0.25]), 3), (ok_w, ok_v, -1)]
    for w, v, n in bad:
        assert L.viorb_kfdb_add(h, ptr(w), ptr(v), n, C.byref(slot)) == capi.ERR_INVALID_ARG
    assert L.viorb_bow_vector(ptr(ok_w), ptr(ok_v), -1, ptr(ok_w), ptr(out), C.byref(cnt)) == capi.ERR_INVALID_ARG
    assert L.viorb_bow_vector(ptr(ok_w), ptr(ok_v), 0, ptr(ok_w), ptr(out), C.byref(cnt)) == capi.VIORB_OK and cnt.value == 0
    one, pa = i32([3]), i32([0])
    desc = i32([9, 3, 50])
    assert L.viorb_bow_score(ptr(desc), ptr(ok_v), ptr(one * 0 + 3), 3, 1, ptr(ok_w), ptr(ok_v), ptr(one * 0 + 3), 3, 1, ptr(pa), ptr(pa), 1, ptr(out)) == capi.ERR_INVALID_ARG
    assert L.viorb_bow_score(ptr(ok_w), ptr(ok_v), ptr(i32([-1])), 3, 1, ptr(ok_w), ptr(ok_v), ptr(i32([3])), 3, 1, ptr(pa), ptr(pa), 1, ptr(out)) == capi.ERR_INVALID_ARG
    assert L.viorb_bow_score(ptr(ok_w), ptr(ok_v), ptr(i32([3])), 3, 1, ptr(ok_w), ptr(ok_v), ptr(i32([3])), 3, 1, ptr(i32([1])), ptr(pa), 1, ptr(out)) == capi.ERR_INVALID_ARG
    cov, cand, nc, st = np.full((1, 10), -1, np.int32), i32([0] * 4), i32([0]), i32([0] * 4)
    q = lambda w, n, mode=pr.RELOC, cap=4: L.viorb_kfdb_query(h, mode, 1, ptr(w), ptr(ok_v), ptr(i32([n])), 3, None, None, None, ptr(cov), cap, ptr(cand), ptr(nc),
                                                               ptr(st), None, None)
    assert q(desc, 3) == capi.ERR_INVALID_ARG                     # descending words
    assert q(i32([3, 9, 100]), 3) == capi.ERR_INVALID_ARG         # word >= n_words
    assert q(ok_w, -1) == capi.ERR_INVALID_ARG                    # negative count
    assert q(ok_w, 3, mode=2) == capi.ERR_INVALID_ARG
    assert q(ok_w, 3, mode=pr.LOOP) == capi.ERR_INVALID_ARG       # loop mode without min_score / excl_start
    assert q(ok_w, 3, cap=0) == capi.ERR_INVALID_ARG
    # the host-mirrored bookkeeping needs no device
    a, b = C.c_int(-1), C.c_int(-1)
    assert L.viorb_kfdb_size(h, C.byref(a), C.byref(b)) == capi.VIORB_OK and (a.value, b.value) == (0, 0)
    assert L.viorb_kfdb_erase(h, 0) == capi.ERR_INVALID_ARG       # no such slot
    assert L.viorb_kfdb_clear(h) == capi.VIORB_OK
    assert L.viorb_kfdb_query_workspace_bytes(h, 3) > 0 and L.viorb_kfdb_query_workspace_bytes(h, 0) == 0
    if L.viorb_device_count() == 0:
        calls = [lambda: L.viorb_kfdb_add(h, ptr(ok_w), ptr(ok_v), 3, C.byref(slot)),
                 lambda: L.viorb_bow_vector(ptr(ok_w), ptr(ok_v), 3, ptr(i32([0] * 3)), ptr(out), C.byref(cnt)),
                 lambda: L.viorb_bow_vector_device(ptr(ok_w), ptr(ok_v), ptr(one), 3, 1, ptr(i32([0] * 3)), ptr(out), ptr(i32([0])), None),
                 lambda: L.viorb_bow_score(ptr(ok_w), ptr(ok_v), ptr(one), 3, 1, ptr(ok_w), ptr(ok_v), ptr(one), 3, 1, ptr(pa), ptr(pa), 1, ptr(out)),
                 lambda: L.viorb_bow_score_device(ptr(ok_w), ptr(ok_v), ptr(one), 3, ptr(ok_w), ptr(ok_v), ptr(one), 3, ptr(pa), ptr(pa), 1, ptr(out), None),
                 lambda: L.viorb_kfdb_add_device(h, ptr(ok_w), ptr(ok_v), ptr(one), 3, 1, C.byref(slot), None),
                 lambda: q(ok_w, 3),
                 lambda: L.viorb_kfdb_query_device(h, pr.RELOC, 1, ptr(ok_w), ptr(ok_v), ptr(one), 3, None, None, None, ptr(cov), 4, ptr(cand), ptr(nc), ptr(st),
                                                   None, None, None, 0, None)]
        for k, f in enumerate(calls):
            assert f() == capi.ERR_NO_DEVICE, k
            assert b"no HIP device" in L.viorb_last_error()
        assert L.viorb_kfdb_size(h, C.byref(a), C.byref(b)) == capi.VIORB_OK and (a.value, b.value) == (0, 0)      # a refused add leaves no slot
        with pytest.raises(viorb_amd.ViorbError) as e:
            place.KeyFrameDatabase(100).add((ok_w, ok_v))
        assert e.value.code == capi.ERR_NO_DEVICE
    # over the LDS capacity: refused, never truncated (the check precedes the device)
    big = place.BOW_VECTOR_MAX_FEATURES + 1
    assert L.viorb_bow_vector(ptr(np.zeros(big, np.int32)), ptr(np.ones(big)), big, ptr(np.zeros(big, np.int32)), ptr(np.zeros(big)), C.byref(cnt)) == capi.ERR_CAPACITY
    assert L.viorb_kfdb_destroy(h) == capi.VIORB_OK


def test_checker_score_equals_one_minus_half_the_l1_distance():
    """The band is four times the checker's own difference between forward and reverse summation of the dense |v - w|, measured here.
    The identity score = 1 - 0.5 * ||v - w||_1 needs both L1 norms to be exactly 1, so the values are multiples of 2^-20 that sum to
    2^20 of them: every sum and difference below is then exact, the band comes out as 0 and the two sides must be equal."""
    rng = np.random.default_rng(5)
    unit = 1 << 20
    for trial in range(20):
        nw = 400
        vecs = []
        for _ in range(2):
            n = int(rng.integers(1, 200))
            ids = np.sort(rng.choice(nw, n, replace=False)).astype(np.int32)
            cuts = np.sort(rng.choice(np.arange(1, unit), n - 1, replace=False)) if n > 1 else np.zeros(0, np.int64)
            parts = np.diff(np.concatenate([[0], cuts, [unit]]))                   # n positive integers that sum to 2^20
            vecs.append((ids, parts / float(unit)))
        a, b = vecs
        da, db = np.zeros(nw), np.zeros(nw)
        da[a[0]] = a[1]; db[b[0]] = b[1]
        assert float(da.sum()) == 1.0 and float(db.sum()) == 1.0
        d = np.abs(da - db)
        fwd = rev = 0.0
        for x in d.tolist():
            fwd += x
        for x in d.tolist()[::-1]:
            rev += x
        band = 4 * abs(fwd - rev)
        assert abs(pr.score(a, b) - (1.0 - 0.5 * fwd)) <= band
        assert abs(pr.score(b, a) - (1.0 - 0.5 * rev)) <= band
    assert pr.score(a, a) == 1.0


def test_list_walk_order_equals_the_smallest_common_word_then_slot_order():
    rng = np.random.default_rng(11)
    n_nontrivial = 0
    for trial in range(50):
        nw, S = int(rng.integers(20, 200)), int(rng.integers(1, 40))
        db = pr.KeyFrameDB()
        mk = lambda: (np.sort(rng.choice(nw, int(rng.integers(1, min(nw, 30))), replace=False)).astype(np.int32),)
        for _ in range(S):
            ids = mk()[0]
            v = rng.uniform(0.1, 1.0, len(ids))
            db.add((ids, v / v.sum()))
        for e in rng.choice(S, S // 5, replace=False).tolist():
            db.erase(e)
        ids = mk()[0]
        v = rng.uniform(0.1, 1.0, len(ids))
        cov = np.full((S, 10), -1, np.int32)
        for mode in (pr.LOOP, pr.RELOC):
            o = db.detect(mode, (ids, v / v.sum()), cov, 0.0, rng.choice(S, S // 6, replace=False).tolist())
            assert o["order"] == pr.order_by_key(o["common"], o["min_word"], int(np.float32(o["stats"][1]) * np.float32(0.8)))
            n_nontrivial += o["order"] != sorted(o["order"])
    assert n_nontrivial >= 10


@pytest.mark.parametrize("n,k,L", [(1, 3, 3), (64, 3, 3), (65, 3, 3), (1000, 3, 3), (2000, 3, 3), (1000, 10, 4)])
def test_checker_bow_vector_equals_the_oracle_bit_for_bit(oracle, n, k, L):
    voc = make_vocabulary(2, k=k, L=L)
    ref = oracle.bow_transform(voc, descriptors_near_words(n, voc, n))
    ids, vals = pr.bow_vector(ref["word"], ref["weight"])
    assert np.array_equal(ids, ref["bow_ids"]) and np.array_equal(vals, ref["bow_vals"])


@pytest.mark.parametrize("N,per,seed,mode", CASES)
def test_host_hooks_equal_the_checker_bit_for_bit(N, per, seed, mode):
    L = viorb_amd.lib()
    p, ms, o = solved(N, per, seed, mode)
    q, S = p["bows"][-1], N - 1
    for s in range(S):
        b = p["bows"][s]
        got = L.viorb_debug_place_score(ptr(q[0]), ptr(q[1]), len(q[0]), ptr(b[0]), ptr(b[1]), len(b[0]))
        assert got == pr.score(q, b)
    score_all = np.array([np.float32(pr.score(q, p["bows"][s])) for s in range(S)], np.float32)      # select reads it where scored only
    cand, nc, st = np.full(S, -1, np.int32), C.c_int(0), np.zeros(4, np.int32)
    cov = np.ascontiguousarray(p["covis10"], np.int32)
    rc = L.viorb_debug_place_select(mode, S, ptr(o["common"]), ptr(o["min_word"]), ptr(score_all), C.c_float(ms), ptr(cov), S, ptr(cand), C.byref(nc), ptr(st))
    assert rc == capi.VIORB_OK
    assert cand[:nc.value].tolist() == o["cand"] and st.tolist() == o["stats"]
    if len(o["cand"]) >= 2:
        assert L.viorb_debug_place_select(mode, S, ptr(o["common"]), ptr(o["min_word"]), ptr(score_all), C.c_float(ms), ptr(cov), 1, ptr(cand), C.byref(nc),
                                          ptr(st)) == capi.ERR_CAPACITY and nc.value == len(o["cand"])


def test_the_problems_exercise_every_branch():
    """Asserted on the checker alone: the cases the GPU tests compare are not vacuous."""
    outs = [solved(*c) for c in CASES]
    assert any(len(o["cand"]) >= 2 for _, _, o in outs)
    assert any(o["n_dup"] >= 1 for _, _, o in outs)
    assert any(any(own != best for own, best, _ in o["groups"]) for _, _, o in outs)
    assert any(o["cand"] != sorted(o["cand"]) for _, _, o in outs)
    assert all(o["unscored_neighbour"] for (_, _, o), c in zip(outs, CASES) if c[3] == pr.RELOC)     # the deviation's case, in every one
    # a min_score placed between two of a case's scores removes a scored slot
    p, _, o = solved(48, 120, 0, pr.LOOP)
    sc = np.sort(o["score"][o["score"] >= 0])
    assert len(sc) >= 2 and sc[0] < sc[-1]
    mid = np.float32((float(sc[0]) + float(sc[-1])) / 2)
    o2 = pr.build(p).detect(pr.LOOP, p["bows"][-1], p["covis10"], mid, p["connected"])
    assert 0 < o2["stats"][3] < o2["stats"][2]
    assert all(len(o["cand"]) >= 1 for _, _, o in outs)


def test_cpp_place_shim_compiles_links_and_throws_without_a_device(tmp_path):
    """viorb_amd/shim/KeyFrameDatabase_shim.h compiles against stand-ins that carry the reference's member names and links
    libviorb_hip.so; without a device add / DetectLoopCandidates / DetectRelocalizationCandidates / loop_min_score throw."""
    exe = str(tmp_path / "shim_place_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_place_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    if viorb_amd.lib().viorb_device_count() > 0:
        return
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
