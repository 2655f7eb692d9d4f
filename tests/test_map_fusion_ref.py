"""Map fusion without a GPU: the literal checker tests/map_fusion_ref.py against hand-written expectations, and the host build of
viorb_amd/csrc/map_fusion_core.h (viorb_debug_apply_fuse_host) against the checker on the hand-built scenes, the scenes sized around the
kernels' strides, every kind of broken snapshot and the seeded random set. Every comparison is exact."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import map_fusion as M
import map_fusion_ref as T
import map_fusion_cases as K


def test_symbols_struct_layout_and_codes():
    L = viorb_amd.lib()
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_map_fusion.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_map_fusion.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_MAP_FUSION) and len(counts) == 6
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_MAP_FUSION[name][1]) == n, name
    assert not set(capi.SIGNATURES_MAP_FUSION) & set(capi.SIGNATURES)
    for name in ("POSE", "SIM3", "OVERFLOW", "ADDED", "REPLACED_KF_POINT", "REPLACED_CANDIDATE", "COUNTED_ONLY", "SKIP_BAD", "SKIP_IN_KF", "NONE", "NULL_POINT"):
        code = int(re.search(r"#define VIORB_FUSE_%s\s+(\d+)\b" % name, text).group(1))
        assert getattr(M, name) == getattr(T, name) == code, name
    assert M.INVALID == T.INVALID == capi.ERR_INVALID_ARG and M.OK == T.OK == 0
    fields = re.search(r"typedef struct viorb_fuse_map \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.FUSE_ARRAYS
    assert tuple(n.strip() for n in re.search(r"int32_t ([\w, ]+);", fields).group(1).split(",")) == capi.FUSE_INTS
    fields = re.search(r"typedef struct viorb_fuse_result \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.FUSE_RESULT_FIELDS
    assert C.sizeof(capi.FuseMap) == 10 * 4 + 25 * C.sizeof(C.c_void_p) and C.sizeof(capi.FuseResult) == 19 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_checker_pins_and_host_core(name):
    _, scene, want = next(c for c in K.CASES if c[0] == name)
    e = K.expected(name)
    assert K.compare_want(e, want) == []
    h = M.apply_fuse_host_core([scene])[0]
    assert K.compare_want(h, want) == []
    assert T.differences(h, e) == [] and h["untouched"]


def test_the_hand_built_scenes_cover_what_they_name():
    ev = {c[0]: K.expected(c[0])["events"] for c in K.CASES}
    for name, what in (("add", "add-mono"), ("add", "add-stereo"), ("replace_kf_point", "replace-kf-point"), ("replace_candidate", "replace-candidate"), ("tie", "replace-tie"),
                       ("bad_in_kf", "counted-only"), ("shared_observer", "shared-observer-erased"), ("same_point", "same-point"), ("duplicate_goes_bad", "duplicate-went-bad"),
                       ("duplicate_enters_kf", "duplicate-entered-kf"), ("null_entry", "null-entry"), ("sim3_lands_on_filled", "sim3-lands-on-filled-feature"),
                       ("sim3_replace_of_bad", "sim3-replace-of-bad-point"), ("sim3_already_found", "sim3-already-found"),
                       ("sim3_already_found", "sim3-add-observation-early-return"), ("two_calls", "second-call-reads-first")):
        assert ev[name].get(what, 0) >= 1, (name, what, ev[name])
    # the permuted keys change the order of the output and nothing else
    a, b = K.expected("tie"), K.expected("permuted_keys")
    assert a["obs"][1] == b["obs"][1][::-1] and np.array_equal(a["kp_point_out"], b["kp_point_out"])
    # without its first call the second call of two_calls goes the other way
    s = dict(next(c[1] for c in K.CASES if c[0] == "two_calls"))
    for f in ("call_kf", "call_kind", "call_list", "call_n", "call_feat"):
        s[f] = s[f][1:]
    assert list(T.apply_fuse(s)["op_reason"]) == [T.REPLACED_CANDIDATE]


def test_the_random_set_holds_every_situation_and_the_host_core_equals_the_checker():
    scenes, exp, events = K.random_streams()
    # the situations the set must hold, counted by the checker alone, before any comparison
    assert all(events.get(what, 0) >= 1 for what in T.EVENTS), {w: events.get(w, 0) for w in T.EVENTS}
    assert K.SEEDS == tuple(range(200, 260)) and len(scenes) == 60
    got = M.apply_fuse_host_core(scenes)
    assert [(b, T.differences(g, e)) for b, (g, e) in enumerate(zip(got, exp)) if T.differences(g, e)] == []
    assert got[0]["untouched"]
    one = [M.apply_fuse_host_core([s])[0] for s in scenes[:10]]
    assert [T.differences(g, e) for g, e in zip(one, exp)] == [[]] * 10


def test_host_core_equals_the_checker_at_the_edges_of_the_kernels_shapes():
    thr, wave, lds_kf, _ = M.shape()
    assert (thr, wave, lds_kf) == (256, 64, 0)
    named = K.sized_scenes()
    assert {n for n, _ in named} == {"%s_%d" % (k, s + d) for k in ("observers", "entries") for s in (wave, thr) for d in (-1, 0, 1)}
    for n, s in named:
        e = T.apply_fuse(s)
        assert T.differences(M.apply_fuse_host_core([s])[0], e) == [], n
        kind, size = n.rsplit("_", 1)
        if kind == "observers":
            assert e["events"]["shared-observer-erased"] == (int(size) + 2) // 3 and len(e["obs"][1]) == int(size) + 1
        else:
            assert list(e["call_nfused"]) == [int(size)] * 2 and int(e["pt_bad_out"].sum()) == int(size)


def test_broken_snapshots_are_refused_and_their_neighbours_intact():
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "shared_observer")
    e_good, e_other = T.apply_fuse(good), T.apply_fuse(other)
    assert int((e_good["op_reason"] == T.ADDED).sum()) >= 1
    kinds = K.broken(other, good)
    assert len(kinds) == 27
    for name, P, statuses in kinds:
        got = M.apply_fuse_host_core(None, packed=P)
        assert [g["status"] for g in got] == statuses, name
        assert T.differences(got[0], e_other) == [], name
        if statuses[2] == T.OK:
            assert T.differences(got[2], e_good) == [], name
        assert got[0]["untouched"], name


def test_overflow_reports_need_and_optional_outputs_may_be_left_out():
    scenes = [c[1] for c in K.CASES]
    exp = [T.apply_fuse(s) for s in scenes]
    got = M.apply_fuse_host_core(scenes)
    assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * len(scenes) and got[0]["untouched"]
    # tight regions: obs_start_out is one CSR over the batch
    tight = M.apply_fuse_host_core(scenes, regions=[e["need"] for e in exp])
    assert [T.differences(g, e) for g, e in zip(tight, exp)] == [[]] * len(scenes) and tight[0]["untouched"]
    # one entry short in stream 1: overflow there, the others as before
    regions = [M.region_bound(s) for s in scenes]
    regions[1] = exp[1]["need"] - 1
    short = M.apply_fuse_host_core(scenes, regions=regions)
    e1 = T.apply_fuse(scenes[1], region=regions[1])
    assert short[1]["status"] == T.OVERFLOW and short[1]["need"] == exp[1]["need"] and T.differences(short[1], e1) == []
    assert [T.differences(g, e) for g, e in zip(short[2:], exp[2:])] == [[]] * (len(scenes) - 2) and T.differences(short[0], exp[0]) == [] and short[0]["untouched"]
    # the required outputs alone
    req = M.apply_fuse_host_core(scenes, fields=capi.FUSE_RESULT_REQUIRED)
    for g, e in zip(req, exp):
        assert T.differences(g, e, fields=("kp_point_out", "pt_bad_out", "pt_nobs_out")) == [] and g["untouched"]
    assert T.differences(req[-1], exp[-1]) == []                       # the last stream's CSR is complete without `need`


def test_argument_checks_come_first():
    s = K.breakable_scene()
    P = M.pack([s])
    o = M.S.outputs(capi.FUSE_RESULT_FIELDS, lambda f: M.out_len(P, f), M.out_dtype)
    m = M._map_struct(P)
    L = viorb_amd.lib()
    for f in capi.FUSE_RESULT_REQUIRED:
        r = M._result_struct(o, [x for x in capi.FUSE_RESULT_FIELDS if x != f])
        assert L.viorb_debug_apply_fuse_host(C.byref(m), C.byref(r)) == capi.ERR_INVALID_ARG, f
        assert L.viorb_apply_fuse(C.byref(m), C.byref(r)) == capi.ERR_INVALID_ARG, f
    r = M._result_struct(o, [x for x in capi.FUSE_RESULT_FIELDS if x != "dirty_obs_kf"])
    assert L.viorb_debug_apply_fuse_host(C.byref(m), C.byref(r)) == capi.ERR_INVALID_ARG
    r = M._result_struct(o, capi.FUSE_RESULT_FIELDS)
    for f, v in (("batch", 0), ("batch", 65536), ("n_op", -1), ("n_obs_out", -1)):
        m2 = M._map_struct(dict(P, **{f: v}))
        assert L.viorb_debug_apply_fuse_host(C.byref(m2), C.byref(r)) == capi.ERR_INVALID_ARG, f
    assert L.viorb_apply_fuse_workspace_bytes(0, 1, 1, 1, 1) == 0 and L.viorb_apply_fuse_workspace_bytes(1, 1, 1, 1, -1) == 0
    assert L.viorb_apply_fuse_workspace_bytes(1, 4, 5, 9, 5) % 256 == 0
    assert L.viorb_apply_fuse_device(C.byref(m), C.byref(r), None, 0, None) == capi.ERR_INVALID_ARG
    assert L.viorb_fuse_merge_descriptors_device(None, None, None, None, 0, None) == capi.ERR_INVALID_ARG
