"""CPU tests of Tracking::UpdateLocalMap (no GPU): the exported symbols against include/viorb_local_map.h, the checker
tests/local_map_ref.py pinned on hand-built scenes whose expected output is written out in tests/local_map_cases.py (no votes, every
voted key frame bad, the tie in key order, the double vote, votes for a bad key frame, the 80-entry limit at 75, 79, 80, 81 and 82 voted
key frames, the choice of neighbour and child, links without a bad test, a key frame added by the loop that is not visited, points at
their first position, both overflows by one), the host build of local_map_core.h (viorb_debug_update_local_map_host) against the checker
on those scenes, on scenes sized around the kernels' strides, on 300 random streams and on every kind of broken snapshot in the middle
of three streams, and the argument checks of every entry, which come before any GPU call."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import local_map as M
import local_map_ref as T
import local_map_cases as K


def test_symbols_struct_layout_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_local_map.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_local_map.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_LOCAL_MAP)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_LOCAL_MAP[name][1]) == n, name
    for name, code in (("NO_VOTES", 1), ("OVERFLOW", 2)):
        assert re.search(r"#define VIORB_ULM_%s\s+%d\b" % (name, code), text) and getattr(M, name) == getattr(T, name) == code
    assert M.INVALID == T.INVALID == capi.ERR_INVALID_ARG and M.OK == T.OK == 0
    fields = re.search(r"typedef struct viorb_local_map_snapshot \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.LOCAL_MAP_ARRAYS
    assert tuple(n.strip() for n in re.search(r"int32_t ([\w, ]+);", fields).group(1).split(",")) == capi.LOCAL_MAP_INTS
    fields = re.search(r"typedef struct viorb_local_map_result \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.LOCAL_MAP_RESULT_FIELDS
    assert C.sizeof(capi.LocalMapSnapshot) == 6 * 4 + 20 * C.sizeof(C.c_void_p) and C.sizeof(capi.LocalMapResult) == 9 * C.sizeof(C.c_void_p)
    thr, chunk, wave, lds_kf = M.shape()
    assert wave == 64 and thr % 64 == 0 and chunk % 64 == 0 and lds_kf >= 85


@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_checker_pins_and_host_core(name):
    _, scene, caps, want = next(c for c in K.CASES if c[0] == name)
    e = K.expected(name)
    for f, v in want.items():
        assert np.asarray(e[f]).tolist() == v, (f, np.asarray(e[f]).tolist(), v)
    h = M.update_local_map_host_core([scene], **caps)[0]
    assert T.differences(h, e) == []


def test_limit_scenes_break_where_the_reference_breaks():
    # the list of 80 and 85 comes from ONE iteration: slot 0 adds its neighbour, child, parent, prev and next, in that order
    for n in (79, 80):
        e = K.expected("limit_%d_voted" % n)
        assert e["lkf"][n:].tolist() == [n, n + 1, n + 2, n + 3, n + 4]
    assert K.expected("limit_75_voted")["lkf"][75:].tolist() == [75, 76, 77, 78, 79, 80]       # the second iteration ran at exactly 80
    for n in (81, 82):
        assert K.expected("limit_%d_voted" % n)["lkf"].tolist() == list(range(n))              # the break before the first iteration


def test_host_core_equals_the_checker_at_the_edges_of_the_kernels_shapes():
    thr, chunk, wave, lds_kf = M.shape()
    named = K.sized_scenes()
    scenes = [s for _, s in named]
    exp = [T.update_local_map(s) for s in scenes]
    got = M.update_local_map_host_core(scenes)
    assert [(n, T.differences(g, e)) for (n, _), g, e in zip(named, got, exp) if T.differences(g, e)] == []
    by_name = {n: e for (n, _), e in zip(named, exp)}
    assert by_name["children_%d" % (wave + 1)]["lkf"].tolist() == [0, wave + 1]     # the only eligible child is the last of wave + 1
    assert any(e["n_voted"] > thr for e in exp) and any(e["n_lpt"] > 100 for e in exp) and all(e["status"] == T.OK for e in exp)
    # above the LDS limit the neighbour loop really runs: few voted key frames, and its pushes make up most of the list
    for d in (0, 1):
        e = by_name["loop_kf_%d" % (lds_kf + d)]
        assert 5 <= e["n_voted"] <= 12 and e["n_lkf"] >= e["n_voted"] + 15


def test_host_core_equals_the_checker_on_random_streams_in_one_batch():
    scenes, exp = K.random_streams()
    got = M.update_local_map_host_core(scenes)
    assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * 300
    st = [e["status"] for e in exp]
    assert st.count(T.NO_VOTES) >= 10 and st.count(T.OK) >= 200
    assert sum(e["n_lkf"] > e["n_voted"] for e in exp) >= 100 and sum((e["frame_point_out"] != s["frame_point"]).any() for s, e in zip(scenes, exp)) >= 50
    assert sum(e["status"] == T.OK and e["n_lkf"] == 0 for e in exp) >= 1          # every voted key frame bad


def test_batches_of_one_of_unequal_streams_and_with_an_empty_stream():
    pick = lambda n: next(c[1] for c in K.CASES if c[0] == n)
    scenes = [pick("limit_80_voted"), pick("no_key_frames"), pick("points_first_position"), pick("no_votes")]
    exp = [T.update_local_map(s) for s in scenes]
    assert [T.differences(g, e) for g, e in zip(M.update_local_map_host_core(scenes), exp)] == [[]] * 4
    for s, e in zip(scenes, exp):
        assert T.differences(M.update_local_map_host_core([s])[0], e) == []


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams():
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "neighbour_choice")
    e_good, e_other = T.update_local_map(good), T.update_local_map(other)
    kinds = K.broken(good)
    assert len(kinds) == 17
    for what, bad in kinds:
        got = M.update_local_map_host_core([other, bad, good])
        assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
        assert T.differences(got[0], e_other) == [] and T.differences(got[2], e_good) == [], what
    # counts outside their row lengths, and more previous key frames than the stream has
    for f, v in (("frame_count", 4), ("frame_count", -1), ("prev_n_lkf", 97), ("prev_n_lkf", 4)):
        P = M.pack([other, good, good])
        P[f][1] = v
        got = M.update_local_map_host_core(None, packed=P)
        assert [g["status"] for g in got] == [T.OK, T.INVALID, T.OK], (f, v)
    # descending offsets of the batch level refuse the stream and every later one
    P = M.pack([other, good, good])
    P["kf_start"][2] = P["kf_start"][1] - 1
    assert [g["status"] for g in M.update_local_map_host_core(None, packed=P)] == [T.OK, T.INVALID, T.INVALID]


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    INV, ND = capi.ERR_INVALID_ARG, capi.ERR_NO_DEVICE
    P = M.pack([K.breakable_scene()])
    wb = L.viorb_update_local_map_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"])
    gb = L.viorb_local_points_gather_workspace_bytes(P["n_pt"])
    assert wb > 0 and wb % 256 == 0 and gb > 0 and gb % 256 == 0
    assert L.viorb_update_local_map_workspace_bytes(0, 1, 1) == 0 and L.viorb_update_local_map_workspace_bytes(65536, 1, 1) == 0
    assert L.viorb_update_local_map_workspace_bytes(1, -1, 1) == 0 and L.viorb_update_local_map_workspace_bytes(1, 1, -1) == 0
    assert L.viorb_local_points_gather_workspace_bytes(-1) == 0
    ws = C.c_void_p(4096)

    def snap(null=None, **ints):
        m = M._map_struct(P)
        for k, v in ints.items():
            setattr(m, k, v)
        if null:
            setattr(m, null, None)
        return m

    def dev(w=ws, bytes_=wb, cap=P["cap"], lcap=P["lcap"], pcap=P["pcap"], **k):
        return L.viorb_update_local_map_device(C.byref(snap(**k)), None, cap, lcap, pcap, w, bytes_, None)

    def host(cap=P["cap"], lcap=P["lcap"], pcap=P["pcap"], **k):
        return L.viorb_update_local_map(C.byref(snap(**k)), None, cap, lcap, pcap)

    def core(cap=P["cap"], lcap=P["lcap"], pcap=P["pcap"], **k):
        return L.viorb_debug_update_local_map_host(C.byref(snap(**k)), None, cap, lcap, pcap)
    for fn in (dev, host, core):
        assert fn(batch=0) == INV and fn(batch=65536) == INV and fn(n_kf=-1) == INV and fn(n_child=-1) == INV and fn(n_kp=-1) == INV and fn(n_obs=-1) == INV
        assert fn(cap=0) == INV and fn(lcap=0) == INV and fn(pcap=0) == INV
        for f in capi.LOCAL_MAP_ARRAYS:
            assert fn(null=f) == INV, f
    assert L.viorb_update_local_map_device(None, None, 1, 1, 1, ws, wb, None) == INV and L.viorb_update_local_map(None, None, 1, 1, 1) == INV
    assert dev(w=None) == INV and dev(bytes_=wb - 1) == INV and dev(w=C.c_void_p(4097)) == INV
    assert L.viorb_update_local_map_shape(None) == INV
    one = C.c_void_p(256)
    res = capi.LocalMapResult(*[one] * 9)

    def gather(m=None, r=res, cap=4, pcap=4, f=one, d=one, nobs=one, of=one, od=one, oc=one, ofl=one, w=ws, bytes_=gb, **k):
        return L.viorb_local_points_gather_device(C.byref(m or snap(**k)), C.byref(r) if r else None, cap, pcap, f, d, nobs, of, od, oc, ofl, w, bytes_, None)
    assert gather(r=None) == INV and gather(batch=0) == INV and gather(n_pt=-1) == INV and gather(cap=0) == INV and gather(pcap=0) == INV
    assert gather(null="pt_start") == INV and gather(null="frame_count") == INV
    for field in ("lpt", "n_lpt", "status", "frame_point_out"):
        r = capi.LocalMapResult(*[one] * 9)
        setattr(r, field, None)
        assert gather(r=r) == INV, field
    for k in ("f", "d", "nobs", "of", "od", "oc", "ofl"):
        assert gather(**{k: None}) == INV, k
    for k in ("f", "d", "of", "od"):
        assert gather(**{k: C.c_void_p(264)}) == INV, k                # not 16-byte aligned
    assert gather(w=None) == INV and gather(bytes_=gb - 1) == INV and gather(w=C.c_void_p(4097)) == INV
    if L.viorb_device_count() < 1:
        assert dev() == ND and host() == ND and gather() == ND
        with pytest.raises(viorb_amd.ViorbError) as e:
            M.update_local_map([K.breakable_scene()])
        assert e.value.code == ND
