"""CPU tests of KeyFrame::UpdateConnections (no GPU): the exported symbols against include/viorb_covisibility.h, the checker
tests/covis_ref.py pinned on hand-built scenes whose expected output is written out in tests/covis_cases.py (one per rule: votes, no
observers, the tie for pKFmax, the threshold at 14 and 15, the target's own map and list, AddConnection kept and rebuilt, stale entries, the
first connection, LoopConnections both ways, a repeated target, streams without targets or key frames, both overflows by one), the host
build of covis_core.h (viorb_debug_update_connections_host) against the checker on those scenes, on scenes sized around the kernels'
strides, on 300 random streams and on every kind of broken snapshot in the middle of three streams, the situations the random set must
hold, and the argument checks of every entry, which come before any GPU call."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import covisibility as M
import covis_ref as T
import covis_cases as K


def test_symbols_struct_layout_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_covisibility.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_covisibility.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_COVISIBILITY)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_COVISIBILITY[name][1]) == n, name
    for name, code, mine in (("OVERFLOW", 1, M.OVERFLOW), ("KF_ID0", 1, M.KF_ID0), ("KF_FIRST", 2, M.KF_FIRST), ("MAP_CHANGED", 1, M.MAP_CHANGED), ("ORD_REBUILT", 2, M.ORD_REBUILT)):
        assert re.search(r"#define VIORB_COVIS_%s\s+%d\b" % (name, code), text) and mine == getattr(T, name) == code
    assert M.INVALID == T.INVALID == capi.ERR_INVALID_ARG and M.OK == T.OK == 0
    fields = re.search(r"typedef struct viorb_covis_map \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.COVIS_ARRAYS
    assert tuple(n.strip() for n in re.search(r"int32_t ([\w, ]+);", fields).group(1).split(",")) == capi.COVIS_INTS
    fields = re.search(r"typedef struct viorb_covis_result \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.COVIS_RESULT_FIELDS
    assert C.sizeof(capi.CovisMap) == 8 * 4 + 18 * C.sizeof(C.c_void_p) and C.sizeof(capi.CovisResult) == 18 * C.sizeof(C.c_void_p)
    thr, wave, lds_kf, th = M.shape()
    assert wave == 64 and thr % 64 == 0 and lds_kf >= thr and th == 15


@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_checker_pins_and_host_core(name):
    _, scene, args, want = next(c for c in K.CASES if c[0] == name)
    e = K.expected(name)
    assert K.compare_want(e, want) == []
    h = M.update_connections_host_core([scene], **args)[0]
    assert T.differences(h, e) == []


def test_children_follow_from_the_parent_output():
    # there is no child output: AddChild(target) is due on t_parent wherever it is set, which is where kf_parent_out differs from kf_parent
    scenes, exp, _ = K.random_streams()
    n = 0
    for s, e in zip(scenes, exp):
        by_target, by_parent = [[] for _ in s["kf_flags"]], [[] for _ in s["kf_flags"]]
        for t, p in zip(s["targets"], e["t_parent"]):
            if p >= 0:
                by_target[p].append(int(t))
        for k, (a, b) in enumerate(zip(s["kf_parent"], e["kf_parent_out"])):
            if a != b:
                by_parent[b].append(k)
        assert [sorted(c) for c in by_target] == [sorted(c) for c in by_parent] == e["children"]
        n += sum(len(c) for c in by_target)
    assert n >= 100


def test_host_core_equals_the_checker_at_the_edges_of_the_kernels_shapes():
    thr, wave, lds_kf, th = M.shape()
    named = K.sized_scenes()
    exp = {n: T.update_connections(s, ccap=cc) for n, s, cc in named}
    for n, s, cc in named:
        assert T.differences(M.update_connections_host_core([s], ccap=cc)[0], exp[n]) == [], n
    assert {"kp_%d" % (thr + d) for d in (-1, 0, 1)} | {"kf_%d" % (lds_kf + d) for d in (0, 1)} <= set(exp)
    for row in (wave - 1, wave, wave + 1):                              # 63, 64, 65 entries before the insert; 62, 63, 64 give them after it
        for j, where in enumerate(("front", "middle", "end")):
            e, s = exp["insert_%s_%d" % (where, row)], next(s for n, s, _ in named if n == "insert_%s_%d" % (where, row))
            at = int(np.where(e["conn_kf_out"][1] == 0)[0][0])
            assert e["conn_n_out"][1] == row + 1 and e["ord_n_out"][1] == row + 1 and (at == 0, row // 4 < at < 3 * row // 4, at == row)[j]
    assert exp["row_reaches_ccap"]["status"] == T.OK and exp["row_reaches_ccap"]["conn_n_out"][1] == wave + 1
    assert (exp["row_needs_ccap_plus_1"]["status"], exp["row_needs_ccap_plus_1"]["need"]) == (T.OVERFLOW, wave + 1)
    assert all(e["status"] == T.OK for n, e in exp.items() if n != "row_needs_ccap_plus_1")


def test_host_core_equals_the_checker_on_random_streams():
    scenes, exp, events = K.random_streams()
    got = M.update_connections_host_core(scenes, ccap=K.RANDOM_CCAP, erase_targets=1)
    assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * 300
    assert all(2 <= len(s["kf_flags"]) <= 40 and 1 <= len(set(s["targets"].tolist())) <= 6 for s in scenes)
    # the situations the set must hold, counted by the checker alone
    assert all(events.get(what, 0) >= 1 for what in T.EVENTS), events
    assert set(T.EVENTS) == {"fallback", "tie", "equal-weights", "early-return", "rebuild-pulls-sub-threshold", "first-parent", "stale", "loop-nonempty", "loop-empty"}
    for i in range(0, 300, 7):                                          # and one stream per call, both values of erase_targets
        for erase in (0, 1):
            e = exp[i] if erase else T.update_connections(scenes[i], ccap=K.RANDOM_CCAP, erase_targets=0)
            assert T.differences(M.update_connections_host_core([scenes[i]], ccap=K.RANDOM_CCAP, erase_targets=erase)[0], e) == []


def test_batches_of_unequal_streams_and_optional_outputs():
    scenes = [c[1] for c in K.CASES]
    cc = max(len(s["kf_flags"]) for s in scenes)
    exp = [T.update_connections(s, ccap=cc) for s in scenes]
    assert [(c[0], T.differences(g, e)) for c, g, e in zip(K.CASES, M.update_connections_host_core(scenes, ccap=cc), exp) if T.differences(g, e)] == []
    # every optional array NULL: the required ones are the same
    P = M.pack(scenes, ccap=cc)
    o = M.S.outputs(capi.COVIS_RESULT_FIELDS, lambda f: M.out_len(P, f), M.out_dtype)
    r = capi.CovisResult(*[capi.ptr(o[f]) if f in capi.COVIS_RESULT_REQUIRED else None for f in capi.COVIS_RESULT_FIELDS])
    assert viorb_amd.lib().viorb_debug_update_connections_host(C.byref(M._map_struct(P)), C.byref(r), cc, 0) == 0
    got = M.split(P, o)
    required = [f for f in T.FIELDS if f in capi.COVIS_RESULT_REQUIRED]
    assert [T.differences(g, dict(e, need=g["need"]), required) for g, e in zip(got, exp)] == [[]] * len(scenes)
    assert all((o[f] == M.S.FILL).all() for f in capi.COVIS_RESULT_FIELDS if f not in capi.COVIS_RESULT_REQUIRED)


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams():
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "loop_connections")
    e_good, e_other = T.update_connections(good, ccap=4), T.update_connections(other, ccap=4)
    kinds = K.broken(good)
    assert len(kinds) == 18
    for what, bad in kinds:
        got = M.update_connections_host_core([other, bad, good], ccap=4)
        assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
        assert T.differences(got[0], e_other) == [] and T.differences(got[2], e_good) == [], what
    # an input row longer than ccap (key frame 0 of `good` holds two entries), in conn and in ord
    got = M.update_connections_host_core([other, good, other], ccap=1)
    assert [g["status"] for g in got] == [T.OVERFLOW, T.INVALID, T.OVERFLOW] and got[1]["untouched"]
    long_ord = dict(good, conn_start=np.zeros(5, np.int32), conn_kf=np.zeros(0, np.int32), conn_w=np.zeros(0, np.int32),
                    ord_start=np.array([0, 2, 2, 2, 2], np.int32), ord_kf=np.array([3, 2], np.int32), ord_w=np.array([16, 3], np.int32))
    assert [g["status"] for g in M.update_connections_host_core([long_ord], ccap=2)] == [T.OK]
    assert [g["status"] for g in M.update_connections_host_core([long_ord], ccap=1)] == [T.INVALID]
    # only the targets' keypoints are read: a wild point index in another key frame's range is not looked at
    wild = dict(good, kp_point=good["kp_point"].copy())
    wild["kp_point"][int(good["kp_start"][1])] = 1 << 30
    assert T.differences(M.update_connections_host_core([wild], ccap=4)[0], e_good) == []
    # descending offsets of the batch level refuse the stream and every later one
    for f in ("kf_start", "pt_start", "target_start"):
        P = M.pack([other, good, good], ccap=4)
        P[f][2] = P[f][1] - 1
        assert [g["status"] for g in M.update_connections_host_core(None, packed=P)] == [T.OK, T.INVALID, T.INVALID], f
    # more than 65535 key frames in one stream
    nk = M.MAX_KF + 1
    big = M.scene_from_lists([K.kf() for _ in range(nk)], [], [])
    assert [g["status"] for g in M.update_connections_host_core([other, big, other], ccap=4)] == [T.OK, T.INVALID, T.OK]
    assert [g["status"] for g in M.update_connections_host_core([M.scene_from_lists([K.kf() for _ in range(nk - 1)], [], [])], ccap=1)] == [T.OK]


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    INV, ND = capi.ERR_INVALID_ARG, capi.ERR_NO_DEVICE
    P = M.pack([K.breakable_scene()])
    cc = P["ccap"]
    wb = L.viorb_update_connections_workspace_bytes(P["batch"], P["n_kf"], P["n_target"], cc)
    assert wb > 0 and wb % 256 == 0
    for bad in ((0, 1, 1, 1), (65536, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, 0)):
        assert L.viorb_update_connections_workspace_bytes(*bad) == 0, bad
    thr, wave, lds_kf, th = M.shape()                                   # above the LDS limit the workspace also holds the votes
    assert L.viorb_update_connections_workspace_bytes(1, lds_kf + 1, 1, 4) >= L.viorb_update_connections_workspace_bytes(1, lds_kf, 1, 4) + 4 * (lds_kf + 1)
    ws = C.c_void_p(4096)
    one = C.c_void_p(256)

    def snap(null=None, **ints):
        m = M._map_struct(P)
        for k, v in ints.items():
            setattr(m, k, v)
        if null:
            setattr(m, null, None)
        return m

    def res(null=None):
        r = capi.CovisResult(*[one] * len(capi.COVIS_RESULT_FIELDS))
        if null:
            setattr(r, null, None)
        return r

    def dev(w=ws, bytes_=wb, ccap=cc, rnull=None, **k):
        return L.viorb_update_connections_device(C.byref(snap(**k)), C.byref(res(rnull)), ccap, 0, w, bytes_, None)

    def host(ccap=cc, rnull=None, **k):
        return L.viorb_update_connections(C.byref(snap(**k)), C.byref(res(rnull)), ccap, 0)

    def core(ccap=cc, rnull=None, **k):
        return L.viorb_debug_update_connections_host(C.byref(snap(**k)), C.byref(res(rnull)), ccap, 0)
    for fn in (dev, host, core):
        assert fn(batch=0) == INV and fn(batch=65536) == INV and fn(ccap=0) == INV
        for f in capi.COVIS_INTS[1:]:
            assert fn(**{f: -1}) == INV, f
        for f in capi.COVIS_ARRAYS:
            assert fn(null=f) == INV, f
        for f in capi.COVIS_RESULT_REQUIRED:
            assert fn(rnull=f) == INV, f
    m = snap()
    assert L.viorb_update_connections_device(None, C.byref(res()), cc, 0, ws, wb, None) == INV and L.viorb_update_connections_device(C.byref(m), None, cc, 0, ws, wb, None) == INV
    assert L.viorb_update_connections(None, C.byref(res()), cc, 0) == INV and L.viorb_update_connections(C.byref(m), None, cc, 0) == INV
    assert L.viorb_debug_update_connections_host(None, C.byref(res()), cc, 0) == INV and L.viorb_debug_update_connections_host(C.byref(m), None, cc, 0) == INV
    assert dev(w=None) == INV and dev(bytes_=wb - 1) == INV and dev(w=C.c_void_p(4097)) == INV
    assert L.viorb_update_connections_shape(None) == INV
    if L.viorb_device_count() < 1:
        assert dev() == ND and host() == ND
        for f in capi.COVIS_RESULT_FIELDS:
            if f not in capi.COVIS_RESULT_REQUIRED:
                assert dev(rnull=f) == ND, f                            # optional: accepted
        with pytest.raises(viorb_amd.ViorbError) as e:
            M.update_connections([K.breakable_scene()])
        assert e.value.code == ND
