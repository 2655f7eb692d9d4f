"""CPU tests of key-frame removal (no GPU): the exported symbols against include/viorb_kf_removal.h, the checker tests/kf_removal_ref.py
pinned on hand-built scenes whose decisive outputs are written out in tests/kf_removal_cases.py (three children, the tie under permuted
keys, the stale list entry, the one-sided neighbour, the points, every guard, SetErase, the links), the host build of kf_removal_core.h
(viorb_debug_remove_key_frames_host) against the checker on those scenes, on scenes sized around the kernels' strides, on the seeded
random set (whose situations are counted first) and on every kind of broken snapshot in the middle of three streams, mspChildrens against
the (parent, bad) rule, mTcp against its definition, and the argument checks of every entry, which come before any GPU call."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import kf_removal as M
import kf_removal_ref as T
import kf_removal_cases as K


def test_symbols_struct_layout_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_kf_removal.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_kf_removal.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_KF_REMOVAL) and len(counts) == 5
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_KF_REMOVAL[name][1]) == n, name
    assert not set(capi.SIGNATURES_KF_REMOVAL) & set(capi.SIGNATURES)
    for name in ("KF_ID0", "KF_BAD", "KF_NOT_ERASE", "KF_TO_BE_ERASED", "KF_LOOP_EDGES", "SET_BAD_FLAG", "SET_ERASE", "REMOVED", "ALREADY_BAD", "FIRST_KF", "DEFERRED",
                 "RELEASED", "MAP_CHANGED", "ORD_REBUILT", "PARENT_CHANGED"):
        code = int(re.search(r"#define VIORB_KFR_%s\s+(\d+)\b" % name, text).group(1))
        assert getattr(M, name) == getattr(T, name) == code, name
    assert M.INVALID == T.INVALID == capi.ERR_INVALID_ARG and M.OK == T.OK == 0
    fields = re.search(r"typedef struct viorb_kfr_map \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.KFR_ARRAYS
    assert tuple(n.strip() for n in re.search(r"int32_t ([\w, ]+);", fields).group(1).split(",")) == capi.KFR_INTS
    fields = re.search(r"typedef struct viorb_kfr_result \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.KFR_RESULT_FIELDS
    assert capi.KFR_RESULT_FIELDS[:7] == capi.COVIS_RESULT_REQUIRED                             # the rows go straight back into the covisibility entry
    assert C.sizeof(capi.KfrMap) == 8 * 4 + 24 * C.sizeof(C.c_void_p) and C.sizeof(capi.KfrResult) == 24 * C.sizeof(C.c_void_p)
    thr, wave, lds_kf, waves = M.shape()
    assert wave == 64 and thr == wave * waves and lds_kf >= thr


@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_checker_pins_and_host_core(name):
    _, scene, want = next(c for c in K.CASES if c[0] == name)
    e = K.expected(name)
    assert K.compare_want(e, want) == []
    h = M.remove_key_frames_host_core([scene])[0]
    assert T.differences(h, e) == [] and h["untouched"]


def test_the_random_set_holds_every_situation_and_the_host_core_equals_the_checker():
    scenes, exp, events = K.random_streams()
    # the situations the set must hold, counted by the checker alone, before any comparison
    assert set(T.EVENTS) == {"adopted-by-adopted-child", "fallback", "tie-by-order-permuted", "rebuild-pulls-sub-threshold", "point-bad", "point-survives", "ref-moves",
                             "stereo-decrement", "deferred", "already-bad", "first-kf", "released", "set-erase-removes", "parent-assigned-earlier", "adjacent-removals"}
    assert all(events.get(what, 0) >= 1 for what in T.EVENTS), events
    assert K.SEEDS == tuple(range(100, 160)) and len(scenes) == 60
    assert all(6 <= len(s["kf_flags"]) <= 14 and 1 <= len(s["op_kf"]) <= 7 for s in scenes)
    for s in scenes:                                                    # the precondition: a key frame holds a point at most once
        for k in range(len(s["kf_flags"])):
            held = [p for p in s["kp_point"][s["kp_start"][k]:s["kp_start"][k + 1]] if p >= 0]
            assert len(held) == len(set(held))
    got = M.remove_key_frames_host_core(scenes, ccap=K.RANDOM_CCAP)
    assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * len(scenes)
    for i in range(0, len(scenes), 7):                                  # and one stream per call
        assert T.differences(M.remove_key_frames_host_core([scenes[i]], ccap=K.RANDOM_CCAP)[0], exp[i]) == []


def test_children_equal_the_parent_and_bad_derivation_after_every_scene():
    scenes, exp, _ = K.random_streams()
    n = 0
    for e in exp + [K.expected(c[0]) for c in K.CASES]:
        assert e["children"] == e["children_by_rule"]
        n += sum(len(c) for c in e["children"] if c)
        # and the same from the outputs alone
        bad = (e["kf_flags_out"] & T.KF_BAD) != 0
        rule = [sorted(int(c) for c in np.where((e["kf_parent_out"] == k) & ~bad)[0]) if not bad[k] else None for k in range(len(bad))]
        assert rule == e["children"]
    assert n >= 300


def test_host_core_equals_the_checker_at_the_edges_of_the_kernels_shapes():
    thr, wave, lds_kf, waves = M.shape()
    named = K.sized_scenes()
    names = {n for n, _, _ in named}
    assert {"neighbours_%d" % (waves + d) for d in (-1, 0, 1)} | {"row_%d" % (wave + d) for d in (-1, 0, 1)} | {"keypoints_%d" % (thr + d) for d in (-1, 0, 1)} \
        | {"children_0", "children_1", "children_%d" % (wave + 1)} | {"kf_%d" % lds_kf, "kf_%d" % (lds_kf + 1)} == names
    for n, s, cc in named:
        e = T.remove_key_frames(s, ccap=cc)
        assert T.differences(M.remove_key_frames_host_core([s], ccap=cc)[0], e) == [], n
        kind, size = n.rsplit("_", 1)
        if kind == "neighbours":
            assert e["op_rebuilt"][0] == int(size)
        if kind == "row":
            assert s["conn_start"][3] - s["conn_start"][2] == int(size) and e["conn_n_out"][2] == int(size) - 1
        if kind == "keypoints":
            assert s["kp_start"][2] - s["kp_start"][1] == int(size) and e["op_points_bad"][0] >= 10
        if kind == "children":
            assert e["op_children"][0] == int(size)
        if kind == "kf":
            assert len(s["kf_flags"]) == int(size) and cc == 8 and (e["op_reason"] == T.REMOVED).sum() >= 4


def test_batches_of_unequal_streams_and_optional_outputs():
    scenes = [c[1] for c in K.CASES]
    exp = [T.remove_key_frames(s, ccap=5) for s in scenes]
    got = M.remove_key_frames_host_core(scenes, ccap=5)
    assert [(c[0], T.differences(g, e)) for c, g, e in zip(K.CASES, got, exp) if T.differences(g, e)] == []
    # every optional array NULL: the required ones are the same
    P = M.pack(scenes, ccap=5)
    o = M.S.outputs(capi.KFR_RESULT_FIELDS, lambda f: M.out_len(P, f), M.out_dtype)
    r = capi.KfrResult(*[capi.ptr(o[f]) if f in capi.KFR_RESULT_REQUIRED else None for f in capi.KFR_RESULT_FIELDS])
    assert viorb_amd.lib().viorb_debug_remove_key_frames_host(C.byref(M._map_struct(P)), C.byref(r), 5) == 0
    required = [f for f in T.FIELDS if f in capi.KFR_RESULT_REQUIRED]
    assert [T.differences(g, e, required) for g, e in zip(M.split(P, o), exp)] == [[]] * len(scenes)
    assert all((o[f] == M.S.FILL).all() for f in capi.KFR_RESULT_FIELDS if f not in capi.KFR_RESULT_REQUIRED)


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams():
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "points")
    e_good, e_other = T.remove_key_frames(good, ccap=4), T.remove_key_frames(other, ccap=4)
    assert (e_good["op_reason"] == [T.REMOVED, T.RELEASED, T.REMOVED]).all()
    kinds = K.broken(good)
    assert len(kinds) == 28
    for what, bad in kinds:
        got = M.remove_key_frames_host_core([other, bad, good], ccap=4)
        assert got[1]["status"] == T.INVALID and got[1]["untouched"] and set(got[1]) == {"status", "untouched"}, what
        assert T.differences(got[0], e_other) == [] and T.differences(got[2], e_good) == [], what
    # what is refused only where the reference would go wrong: a first or bad key frame needs no parent, and only the operations' poses are read
    ok = dict(good, kf_parent=np.array([-1, 0, 1, 0, -1], np.int32), kf_pose12=good["kf_pose12"].copy())
    ok["kf_pose12"][2, 0] = np.nan
    assert M.remove_key_frames_host_core([ok], ccap=4)[0]["status"] == T.OK
    # an input row longer than ccap (key frame 1 of `good` holds two entries)
    got = M.remove_key_frames_host_core([other, good, other], ccap=1)
    assert [g["status"] for g in got] == [T.OK, T.INVALID, T.OK] and got[1]["untouched"]
    # descending offsets of the batch level refuse the stream and every later one
    for f in ("kf_start", "pt_start", "op_start"):
        P = M.pack([other, good, good], ccap=4)
        P[f][2] = P[f][1] - 1
        assert [g["status"] for g in M.remove_key_frames_host_core(None, packed=P)] == [T.OK, T.INVALID, T.INVALID], f


def test_mtcp_of_the_checker_against_its_definition():
    """mTcp = Tcw * Tpw^-1 in float64 against the checker's float32 restatement. The bound is derived, not measured: an entry of Twc's
    translation and an entry of the product are each a sum of three float products (the fourth term is an exact 0 or the translation
    itself), rotation entries are at most 1 in magnitude, so twice over the rounding adds up to less than
    24 * 2^-24 * (1 + |t_c|_1 + |t_p|_1) per entry."""
    scenes, exp, _ = K.random_streams()
    n = 0
    for s, e in zip(scenes, exp):
        for k, Tcp in enumerate(e["kf_Tcp"]):
            if Tcp is None:
                continue
            p = int(e["kf_parent_out"][k])                              # a removed key frame keeps the parent it was removed under
            T4 = lambda T12: np.block([[T12[:9].reshape(3, 3).astype(np.float64), T12[9:].reshape(3, 1).astype(np.float64)], [np.zeros((1, 3)), np.ones((1, 1))]])
            Tc, Tp = T4(s["kf_pose12"][k]), T4(s["kf_pose12"][p])
            want = Tc @ np.linalg.inv(Tp)
            bound = 24 * 2.0 ** -24 * (1 + np.abs(Tc[:3, 3]).sum() + np.abs(Tp[:3, 3]).sum())
            got = np.concatenate([Tcp[:9].reshape(3, 3), Tcp[9:].reshape(3, 1)], axis=1).astype(np.float64)
            assert np.abs(got - want[:3]).max() <= bound, (k, np.abs(got - want[:3]).max(), bound)
            n += 1
    assert n >= 50


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    INV, ND = capi.ERR_INVALID_ARG, capi.ERR_NO_DEVICE
    P = M.pack([K.breakable_scene()])
    cc = P["ccap"]
    wb = L.viorb_remove_key_frames_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"], P["n_op"])
    assert wb > 0 and wb % 256 == 0
    for bad in ((0, 1, 1, 1), (65536, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)):
        assert L.viorb_remove_key_frames_workspace_bytes(*bad) == 0, bad
    ws, one = C.c_void_p(4096), C.c_void_p(256)

    def snap(null=None, **ints):
        m = M._map_struct(P)
        for k, v in ints.items():
            setattr(m, k, v)
        if null:
            setattr(m, null, None)
        return m

    def res(null=None):
        r = capi.KfrResult(*[one] * len(capi.KFR_RESULT_FIELDS))
        if null:
            setattr(r, null, None)
        return r

    def dev(w=ws, bytes_=wb, ccap=cc, rnull=None, **k):
        return L.viorb_remove_key_frames_device(C.byref(snap(**k)), C.byref(res(rnull)), ccap, w, bytes_, None)

    def host(ccap=cc, rnull=None, **k):
        return L.viorb_remove_key_frames(C.byref(snap(**k)), C.byref(res(rnull)), ccap)

    def core(ccap=cc, rnull=None, **k):
        return L.viorb_debug_remove_key_frames_host(C.byref(snap(**k)), C.byref(res(rnull)), ccap)
    for fn in (dev, host, core):
        assert fn(batch=0) == INV and fn(batch=65536) == INV and fn(ccap=0) == INV
        for f in capi.KFR_INTS[1:]:
            assert fn(**{f: -1}) == INV, f
        for f in capi.KFR_ARRAYS:
            assert fn(null=f) == INV, f
        for f in capi.KFR_RESULT_REQUIRED:
            assert fn(rnull=f) == INV, f
    m = snap()
    assert L.viorb_remove_key_frames_device(None, C.byref(res()), cc, ws, wb, None) == INV and L.viorb_remove_key_frames_device(C.byref(m), None, cc, ws, wb, None) == INV
    assert L.viorb_remove_key_frames(None, C.byref(res()), cc) == INV and L.viorb_remove_key_frames(C.byref(m), None, cc) == INV
    assert L.viorb_debug_remove_key_frames_host(None, C.byref(res()), cc) == INV and L.viorb_debug_remove_key_frames_host(C.byref(m), None, cc) == INV
    assert dev(w=None) == INV and dev(bytes_=wb - 1) == INV and dev(w=C.c_void_p(4097)) == INV
    assert L.viorb_remove_key_frames_shape(None) == INV
    if L.viorb_device_count() < 1:
        assert dev() == ND and host() == ND
        for f in capi.KFR_RESULT_FIELDS:
            if f not in capi.KFR_RESULT_REQUIRED:
                assert dev(rnull=f) == ND, f                            # optional: accepted
        with pytest.raises(viorb_amd.ViorbError) as e:
            M.remove_key_frames([K.breakable_scene()])
        assert e.value.code == ND
