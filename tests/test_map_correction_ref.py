"""CPU tests of the map correction of loop closing (no GPU): the exported symbols against include/viorb_map_correction.h, the checker
tests/map_correction_ref.py pinned on hand-built scenes whose expected output is written out in tests/map_correction_cases.py (one per
rule: the lower key wins, a point twice in a member, already corrected, bad, null, no observations, three centres in one normal, the
reference key frame on both sides, a scale of 2, the four branches of Quaterniond(Matrix3d), an empty list, no points), the host build of
map_correct_core.h (viorb_debug_correct_loop_host) against the checker, bit for bit, on those scenes, on scenes sized around the kernels'
strides, on 300 random streams and on every kind of broken snapshot in the middle of three streams, the situations the random set must
hold, and the argument checks of every entry, which come before any GPU call."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import map_correction as M
import map_correction_ref as T
import map_correction_cases as K


def test_symbols_struct_layout_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    main = open(os.path.join(inc, "viorb.h")).read()
    assert main.index('#include "viorb_essential_graph.h"') < main.index('#include "viorb_map_correction.h"')
    text = open(os.path.join(inc, "viorb_map_correction.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_MAP_CORRECTION)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_MAP_CORRECTION[name][1]) == n, name
    assert M.INVALID == T.INVALID == capi.ERR_INVALID_ARG and M.OK == T.OK == 0
    fields = re.search(r"typedef struct viorb_correct_loop_map \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.CORRECT_LOOP_ARRAYS
    assert tuple(n.strip() for n in re.search(r"int32_t ([\w, ]+);", fields).group(1).split(",")) == capi.CORRECT_LOOP_INTS
    fields = re.search(r"typedef struct viorb_correct_loop_result \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.CORRECT_LOOP_RESULT_FIELDS == ("status",) + T.FIELDS
    assert C.sizeof(capi.CorrectLoopMap) == 6 * 4 + 17 * C.sizeof(C.c_void_p) and C.sizeof(capi.CorrectLoopResult) == 12 * C.sizeof(C.c_void_p)
    thr_kf, thr_pt, wave, lds_kf = M.shape()
    assert wave == 64 and thr_kf % 64 == 0 and thr_pt % 64 == 0 and lds_kf >= thr_pt
    fields = re.search(r"typedef struct viorb_apply_gba_map \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.APPLY_GBA_ARRAYS
    assert tuple(n.strip() for n in re.search(r"int32_t ([\w, ]+);", fields).group(1).split(",")) == capi.APPLY_GBA_INTS
    fields = re.search(r"typedef struct viorb_apply_gba_result \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.APPLY_GBA_RESULT_FIELDS == ("status",) + T.AG_FIELDS
    assert C.sizeof(capi.ApplyGbaMap) == 5 * 4 + 4 + 16 * C.sizeof(C.c_void_p) and C.sizeof(capi.ApplyGbaResult) == 11 * C.sizeof(C.c_void_p)
    for name, code in (("BAD", 0), ("POS_GBA", 1), ("BY_REF", 2), ("UNTOUCHED", 3), ("REF_UNREACHED", 4)):
        assert re.search(r"#define VIORB_AGBA_PT_%s\s+%d\b" % (name, code), text) and getattr(M, "AG_" + name) == getattr(T, "AG_" + name) == code
    g_kf, g_pt, g_wave, groups = M.gba_shape()
    assert g_wave == 64 and g_kf % 64 == 0 and g_pt % 64 == 0 and groups >= 1


@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_checker_pins_and_host_core(name):
    _, scene, want = next(c for c in K.CASES if c[0] == name)
    e = K.expected(name)
    assert K.compare_want(e, want) == []
    assert T.differences(M.correct_loop_host_core([scene])[0], e) == []


def test_the_order_of_the_observations_in_the_snapshot_does_not_matter():
    # mObservations is a std::map: the normal's float sum runs in key order however the snapshot lists a point's observers
    scenes, exp, _ = K.random_streams()
    rng = np.random.default_rng(5)
    moved = 0
    for s, e in list(zip(scenes, exp))[:60]:
        obs = s["obs"].copy()
        for p in range(len(s["pt_bad"])):
            a, b = int(s["obs_start"][p]), int(s["obs_start"][p + 1])
            obs[a:b] = rng.permutation(obs[a:b])
        moved += int((obs != s["obs"]).any())
        assert T.differences(M.correct_loop_host_core([dict(s, obs=obs)])[0], e) == []
    assert moved >= 30


def test_host_core_equals_the_checker_at_the_edges_of_the_kernels_shapes():
    thr_kf, thr_pt, wave, lds_kf = M.shape()
    named = K.sized_scenes()
    exp = {n: T.correct_loop(s) for n, s in named}
    for n, s in named:
        assert T.differences(M.correct_loop_host_core([s])[0], exp[n]) == [], n
    assert {"kp_%d" % (thr_kf + d) for d in (-1, 0, 1)} | {"kf_%d" % (thr_kf + d) for d in (-1, 0, 1)} | {"pt_%d" % (wave + d) for d in (-1, 0, 1)} \
        | {"pt_%d" % (thr_pt + d) for d in (-1, 0, 1)} | {"obs_%d" % (wave + d) for d in (-1, 0, 1)} <= set(exp)
    for d in (-1, 0, 1):                                                # two corrected points with exactly that many observers
        s = next(s for n, s in named if n == "obs_%d" % (wave + d))
        assert np.diff(s["obs_start"])[:2].tolist() == [wave + d] * 2 and exp["obs_%d" % (wave + d)]["pt_touched"][:2].all()
        assert exp["kf_%d" % (thr_kf + d)]["n_member"] == thr_kf + d
    # one stream above the LDS key-frame limit, one at it and one below it
    for nk in (lds_kf + 1, lds_kf, lds_kf - 1):
        s = K.random_scene(11, nk=nk, n_pt=120, n_kp=1, max_obs=9, n_members=200)
        assert T.differences(M.correct_loop_host_core([s])[0], T.correct_loop(s)) == []


def test_host_core_equals_the_checker_on_random_streams():
    scenes, exp, events = K.random_streams()
    got = M.correct_loop_host_core(scenes)
    assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * 300
    # the situations the set must hold, counted by the checker alone
    assert all(events.get(what, 0) >= 1 for what in T.EVENTS), events
    assert set(T.EVENTS) == {"two-members", "twice-in-member", "already-corrected", "bad-point", "null-keypoint", "no-observations", "observer-below", "observer-equal",
                             "observer-above", "observer-not-member", "ref-below", "ref-not-below", "scale-not-1", "mat2q-trace", "mat2q-x", "mat2q-y", "mat2q-z",
                             "empty-list", "no-points"}
    for i in range(0, 300, 7):                                          # and one stream per call
        assert T.differences(M.correct_loop_host_core([scenes[i]])[0], exp[i]) == []
    # another scale table: the range follows the camera's factors and its last level
    cam = M.camera(nlevels=5, scale_factor=1.5)
    sf = M.scale_factors(cam)
    for i in range(0, 40):
        assert T.differences(M.correct_loop_host_core([scenes[i]], cam=cam)[0], T.correct_loop(scenes[i], sf=sf, nlevels=5)) == []


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams():
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "three_centres_and_both_reference_sides")
    e_good, e_other = T.correct_loop(good), T.correct_loop(other)
    assert e_good["pt_touched"].tolist() == [1, 1, 1, 0]
    kinds = K.broken(good)
    assert len(kinds) == 25
    for what, bad in kinds:
        got = M.correct_loop_host_core([other, bad, good])
        assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
        assert T.differences(got[0], e_other) == [] and T.differences(got[2], e_good) == [], what
    # only the members' keypoints are read: a wild point index in another key frame's range is not looked at; nor is the reference key
    # frame of a point no member holds, or of a bad one
    wild = dict(good, kp_point=good["kp_point"].copy(), pt_ref=good["pt_ref"].copy())
    wild["kp_point"][int(good["kp_start"][3])] = 1 << 30
    wild["pt_ref"][3] = 1 << 20
    assert T.differences(M.correct_loop_host_core([wild])[0], dict(e_good)) == []
    # descending offsets of the batch level refuse the stream and every later one
    for f in ("kf_start", "pt_start", "conn_start"):
        P = M.pack([other, good, good])
        P[f][2] = P[f][1] - 1
        assert [g["status"] for g in M.correct_loop_host_core(None, packed=P)] == [T.OK, T.INVALID, T.INVALID], f
    # a stream without key frames has no current key frame; more than 65535 key frames in one stream
    none = M.scene_from_lists([], [], 0, [], K.SHIFT)
    assert [g["status"] for g in M.correct_loop_host_core([other, none, other])] == [T.OK, T.INVALID, T.OK]
    big = M.scene_from_lists([K.kf() for _ in range(M.MAX_KF + 1)], [], 0, [], K.SHIFT)
    assert [g["status"] for g in M.correct_loop_host_core([other, big, other])] == [T.OK, T.INVALID, T.OK]
    assert [g["status"] for g in M.correct_loop_host_core([M.scene_from_lists([K.kf() for _ in range(M.MAX_KF)], [], 0, [], K.SHIFT)])] == [T.OK]


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    INV, ND = capi.ERR_INVALID_ARG, capi.ERR_NO_DEVICE
    P = M.pack([K.breakable_scene()])
    wb = L.viorb_correct_loop_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"], P["n_obs"])
    assert wb > 0 and wb % 256 == 0
    for bad in ((0, 1, 1, 1), (65536, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)):
        assert L.viorb_correct_loop_workspace_bytes(*bad) == 0, bad
    assert L.viorb_correct_loop_workspace_bytes(1, 10, 10, 1000) >= L.viorb_correct_loop_workspace_bytes(1, 10, 10, 10) + 12 * 990 - 256      # a term per observation, in 256-byte steps
    ws, one, cam = C.c_void_p(4096), C.c_void_p(256), M.camera()

    def snap(null=None, **ints):
        m = M._map_struct(P)
        for k, v in ints.items():
            setattr(m, k, v)
        if null:
            setattr(m, null, None)
        return m

    def res(null=None):
        r = capi.CorrectLoopResult(*[one] * len(capi.CORRECT_LOOP_RESULT_FIELDS))
        if null:
            setattr(r, null, None)
        return r

    def dev(w=ws, bytes_=wb, rnull=None, cam=cam, **k):
        return L.viorb_correct_loop_device(C.byref(snap(**k)), C.byref(cam) if cam else None, C.byref(res(rnull)), w, bytes_, None)

    def host(rnull=None, cam=cam, **k):
        return L.viorb_correct_loop(C.byref(snap(**k)), C.byref(cam) if cam else None, C.byref(res(rnull)))

    def core(rnull=None, cam=cam, **k):
        return L.viorb_debug_correct_loop_host(C.byref(snap(**k)), C.byref(cam) if cam else None, C.byref(res(rnull)))
    for fn in (dev, host, core):
        assert fn(batch=0) == INV and fn(batch=65536) == INV and fn(cam=None) == INV
        assert fn(cam=M.camera(nlevels=0)) == INV and fn(cam=M.camera(nlevels=17)) == INV
        for f in capi.CORRECT_LOOP_INTS[1:]:
            assert fn(**{f: -1}) == INV, f
        for f in capi.CORRECT_LOOP_ARRAYS:
            assert fn(null=f) == INV, f
        for f in capi.CORRECT_LOOP_RESULT_FIELDS:
            assert fn(rnull=f) == INV, f
    m = snap()
    assert L.viorb_correct_loop_device(None, C.byref(cam), C.byref(res()), ws, wb, None) == INV and L.viorb_correct_loop_device(C.byref(m), C.byref(cam), None, ws, wb, None) == INV
    assert L.viorb_correct_loop(None, C.byref(cam), C.byref(res())) == INV and L.viorb_correct_loop(C.byref(m), C.byref(cam), None) == INV
    assert L.viorb_debug_correct_loop_host(None, C.byref(cam), C.byref(res())) == INV and L.viorb_debug_correct_loop_host(C.byref(m), C.byref(cam), None) == INV
    assert dev(w=None) == INV and dev(bytes_=wb - 1) == INV and dev(w=C.c_void_p(4097)) == INV
    assert L.viorb_correct_loop_shape(None) == INV
    if L.viorb_device_count() < 1:
        assert dev() == ND and host() == ND
        with pytest.raises(viorb_amd.ViorbError) as e:
            M.correct_loop([K.breakable_scene()])
        assert e.value.code == ND


# ---- the map update after a global bundle adjustment ---------------------------------------------------------------------------------------------
def gba_diff(got, want):
    return T.differences(got, want, T.AG_FIELDS)


def test_apply_global_ba_checker_pins_and_host_core():
    # one hand-built map holds every rule: a chain of three key frames outside the adjustment, siblings, two origins, a root outside
    # the adjustment, an unreached flagged reference, a point in each pt_code
    s, want = K.gba_all_rules()
    e = T.apply_global_ba(s, K.TBC_I)
    assert K.compare_want(e, want) == []
    assert sorted(set(want["pt_code"])) == [0, 1, 2, 3, 4]
    assert gba_diff(M.apply_global_ba_host_core([s], K.TBC_I)[0], e) == []
    # the velocity turns with the body: a quarter turn about z between the NavState's rotation and the derived one
    h = 0.5 ** 0.5
    turned = dict(s, ns22=s["ns22"].copy())
    turned["ns22"][1, 6:10] = [0, 0, h, h]
    e2 = T.apply_global_ba(turned, K.TBC_I)
    assert np.allclose(e2["nsGBA_out"][1, 3:6], [2, -1, 3], atol=1e-15) and np.array_equal(e2["nsGBA_out"][1, 6:10], [0, 0, 0, 1])      # Rwb2 Rwb1^T V1, Set_Rot of the identity
    assert gba_diff(M.apply_global_ba_host_core([turned], K.TBC_I)[0], e2) == []


def test_apply_global_ba_host_core_equals_the_checker_on_random_and_sized_maps():
    scenes, exp, events = K.gba_random_streams()
    got = M.apply_global_ba_host_core(scenes, K.TBC)
    assert [gba_diff(g, e) for g, e in zip(got, exp)] == [[]] * 300
    assert all(events.get(what, 0) >= 1 for what in T.AG_EVENTS), events
    assert set(T.AG_EVENTS) == {"chain-of-three-outside", "root-outside", "siblings", "code-0", "code-1", "code-2", "code-3", "code-4", "two-origins", "set-rot-normalises",
                                "unreached-kf"}
    for i in range(0, 300, 7):
        assert gba_diff(M.apply_global_ba_host_core([scenes[i]], K.TBC)[0], exp[i]) == []
    thr_kf, thr_pt, wave, groups = M.gba_shape()
    named = K.gba_sized_scenes()
    assert {"kf_%d" % (thr_kf + d) for d in (-1, 0, 1)} | {"pt_%d" % (thr_pt + d) for d in (-1, 0, 1)} | {"pt_%d" % (2 * thr_pt + d) for d in (-1, 0, 1)} <= {n for n, _ in named}
    for n, s in named:
        assert gba_diff(M.apply_global_ba_host_core([s], K.TBC)[0], T.apply_global_ba(s, K.TBC)) == [], n
    # the order of the walk does not matter: the child lists reversed give the same map
    for s, e in list(zip(scenes, exp))[:60]:
        rev = dict(s, child_kf=np.concatenate([s["child_kf"][a:b][::-1] for a, b in zip(s["child_start"][:-1], s["child_start"][1:])] + [np.zeros(0, np.int32)]).astype(np.int32),
                   origins=s["origins"][::-1].copy())
        assert gba_diff(M.apply_global_ba_host_core([rev], K.TBC)[0], e) == []


def test_apply_global_ba_a_broken_map_is_refused_alone_between_two_good_streams():
    good, _ = K.gba_all_rules()
    other = K.gba_random_streams()[0][3]
    e_good, e_other = T.apply_global_ba(good, K.TBC_I), T.apply_global_ba(other, K.TBC_I)
    kinds = K.gba_broken(good)
    assert len(kinds) == 19
    for what, bad in kinds:
        got = M.apply_global_ba_host_core([other, bad, good], K.TBC_I)
        assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
        assert gba_diff(got[0], e_other) == [] and gba_diff(got[2], e_good) == [], what
    # what the walk never reads is not looked at: the GBA pose of a key frame outside the adjustment that is no root, the reference of a bad point
    wild = dict(good, TcwGBA12=good["TcwGBA12"].copy(), pt_ref=good["pt_ref"].copy())
    wild["TcwGBA12"][2, 4], wild["pt_ref"][0] = np.nan, 1 << 20
    g = M.apply_global_ba_host_core([wild], K.TBC_I)[0]
    assert g["status"] == T.OK and gba_diff(dict(g, TcwGBA_out=e_good["TcwGBA_out"]), e_good) == [] and np.array_equal(g["TcwGBA_out"][2], e_good["TcwGBA_out"][2])
    for f in ("kf_start", "pt_start", "origin_start"):
        P = M.gba_pack([other, good, good])
        P[f][2] = P[f][1] - 1
        assert [x["status"] for x in M.apply_global_ba_host_core(None, K.TBC_I, packed=P)] == [T.OK, T.INVALID, T.INVALID], f


def test_apply_global_ba_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    INV, ND = capi.ERR_INVALID_ARG, capi.ERR_NO_DEVICE
    P = M.gba_pack([K.gba_all_rules()[0]])
    wb = L.viorb_apply_global_ba_workspace_bytes(P["batch"], P["n_kf"])
    assert wb > 0 and wb % 256 == 0
    for bad in ((0, 1), (65536, 1), (1, -1)):
        assert L.viorb_apply_global_ba_workspace_bytes(*bad) == 0, bad
    ws, one = C.c_void_p(4096), C.c_void_p(256)
    Tbc = np.array(K.TBC, np.float32)
    nan = Tbc.copy(); nan[5] = np.nan

    def snap(null=None, **ints):
        m = M._gba_struct(P)
        for k, v in ints.items():
            setattr(m, k, v)
        if null:
            setattr(m, null, None)
        return m

    def res(null=None):
        r = capi.ApplyGbaResult(*[one] * len(capi.APPLY_GBA_RESULT_FIELDS))
        if null:
            setattr(r, null, None)
        return r

    def dev(w=ws, bytes_=wb, rnull=None, tbc=Tbc, **k):
        return L.viorb_apply_global_ba_device(C.byref(snap(**k)), capi.ptr(tbc), C.byref(res(rnull)), w, bytes_, None)

    def host(rnull=None, tbc=Tbc, **k):
        return L.viorb_apply_global_ba(C.byref(snap(**k)), capi.ptr(tbc), C.byref(res(rnull)))

    def core(rnull=None, tbc=Tbc, **k):
        return L.viorb_debug_apply_global_ba_host(C.byref(snap(**k)), capi.ptr(tbc), C.byref(res(rnull)))
    for fn in (dev, host, core):
        assert fn(batch=0) == INV and fn(batch=65536) == INV and fn(tbc=None) == INV and fn(tbc=nan) == INV
        for f in capi.APPLY_GBA_INTS[1:]:
            assert fn(**{f: -1}) == INV, f
        for f in capi.APPLY_GBA_ARRAYS:
            assert fn(null=f) == INV, f
        for f in capi.APPLY_GBA_RESULT_FIELDS:
            assert fn(rnull=f) == INV, f
    assert L.viorb_apply_global_ba_device(None, capi.ptr(Tbc), C.byref(res()), ws, wb, None) == INV and L.viorb_apply_global_ba(C.byref(snap()), capi.ptr(Tbc), None) == INV
    assert dev(w=None) == INV and dev(bytes_=wb - 1) == INV and dev(w=C.c_void_p(4097)) == INV
    assert L.viorb_apply_global_ba_shape(None) == INV
    if L.viorb_device_count() < 1:
        assert dev() == ND and host() == ND
        with pytest.raises(viorb_amd.ViorbError) as e:
            M.apply_global_ba([K.gba_all_rules()[0]], K.TBC_I)
        assert e.value.code == ND
