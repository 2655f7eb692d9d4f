"""CPU tests of key-frame and map-point culling (no GPU): the exported symbols against include/viorb_culling.h, the checker
tests/kf_culling_ref.py pinned on hand-built scenes whose expected output is written out in tests/kf_culling_cases.py (the three
cascades in both orders, the 0.9 threshold, octaves, stereo weights, nObs at 3 and 4, the candidate's own observation, the 0.2 s test at
equality, mnId 0, mbNotErase, depths, a point at two keypoints, a table entry without the candidate's observation), the host build of
culling_core.h (viorb_debug_key_frame_culling_host) against the checker on those scenes and on random streams, the found-ratio identity,
and the argument checks of every entry, which come before any GPU call."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import culling as M
import kf_culling_ref as T
import kf_culling_cases as K


def test_symbols_struct_layout_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_culling.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_culling.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_CULLING)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_CULLING[name][1]) == n, name
    for code, name in enumerate(T.REASON_NAMES):
        assert re.search(r"#define VIORB_KFC_%s\s+%d\b" % (name, code), text), name
        assert getattr(M, name) == getattr(T, name) == code
    for code, name in enumerate(T.MPC_NAMES):
        assert re.search(r"#define VIORB_MPC_%s\s+%d\b" % (name, code), text), name
        assert getattr(M, "MPC_" + name) == getattr(T, "MPC_" + name) == code
    fields = re.search(r"typedef struct viorb_cull_map \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.CULL_MAP_ARRAYS
    assert tuple(n.strip() for n in re.search(r"int32_t ([\w, ]+);", fields).group(1).split(",")) == capi.CULL_MAP_INTS
    fields = re.search(r"typedef struct viorb_cull_result \{(.*?)\}", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.CULL_RESULT_FIELDS
    assert C.sizeof(capi.CullMap) == 6 * 4 + 19 * C.sizeof(C.c_void_p) and C.sizeof(capi.CullResult) == 15 * C.sizeof(C.c_void_p)
    thr, chunk, wave, shared = M.shape()
    assert wave == 64 and thr % 64 == 0 and chunk % 64 == 0 and shared >= 0


@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_checker_pins_and_host_core(name):
    _, scene, mono, want = next(c for c in K.CASES if c[0] == name)
    e = K.expected(name)
    for f, v in want.items():
        assert np.asarray(e[f]).tolist() == list(v), (f, np.asarray(e[f]).tolist(), v)
    assert (e["cand_mps"][e["cand_reason"] < T.KEPT] == 0).all() and e["n_culled"] == (e["cand_reason"] == T.CULLED).sum() == e["kf_bad"].sum()
    h = M.key_frame_culling_host_core([scene], mono)[0]
    assert K.differences(h, e) == [] and (h["cand_recounted"] == (e["cand_reason"] >= T.KEPT)).all()


def test_cascades_show_in_the_checker_only_through_the_ordered_state():
    # each cascade: judged on the snapshot state alone the second candidate would end differently
    for name, j in (("fewer_observers_ab", 1), ("shrinking_mps_ab", 1), ("link_changes_12", 1), ("table_entry_without_observation", 1)):
        _, scene, mono, _ = next(c for c in K.CASES if c[0] == name)
        assert T.key_frame_culling(scene, mono, frozen=True)["cand_reason"][j] != K.expected(name)["cand_reason"][j], name
    _, scene, mono, _ = next(c for c in K.CASES if c[0] == "not_erase_defers")
    assert T.key_frame_culling(scene, mono, frozen=True)["cand_reason"].tolist() == K.expected("not_erase_defers")["cand_reason"].tolist()


def test_host_core_equals_the_checker_on_random_streams_in_one_batch():
    for mono in (True, False):
        scenes, exp = K.random_batch(7, 40, mono)
        scenes = list(scenes) + [K.CASES[0][1]]
        got = M.key_frame_culling_host_core(scenes, mono)
        assert [K.differences(g, e) for g, e in zip(got, exp)] == [[]] * 40
        assert sum(e["n_culled"] for e in exp) >= 10
        rec = np.concatenate([g["cand_recounted"] for g in got[:40]])
        assert rec.any() and not rec.all() and (rec == (np.concatenate([e["cand_reason"] for e in exp]) >= T.KEPT)).all()


def test_host_core_refuses_a_broken_snapshot_alone_between_two_good_streams():
    good, (name, other) = K.breakable_scene(), next((c[0], c[1]) for c in K.CASES if c[0] == "shrinking_mps_ab")
    e_good, e_other = T.key_frame_culling(good, True), K.expected(name)
    kinds = K.broken(good)
    assert len(kinds) == 16
    for what, bad in kinds:
        scenes = [other, bad, good]
        P = M.pack(scenes)
        flat = M._run_host(viorb_amd.lib().viorb_debug_key_frame_culling_host, P, True)
        got = M.split(P, flat)
        assert got[1] == dict(status=capi.ERR_INVALID_ARG, n_culled=0), what
        assert K.untouched(scenes, 1, flat), what
        assert K.differences(got[0], e_other) == [] and K.differences(got[2], e_good) == [], what
    # the helper tells a written range from an untouched one
    assert not K.untouched(scenes, 0, flat) and not K.untouched(scenes, 2, flat)


def test_map_point_codes_and_the_found_ratio_identity():
    rng = np.random.default_rng(2)
    f = np.concatenate([[0, 0, 1, 1, 1, 5, 4194303, 4194303, 4194304, 4194303, 16777215 // 4], rng.integers(0, 2 ** 22, 3000), rng.integers(0, 40, 3000)])
    d = np.concatenate([[0, 1, 0, -1, 1, 0, 0, 1, -1, -1, 1], rng.integers(-2, 3, 6000)])
    v = np.clip(4 * f + d, 0, 2 ** 24 - 1)
    v[:3] = [0, 1, 0]
    n = len(f)
    bad, first, nobs = (rng.random(n) < 0.1), rng.integers(0, 5, n), rng.integers(0, 6, n)
    for mono in (True, False):
        want = T.map_point_culling(bad, f, v, first, nobs, 4, mono)
        got = np.array([M.map_point_code(bad[i], f[i], v[i], first[i], nobs[i], 4, mono) for i in range(n)])
        assert np.array_equal(got, want)
        assert set(want.tolist()) == set(range(5))
    near = v > 2 ** 23
    assert near.sum() >= 3 and ((4 * f < v) == (f.astype(np.float32) / np.maximum(v, 1).astype(np.float32) < np.float32(0.25)))[v > 0].all()
    # the branch order and both thresholds
    code = lambda **k: M.map_point_code(k.get("bad", 0), k.get("found", 1), k.get("visible", 1), k.get("first", 0), k.get("nobs", 9), k.get("cur", 0), k.get("mono", 1))
    assert code(bad=1, found=0, visible=9) == T.MPC_DROP_BAD and code(found=1, visible=5) == T.MPC_CULL_FOUND_RATIO and code(found=1, visible=4) == T.MPC_KEEP
    assert code(found=1, visible=3) == T.MPC_KEEP and code(found=0, visible=0) == T.MPC_KEEP
    assert [code(cur=a, nobs=2) for a in (1, 2, 3)] == [T.MPC_KEEP, T.MPC_CULL_FEW_OBS, T.MPC_CULL_FEW_OBS]
    assert [code(cur=a, nobs=3) for a in (1, 2, 3)] == [T.MPC_KEEP, T.MPC_KEEP, T.MPC_RETIRE]
    assert [code(cur=a, nobs=3, mono=0) for a in (1, 2, 3)] == [T.MPC_KEEP, T.MPC_CULL_FEW_OBS, T.MPC_CULL_FEW_OBS]
    assert [code(cur=a, nobs=4, mono=0) for a in (1, 2, 3)] == [T.MPC_KEEP, T.MPC_KEEP, T.MPC_RETIRE]


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    INV, ND = capi.ERR_INVALID_ARG, capi.ERR_NO_DEVICE
    P = M.pack([K.CASES[0][1]])
    wb = L.viorb_key_frame_culling_workspace_bytes(P["batch"], P["n_kf"], P["n_cand"], P["n_pt"], P["n_obs"])
    assert wb > 0 and wb % 256 == 0
    assert L.viorb_key_frame_culling_workspace_bytes(0, 1, 1, 1, 1) == 0 and L.viorb_key_frame_culling_workspace_bytes(65536, 1, 1, 1, 1) == 0
    assert L.viorb_key_frame_culling_workspace_bytes(1, -1, 1, 1, 1) == 0 and L.viorb_key_frame_culling_workspace_bytes(1, 1, 1, 1, -1) == 0
    ws = C.c_void_p(4096)

    def dev(mono=1, w=ws, bytes_=wb, null=None, **ints):
        m = M._map_struct(P)
        for k, v in ints.items():
            setattr(m, k, v)
        if null:
            setattr(m, null, None)
        return L.viorb_key_frame_culling_device(C.byref(m), mono, None, w, bytes_, None)

    def host(mono=1, null=None, **ints):
        m = M._map_struct(P)
        for k, v in ints.items():
            setattr(m, k, v)
        if null:
            setattr(m, null, None)
        return L.viorb_key_frame_culling(C.byref(m), mono, None)
    for fn in (dev, host):
        assert fn(batch=0) == INV and fn(batch=65536) == INV and fn(n_kf=-1) == INV and fn(n_kp=-1) == INV and fn(n_obs=-1) == INV
        for f in capi.CULL_MAP_ARRAYS:
            if f != "kp_depth":
                assert fn(null=f) == INV, f
        assert fn(mono=0, null="kp_depth") == INV
    assert L.viorb_key_frame_culling_device(None, 1, None, ws, wb, None) == INV and L.viorb_key_frame_culling(None, 1, None) == INV
    assert dev(w=None) == INV and dev(bytes_=wb - 1) == INV and dev(w=C.c_void_p(4097)) == INV
    assert L.viorb_key_frame_culling_shape(None) == INV
    one = C.c_void_p(256)

    def mp(bad=one, nobs=one, count=one, cur=one, cap=8, batch=2, code=one):
        return L.viorb_map_point_culling_device(bad, one, one, one, nobs, count, cur, cap, batch, 1, code, None)
    assert mp(bad=None) == INV and mp(nobs=None) == INV and mp(count=None) == INV and mp(cur=None) == INV and mp(code=None) == INV
    assert mp(cap=0) == INV and mp(batch=0) == INV and mp(batch=65536) == INV
    assert L.viorb_map_point_culling(None, None, None, None, None, -1, 0, 1, None) == INV and L.viorb_map_point_culling(None, one, one, one, one, 3, 0, 1, one) == INV
    if L.viorb_device_count() < 1:
        assert dev() == ND and dev(mono=1, null="kp_depth") == ND and host() == ND and mp() == ND
        with pytest.raises(viorb_amd.ViorbError) as e:
            M.map_point_culling([0], [1], [1], [0], [3], 2, True)
        assert e.value.code == ND
