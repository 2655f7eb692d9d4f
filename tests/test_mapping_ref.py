"""CPU checks of map-point creation: the library's per-pair and per-point functions compiled for the host
(viorb_debug_triangulate_pair, viorb_debug_map_point_update) against the numpy restatement tests/mapping_ref.py, and that
restatement's float32 form against its float64 definitional form (which fixes the position tolerance and the decision bands the GPU
tests use)."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi
from viorb_amd.capi import ptr
from viorb_amd.mapping import _csr, _kf_pool
from viorb_amd.synth import make_mapping_problem
import mapping_ref as mr

_f32 = lambda a: np.ascontiguousarray(a, np.float32)


def hook_pairs(cam, kf1, kf2, m12):
    """viorb_debug_triangulate_pair over every pair of match12: (reason [n1], Pw [n1,3])."""
    L = viorb_amd.lib()
    c = viorb_amd.mapping_camera(cam)
    n1 = len(kf1["kps"])
    rea, Pw = np.full(n1, 255, np.uint8), np.zeros((n1, 3), np.float32)
    T1, O1, T2, O2 = _f32(kf1["pose12"]), _f32(kf1["Ow"]), _f32(kf2["pose12"]), _f32(kf2["Ow"])
    key = lambda kf, i: _f32([kf["kps"]["x"][i], kf["kps"]["y"][i], kf["ur"][i], kf["depth"][i], kf["xy_dist"][i, 0], kf["xy_dist"][i, 1]])
    for i1 in np.nonzero(np.asarray(m12) >= 0)[0]:
        i2 = int(m12[i1])
        a, b, P = key(kf1, i1), key(kf2, i2), np.zeros(3, np.float32)
        rea[i1] = L.viorb_debug_triangulate_pair(C.byref(c), ptr(T1), ptr(O1), ptr(T2), ptr(O2), ptr(a), int(kf1["kps"]["octave"][i1]), ptr(b),
                                                 int(kf2["kps"]["octave"][i2]), ptr(P))
        Pw[i1] = P
    return rea, Pw


def test_entry_points_are_exported_and_refuse_without_a_device():
    L = viorb_amd.lib()
    names = ["viorb_triangulate_pairs_device", "viorb_triangulate_pairs", "viorb_map_points_update_device", "viorb_map_points_update",
             "viorb_create_new_map_points_device", "viorb_create_new_map_points", "viorb_create_new_map_points_workspace_bytes",
             "viorb_debug_triangulate_pair", "viorb_debug_map_point_update"]
    for n in names:
        assert hasattr(L, n), n
    assert L.viorb_abi_version() == 2
    assert L.viorb_create_new_map_points_workspace_bytes(1000, 4) >= 4 * 1000 * (28 + 32 + 1 + 4 + 4 + 4 + 1 + 1 + 12)
    if L.viorb_device_count() > 0:
        return
    p = make_mapping_problem(3, J=2, n1=40, n2=40)
    cam, kf1, kf2 = p["cam"], p["kf1"], p["neigh"][1]
    codes = []
    try:
        viorb_amd.TriangulatePairs(cam, kf1, kf2, kf2["match_gen"])
    except viorb_amd.ViorbError as e:
        codes.append(e.code)
    try:
        viorb_amd.MapPointUpdate(cam, [[(0, 1), (1, 2)]], [0], np.ones((1, 3)), [kf1["desc"], kf2["desc"]], [kf1["kps"]["octave"], kf2["kps"]["octave"]],
                                 [kf1["Ow"], kf2["Ow"]])
    except viorb_amd.ViorbError as e:
        codes.append(e.code)
    try:
        viorb_amd.CreateNewMapPointsHost(cam, p, 64)
    except viorb_amd.ViorbError as e:
        codes.append(e.code)
    # the device forms check for a device before they touch a pointer: host arrays stand in for device memory here
    c = viorb_amd.mapping_camera(cam)
    z = np.zeros(4096, np.uint8); v = ptr(z)
    codes.append(L.viorb_triangulate_pairs_device(C.byref(c), *([v] * 14), 8, 1, v, v, v, None))
    codes.append(L.viorb_map_points_update_device(v, v, v, v, v, 1, v, v, 1, v, v, 1, C.byref(c), v, v, v, None))
    ws = np.zeros(L.viorb_create_new_map_points_workspace_bytes(8, 1) + 256, np.uint8)
    wp = (ws.ctypes.data + 255) & ~255
    codes.append(L.viorb_create_new_map_points_device(C.byref(c), 1, *([v] * 24), 2, 0, 2, 8, 1, 4, v, v, v, v, v, C.c_void_p(wp), len(ws) - 256, None))
    assert codes == [capi.ERR_NO_DEVICE] * 6, codes
    assert b"no HIP device" in L.viorb_last_error()


def _point_case(rng, N, dup):
    """One point with N observations over N key frames of 12 features each; `dup` copies descriptors so that rows tie."""
    nk = N
    kf_desc = [rng.integers(0, 256, (12, 32), dtype=np.uint8) for _ in range(nk)]
    kf_oct = [rng.integers(0, 8, 12).astype(np.int32) for _ in range(nk)]
    kf_Ow = [rng.normal(0, 1, 3).astype(np.float32) for _ in range(nk)]
    feats = rng.integers(0, 12, N)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    for k in range(nk):                                   # observations of one point look alike: a base descriptor with a few flipped bits
        d = base.copy()
        for bit in rng.integers(0, 256, rng.integers(0, 40)):
            d[bit >> 3] ^= np.uint8(1 << (bit & 7))
        kf_desc[k][feats[k]] = d
    if dup and N >= 3:
        for k in range(1, N, 2):                          # every second observation repeats the first one's descriptor: tied medians
            kf_desc[k][feats[k]] = kf_desc[0][feats[0]]
    obs = [(k, int(feats[k])) for k in range(nk)]
    return obs, int(rng.integers(0, N)), rng.normal(0, 4, 3).astype(np.float32) + np.float32([0, 0, 8]), kf_desc, kf_oct, kf_Ow


@pytest.mark.parametrize("N", [1, 2, 3, 7, 64, 65, 300])
@pytest.mark.parametrize("dup", [False, True])
def test_map_point_update_hook_equals_the_restatement(N, dup):
    rng = np.random.Generator(np.random.PCG64(1000 + N + int(dup)))
    L = viorb_amd.lib()
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    cam = dict(intr4=[458.0, 457.0, 367.0, 248.0], mb=0.11, mbf=50.0, scale_factor=1.2, sf=sf, level_sigma2=sf * sf)
    c = viorb_amd.mapping_camera(cam)
    ties = 0
    for rep in range(3):
        obs, ro, Pw, kf_desc, kf_oct, kf_Ow = _point_case(rng, N, dup)
        want_d, want_best, want_f = mr.map_point_update([o[0] for o in obs], [o[1] for o in obs], ro, Pw, kf_desc, kf_oct, kf_Ow, sf)
        # two points in the arrays, the second is the one under test (obs_start offsets are exercised)
        start, okf, ofe = _csr([[(0, 0)], obs])
        base, drows, orows = _kf_pool(kf_desc, kf_oct)
        P2 = _f32(np.stack([Pw, Pw])); Ow = _f32(np.stack(kf_Ow)); ref = np.array([0, ro], np.int32)
        d, bo, pf = np.zeros(32, np.uint8), C.c_int32(-7), np.zeros(8, np.float32)
        rc = L.viorb_debug_map_point_update(ptr(start), ptr(okf), ptr(ofe), ptr(ref), ptr(P2), 1, ptr(base), ptr(Ow), len(base), ptr(drows), ptr(orows),
                                            len(orows), C.byref(c), ptr(d), C.byref(bo), ptr(pf))
        assert rc == 0
        assert bo.value == want_best and (d == want_d).all()
        assert pf.tobytes() == want_f.tobytes(), (pf, want_f)
        H = mr.hamming_matrix(np.stack([kf_desc[k][i] for k, i in obs]))
        med = np.sort(H, 1)[:, int(0.5 * (N - 1))]
        ties += int((med == med.min()).sum() > 1)
        assert want_best == int(np.argmax(med == med.min()))          # the first row with the smallest median
    if dup and N >= 3:
        assert ties == 3, "the duplicate descriptors must make several rows share the smallest median"


@pytest.mark.parametrize("params", mr.PARAM_SETS)
def test_triangulate_pair_hook_equals_the_restatement(params):
    seed, J, n, sfrac = params
    p = make_mapping_problem(seed, J=J, n1=n, n2=n, stereo_frac=sfrac)
    counts = np.zeros(256, np.int64)
    npairs = nband = 0
    worst_pos = 0.0
    branches = np.zeros(4, np.int64)
    for kf2 in p["neigh"]:
        m = kf2["match_gen"]
        r32 = mr.triangulate_pairs(p["cam"], p["kf1"], kf2, m, "f32")
        r64 = mr.triangulate_pairs(p["cam"], p["kf1"], kf2, m, "f64")
        counts += np.bincount(r32["reason"], minlength=256)
        branches += np.bincount(r32["branch"][r32["idx1"]], minlength=4)
        rea, Pw = hook_pairs(p["cam"], p["kf1"], kf2, m)
        band = mr.in_band(r32)
        i1 = r32["idx1"]
        npairs += len(i1); nband += int(band[i1].sum())
        keep = ~band
        np.testing.assert_array_equal(rea[keep], r32["reason"][keep])
        ok = (rea == mr.ACCEPT) & (r64["accept"] == 1) & keep
        if ok.any():
            dev = np.linalg.norm(Pw[ok] - r64["Pw"][ok], axis=1) / np.linalg.norm(r64["Pw"][ok], axis=1)
            worst_pos = max(worst_pos, float(dev.max()))
    print("params", params, "reasons 0..6", counts[:7], "branches", branches, "pairs", npairs, "in band", nband, "worst position deviation", worst_pos)
    assert (counts[:7] >= 10).all(), "every reason code must occur at least 10 times in the reference: %s" % counts[:7]
    if sfrac > 0:          # with every near key point stereo, key frame 1's `if` shadows key frame 2's `else if` (:1341): only a mixed set takes branch 3
        need = branches[1:] if sfrac < 1 else branches[1:3]
        assert (need >= 10).all(), "linear triangulation and the UnprojectStereo branches must be taken: %s" % branches
    assert nband <= mr.MAX_BAND_SHARE * npairs
    assert worst_pos <= mr.POS_TOL_GPU


def test_float32_restatement_against_float64():
    """Fixes POS_DEV_F32 and GATE_DEV_F32 of mapping_ref.py: the float32 restatement (LAPACK's float32 SVD) against the float64
    definitional form on the parameter sets every other test uses."""
    worst = {g: 0.0 for g in mr.GATES}
    pos_max, pos_all = 0.0, []
    for seed, J, n, sfrac in mr.PARAM_SETS:
        p = make_mapping_problem(seed, J=J, n1=n, n2=n, stereo_frac=sfrac)
        for kf2 in p["neigh"]:
            r32 = mr.triangulate_pairs(p["cam"], p["kf1"], kf2, kf2["match_gen"], "f32")
            r64 = mr.triangulate_pairs(p["cam"], p["kf1"], kf2, kf2["match_gen"], "f64")
            w, pos = mr.gate_deviation(r32, r64)
            for g in worst:
                worst[g] = max(worst[g], w[g])
            pos_all += list(pos)
            # outside the band the two forms decide alike
            keep = ~mr.in_band(r32)
            np.testing.assert_array_equal(r32["reason"][keep], r64["reason"][keep])
    pos_max = float(np.max(pos_all))
    print("float32 vs float64: position max %.3g median %.3g over %d pairs; gate deviations %s" % (pos_max, float(np.median(pos_all)), len(pos_all), worst))
    assert mr.POS_DEV_F32 / 10 <= pos_max <= mr.POS_DEV_F32
    for g in worst:
        assert mr.GATE_DEV_F32[g] / 10 <= worst[g] <= mr.GATE_DEV_F32[g], (g, worst[g])


def test_mapping_shim_compiles_links_and_refuses_without_a_device(tmp_path):
    """viorb_amd/shim/LocalMapping_shim.h compiles against stand-ins that carry the reference's member names and links the library;
    without a device both templates throw with the library's error text (tests/cpp/shim_mapping_test.cpp)."""
    import subprocess
    from test_gpu_mapping_shim import build_mapping_shim_test, write_problem
    exe = build_mapping_shim_test(tmp_path)
    if viorb_amd.lib().viorb_device_count() > 0:
        return
    p = make_mapping_problem(31, J=3, n1=60, n2=50)
    fin = str(tmp_path / "problem.bin")
    write_problem(fin, p, True)
    out = subprocess.run([exe, fin, str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK no device"), out.stdout + out.stderr
