"""The relocalisation templates of viorb_amd/shim (relocalization_refine of viorb_tracking_shim.h, search_by_projection_reloc of
ORBmatcher_shim.h) driven from a C++ program with stand-in Frame / KeyFrame / MapPoint / cv types (tests/cpp/shim_reloc_test.cpp): they
leave mvpMapPoints, mvbOutlier and mTcw as the checker's statement-by-statement cascade (tests/reloc_ref.py) leaves them, and the matcher
alone writes mvpMapPoints as the checker's loop does. A map point that repeats in GetMapPointMatches() throws, and so does a missing
device (the program exits with 3): nothing falls back to the CPU."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
import reloc_ref as T
import reloc_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "shim_reloc_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_reloc_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def run(exe, tmp_path, s, sf, found, taken, repeat=0):
    h = s["hyp"]
    n, npts = len(s["kps"]), len(h["pts_f"])
    sf16 = np.zeros(16, np.float32); sf16[:len(sf)] = sf
    c = lambda x, dt: np.ascontiguousarray(x, dt).tobytes()
    ur = s["uright"] if s["uright"] is not None else np.full(n, -1, np.float32)
    blob = c([n, npts, len(sf), repeat], np.int32) + c(np.concatenate([K.INTR, [K.BF]]), np.float32) + c(K.BOUNDS, np.float32) + c(sf16, np.float32) + \
        c(s["kps"], s["kps"].dtype) + c(s["desc"], np.uint8) + c(ur, np.float32) + c(h["pose12"], np.float32) + c(h["kf_angle"], np.float32) + \
        c(h["kf_valid"], np.uint8) + c(np.zeros(npts), np.uint8) + c(h["pts_f"], np.float32) + c(h["pts_desc"], np.uint8) + c(h["bow_match"], np.int32) + \
        c(h["inlier"], np.uint8) + c(found, np.uint8) + c(taken, np.uint8)
    prob, out = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    open(prob, "wb").write(blob)
    r = subprocess.run([exe, prob, out], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r, (np.fromfile(out, np.int32) if r.returncode == 0 else None)


def _scene(stereo, k):
    F = K.cascade_fixture(stereo)
    s = F["scenes"][k]
    rng = np.random.default_rng(5)
    npts, n = len(s["hyp"]["pts_f"]), len(s["kps"])
    return F, s, (rng.uniform(size=npts) < 0.1).astype(np.uint8), (rng.uniform(size=n) < 0.1).astype(np.uint8)


def test_shim_compiles_and_a_failure_throws(tmp_path):
    exe = build(tmp_path)
    F, s, found, taken = _scene(False, 0)
    r, _ = run(exe, tmp_path, s, F["sf"], found, taken, repeat=1)          # the precondition: a key frame holds a map point at most once
    assert r.returncode == 3 and "repeats in GetMapPointMatches" in r.stdout
    if viorb_amd.lib().viorb_device_count() < 1:                           # no CPU fallback: the failure is an exception, not "0 inliers"
        r, _ = run(exe, tmp_path, s, F["sf"], found, taken)
        assert r.returncode == 3 and "exception: Relocalization" in r.stdout and "no HIP device" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("stereo,exit_code", [(False, T.ACCEPTED_THIRD), (True, T.NARROW_SHORT), (False, T.FEW_INLIERS)], ids=["accepted_third", "stereo_narrow_short", "few_inliers"])
def test_shim_write_back_equals_the_checker(oracle, tmp_path, stereo, exit_code):
    exe = build(tmp_path)
    k = K.CASCADE_EXITS.index(exit_code)
    F, s, found, taken = _scene(stereo, k)
    r, o = run(exe, tmp_path, s, F["sf"], found, taken)
    assert r.returncode == 0
    want = K.cascade_expected(oracle.pose_opt_se3, stereo)[k]
    n = len(s["kps"])
    assert want["stage"] == exit_code and o[0] == want["n_good"] and o[1] == want["stage"]
    assert np.array_equal(o[2:2 + n], want["frame_match"]) and np.array_equal(o[2 + n:2 + 2 * n], want["outlier"])
    pose = o[2 + 2 * n:14 + 2 * n].view(np.float32)
    np.testing.assert_allclose(pose, want["pose12"], rtol=0, atol=2e-6)
    # the matcher alone at the hypothesis' pose
    h = dict(s["hyp"], kf_found=found, feat_taken=taken)
    m = K.ref_search(T.Frame(s["cam"], s["kps"], s["desc"]), h)
    rest = o[14 + 2 * n:]
    assert rest[0] == m["nmatches"] > 0
    mvp = np.where(taken != 0, -2, -1)
    hit = np.nonzero(m["best_idx"] >= 0)[0]
    mvp[m["best_idx"][hit]] = hit
    assert np.array_equal(rest[1:], mvp)
