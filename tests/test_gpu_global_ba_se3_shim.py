"""viorb_shim::global_bundle_adjustment (viorb_amd/shim/Optimizer_shim.h) driven from a C++ program with stand-in Map / KeyFrame /
MapPoint types (tests/cpp/shim_global_ba_se3_test.cpp). The map holds one bad key frame, one bad point, one point nobody observes and
mixed monocular / stereo observations; what the template leaves in the objects equals the Python path on independently flattened
arrays, for both write-back branches (nLoopKF == 0: SetPose / SetWorldPos; nLoopKF != 0: mTcwGBA / mPosGBA / mnBAGlobalForKF). The
build helper is used by the CPU suite too (tests/test_global_ba_se3_ref.py)."""
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd.synth import make_global_ba_se3_problem
from global_ba_ref import mat2q, qmat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_global_ba_se3_shim_test(tmp_path):
    exe = str(tmp_path / "shim_global_ba_se3_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_global_ba_se3_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def float_poses(kfs):
    """KeyFrame::Tcw as the map holds it: [N,12] = R row-major, t, every entry a float"""
    return np.float32(np.concatenate([qmat(kfs[:, :4]).reshape(-1, 9), kfs[:, 4:7]], 1)).astype(np.float64)


def to_qt(pose12):
    """Converter::toSE3Quat of a float pose, flattened here without the C++ program: Eigen's matrix -> quaternion, w >= 0, unit norm"""
    out = np.zeros((len(pose12), 7))
    for k, p in enumerate(pose12):
        q = mat2q(p[:9].reshape(3, 3)); q = -q if q[3] < 0 else q
        out[k, :4] = q / np.sqrt(q @ q); out[k, 4:] = p[9:]
    return out


def write_problem(path, p, poses, iterations, robust, bad_kf, bad_pt):
    edges = np.column_stack([p["edge_idx"].astype(np.float64), p["edge_obs"]])
    out = [np.array([len(poses), len(p["points"]), len(edges), iterations, robust, bad_kf, bad_pt, 0], np.float64), p["intr5"], poses.ravel(), p["points"].ravel(), edges.ravel()]
    with open(path, "wb") as f:
        f.write(b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in out))


@pytest.mark.gpu
@pytest.mark.parametrize("nloop", [0, 7])
def test_global_ba_se3_shim_equals_the_python_path(tmp_path, nloop):
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    N, bad_kf, bad_pt, iterations, robust = 16, 9, 33, 10, 1
    p = make_global_ba_se3_problem(731, N, stereo_frac=0.5)
    p["edge_obs"] = np.float32(p["edge_obs"]).astype(np.float64)        # mvKeysUn, mvuRight and mvInvLevelSigma2 are float tables
    p["intr5"] = np.float32(p["intr5"]).astype(np.float64)              # and fx, fy, cx, cy, mbf are float members
    p["points"] = np.vstack([p["points"], [[0.25, 0.5, 30.0]]])         # and a good point nobody observes: not a vertex, not written back
    assert (p["edge_obs"][:, 2] >= 0).any() and (p["edge_obs"][:, 2] < 0).any()
    poses = float_poses(p["kfs"])
    fin, fout = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    write_problem(fin, p, poses, iterations, robust, bad_kf, bad_pt)
    exe = build_global_ba_se3_shim_test(tmp_path)
    out = subprocess.run([exe, fin, fout, str(nloop)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK iterations"), out.stdout + out.stderr
    # the arrays the template should hand to the library: the bad key frame and the bad point gone, indices closed up; the program lists the
    # key frames in reverse (GetAllKeyFrames promises no order), so the rows are reversed too
    P = len(p["points"])
    keep_k = np.arange(N) != bad_kf; keep_p = np.arange(P) != bad_pt
    order = [k for k in range(N - 1, -1, -1) if k != bad_kf]
    kmap = np.full(N, -1); kmap[order] = np.arange(len(order)); pmap = np.cumsum(keep_p) - 1
    ei = p["edge_idx"]; keep_e = (ei[:, 1] != bad_kf) & (ei[:, 0] != bad_pt)
    # the template walks a point's observations in std::map order of the KeyFrame pointers = ascending key-frame number here (one vector)
    e2 = np.column_stack([pmap[ei[keep_e, 0]], kmap[ei[keep_e, 1]]]).astype(np.int32)
    fixed = np.zeros(len(order), np.uint8); fixed[kmap[0]] = 1
    ref = viorb_amd.GlobalBundleAdjustmentSE3(to_qt(poses[order]), fixed, p["points"][keep_p], e2, p["edge_obs"][keep_e], p["intr5"], iterations=iterations, robust=robust)
    blob = np.frombuffer(open(fout, "rb").read(), np.float64)
    assert len(blob) == 6 + N * 34 + P * 9
    info = blob[:6]; K = blob[6:6 + N * 34].reshape(N, 34); M = blob[6 + N * 34:].reshape(P, 9)
    assert (int(info[2]), int(info[3])) == (ref["iterations"], ref["trials"]) and abs(info[1] - ref["chi2_after"]) <= 1e-9 * ref["chi2_after"]
    tcw, gba, pose_sets, kf_mark = K[:, :16].reshape(N, 4, 4), K[:, 16:32].reshape(N, 4, 4), K[:, 32], K[:, 33]
    pw, pgba, pos_sets, normal_up, pt_mark = M[:, :3], M[:, 3:6], M[:, 6], M[:, 7], M[:, 8]
    inc = np.zeros(P, bool); inc[keep_p] = ref["point_included"].astype(bool)
    assert not inc[-1] and inc[:-1].sum() == P - 2
    want = np.zeros((N, 4, 4)); want[:, 3, 3] = 1
    want[order, :3, :3] = qmat(ref["kfs"][:, :4]); want[order, :3, 3] = ref["kfs"][:, 4:7]
    start = np.zeros((N, 4, 4)); start[:, 3, 3] = 1; start[:, :3, :3] = poses[:, :9].reshape(N, 3, 3); start[:, :3, 3] = poses[:, 9:]
    tol_k, tol_p = 2e-6, 1e-5                                          # one float rounding of a pose entry (|t| up to 5 m) / of a point coordinate (up to 50 m) on top of two runs of the device
    full = np.zeros((P, 3)); full[keep_p] = ref["points"]
    got = tcw if nloop == 0 else gba
    np.testing.assert_allclose(got[keep_k], want[keep_k], rtol=0, atol=tol_k)
    np.testing.assert_array_equal(tcw[bad_kf], start[bad_kf])          # the bad key frame is never touched
    assert pose_sets[bad_kf] == 0 and kf_mark[bad_kf] == 0 and not gba[bad_kf].any()
    if nloop == 0:
        assert (pose_sets[keep_k] == 1).all() and (kf_mark == 0).all() and not gba.any()
        np.testing.assert_allclose(pw[inc], full[inc], rtol=0, atol=tol_p)
        np.testing.assert_array_equal(pw[~inc], np.float32(p["points"][~inc]).astype(np.float64))
        assert (pos_sets[inc] == 1).all() and (normal_up[inc] == 1).all() and not pos_sets[~inc].any() and not pgba.any() and not pt_mark.any()
    else:
        assert not pose_sets.any() and (kf_mark[keep_k] == nloop).all()
        np.testing.assert_array_equal(tcw, start)                      # the key frames keep their poses
        np.testing.assert_array_equal(pw, np.float32(p["points"]).astype(np.float64))
        np.testing.assert_allclose(pgba[inc], full[inc], rtol=0, atol=tol_p)
        assert (pt_mark[inc] == nloop).all() and not pt_mark[~inc].any() and not pos_sets.any()
