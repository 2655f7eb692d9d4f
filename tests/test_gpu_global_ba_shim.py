"""viorb_shim::global_bundle_adjustment_navstate (viorb_amd/shim/Optimizer_shim.h) driven from a C++ program with stand-in Map / KeyFrame /
MapPoint / NavState / IMUPreintegrator types (tests/cpp/shim_global_ba_test.cpp). The map holds one bad key frame (in the middle: its
successor loses its IMU factor) and one bad point, which the template has to skip; what it leaves in the objects equals the Python path
on independently flattened arrays, for both write-back branches (nLoopKF == 0: the key frames and points themselves; nLoopKF != 0:
mNavStateGBA / mTcwGBA / mPosGBA / mnBAGlobalForKF). The build helper is used by the CPU suite too (tests/test_global_ba_ref.py)."""
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd.synth import make_global_ba_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_global_ba_shim_test(tmp_path):
    exe = str(tmp_path / "shim_global_ba_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_global_ba_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def write_problem(path, p, iterations, robust, bad_kf, bad_pt):
    eo = p["edge_obs"]
    edges = np.column_stack([p["edge_idx"].astype(np.float64), eo])
    out = [np.array([len(p["kfs"]), len(p["points"]), len(edges), iterations, robust, bad_kf, bad_pt, 0], np.float64), p["gw"], p["cam"],
           p["kfs"].ravel(), p["preint"].ravel(), p["points"].ravel(), edges.ravel()]
    with open(path, "wb") as f:
        f.write(b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in out))


def without_bad(p, bad_kf, bad_pt):
    """the arrays the template should hand to the library: the bad key frame and the bad point gone, indices closed up"""
    N, P = len(p["kfs"]), len(p["points"])
    kmap = np.cumsum(np.arange(N) != bad_kf) - 1; pmap = np.cumsum(np.arange(P) != bad_pt) - 1
    keep_k = np.arange(N) != bad_kf; keep_p = np.arange(P) != bad_pt
    ei = p["edge_idx"]; keep_e = (ei[:, 1] != bad_kf) & (ei[:, 0] != bad_pt)
    prev = p["prev"].copy(); prev[bad_kf + 1] = -1                      # the successor of the bad key frame has no usable predecessor
    prev = np.where(prev > bad_kf, prev - 1, prev)[keep_k]
    pre = p["preint"][keep_k].copy(); pre[prev < 0] = 0
    e2 = np.column_stack([pmap[ei[keep_e, 0]], kmap[ei[keep_e, 1]]]).astype(np.int32)
    return dict(kfs=p["kfs"][keep_k], prev=prev.astype(np.int32), fixed=p["fixed"][keep_k], preint=pre, points=p["points"][keep_p],
                edge_idx=e2, edge_obs=p["edge_obs"][keep_e], gw=p["gw"], cam=p["cam"]), keep_k, keep_p


@pytest.mark.gpu
@pytest.mark.parametrize("nloop", [0, 7])
def test_global_ba_shim_equals_the_python_path(tmp_path, nloop):
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    N, bad_kf, bad_pt, iterations, robust = 16, 9, 33, 10, 1
    p = make_global_ba_problem(302, N)
    p["edge_obs"][:, 2] = np.float32(p["edge_obs"][:, 2])               # KeyFrame::mvInvLevelSigma2 is a float table
    p["cam"][:4] = np.float32(p["cam"][:4])                             # and fx, fy, cx, cy are float members
    p["points"] = np.vstack([p["points"], [[0.25, 0.5, 3.0]]])          # and a good point nobody observes: not a vertex, not written back
    fin, fout = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    write_problem(fin, p, iterations, robust, bad_kf, bad_pt)
    exe = build_global_ba_shim_test(tmp_path)
    out = subprocess.run([exe, fin, fout, str(nloop)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK iterations"), out.stdout + out.stderr
    q, keep_k, keep_p = without_bad(p, bad_kf, bad_pt)
    ref = viorb_amd.GlobalBundleAdjustmentNavState(q["kfs"], q["prev"], q["fixed"], q["preint"], q["points"], q["edge_idx"], q["edge_obs"], q["gw"], q["cam"],
                                                   iterations=iterations, robust=robust)
    blob = np.frombuffer(open(fout, "rb").read(), np.float64)
    P = len(p["points"])
    assert len(blob) == 6 + N * 63 + P * 9
    info = blob[:6]; K = blob[6:6 + N * 63].reshape(N, 63); M = blob[6 + N * 63:].reshape(P, 9)
    assert (int(info[2]), int(info[3])) == (ref["iterations"], ref["trials"]) and abs(info[1] - ref["chi2_after"]) <= 1e-9 * ref["chi2_after"]
    ns, gba, tcw, ns_sets, pose_up, kf_mark = K[:, :22], K[:, 22:44], K[:, 44:60].reshape(N, 4, 4), K[:, 60], K[:, 61], K[:, 62]
    pw, pgba, pos_sets, normal_up, pt_mark = M[:, :3], M[:, 3:6], M[:, 6], M[:, 7], M[:, 8]
    inc = np.zeros(P, bool); inc[keep_p] = ref["point_included"].astype(bool)
    assert not inc[-1] and inc[:-1].sum() == P - 2
    tol_k, tol_p = 1e-9, 1e-6                                          # two runs of the device (atomics) / one float rounding of a point
    got_ns = ns if nloop == 0 else gba
    np.testing.assert_allclose(got_ns[keep_k], ref["kfs"], rtol=0, atol=tol_k)
    np.testing.assert_array_equal(ns[bad_kf], p["kfs"][bad_kf])        # the bad key frame is never touched
    assert ns_sets[bad_kf] == 0 and kf_mark[bad_kf] == 0
    full = np.zeros((P, 3)); full[keep_p] = ref["points"]
    if nloop == 0:
        assert (ns_sets[keep_k] == 1).all() and (pose_up[keep_k] == 1).all() and (kf_mark == 0).all() and not gba[:, :9].any()
        np.testing.assert_allclose(pw[inc], full[inc], rtol=0, atol=tol_p)
        np.testing.assert_array_equal(pw[~inc], np.float32(p["points"][~inc]).astype(np.float64))
        assert (pos_sets[inc] == 1).all() and (normal_up[inc] == 1).all() and not pos_sets[~inc].any() and not pgba.any() and not pt_mark.any()
    else:
        assert not ns_sets.any() and not pose_up.any() and (kf_mark[keep_k] == nloop).all()
        np.testing.assert_array_equal(ns, p["kfs"])                    # the key frames keep their states
        np.testing.assert_array_equal(pw, np.float32(p["points"]).astype(np.float64))
        np.testing.assert_allclose(pgba[inc], full[inc], rtol=0, atol=tol_p)
        assert (pt_mark[inc] == nloop).all() and not pt_mark[~inc].any() and not pos_sets.any()
        # mTcwGBA = (Twb Tbc)^-1 of mNavStateGBA
        from scipy.spatial.transform import Rotation
        Tbc = np.eye(4); Tbc[:3, :3] = p["cam"][4:13].reshape(3, 3); Tbc[:3, 3] = p["cam"][13:16]
        for k in np.flatnonzero(keep_k):
            Twb = np.eye(4); Twb[:3, :3] = Rotation.from_quat(gba[k, 6:10]).as_matrix(); Twb[:3, 3] = gba[k, :3]
            np.testing.assert_allclose(tcw[k], np.linalg.inv(Twb @ Tbc), rtol=0, atol=2e-5)
