"""viorb_amd/shim/Optimizer_shim.h: optimize_essential_graph driven from a C++ program with stand-in Map / KeyFrame / MapPoint / LoopClosing
types (tests/cpp/shim_essential_graph_test.cpp). The map the program builds holds what the reference's edge selection has to leave out: a
bad key frame, covisibility entries under minFeat = 100, to the parent, to a child, to a loop-edge partner and to a pair already in
sInsertedEdges, LoopConnections entries under minFeat (kept only for the pair (pCurKF, pLoopKF)), loop edges seen from the older side.
What the template leaves in the map equals the direct host-form call viorb_optimize_essential_graph on the snapshot this file builds
with the same rules, bit for bit. Without a device the template throws and touches nothing."""
import os
import subprocess
import sys
import numpy as np
import pytest
import viorb_amd
from viorb_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sim3_ref import mat2q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_FEAT = 100


def build(tmp_path):
    exe = str(tmp_path / "shim_essential_graph_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_essential_graph_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_shim_compiles_and_handles_the_cases_that_need_no_device(tmp_path):
    exe = build(tmp_path)
    if viorb_amd.lib().viorb_device_count() < 1:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout, r.stderr)
        assert r.returncode == 0 and "OK threw" in r.stdout


def make_map(seed, N, fix_scale):
    """The key-frame graph of a loop closure around synth.make_essential_graph_problem's poses: (arrays for the program, the snapshot the
    template must build)."""
    p = synth.make_essential_graph_problem(seed, N=N, fix_scale=fix_scale, n_points=60, skip_frac=0.0, turn=0.3, rot_drift=0.05, scale_drift=0.05, trans_drift=0.05)
    cur, loop = N - 1, 0
    has_corr = (p["Scw"] != p["Smeas"]).any(1)
    # key-frame poses as the map holds them: float matrices of the drifted poses
    from scipy.spatial.transform import Rotation
    poses = np.zeros((N, 12))
    for k in range(N):
        poses[k, :9] = Rotation.from_quat(p["Smeas"][k, :4]).as_matrix().astype(np.float32).ravel()
        poses[k, 9:] = p["Smeas"][k, 4:7].astype(np.float32)
    parent = np.arange(-1, N - 1).astype(np.float64)
    weights = {}
    covis = []
    for k in range(N):
        for other, w in ((k - 2, 150), (k - 3, 80), (k - 1, 200), (k + 1, 200), (k - 4, 101)):
            if 0 <= other < N:
                covis.append((k, other, w)); weights[(min(k, other), max(k, other))] = w
    loop_edges = [(N - 3, N - 7)]
    covis.append((N - 3, N - 7, 120))                                   # a loop-edge partner among the covisibles
    lc = [(cur, loop), (cur, 1), (cur, 2), (cur - 1, loop), (cur - 1, 1)]
    for (a, b), w in (((cur, loop), 50), ((cur, 1), 130), ((cur, 2), 60), ((cur - 1, loop), 120), ((cur - 1, 1), 90)):
        weights[(min(a, b), max(a, b))] = w
    covis.append((cur - 1, loop, 120))                                  # a pair LoopConnections has already inserted
    # ---- the snapshot, by the reference's rules
    Scw = np.zeros((N, 8)); Smeas = np.zeros((N, 8))
    for k in range(N):
        plain = np.concatenate([mat2q(poses[k, :9].reshape(3, 3)), poses[k, 9:], [1.0]])
        Scw[k] = p["Scw"][k] if has_corr[k] else plain
        Smeas[k] = p["Smeas"][k] if has_corr[k] else Scw[k]
    wt = lambda a, b: weights.get((min(a, b), max(a, b)), 0)
    edges, corr, inserted = [], [], set()
    for a in sorted({a for a, _ in lc}):
        for b in sorted(b for x, b in lc if x == a):
            if (a != cur or b != loop) and wt(a, b) < MIN_FEAT:
                continue
            edges.append((a, b)); corr.append(1); inserted.add((min(a, b), max(a, b)))
    le = {k: set() for k in range(N)}
    for a, b in loop_edges:
        le[a].add(b); le[b].add(a)
    for k in range(N):
        if k > 0:
            edges.append((k, k - 1)); corr.append(0)
        for l in sorted(le[k]):
            if l < k:
                edges.append((k, l)); corr.append(0)
        for a, b, w in covis:
            if a != k or w < MIN_FEAT or b == k - 1 or b == k + 1 or b in le[k] or not b < k or (min(a, b), max(a, b)) in inserted:
                continue
            edges.append((k, b)); corr.append(0)
    fixed = np.zeros(N, np.uint8); fixed[loop] = 1
    by_cur = (np.arange(len(p["points"])) % 3 == 0).astype(np.float64)
    snap = dict(Scw=Scw, Smeas=Smeas, fixed=fixed, edge_idx=np.array(edges, np.int32), edge_corrected=np.array(corr, np.uint8), points=p["points"],
                point_ref=p["point_ref"], fix_scale=fix_scale)
    wrec = np.array([(a, b, w) for (a, b), w in sorted(weights.items())], np.float64)
    bad_pos = 5
    blob = np.concatenate([np.array([N, len(p["points"]), int(fix_scale), cur, loop, bad_pos, len(wrec), len(lc), len(loop_edges), len(covis)], np.float64), poses.ravel(),
                           has_corr.astype(np.float64), p["Scw"].ravel(), has_corr.astype(np.float64), p["Smeas"].ravel(), parent, wrec.ravel(),
                           np.array(lc, np.float64).ravel(), np.array(loop_edges, np.float64).ravel(), np.array(covis, np.float64).ravel(),
                           p["points"].astype(np.float64).ravel(), p["point_ref"].astype(np.float64), by_cur])
    return blob, snap, bad_pos


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [False, True])
def test_shim_equals_the_direct_call_on_the_same_snapshot(tmp_path, fix_scale):
    from viorb_amd import essential_graph as EG
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)          # the tiny map: throws for a bad parent, then solves and writes back
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("OK iterations")
    N = 14
    blob, snap, bad_pos = make_map(41 + int(fix_scale), N, fix_scale)
    # the selection kept and dropped what it should: 3 of 5 LoopConnections, one loop edge, covisibles of weight 150 and 101 only
    ei = [tuple(e) for e in snap["edge_idx"]]
    assert snap["edge_corrected"].sum() == 3 and (N - 1, 2) not in ei and (N - 2, 1) not in ei and (N - 3, N - 7) in ei and ei.count((N - 2, 0)) == 1
    assert (6, 3) not in ei and (6, 4) in ei and (6, 2) in ei and (6, 5) in ei and (6, 7) not in ei and (5, 6) not in ei
    prob, out = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    blob.tofile(prob)
    r = subprocess.run([exe, prob, out], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    got = np.fromfile(out, np.float64)
    d = EG.solve(snap)
    assert np.array_equal(got[:6], d["info"]) and d["iterations"] >= 2 and d["chi2_after"] < 0.5 * d["chi2_before"]
    kf = got[6:6 + 18 * (N + 1)].reshape(N + 1, 18)
    good = [l for l in range(N + 1) if l != bad_pos]
    assert (kf[bad_pos] == 0).all()                                                    # the bad key frame is neither a vertex nor written
    assert (kf[good, 16] == 1).all() and (kf[good, 17] == 1).all()                     # SetPose and UpdateNavStatePVRFromTcw once each
    T = kf[good, :16].reshape(N, 4, 4)
    want = d["Tcw_out"].astype(np.float32).astype(np.float64)
    assert np.array_equal(T[:, :3, :3].reshape(N, 9), want[:, :9]) and np.array_equal(T[:, :3, 3], want[:, 9:]) and (T[:, 3] == [0, 0, 0, 1]).all()
    npt = len(snap["points"])
    pt = got[6 + 18 * (N + 1):6 + 18 * (N + 1) + 5 * npt].reshape(npt, 5)
    assert np.array_equal(pt[:, :3], d["points_out"].astype(np.float64)) and (pt[:, 3] == 1).all() and (pt[:, 4] == 1).all()
    assert list(got[-2:]) == [1, 1]                                                    # SetMapUpdateFlagInTracking(true), once
