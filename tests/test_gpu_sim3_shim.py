"""viorb_amd/shim/Sim3Solver_shim.h driven from a C++ program with stand-in KeyFrame / MapPoint / cv types (tests/cpp/shim_sim3_test.cpp):
the constructor's filtering and index mapping, and iterate(5, ...) until a model or bNoMore the way LoopClosing::ComputeSim3 calls it,
equal the direct host-form calls viorb_sim3_ransac in chunks of 5 with the sets of the same seed, bit for bit, and
viorb_shim::optimize_sim3 on the model's inliers equals viorb_optimize_sim3 on the same snapshot. Without a device the
class throws (the program exits with 3); with fewer correspondences than minInliers it sets bNoMore and returns an empty matrix
without a call."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
from viorb_amd import sim3
from viorb_amd.synth import make_sim3_problem
import sim3_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "shim_sim3_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_sim3_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def make(seed, kind, n, outliers, holes=True):
    """A problem and the state of every key point of key frame 1: every seventh has no match, and one each has no map point in key frame
    1, a bad map point, a map point key frame 2 no longer indexes."""
    p = make_sim3_problem(seed, kind, n, outliers, 0.5, 0.002)
    state = np.ones(n, np.int32)
    if holes:
        state[3::7] = 0
        state[[5, 12, 19]] = (2, 3, 4)
    return p, state


def run(exe, tmp_path, p, state, seed, fix, min_inliers=20):
    prob, out = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    n = len(state)
    with open(prob, "wb") as f:
        f.write(np.array([n, seed, int(fix), min_inliers], np.int32).tobytes() + np.asarray(p["K1"], np.float32).tobytes() + state.tobytes() +
                np.ascontiguousarray(p["octave1"], np.int32).tobytes() + np.ascontiguousarray(p["octave2"], np.int32).tobytes() +
                np.ascontiguousarray(p["X1c"], np.float32).tobytes() + np.ascontiguousarray(p["X2c"], np.float32).tobytes() +
                np.ascontiguousarray(np.concatenate([p["obs1"], p["obs2"]], 1), np.float32).tobytes())
    r = subprocess.run([exe, prob, out], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r, (open(out, "rb").read() if r.returncode == 0 else b"")


def test_shim_compiles_and_handles_the_cases_that_need_no_device(tmp_path):
    exe = build(tmp_path)
    p, state = make(1, "general", 30, 0.0)                              # 22 matches survive the filtering... of which minInliers = 25 asks too many
    r, blob = run(exe, tmp_path, p, state, 0, False, min_inliers=25)
    head = np.frombuffer(blob[:32], np.int32)
    keep = int((state == 1).sum())
    assert r.returncode == 0 and list(head[:5]) == [0, 1, 0, 1, keep] and keep < 25       # no model, bNoMore, no inliers, one call
    assert not np.frombuffer(blob[32 + 4 * 29:32 + 4 * 29 + 30], np.uint8).any()
    if viorb_amd.lib().viorb_device_count() < 1:                       # no CPU fallback: the failure is an exception, not an empty matrix
        p, state = make(2, "general", 130, 0.2)
        r, _ = run(exe, tmp_path, p, state, 0, False)
        assert r.returncode == 3 and "exception: Sim3Solver::iterate" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,outliers,seed", [("general", 130, 0.3, 5), ("fix_scale", 300, 0.3, 6), ("general", 40, 0.5, 7)])
def test_shim_iterate_in_chunks_of_five_equals_the_direct_calls(tmp_path, kind, n, outliers, seed):
    exe = build(tmp_path)
    fix = kind == "fix_scale"
    p, state = make(seed, kind, n, outliers)
    r, blob = run(exe, tmp_path, p, state, seed, fix)
    assert r.returncode == 0
    idx = np.nonzero(state == 1)[0]                                     # mvnIndices1
    q = dict(p); q.update({k: p[k][idx] for k in ("X1c", "X2c", "sigma2_1", "sigma2_2")})
    N = len(idx)
    max_its = sim3.ransac_iterations(N, 0.99, 20, 300)
    sets = sim3.draw_sets(N, max_its, seed)
    first = best = calls = 0
    while True:
        w = sim3.sim3_ransac(q, sets, first_iteration=first, best_inliers_in=best, min_inliers=20, fix_scale=fix, iterations_per_call=5)
        calls += 1
        first, best = w["iterations_done"], w["best_inliers"]
        if w["status"] != T.CONTINUE:
            break
    head = np.frombuffer(blob[:32], np.int32)
    found = w["status"] == T.FOUND
    assert list(head) == [int(found), int(not found), w["n_inliers"], calls, N, max_its, first, best]
    f = np.frombuffer(blob[32:32 + 4 * 29], np.float32)
    flags = np.frombuffer(blob[32 + 4 * 29:32 + 4 * 29 + n], np.uint8)
    want = np.zeros(n, np.uint8)
    if found:
        want[idx] = w["inliers"]
        assert np.array_equal(f[:16].reshape(4, 4), w["T12"]) and np.array_equal(f[16:25].reshape(3, 3), w["R12"])
        assert np.array_equal(f[25:28], w["t12"]) and f[28] == w["s12"]
    assert np.array_equal(flags, want)
    tail = blob[32 + 4 * 29 + n:]
    n_opt, S_opt, left = np.frombuffer(tail[:4], np.int32)[0], np.frombuffer(tail[4:68], np.float64), np.frombuffer(tail[68:], np.uint8)
    if found:                                                          # optimize_sim3 of the shim against the direct host-form call
        R = w["R12"].astype(np.float64)
        sq = np.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1.0); rq = 0.5 / sq
        S0 = np.array([(R[2, 1] - R[1, 2]) * rq, (R[0, 2] - R[2, 0]) * rq, (R[1, 0] - R[0, 1]) * rq, 0.5 * sq, *w["t12"].astype(np.float64), float(w["s12"])])
        valid = ((state == 1) & (want != 0)).astype(np.uint8)
        lev = [np.float32(1)]
        for _ in range(7):
            lev.append(np.float32(lev[-1] * np.float32(1.2)))              # mvInvLevelSigma2 as the test program fills it: 1 / (s * s), s *= 1.2f
        inv = np.array([np.float32(1) / np.float32(v * v) for v in lev], np.float32)
        d = sim3.optimize_sim3(dict(p, inv_sigma2_1=inv[p["octave1"]], inv_sigma2_2=inv[p["octave2"]]), S0, 10.0, fix, valid)
        assert n_opt == d["n_in"] and np.array_equal(left, d["keep"])
        assert np.array_equal(S_opt, d["S12"] if d["info"][0] - d["info"][1] >= 10 else S0)
    else:
        assert n_opt == -1
    assert found == (kind != "general" or n != 40)                    # 40 key points with half the matches wrong hold no model
