"""viorb_shim::search_for_initialization (viorb_amd/shim/ORBmatcher_shim.h) and viorb_shim::compute_scene_median_depth
(LocalMapping_shim.h) driven from a C++ program with stand-in Frame / KeyFrame / cv types (tests/cpp/shim_search_init_test.cpp): they
leave vnMatches12, vbPrevMatched and the return values exactly as the checker tests/search_init_ref.py does. Without a device the
templates throw (the program exits with 3)."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
import search_init_ref as T
import search_init_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def build(tmp_path):
    exe = str(tmp_path / "shim_search_init_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_search_init_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def make():
    P = K.problem(1)
    rng = np.random.default_rng(4)
    T44 = np.eye(4, dtype=f32)
    T44[:3, :3] = np.linalg.qr(rng.normal(0, 1, (3, 3)))[0]
    T44[:3, 3] = rng.normal(0, 1, 3)
    X = rng.normal(0, 5, (333, 3)).astype(f32)
    has = (rng.random(333) < 0.7).astype(np.uint8)
    return dict(P=P, T44=T44, X=X, has=has, q=2)


def run(exe, tmp_path, S):
    P = S["P"]
    c = lambda x, dt: np.ascontiguousarray(x, dt).tobytes()
    blob = c([len(P["kps1"]), len(P["kps2"]), P["window_size"], 1, len(S["X"]), S["q"]], np.int32) + c(list(P["bounds4"]) + [P["nnratio"]], f32) + \
        c(P["kps1"], P["kps1"].dtype) + c(P["desc1"], np.uint8) + c(P["kps2"], P["kps2"].dtype) + c(P["desc2"], np.uint8) + c(P["prev_matched"], f32) + \
        c(S["T44"], f32) + c(S["X"], f32) + c(S["has"], np.uint8)
    prob, out = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    open(prob, "wb").write(blob)
    r = subprocess.run([exe, prob, out], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r, (open(out, "rb").read() if r.returncode == 0 else None)


def test_shim_compiles_and_a_failure_throws(tmp_path):
    exe = build(tmp_path)
    if viorb_amd.lib().viorb_device_count() < 1:                       # no CPU fallback: the failure is an exception, not "0 matches"
        r, _ = run(exe, tmp_path, make())
        assert r.returncode == 3 and "exception: SearchForInitialization" in r.stdout and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_shim_leaves_what_the_reference_leaves(tmp_path):
    exe = build(tmp_path)
    S = make()
    r, o = run(exe, tmp_path, S)
    assert r.returncode == 0
    n1 = len(S["P"]["kps1"])
    e = K.expected(1)
    nm = np.frombuffer(o, np.int32, 1)[0]
    m12 = np.frombuffer(o, np.int32, n1, 4)
    prev = np.frombuffer(o, f32, 2 * n1, 4 + 4 * n1).reshape(n1, 2)
    med = np.frombuffer(o, f32, 1, 4 + 12 * n1)[0]
    assert nm == e["nmatches"] and np.array_equal(m12, e["matches12"]) and np.array_equal(prev, e["prev_matched"])
    pose12 = np.concatenate([S["T44"][:3, :3].ravel(), S["T44"][:3, 3]])
    want, n = T.scene_median_depth(pose12, S["X"], S["has"], S["q"])
    assert n > 100 and f32(med).tobytes() == f32(want).tobytes()
