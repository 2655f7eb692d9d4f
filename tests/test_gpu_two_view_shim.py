"""viorb_amd/shim/Initializer_shim.h driven from a C++ program with stand-in Frame / cv types (tests/cpp/shim_two_view_test.cpp): what
Initializer::Initialize returns equals the direct host-form call viorb_two_view_init with the sets of the same seed. Without a device
the class throws (the program exits with 3); with fewer than eight matches it returns false without a call."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
from viorb_amd import two_view as tv
from viorb_amd.synth import make_two_view_init_problem
import two_view_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "shim_two_view_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_two_view_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def run(exe, tmp_path, p, seed):
    prob, out = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    with open(prob, "wb") as f:
        f.write(np.array([len(p["xy1"]), len(p["xy2"]), seed], np.int32).tobytes() + np.asarray(p["K4"], np.float32).tobytes() +
                np.ascontiguousarray(p["xy1"], np.float32).tobytes() + np.ascontiguousarray(p["xy2"], np.float32).tobytes() +
                np.ascontiguousarray(p["matches12"], np.int32).tobytes())
    r = subprocess.run([exe, prob, out], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r, (open(out, "rb").read() if r.returncode == 0 else b"")


def test_shim_compiles_and_handles_the_cases_that_need_no_device(tmp_path):
    exe = build(tmp_path)
    few = make_two_view_init_problem(1, "general", 60, 70, 8, 0.0, 0.5)
    few["matches12"][np.nonzero(few["matches12"] >= 0)[0][:3]] = -1
    r, blob = run(exe, tmp_path, few, 0)
    assert r.returncode == 0 and list(np.frombuffer(blob[:12], np.int32)) == [0, T.FAILED, T.FEW_MATCHES]
    if viorb_amd.lib().viorb_device_count() < 1:                   # no CPU fallback: the failure is an exception, not "false"
        r, _ = run(exe, tmp_path, make_two_view_init_problem(0, "general", 200, 210, 130, 0.1, 0.5), 0)
        assert r.returncode == 3 and "exception: Initializer::Initialize" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed", [("general", 5), ("planar", 6), ("low_parallax", 7)])
def test_shim_equals_the_direct_call(tmp_path, kind, seed):
    exe = build(tmp_path)
    p = make_two_view_init_problem(seed, kind, 330, 350, 250, 0.1, 0.5)
    r, blob = run(exe, tmp_path, p, seed)
    assert r.returncode == 0
    want = tv.TwoViewInit(p, tv.draw_sets(250, 200, seed))
    ok, status, reason = np.frombuffer(blob[:12], np.int32)
    assert (status, reason) == (want["status"], want["reason"]) and bool(ok) == (want["status"] != T.FAILED)
    assert bool(ok) == (kind != "low_parallax")
    if ok:
        n1 = len(p["xy1"])
        f = np.frombuffer(blob[12:12 + 4 * (12 + 3 * n1)], np.float32)
        assert np.array_equal(f[:9].reshape(3, 3), want["R21"]) and np.array_equal(f[9:12], want["t21"])
        assert np.array_equal(f[12:].reshape(n1, 3), want["P3D"])
        assert np.array_equal(np.frombuffer(blob[12 + 4 * (12 + 3 * n1):], np.uint8), want["triangulated"])
