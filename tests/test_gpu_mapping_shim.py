"""viorb_amd/shim/LocalMapping_shim.h driven from a C++ program with stand-in KeyFrame / MapPoint types
(tests/cpp/shim_mapping_test.cpp): what the templates return equals the direct C-ABI call on the same problem. The build helper and
the problem file writer are used by the CPU suite too (tests/test_mapping_ref.py: without a device both templates must throw)."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd.synth import make_mapping_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_mapping_shim_test(tmp_path):
    exe = str(tmp_path / "shim_mapping_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_mapping_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def write_problem(path, p, monocular):
    cam = p["cam"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()
    out = [i32([len(p["neigh"]), int(monocular), len(cam["sf"])]), f32(list(cam["intr4"]) + [cam["mb"], cam["mbf"], cam["scale_factor"], 0.0]),
           f32(cam["sf"]), f32(cam["level_sigma2"]), np.array([n["kf2_first"] for n in p["neigh"]], np.uint8).tobytes()]
    for kf in [p["kf1"]] + list(p["neigh"]):
        out += [i32([len(kf["kps"])]), np.ascontiguousarray(kf["kps"], capi.KP_DTYPE).tobytes(), np.ascontiguousarray(kf["desc"], np.uint8).tobytes(),
                np.ascontiguousarray(kf["hp"], np.uint8).tobytes(), f32(kf["ur"]), f32(kf["depth"]), f32(kf["xy_dist"]), i32(kf["node"]), f32(kf["pose12"]),
                f32(kf["Ow"]), f32(kf.get("F12", np.zeros(9))), f32([kf.get("median_depth", 1.0)])]
    with open(path, "wb") as f:
        f.write(b"".join(out))


@pytest.mark.gpu
@pytest.mark.parametrize("sfrac", [0.0, 0.4])
def test_mapping_shim_equals_direct_calls(tmp_path, sfrac):
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    p = make_mapping_problem(31, J=12, n1=700, n2=650, stereo_frac=sfrac)
    mono = sfrac == 0.0
    fin, fout = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    write_problem(fin, p, mono)
    exe = build_mapping_shim_test(tmp_path)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    want = viorb_amd.CreateNewMapPointsHost(p["cam"], p, len(p["kf1"]["kps"]), monocular=mono)
    assert want["status"] == 0 and want["n_new"] > 100
    blob = open(fout, "rb").read()
    n = int(np.frombuffer(blob, np.int32, 1)[0])
    assert n == want["n_new"]
    rec = np.frombuffer(blob, np.dtype([("idx", "i4", 3), ("f", "f4", 8), ("d", "u1", 32)]), n, 4)
    np.testing.assert_array_equal(rec["idx"], want["new_idx"])
    assert rec["f"].tobytes() == want["new_pts_f"].tobytes()
    np.testing.assert_array_equal(rec["d"], want["new_desc"])
