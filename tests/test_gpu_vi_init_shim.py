"""viorb_shim::try_init_vio / try_init_vio_apply (viorb_amd/shim/LocalMapping_shim.h) driven from a C++ program with stand-in KeyFrame /
MapPoint / IMUData / IMUPreintegrator types (tests/cpp/shim_vi_init_test.cpp): what the templates leave in the objects equals the
Python path (the host forms on independently flattened arrays), bit for bit. The build helper and the problem file writer are used by
the CPU suite too (tests/test_vi_init_ref.py: without a device the template must throw)."""
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi
from viorb_amd.synth import make_vi_init_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_vi_init_shim_test(tmp_path):
    exe = str(tmp_path / "shim_vi_init_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_vi_init_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def tcw_of(p):
    """Tcw = Rcw(9) tcw(3) as float from the float Twc of the stream (inverted in double, rounded once)."""
    T = np.asarray(p["twc12"], np.float64)
    out = np.zeros((len(T), 12), np.float32)
    for i, t in enumerate(T):
        R = t[:9].reshape(3, 3)
        out[i, :9] = R.T.ravel(); out[i, 9:] = -R.T @ t[9:]
    return out


def write_problem(path, p, n_est, n_kf, tcw, preint_own, pts, dmin, dmax):
    f64 = lambda a: np.ascontiguousarray(a, np.float64).tobytes()
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()
    out = [i32([n_est, n_kf, len(pts), 0]), f64(p["Tbc"]), f64([p["g"]])]
    for i in range(n_kf):
        S = np.asarray(p["imu"], np.float64).reshape(-1, 7)[p["imu_start"][i]:p["imu_start"][i + 1]]
        out += [f64([p["kf_time"][i]]), f32(p["twc12"][i]), f32(tcw[i]), f64(preint_own[i]), i32([len(S), 0]), f64(S)]
    out += [f32(pts), f32(dmin), f32(dmax)]
    with open(path, "wb") as f:
        f.write(b"".join(out))


@pytest.mark.gpu
@pytest.mark.parametrize("n_est,n_kf", [(24, 24), (20, 27)])
def test_vi_init_shim_equals_the_python_path(tmp_path, n_est, n_kf):
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    p = make_vi_init_problem(41, n_kf)
    cfg = dict(Tbc=p["Tbc"], g=p["g"])
    own = viorb_amd.PreintegrateIntervals(p)                   # what the key frames hold before initialisation: zero biases
    tcw = tcw_of(p)
    rng = np.random.default_rng(9)
    pts = rng.normal(size=(333, 3)).astype(np.float32) * 4; dmin = rng.uniform(0.5, 2, 333).astype(np.float32); dmax = dmin * 6
    fin, fout = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    write_problem(fin, p, n_est, n_kf, tcw, own, pts, dmin, dmax)
    exe = build_vi_init_shim_test(tmp_path)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK status 0"), out.stdout + out.stderr
    est, st, pbg = viorb_amd.ViInitHost(cfg, p, own, n_est=n_est)
    assert st == 0
    pv = own.copy(); pv[n_est:] = 0                            # the shim passes the key frames' own pre-integrations; rows >= n_est are not read
    ns, pose, pre = viorb_amd.ViInitApplyHost(cfg, p, tcw, est, pv, n_est, n_kf)
    blob = open(fout, "rb").read()
    at = 0
    def take(dt, n):
        nonlocal at
        a = np.frombuffer(blob, dt, n, at); at += a.nbytes
        return a
    assert take(np.int32, 1)[0] == 0
    assert take(np.float64, 48).tobytes() == est.tobytes()
    assert take(np.float64, n_est * 142).tobytes() == pbg.tobytes()
    rec = take(np.dtype([("ns", "f8", 22), ("pose", "f4", 12)]), n_kf)
    assert np.ascontiguousarray(rec["ns"]).tobytes() == ns.tobytes()
    assert np.ascontiguousarray(rec["pose"]).tobytes() == pose.tobytes()
    assert take(np.float64, n_kf * 142).tobytes() == pre.tobytes()
    sf = np.float32(est[7])
    assert (take(np.float32, 333 * 3).reshape(333, 3) == pts * sf).all()
    assert (take(np.float32, 333) == dmin * sf).all() and (take(np.float32, 333) == dmax * sf).all()
    assert at == len(blob)
