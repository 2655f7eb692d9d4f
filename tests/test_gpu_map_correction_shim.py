"""viorb_shim::correct_loop_propagate and viorb_shim::apply_global_ba (viorb_amd/shim/LoopClosing_shim.h) driven from a C++ program with the
stand-in KeyFrame / MapPoint / Map of tests/cpp/map_correction_standin.h (tests/cpp/shim_map_correction_test.cpp). The program writes what
the templates left in the objects (poses, points with normal and range, mnCorrectedByKF / mnCorrectedReference, both Sim3 maps in their
iteration order; NavStates, mTcwGBA / mTcwBefGBA, flags), and this test compares every number with the checker
tests/map_correction_ref.py, bit for bit. Without a device the templates throw (the program exits with 3)."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
import map_correction_ref as T
import map_correction_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32 = lambda x: np.ascontiguousarray(x, np.int32).tobytes()
f32 = lambda x: np.ascontiguousarray(x, np.float32).tobytes()
f64 = lambda x: np.ascontiguousarray(x, np.float64).tobytes()


def build(tmp_path):
    exe = str(tmp_path / "shim_map_correction_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_map_correction_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def loop_blob(s):
    h = [0, len(s["kf_by_key"]), len(s["kp_point"]), len(s["pt_bad"]), len(s["obs"]), len(s["conn"]), s["cur_kf"], s["cur_id"]]
    return i32(h) + b"".join(i32(s[f]) for f in ("kf_by_key", "kp_start", "kp_point", "pt_bad", "obs_start", "obs", "pt_ref", "pt_corrected_by", "conn")) \
        + f32(s["pose12"]) + f32(s["pts_f"]) + f64(s["Scw8"])


def gba_blob(s, Tbc):
    h = [1, len(s["kf_in_gba"]), len(s["child_kf"]), len(s["origins"]), len(s["pt_bad"]), 0, 0, 0]
    return i32(h) + b"".join(i32(s[f]) for f in ("child_start", "child_kf", "origins", "kf_in_gba", "pt_bad", "pt_in_gba", "pt_ref")) \
        + b"".join(f32(s[f]) for f in ("pose12", "TcwGBA12", "Pw", "PosGBA")) + f32(Tbc) + f64(s["ns22"]) + f64(s["nsGBA22"])


def run(exe, tmp_path, blobs):
    args = []
    for i, blob in enumerate(blobs):
        args += [str(tmp_path / ("problem%d.bin" % i)), str(tmp_path / ("out%d.bin" % i))]
        open(args[-2], "wb").write(blob)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r, [np.frombuffer(open(o, "rb").read(), np.float64) if r.returncode == 0 else None for o in args[1::2]]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_loop(s, o):
    e = T.correct_loop(s)
    nk, npt = len(s["kf_by_key"]), len(s["pt_bad"])
    kf = o[:nk * 13].reshape(nk, 13)
    assert same(kf[:, :12].astype(np.float32), e["pose12_out"])
    members = set(e["member_kf"].tolist())
    assert kf[:, 12].tolist() == [1.0 if k in members else 0.0 for k in range(nk)]               # SetPose on the members, once
    pt = o[nk * 13:nk * 13 + npt * 12].reshape(npt, 12)
    observed = np.diff(s["obs_start"]) > 0
    touched = e["pt_touched"].astype(bool)
    assert pt[:, 10].tolist() == touched.astype(float).tolist() and pt[:, 11].tolist() == (touched & observed).astype(float).tolist()
    assert same(pt[:, :8].astype(np.float32), e["pts_f_out"])                                       # a point nobody corrects keeps its members
    assert same(pt[:, 8].astype(np.int32), e["pt_corrected_by_out"])
    assert pt[touched, 9].astype(np.int32).tolist() == e["pt_corrected_ref_out"][touched].tolist()
    rest = o[nk * 13 + npt * 12:]
    assert int(rest[0]) == e["n_member"]
    maps = rest[1:].reshape(e["n_member"], 17)
    assert maps[:, 0].astype(np.int32).tolist() == e["member_kf"].tolist()                        # the iteration order of CorrectedSim3
    assert same(maps[:, 1:9], e["Scw_out"][e["member_kf"]]) and same(maps[:, 9:17], e["Smeas_out"][e["member_kf"]])
    return int(touched.sum())


def check_gba(s, Tbc, o):
    e = T.apply_global_ba(s, Tbc)
    nk, npt = len(s["kf_in_gba"]), len(s["pt_bad"])
    kf = o[:nk * 104].reshape(nk, 104)
    r = e["kf_reached"].astype(bool)
    assert same(kf[:, :12].astype(np.float32), e["pose12_out"]) and same(kf[:, 12:34], e["ns22_out"])
    assert same(kf[r, 34:46].astype(np.float32), e["TcwBef_out"][r]) and same(kf[r, 46:68], e["nsBef_out"][r])
    assert same(kf[r, 68:80].astype(np.float32), e["TcwGBA_out"][r]) and same(kf[r, 80:102], e["nsGBA_out"][r])
    assert kf[:, 102].tolist() == e["kf_in_gba_out"].astype(float).tolist() and kf[:, 103].tolist() == e["kf_reached"].astype(float).tolist()
    pt = o[nk * 104:].reshape(npt, 4)
    assert same(pt[:, :3].astype(np.float32), e["Pw_out"])
    assert pt[:, 3].tolist() == np.isin(e["pt_code"], (T.AG_POS_GBA, T.AG_BY_REF)).astype(float).tolist()
    return int(r.sum())


def test_shim_compiles_and_a_failure_throws(tmp_path):
    exe = build(tmp_path)
    if viorb_amd.lib().viorb_device_count() < 1:                       # no CPU fallback: the failure is an exception, not an unchanged map
        r, _ = run(exe, tmp_path, [loop_blob(K.CASES[4][1])])
        assert r.returncode == 3 and "exception: CorrectLoop" in r.stdout and "no HIP device" in r.stdout
        r, _ = run(exe, tmp_path, [gba_blob(K.gba_all_rules()[0], K.TBC_I)])
        assert r.returncode == 3 and "exception: apply_global_ba" in r.stdout and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_shim_writes_back_what_the_reference_leaves(tmp_path):
    exe = build(tmp_path)
    loops = [c[1] for c in K.CASES] + K.random_streams()[0][:25]
    maps = [(K.gba_all_rules()[0], K.TBC_I)] + [(s, K.TBC) for s in K.gba_random_streams()[0][:25]]
    r, outs = run(exe, tmp_path, [loop_blob(s) for s in loops] + [gba_blob(s, t) for s, t in maps])
    assert r.returncode == 0
    assert sum(check_loop(s, o) for s, o in zip(loops, outs)) >= 100
    assert sum(check_gba(s, t, o) for (s, t), o in zip(maps, outs[len(loops):])) >= 100
