"""viorb_amd/shim/KeyFrameDatabase_shim.h driven from a C++ program with stand-in KeyFrame / Frame types (tests/cpp/shim_place_test.cpp):
what the class template returns equals the direct C-ABI calls on the same problem."""
import os
import subprocess
import sys
import numpy as np
import pytest
import viorb_amd
from viorb_amd import place
from viorb_amd.synth import make_place_problem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_place_shim_test(tmp_path):
    exe = str(tmp_path / "shim_place_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_place_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def write_problem(path, p):
    N = len(p["bows"])
    out = [np.array([p["n_words"], N, len(p["erased"]), len(p["connected"])], np.float64), np.array(p["erased"], np.float64),
           np.array(p["connected"], np.float64), np.asarray(p["covis10"], np.float64).ravel()]
    for ids, vals in p["bows"]:
        out += [np.array([len(ids)], np.float64), ids.astype(np.float64), vals]
    with open(path, "wb") as f:
        f.write(b"".join(a.tobytes() for a in out))


@pytest.mark.gpu
def test_place_shim_equals_direct_calls(tmp_path):
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    p = make_place_problem(1, 48, 120, 4096)
    fin, fout = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    write_problem(fin, p)
    exe = build_place_shim_test(tmp_path)
    tiny = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert tiny.returncode == 0 and tiny.stdout.startswith("OK device"), tiny.stdout + tiny.stderr
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    got = np.fromfile(fout, np.float64)
    q = p["bows"][-1]
    scores = viorb_amd.BowScorePairs([q], [p["bows"][c] for c in p["connected"]], [(0, i) for i in range(len(p["connected"]))])
    ms = min(np.float32(1), scores.astype(np.float32).min())
    assert np.float32(got[0]) == ms == pr.loop_min_score(p)
    db = place.KeyFrameDatabase(p["n_words"])
    for b in p["bows"][:-1]:
        db.add(b)
    for e in p["erased"]:
        db.erase(e)
    # an erased key frame is no longer in the shim's map, so it is no covisible of anyone: the direct call gets the same table
    cov = p["covis10"].copy()
    cov[np.isin(cov, p["erased"])] = -1
    cov[p["erased"]] = -1
    loop, reloc = db.detect_loop_candidates(q, ms, p["connected"], cov), db.detect_relocalization_candidates(q, cov)
    nl = int(got[1])
    assert (got[2:2 + nl] - 1000).astype(int).tolist() == loop and len(loop) == 2
    nr = int(got[2 + nl])
    assert (got[3 + nl:3 + nl + nr] - 1000).astype(int).tolist() == reloc and len(reloc) >= 1
