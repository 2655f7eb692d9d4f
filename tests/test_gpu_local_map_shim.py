"""viorb_shim::update_local_map (viorb_amd/shim/viorb_tracking_shim.h) driven from a C++ program with the stand-in Frame / KeyFrame /
MapPoint of tests/cpp/local_map_standin.h (tests/cpp/shim_local_map_test.cpp). The program compares the members the shim wrote back
(mvpLocalKeyFrames, mpReferenceKF, mCurrentFrame.mpReferenceKF, mvpLocalMapPoints, the cleared mvpMapPoints) with a restatement of
the routine over the same objects; here they are compared with the checker tests/local_map_ref.py as well. Without a device
the template throws (the program exits with 3)."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
import local_map_ref as T
import local_map_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "shim_local_map_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_local_map_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def in_pointer_order(s):
    """The scene as the stand-in objects hold it: GetChilds() is a std::set<KeyFrame*>, so a key frame's children come in key order."""
    s = dict(s)
    pos = np.empty(len(s["kf_by_key"]), np.int64)
    pos[s["kf_by_key"]] = np.arange(len(pos))
    ch = np.array(s["child_kf"], copy=True)
    for k in range(len(pos)):
        a, b = s["child_start"][k], s["child_start"][k + 1]
        assert len(set(ch[a:b].tolist())) == b - a                     # the generators list no child twice
        ch[a:b] = sorted(ch[a:b].tolist(), key=lambda c: pos[c])
    s["child_kf"] = ch
    return s


def run(exe, tmp_path, scenes):
    """All scenes through one process; the outputs of those that ran, or None each when the program failed."""
    c = lambda x: np.ascontiguousarray(x, np.int32).tobytes()
    args = []
    for i, s in enumerate(scenes):
        blob = c([len(s["kf_bad"]), len(s["child_kf"]), len(s["kp_point"]), len(s["pt_bad"]), len(s["obs"]), len(s["frame_point"]), len(s["prev_lkf"]), s["prev_ref"]])
        for f in ("kf_bad", "kf_parent", "kf_prev", "kf_next", "covis10", "child_start", "child_kf", "kf_by_key", "kp_start", "kp_point", "pt_bad", "obs_start", "obs",
                  "frame_point", "prev_lkf"):
            blob += c(s[f])
        args += [str(tmp_path / ("problem%d.bin" % i)), str(tmp_path / ("out%d.bin" % i))]
        open(args[-2], "wb").write(blob)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r, [np.frombuffer(open(o, "rb").read(), np.int32) if r.returncode == 0 else None for o in args[1::2]]


def scenes():
    """The hand-built scenes that do not depend on lcap / pcap, and the first 25 random streams."""
    return [(c[0], in_pointer_order(c[1])) for c in K.CASES if not c[2]] + [("random_%d" % i, in_pointer_order(s)) for i, s in enumerate(K.random_streams()[0][:25])]


def test_shim_compiles_and_a_failure_throws(tmp_path):
    exe = build(tmp_path)
    if viorb_amd.lib().viorb_device_count() < 1:                       # no CPU fallback: the failure is an exception, not an empty local map
        r, _ = run(exe, tmp_path, [scenes()[0][1]])
        assert r.returncode == 3 and "exception: UpdateLocalMap" in r.stdout and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_shim_writes_back_what_the_reference_leaves(tmp_path):
    exe = build(tmp_path)
    named = scenes()
    r, outs = run(exe, tmp_path, [s for _, s in named])
    assert r.returncode == 0                                           # 4: the members differ from the program's own restatement
    seen = set()
    for (name, s), o in zip(named, outs):
        e = T.update_local_map(s)
        status, n_lkf, n_lpt, ref, frame_ref = o[:5]
        lkf, lpt, frame = o[5:5 + n_lkf], o[5 + n_lkf:5 + n_lkf + n_lpt], o[5 + n_lkf + n_lpt:]
        assert status == e["status"] and ref == e["ref_kf"], name
        assert np.array_equal(lkf, e["lkf"]) and np.array_equal(lpt, e["lpt"]) and np.array_equal(frame, e["frame_point_out"]), name
        assert frame_ref == (e["ref_kf"] if e["n_voted"] > 0 else -1), name          # mCurrentFrame.mpReferenceKF only when a key frame won the vote
        seen.add(int(status))
    assert seen == {T.OK, T.NO_VOTES}
