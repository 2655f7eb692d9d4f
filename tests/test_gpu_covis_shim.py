"""viorb_shim::update_connections and viorb_shim::update_connections_loop (viorb_amd/shim/KeyFrame_shim.h) driven from a C++ program with
the stand-in KeyFrame / MapPoint of tests/cpp/covis_standin.h (tests/cpp/shim_covis_test.cpp): the first on every target in turn, one call
of the library each, the second on the targets as one group. The program compares the members the shim wrote back
(mConnectedKeyFrameWeights, the ordered vectors, mpParent, mbFirstConnection, mspChildrens) and the LoopConnections map with a
restatement of the routine over the same objects; here they are compared with the checker tests/covis_ref.py as well. Without a device
the templates throw (the program exits with 3)."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
import covis_ref as T
import covis_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("kf_by_key", "kf_flags", "kf_parent", "kp_start", "kp_point", "pt_bad", "obs_start", "obs", "conn_start", "conn_kf", "conn_w", "ord_start", "ord_kf", "ord_w", "targets")


def build(tmp_path, extra=()):
    exe = str(tmp_path / "shim_covis_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_covis_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe] + list(extra))
    return exe


def run(exe, tmp_path, problems):
    """All (mode, scene) through one process; the outputs of those that ran, or None each when the program failed."""
    c = lambda x: np.ascontiguousarray(x, np.int32).tobytes()
    args = []
    for i, (mode, s) in enumerate(problems):
        blob = c([mode, len(s["kf_flags"]), len(s["kp_point"]), len(s["pt_bad"]), len(s["obs"]), len(s["conn_kf"]), len(s["ord_kf"]), len(s["targets"])])
        for f in FIELDS:
            blob += c(s[f])
        args += [str(tmp_path / ("problem%d.bin" % i)), str(tmp_path / ("out%d.bin" % i))]
        open(args[-2], "wb").write(blob)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r, [np.frombuffer(open(o, "rb").read(), np.int32).tolist() if r.returncode == 0 else None for o in args[1::2]]


def parse(o, nk):
    """(per key frame: conn [(kf, w)], ord [(kf, w)], parent, first, children), {target: [loop connections]} from the program's output."""
    it = iter(o)
    kfs = []
    for _ in range(nk):
        conn = [(next(it), next(it)) for _ in range(next(it))]
        order = [(next(it), next(it)) for _ in range(next(it))]
        parent, first = next(it), next(it)
        kfs.append((conn, order, parent, first, [next(it) for _ in range(next(it))]))
    loop = {}
    for _ in range(next(it)):
        k = next(it)
        loop[k] = [next(it) for _ in range(next(it))]
    assert list(it) == []
    return kfs, loop


def problems():
    """The hand-built scenes that do not depend on ccap and the first 25 random streams, each in both modes."""
    named = [(c[0], c[1]) for c in K.CASES if "ccap" not in c[2]] + [("random_%d" % i, s) for i, s in enumerate(K.random_streams()[0][:25])]
    return [(name, mode, s) for name, s in named for mode in (0, 1)]


def compare(named, outs):
    n_loop = n_parent = 0
    for (name, mode, s), o in zip(named, outs):
        nk = len(s["kf_flags"])
        e = T.update_connections(s, erase_targets=1)
        kfs, loop = parse(o, nk)
        pos = np.empty(nk, np.int64)
        pos[s["kf_by_key"]] = np.arange(nk)
        for k, (conn, order, parent, first, children) in enumerate(kfs):
            assert conn == K.rows(e, "conn", k) and order == K.rows(e, "ord", k), (name, mode, k)
            assert parent == e["kf_parent_out"][k] and first == (int(e["kf_flags_out"][k]) >> 1), (name, mode, k)
            assert children == sorted(e["children"][k], key=lambda c: pos[c]), (name, mode, k)     # a std::set<KeyFrame*>: key order
            n_parent += parent != s["kf_parent"][k]
        if mode == 0:
            assert loop == {}
            continue
        want = {}
        for t, kt in enumerate(s["targets"].tolist()):                  # LoopConnections[pKFi] = ...: a repeated target keeps its last set
            want[kt] = e["loop_conn"][t][:e["n_loop_conn"][t]].tolist()
        assert {k: sorted(v, key=lambda c: pos[c]) for k, v in loop.items()} == want and list(loop) == sorted(want, key=lambda c: pos[c]), (name, mode)
        n_loop += sum(len(v) > 0 for v in want.values())
    assert n_loop >= 10 and n_parent >= 10


def test_shim_compiles_and_a_failure_throws(tmp_path):
    exe = build(tmp_path)
    if viorb_amd.lib().viorb_device_count() < 1:                       # no CPU fallback: the failure is an exception, not an unchanged graph
        for mode in (0, 1):
            r, _ = run(exe, tmp_path, [(mode, next(c[1] for c in K.CASES if c[0] == "loop_connections"))])
            assert r.returncode == 3 and "exception: UpdateConnections" in r.stdout and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_shim_writes_back_what_the_reference_leaves(tmp_path):
    exe = build(tmp_path)
    named = problems()
    r, outs = run(exe, tmp_path, [(mode, s) for _, mode, s in named])
    assert r.returncode == 0                                           # 4: the members differ from the program's own restatement
    compare(named, outs)
