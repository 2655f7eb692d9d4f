"""viorb_shim::set_bad_flag, set_erase and remove_key_frames (viorb_amd/shim/KeyFrame_shim.h) driven from a C++ program with the stand-in
KeyFrame / MapPoint / Map / KeyFrameDatabase of tests/cpp/kf_removal_standin.h (tests/cpp/shim_kf_removal_test.cpp): the first two on every
operation in turn, one call of the library each, the third on all operations in one call. The program compares the state the templates
left in the objects (maps, lists, mpParent, mspChildrens of the good key frames, the flags, the links, mTcp bit for bit, mvpMapPoints,
mObservations, nObs, mpRefKF, mbBad, what was erased from the map and the database, the IMU appends) with a restatement of the routine
over a second description of the same map; here it is compared with the checker tests/kf_removal_ref.py as well. Without a device the
templates throw (the program exits with 3)."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
import kf_removal_ref as T
import kf_removal_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("kf_by_key", "kf_flags", "kf_parent", "kf_prev", "kf_next", "kf_pose12", "kp_start", "kp_point", "pt_bad", "pt_nobs", "pt_ref", "obs_start", "obs",
          "conn_start", "conn_kf", "conn_w", "ord_start", "ord_kf", "ord_w", "op_kf", "op_kind")


def build(tmp_path):
    exe = str(tmp_path / "shim_kf_removal_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_kf_removal_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def run(exe, tmp_path, problems):
    """All (mode, scene) through one process; the outputs of those that ran, or None each when the program failed."""
    c = lambda x: (np.ascontiguousarray(x, np.float32).view(np.int32) if np.asarray(x).dtype == np.float32 else np.ascontiguousarray(x, np.int32)).tobytes()
    args = []
    for i, (mode, s) in enumerate(problems):
        blob = c([mode, len(s["kf_flags"]), len(s["kp_point"]), len(s["pt_bad"]), len(s["obs"]), len(s["conn_kf"]), len(s["ord_kf"]), len(s["op_kf"])])
        for f in FIELDS:
            blob += c(s[f])
        args += [str(tmp_path / ("problem%d.bin" % i)), str(tmp_path / ("out%d.bin" % i))]
        open(args[-2], "wb").write(blob)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    return r, [np.frombuffer(open(o, "rb").read(), np.int32).tolist() if r.returncode == 0 else None for o in args[1::2]]


def parse(o, nk, n_pt):
    it = iter(o)
    many = lambda: [next(it) for _ in range(next(it))]
    kfs, pts = [], []
    for _ in range(nk):
        conn = [(next(it), next(it)) for _ in range(next(it))]
        order = [(next(it), next(it)) for _ in range(next(it))]
        parent, flags, prev, nxt = next(it), next(it), next(it), next(it)
        n = next(it)
        children = None if n < 0 else [next(it) for _ in range(n)]
        tcp = np.array([next(it) for _ in range(12)], np.int32).view(np.float32) if next(it) else None
        kfs.append(dict(conn=conn, ord=order, parent=parent, flags=flags, prev=prev, next=nxt, children=children, tcp=tcp, table=many()))
    for _ in range(n_pt):
        pts.append(dict(nobs=next(it), bad=next(it), ref=next(it), obs=many()))
    out = dict(kfs=kfs, pts=pts, map_kfs=many(), db=many(), map_pts=many())
    out["imu"] = [(next(it), next(it)) for _ in range(next(it))]
    assert list(it) == []
    return out


def problems():
    """The hand-built scenes and the first 20 streams of the random set, each in both modes."""
    named = [(c[0], c[1]) for c in K.CASES] + [("random_%d" % i, s) for i, s in enumerate(K.random_streams()[0][:20])]
    return [(name, mode, s) for name, s in named for mode in (0, 1)]


def compare(named, outs):
    n_removed = n_parent = 0
    for (name, mode, s), o in zip(named, outs):
        nk, n_pt = len(s["kf_flags"]), len(s["pt_bad"])
        e = T.remove_key_frames(s)
        g = parse(o, nk, n_pt)
        pos = np.empty(nk, np.int64)
        pos[s["kf_by_key"]] = np.arange(nk)
        by_key = lambda slots: sorted(slots, key=lambda c: pos[c])
        for k, kf in enumerate(g["kfs"]):
            where = (name, mode, k)
            assert kf["conn"] == K.rows(e, "conn", k) and kf["ord"] == K.rows(e, "ord", k), where
            assert (kf["parent"], kf["flags"], kf["prev"], kf["next"]) == (e["kf_parent_out"][k], e["kf_flags_out"][k], e["kf_prev_out"][k], e["kf_next_out"][k]), where
            assert kf["children"] == (None if e["children"][k] is None else by_key(e["children"][k])), where      # a std::set<KeyFrame*>: key order
            want = e["kf_Tcp"][k]
            assert (kf["tcp"] is None) == (want is None) and (want is None or np.array_equal(kf["tcp"].view(np.uint32), want.view(np.uint32))), where
            assert kf["table"] == e["kp_point_out"][s["kp_start"][k]:s["kp_start"][k + 1]].tolist(), where
            n_parent += kf["parent"] != s["kf_parent"][k]
        for p, pt in enumerate(g["pts"]):
            a, b = s["obs_start"][p], s["obs_start"][p + 1]
            alive = [int(w) & 0xffff for w, keep in zip(s["obs"][a:b], e["obs_alive"][a:b]) if keep]
            assert (pt["nobs"], pt["bad"], pt["ref"], pt["obs"]) == (e["pt_nobs_out"][p], e["pt_bad_out"][p], e["pt_ref_out"][p], by_key(alive)), (name, mode, p)
        # what left the map and the database, the IMU appends: a replay of the operations over the checker's reasons
        left = [int(x) for x, why in zip(s["op_kf"], e["op_reason"]) if why in (T.REMOVED, T.ALREADY_BAD)]
        assert g["map_kfs"] == left and g["db"] == left, (name, mode)
        cleared = [p for p in range(n_pt) if s["obs_start"][p + 1] > s["obs_start"][p] and e["pt_bad_out"][p] and not e["obs_alive"][s["obs_start"][p]:s["obs_start"][p + 1]].any()
                   and e["pt_nobs_out"][p] != s["pt_nobs"][p]]
        assert sorted(g["map_pts"]) == cleared, (name, mode)
        prev, nxt, imu = s["kf_prev"].copy(), s["kf_next"].copy(), []
        for x, why in zip(s["op_kf"], e["op_reason"]):
            if why != T.REMOVED:
                continue
            a, b = prev[x], nxt[x]
            if a >= 0:
                nxt[a] = b
            if b >= 0:
                prev[b] = a
            if a >= 0 and b >= 0:
                imu.append((int(b), int(x)))
            prev[x] = nxt[x] = -1
        assert g["imu"] == imu, (name, mode)
        n_removed += int((e["op_reason"] == T.REMOVED).sum())
    assert n_removed >= 40 and n_parent >= 20


def test_shim_compiles_and_a_failure_throws(tmp_path):
    exe = build(tmp_path)
    if viorb_amd.lib().viorb_device_count() < 1:                       # no CPU fallback: the failure is an exception, not an unchanged map
        for mode in (0, 1):
            r, _ = run(exe, tmp_path, [(mode, next(c[1] for c in K.CASES if c[0] == "three_children"))])
            assert r.returncode == 3 and "exception: remove_key_frames" in r.stdout and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_shim_leaves_what_the_reference_leaves(tmp_path):
    exe = build(tmp_path)
    named = problems()
    r, outs = run(exe, tmp_path, [(mode, s) for _, mode, s in named])
    assert r.returncode == 0                                           # 4: the members differ from the program's own restatement
    compare(named, outs)
