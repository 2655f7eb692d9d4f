"""The three Sim3 matcher templates of viorb_amd/shim/ORBmatcher_shim.h (search_by_sim3, search_by_projection_sim3, fuse_sim3) driven from
a C++ program with stand-in KeyFrame / MapPoint / cv types (tests/cpp/shim_sim3_match_test.cpp): they leave vpMatches12, vpMatched,
vpReplacePoint, the added observations and the key frame's map points exactly as the direct host-form calls plus the reference's
write-back rules (src/ORBmatcher.cc:1319, :396, :1081-1096) give. Without a device the templates throw (the program exits with 3)."""
import os
import subprocess
import numpy as np
import pytest
import viorb_amd
from viorb_amd import sim3_match as M
import sim3_match_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_ID, KF2_ID = 1000000, 100000


def build(tmp_path):
    exe = str(tmp_path / "shim_sim3_match_test")
    lib_dir = os.path.join(ROOT, "viorb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viorb_amd", "shim"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "shim_sim3_match_test.cpp"),
                           "-L", lib_dir, "-lviorb_hip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def make():
    """The small fixture and the map state around it: bad points in both key frames, vpMatches12 / vpMatched on entry, loop points that
    key frame 1 already holds."""
    P = K.problem(3, 40, 0, 1, 8, 100, 300, 300, 150)
    rng = np.random.default_rng(9)
    a, b, L = P["kf1"], P["kf2"], P["loop"]
    n1, n2, npts = len(a["kps"]), len(b["kps"]), len(L["pts_f"])
    bad1, bad2 = (rng.random(n1) < 0.04) & (a["has_point"] != 0), (rng.random(n2) < 0.04) & (b["has_point"] != 0)
    partner1 = np.where((a["already"] != 0) & (np.arange(n1) < 150), np.arange(n1), -1).astype(np.int32)      # common feature i of both key frames
    bad2[partner1[partner1 >= 0]] = False
    has1 = a["has_point"].copy()                                            # some common features of key frame 1 hold no point yet: Fuse adds there
    has1[rng.permutation(np.nonzero((np.arange(n1) < 150) & (a["already"] == 0))[0])[:40]] = 0
    bad1 &= has1 != 0
    matched_init = np.full(n1, -1, np.int32)
    for p in np.nonzero((L["valid"] == 0) & (L["source"] >= 0) & (L["source"] < 150))[0]:
        if b["already"][L["source"][p]] and matched_init[L["source"][p]] == -1:
            matched_init[L["source"][p]] = p                                 # key frame 1 holds loop point p at the common feature
    matched_init[(L["feat_taken"] != 0) & (matched_init == -1)] = -2
    lbad = ((L["valid"] == 0) & ~np.isin(np.arange(npts), matched_init)).astype(np.uint8)
    in_kf = np.full(npts, -1, np.int32)
    free_feats = np.nonzero(a["has_point"] == 0)[0]
    hold = rng.permutation(np.nonzero(lbad == 0)[0])[:12]
    in_kf[hold] = free_feats[:12]
    return dict(P=P, has1=has1, bad1=bad1.astype(np.uint8), bad2=bad2.astype(np.uint8), partner1=partner1, matched_init=matched_init, lbad=lbad, in_kf=in_kf)


def run(exe, tmp_path, S):
    P = S["P"]
    a, b, L = P["kf1"], P["kf2"], P["loop"]
    sf16 = np.zeros(16, np.float32); sf16[:len(P["sf"])] = P["sf"]
    c = lambda x, dt: np.ascontiguousarray(x, dt).tobytes()
    side = lambda s, bad: c(s["kps"], s["kps"].dtype) + c(s["desc"], np.uint8) + c(s["pose12"], np.float32) + c(s["has_point"], np.uint8) + c(bad, np.uint8) + \
        c(s["pts_f"], np.float32) + c(s["pts_desc"], np.uint8)
    blob = c([len(a["kps"]), len(b["kps"]), len(L["pts_f"]), len(P["sf"])], np.int32) + c(P["intr4"], np.float32) + c(P["bounds4"], np.float32) + c(sf16, np.float32) + \
        c(np.concatenate([P["R12"].ravel(), P["t12"], [P["s12"]]]), np.float32) + c(L["Scw"], np.float32) + c([K.TH_SIM3, K.TH_PROJ, K.TH_FUSE], np.float32) + \
        side(dict(a, has_point=S["has1"]), S["bad1"]) + side(b, S["bad2"]) + c(S["partner1"], np.int32) + c(L["pts_f"], np.float32) + c(L["pts_desc"], np.uint8) + c(S["lbad"], np.uint8) + \
        c(S["matched_init"], np.int32) + c(S["in_kf"], np.int32)
    prob, out = str(tmp_path / "problem.bin"), str(tmp_path / "out.bin")
    open(prob, "wb").write(blob)
    r = subprocess.run([exe, prob, out], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r, (np.fromfile(out, np.int32) if r.returncode == 0 else None)


def test_shim_compiles_and_a_failure_throws(tmp_path):
    exe = build(tmp_path)
    if viorb_amd.lib().viorb_device_count() < 1:                       # no CPU fallback: the failure is an exception, not "0 matches"
        r, _ = run(exe, tmp_path, make())
        assert r.returncode == 3 and "exception: SearchBySim3" in r.stdout and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_shim_write_back_equals_the_direct_calls_and_the_reference_rules(tmp_path):
    exe = build(tmp_path)
    S = make()
    r, o = run(exe, tmp_path, S)
    assert r.returncode == 0
    P = S["P"]
    a, b, L, cam = P["kf1"], P["kf2"], P["loop"], K.lib_camera(P)
    n1, n2, npts = len(a["kps"]), len(b["kps"]), len(L["pts_f"])
    nfound, nmatches, nfused = o[:3]
    o = o[3:]
    m12, matched, replace, add_idx, add_n, kfpts = o[:n1], o[n1:2 * n1], o[2 * n1:2 * n1 + npts], o[2 * n1 + npts:2 * n1 + 2 * npts], \
        o[2 * n1 + 2 * npts:2 * n1 + 3 * npts], o[2 * n1 + 3 * npts:]
    # SearchBySim3: has_point excludes the bad points; vbAlreadyMatched1 / 2 come from vpMatches12 and GetIndexInKeyFrame
    s1 = dict(a, has_point=S["has1"] * (1 - S["bad1"]), already=(S["partner1"] >= 0).astype(np.uint8))
    al2 = np.zeros(n2, np.uint8); al2[S["partner1"][S["partner1"] >= 0]] = 1
    s2 = dict(b, has_point=b["has_point"] * (1 - S["bad2"]), already=al2)
    d = M.search_by_sim3(s1, s2, P["R12"], P["t12"], P["s12"], cam, P["bounds4"], K.TH_SIM3)
    want = np.where(S["partner1"] >= 0, KF2_ID + S["partner1"], -1)
    want[d["match12"] >= 0] = KF2_ID + d["match12"][d["match12"] >= 0]
    assert nfound == d["nfound"] and nfound >= 30 and np.array_equal(m12, want)
    # SearchByProjection: valid = not bad and not in vpMatched on entry; vpMatched[bestIdx] = pMP
    valid = ((S["lbad"] == 0) & ~np.isin(np.arange(npts), S["matched_init"])).astype(np.uint8)
    d = M.search_by_projection_sim3(a["kps"], a["desc"], L["Scw"], L["pts_f"], L["pts_desc"], valid, (S["matched_init"] != -1).astype(np.uint8), cam,
                                    P["bounds4"], K.TH_PROJ)
    want = np.where(S["matched_init"] >= 0, LOOP_ID + S["matched_init"], S["matched_init"])
    hit = np.nonzero(d["best_idx"] >= 0)[0]
    want[d["best_idx"][hit]] = LOOP_ID + hit
    assert nmatches == d["nmatches"] and nmatches >= 30 and np.array_equal(matched, want)
    # Fuse: valid = not bad and not in the key frame; the block of :1081-1096 in point order
    valid = ((S["lbad"] == 0) & (S["in_kf"] < 0)).astype(np.uint8)
    d = M.fuse_sim3(a["kps"], a["desc"], L["Scw"], L["pts_f"], L["pts_desc"], valid, cam, P["bounds4"], K.TH_FUSE)
    holder = np.where(S["has1"] != 0, np.arange(n1), -1)                                     # the id of the point a feature holds, -1 none
    isbad = {int(i): bool(S["bad1"][i]) for i in range(n1)}
    for p in np.nonzero(S["in_kf"] >= 0)[0]:
        holder[S["in_kf"][p]] = LOOP_ID + p
    w_rep, w_add = np.full(npts, -1), np.full(npts, -1)
    for p in range(npts):
        f = d["best_idx"][p]
        if f < 0:
            continue
        if holder[f] >= 0:
            if not isbad.get(int(holder[f]), False):
                w_rep[p] = holder[f]
        else:
            w_add[p] = f
            holder[f] = LOOP_ID + p
    assert nfused == d["nfused"] and nfused >= 30
    assert np.array_equal(replace, w_rep) and np.array_equal(add_idx, w_add) and np.array_equal(add_n, (w_add >= 0).astype(np.int32))
    assert np.array_equal(kfpts, holder)
    assert (w_rep >= LOOP_ID).sum() >= 1 and (w_add >= 0).sum() >= 5 and ((w_rep >= 0) & (w_rep < LOOP_ID)).sum() >= 5
