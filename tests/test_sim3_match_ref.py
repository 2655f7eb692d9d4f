"""CPU tests of the Sim3 matchers (no GPU): the exported symbols, the host hooks viorb_debug_sim3_decompose / _pair / _project and
viorb_debug_claim_in_order (sim3_match_core.h compiled for the host) against the numpy checker tests/sim3_match_ref.py bit for bit, the
conditions the fixtures of the GPU tests have to meet (asserted on the checker alone), and the argument checks."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import sim3_match as M
from viorb_amd.synth import _rotvec_to_R
import sim3_match_ref as T
import sim3_match_cases as K

f32, f64 = np.float32, np.float64
BOUNDS = np.array([0, 752, 0, 480], f32)
SF = (f32(1.2) ** np.arange(8)).astype(f32)


def test_symbols_struct_sizes_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(capi.S3mKeyframes) == 6 * vp and C.sizeof(capi.S3mSide) == 11 * vp
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_sim3_match.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_sim3_match.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_SIM3_MATCH)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_SIM3_MATCH[name][1]) == n, name
    for code, name in enumerate(T.REASON_NAMES):
        assert re.search(r"#define VIORB_S3M_%s\s+%d\b" % (name, code), text), name
        assert getattr(M, name) == getattr(T, name) == code
    for name in ("Sim3MatchBatch", "search_by_sim3", "search_by_projection_sim3", "fuse_sim3", "keyframe_grid"):
        assert hasattr(viorb_amd, name)
    assert M.shape()[1] == 64 and M.shape()[0] % 64 == 0 and M.shape()[2] >= 1


# ---- the host hooks against the checker, bit for bit --------------------------------------------------------------------------------------
def _random_scw(rng):
    R = _rotvec_to_R(rng.normal(0, 0.5, 3))
    s = rng.uniform(0.4, 2.5)
    return np.concatenate([s * R, rng.normal(0, 2.0, (3, 1))], 1).astype(f32).ravel()


def test_decompose_and_pair_equal_the_checker():
    rng = np.random.default_rng(1)
    for _ in range(2000):
        S = _random_scw(rng)
        scw, R, t, Ow = M.debug_decompose(S)
        e = T.decompose(S)
        assert scw == e[0] and np.array_equal(R, e[1]) and np.array_equal(t, e[2]) and np.array_equal(Ow, e[3])
        R12, t12, s12 = _rotvec_to_R(rng.normal(0, 0.6, 3)).astype(f32), rng.normal(0, 1, 3).astype(f32), f32(rng.uniform(0.3, 3.0))
        a, b, c = M.debug_pair(R12, t12, s12)
        e = T.pair(R12, t12, s12)
        assert np.array_equal(a, e[0]) and np.array_equal(b, e[1]) and np.array_equal(c, e[2])
    assert np.abs(T.decompose(S)[1] @ T.decompose(S)[1].T - np.eye(3)).max() < 1e-5          # Rcw is a rotation again


def _same_projection(got, want):
    for k in ("u", "v", "dist3D", "radius"):
        assert np.array_equal(f32(got[k]), f32(want[k]), equal_nan=True), (k, got, want)
    assert got["reason"] == want["reason"] and got["level"] == want["level"], (got, want)
    if want["reason"] == T.MATCHED:
        assert got["rect"] == want["rect"], (got, want)


def _points_for(rng, cam, which, n):
    """Random transforms and map points that spread over every gate: (T12, sR, t, pt8) per point, T12 the pose or the similarity."""
    out = []
    for i in range(n):
        if which == T.SEARCH_BY_SIM3:
            pose = np.concatenate([_rotvec_to_R(rng.normal(0, 0.3, 3)).ravel(), rng.normal(0, 1, 3)]).astype(f32)
            sR12, sR21, t21 = T.pair(_rotvec_to_R(rng.normal(0, 0.3, 3)).astype(f32), rng.normal(0, 0.5, 3).astype(f32), f32(rng.uniform(0.5, 2)))
            sR, t = sR21, t21
            A = np.eye(4); A[:3, :3] = pose[:9].reshape(3, 3); A[:3, 3] = pose[9:]
            Bm = np.eye(4); Bm[:3, :3] = sR; Bm[:3, 3] = t
            full = Bm @ A
        else:
            pose, sR, t = _random_scw(rng), None, None
            scw, R, tc, _ = T.decompose(pose)
            full = np.eye(4); full[:3, :3] = R; full[:3, 3] = tc
        z = rng.uniform(0.5, 12) * (-1 if rng.random() < 0.08 else 1)
        uv = np.array([rng.uniform(-80, 832), rng.uniform(-60, 540)])
        Xc = np.array([(uv[0] - cam.cx) / cam.fx * z, (uv[1] - cam.cy) / cam.fy * z, z])
        Pw = np.linalg.solve(full, np.append(Xc, 1))[:3]
        dist = np.linalg.norm(Xc)
        normal = rng.normal(0, 1, 3); normal /= np.linalg.norm(normal)
        if which != T.SEARCH_BY_SIM3 and rng.random() < 0.7:                 # mostly seen from the front
            Ow = np.linalg.solve(full, np.array([0, 0, 0, 1.0]))[:3]
            normal = (Pw - Ow) / np.linalg.norm(Pw - Ow)
        lo, hi = dist * rng.uniform(0.05, 1.4), dist * rng.uniform(0.7, 1.2 ** 9)
        out.append((pose, sR, t, np.concatenate([Pw, normal, [lo, hi]]).astype(f32)))
    return out


@pytest.mark.parametrize("which", [T.SEARCH_BY_SIM3, T.SEARCH_BY_PROJECTION, T.FUSE])
def test_project_equals_the_checker_on_random_points(which):
    rng = np.random.default_rng(10 + which)
    cam, lc = T.Camera([458.654, 457.296, 367.215, 248.375], BOUNDS, SF), M.camera([458.654, 457.296, 367.215, 248.375], SF)
    th = {T.SEARCH_BY_SIM3: 7.5, T.SEARCH_BY_PROJECTION: 10.0, T.FUSE: 4.0}[which]
    seen = np.zeros(9, int)
    for pose, sR, t, pt in _points_for(rng, cam, which, 3000):
        want = T.project_pair(cam, pose, sR, t, pt, th) if which == T.SEARCH_BY_SIM3 else T.project_scw(cam, T.decompose(pose), pt, th)
        _same_projection(M.debug_project(which, pose, pt, lc, BOUNDS, th, sR, t), want)
        seen[want["reason"]] += 1
    gates = [T.MATCHED, T.BEHIND, T.OUT_OF_IMAGE, T.OUT_OF_RANGE] + ([] if which == T.SEARCH_BY_SIM3 else [T.VIEW_ANGLE])
    assert (seen[gates] >= 50).all(), seen


@pytest.mark.parametrize("which", [T.SEARCH_BY_SIM3, T.SEARCH_BY_PROJECTION, T.FUSE])
def test_project_equals_the_checker_on_the_edges(which):
    """A unit camera (fx = fy = 1, cx = cy = 0) under the identity, so that u, v and the distance are exact: z == 0, the image border, the
    distance gate at equality, levels predicted below 0 and at nlevels."""
    cam, lc = T.Camera([1, 1, 0, 0], BOUNDS, SF), M.camera([1, 1, 0, 0], SF)
    ident = np.concatenate([np.eye(3).ravel(), np.zeros(3)]).astype(f32) if which == T.SEARCH_BY_SIM3 else np.eye(4)[:3].astype(f32).ravel()
    sR, t = (np.eye(3, dtype=f32), np.zeros(3, f32)) if which == T.SEARCH_BY_SIM3 else (None, None)
    th = 7.5

    def run(pt):
        want = T.project_pair(cam, ident, sR, t, pt, th) if which == T.SEARCH_BY_SIM3 else T.project_scw(cam, T.decompose(ident), pt, th)
        _same_projection(M.debug_project(which, ident, pt, lc, BOUNDS, th, sR, t), want)
        return want
    pt = lambda x, y, z, lo, hi: np.array([x, y, z, x, y, z, lo, hi], f32)              # the normal along the ray: the view gate passes
    for x, y in ((0, 0), (1, 2), (-1, 0), (0, -3), (5, 5)):                             # z == 0: invz is infinite, u / v are infinite or NaN
        assert run(pt(x, y, 0, 0.1, 100))["reason"] == T.OUT_OF_IMAGE
    below = lambda v: np.nextafter(f32(v), f32(-1e9))
    for u, v, inside in ((0, 0, True), (752, 10, False), (below(752), 10, True), (10, 480, False), (10, below(480), True), (below(0), 5, False),
                         (5, below(0), False), (-0.0, 479, True), (751.99994, 479.99997, True)):
        r = run(pt(u, v, 1, 0.1, 4000))
        assert (r["reason"] != T.OUT_OF_IMAGE) == inside and (not inside or (r["u"] == f32(u) and r["v"] == f32(v)))
    rng, hits = np.random.default_rng(5), np.zeros(2, int)
    for _ in range(400):
        x, y, z = rng.uniform(0, 700), rng.uniform(0, 450), rng.uniform(1, 3)
        p = pt(x * z, y * z, z, 1, 1)
        dist = T._norm3(p[:3])
        for side, col, c in ((0, 6, f32(0.8)), (1, 7, f32(1.2))):
            for cand in (dist / c, np.nextafter(dist / c, f32(0)), np.nextafter(dist / c, f32(1e9))):
                q = p.copy(); q[6], q[7] = f32(0.01), f32(1e6); q[col] = cand
                exact = c * f32(cand) == dist
                r = run(q)
                if exact:
                    hits[side] += 1
                    assert r["reason"] != T.OUT_OF_RANGE                        # equality passes: the gate is dist < min || dist > max
    assert (hits >= 50).all(), hits
    levels = set()
    for _ in range(300):
        x, y, z = rng.uniform(100, 600), rng.uniform(100, 400), rng.uniform(1, 3)
        p = pt(x * z, y * z, z, 0.001, 1)
        dist = T._norm3(p[:3])
        for ratio in (1 / 1.2, 1 / 1.19, 0.95, 1.0, 1.2 ** 7, 1.2 ** 8, 1.2 ** 8.5, 1.2 ** 12):
            q = p.copy(); q[7] = f32(dist * ratio)
            r = run(q)
            with np.errstate(all="ignore"):
                raw = np.ceil(f32(np.log(f64(q[7] / dist))) / cam.log_sf)
            levels.add(int(raw))
            assert r["reason"] != T.MATCHED or r["level"] == min(max(int(raw), 0), 7)
    assert min(levels) < 0 and max(levels) >= 8, levels                       # both clamps were exercised
    one = T.Camera([1, 1, 0, 0], BOUNDS, SF[:1])                              # nlevels == 1: log(scale factor) == 0, every quotient is non-finite
    for ratio in (0.9, 1.0, 1.1):
        q = pt(300, 200, 1, 0.001, 1); q[7] = f32(T._norm3(q[:3]) * ratio)
        want = T.project_scw(one, T.decompose(np.eye(4)[:3].astype(f32).ravel()), q, th)
        got = M.debug_project(T.FUSE, np.eye(4)[:3].astype(f32).ravel(), q, M.camera([1, 1, 0, 0], SF[:1]), BOUNDS, th)
        _same_projection(got, want)
        assert want["level"] == 0 and want["reason"] == T.MATCHED


def test_claim_in_order_equals_the_literal_loop_under_heavy_contention():
    rng = np.random.default_rng(7)
    worst = 0
    for trial in range(60):
        nfeat, npts = int(rng.integers(1, 40)), int(rng.integers(0, 200))
        taken = rng.random(nfeat) < 0.2
        cands = []
        for p in range(npts):
            k = int(rng.integers(0, min(nfeat, 9) + 1))
            feats = rng.choice(nfeat, k, replace=False)
            cands.append([(int(rng.integers(0, 70)), int(f)) for f in feats])         # some above TH_LOW, ties in the distance
        if trial == 0:                                                                  # the longest chain: point p wants feature p, then p + 1
            nfeat, npts = 64, 64
            taken = np.zeros(nfeat, bool)
            cands = [[(10, 0)]] + [[(10, p - 1), (20, p)] for p in range(1, npts)]
        best, nm, sweeps = M.debug_claim_in_order(cands, taken)
        want = T.claim_in_order(cands, taken)
        assert np.array_equal(best, want) and nm == (want >= 0).sum()
        assert 1 <= sweeps <= npts + 1
        worst = max(worst, sweeps)
    assert worst >= 60                                                                  # the chain case needed a sweep per point


# ---- the conditions the fixtures meet (the checker alone) --------------------------------------------------------------------------------
def test_fixture_conditions_search_by_sim3():
    P, r = K.problem(), K.expected_sim3()
    codes = [T.MATCHED, T.NOT_CANDIDATE, T.BEHIND, T.OUT_OF_IMAGE, T.OUT_OF_RANGE, T.NO_FEATURE_IN_WINDOW, T.ABOVE_THRESHOLD, T.NOT_MUTUAL]
    for side in ("reason1", "reason2"):
        assert (np.bincount(r[side], minlength=9)[codes] >= 5).all(), np.bincount(r[side], minlength=9)
        assert (r[side] == T.VIEW_ANGLE).sum() == 0
    assert len(P["kf1"]["kps"]) == 1000 and r["nfound"] >= 100 and r["nfound"] == (r["match12"] >= 0).sum()
    assert (r["reason1"] == T.NOT_MUTUAL).sum() >= 10
    for s in ("kf1", "kf2"):
        assert ((P[s]["already"] != 0) & (P[s]["has_point"] != 0)).sum() >= 10
    hit = r["match12"] >= 0
    assert (r["match12"][hit] == P["truth12"][hit]).mean() > 0.95                      # the matches are the true partners


def test_fixture_conditions_search_by_projection():
    o, u = K.expected_projection(True), K.expected_projection(False)
    assert (np.bincount(o["reason"], minlength=9)[:8] >= 5).all(), np.bincount(o["reason"], minlength=9)
    differ = o["best_idx"] != u["best_idx"]
    assert differ.sum() >= 20 and (differ & (o["best_idx"] >= 0)).sum() >= 5
    got = o["best_idx"][o["best_idx"] >= 0]
    assert len(np.unique(got)) == len(got) and not K.problem()["loop"]["feat_taken"][got].any()       # a feature is taken once
    shape = M.shape()
    P = K.problem()
    j = P["loop"]["source"][-1]
    assert (o["best_idx"][P["loop"]["source"] == j] >= 0).sum() > shape[2]               # more claims on one window than a list holds


def test_fixture_conditions_fuse():
    fs = K.expected_fuse()
    assert len(fs) == 3
    for f in fs:
        assert f["nfused"] >= 100 and (np.bincount(f["reason"], minlength=9)[:8] >= 5).all()
    V = K.problem()["fuse"]["valid"]
    assert (V[0] != V[1]).any() and (V[1] != V[2]).any()


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def _code(fn, *a, **k):
    with pytest.raises(viorb_amd.ViorbError) as e:
        fn(*a, **k)
    return e.value.code


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    P = K.problem()
    cam, a, b, Lp = K.lib_camera(P), P["kf1"], P["kf2"], P["loop"]
    sim3 = lambda **kw: M.search_by_sim3(a, b, P["R12"], P["t12"], P["s12"], kw.pop("cam", cam), kw.pop("bounds", P["bounds4"]), **kw)
    proj = lambda **kw: M.search_by_projection_sim3(a["kps"], a["desc"], Lp["Scw"], Lp["pts_f"], Lp["pts_desc"], Lp["valid"], Lp["feat_taken"],
                                                    kw.pop("cam", cam), kw.pop("bounds", P["bounds4"]), **kw)
    fuse = lambda **kw: M.fuse_sim3(a["kps"], a["desc"], Lp["Scw"], Lp["pts_f"], Lp["pts_desc"], Lp["valid"], kw.pop("cam", cam),
                                    kw.pop("bounds", P["bounds4"]), **kw)
    bad_cam = M.camera(P["intr4"], P["sf"]); bad_cam.nlevels = 17
    for fn in (sim3, proj, fuse):
        assert _code(fn, th=0.0) == capi.ERR_INVALID_ARG and _code(fn, th=-1.0) == capi.ERR_INVALID_ARG
        assert _code(fn, cam=bad_cam) == capi.ERR_INVALID_ARG
        assert _code(fn, bounds=[0, 0, 0, 480]) == capi.ERR_INVALID_ARG
    big = np.zeros(M.MAX_FEATURES + 1, capi.KP_DTYPE)
    assert _code(M.keyframe_grid, big, P["bounds4"]) == capi.ERR_CAPACITY
    assert _code(M.fuse_sim3, big, np.zeros((len(big), 32), np.uint8), Lp["Scw"], Lp["pts_f"], Lp["pts_desc"], Lp["valid"], cam, P["bounds4"]) == capi.ERR_CAPACITY
    assert _code(M.keyframe_grid, a["kps"], [0, 752, 480, 480]) == capi.ERR_INVALID_ARG
    # the device entries: every refusal comes before any GPU call, so it needs no device and no valid pointer
    one = C.c_void_p(256)
    kf = capi.S3mKeyframes(one, one, one, one, one, 100)
    side = capi.S3mSide(kf, one, one, one, one, one)
    bounds, ws = capi.ptr(np.asarray(P["bounds4"], f32)), C.c_void_p(4096)
    wb = L.viorb_sim3_match_workspace_bytes(100, 50, 2)
    assert wb > 0 and L.viorb_sim3_match_workspace_bytes(0, 50, 2) == 0 and L.viorb_sim3_match_workspace_bytes(100, 50, 65536) == 0
    assert L.viorb_sim3_match_workspace_bytes(M.MAX_FEATURES + 1, 50, 1) == 0

    def dev_sim3(s1=side, s2=side, R=one, th=7.5, batch=2, m12=one, w=ws, bytes_=wb):
        return L.viorb_search_by_sim3_device(C.byref(s1), C.byref(s2), R, one, one, C.byref(cam), bounds, th, batch, m12, one, None, None, None, None, w, bytes_, None)

    def dev_proj(k=kf, S=one, pcap=50, th=10.0, batch=2, w=ws, bytes_=wb):
        return L.viorb_search_by_projection_sim3_device(C.byref(k), S, one, one, one, one, pcap, one, C.byref(cam), bounds, th, batch, one, one, None, w, bytes_, None)

    def dev_fuse(k=kf, S=one, npts=50, pcap=50, th=4.0, batch=2, w=ws, bytes_=wb):
        return L.viorb_fuse_sim3_device(C.byref(k), S, one, one, one, npts, pcap, C.byref(cam), bounds, th, batch, one, one, None, w, bytes_, None)

    def dev_grid(kps=one, cap=100, batch=2):
        return L.viorb_keyframe_grid_device(kps, one, cap, batch, bounds, one, one, None)
    kf0 = capi.S3mKeyframes(one, one, one, one, one, 0)
    kf_null = capi.S3mKeyframes(one, None, one, one, one, 100)
    kf_big = capi.S3mKeyframes(one, one, one, one, one, M.MAX_FEATURES + 1)
    INV, CAPY = capi.ERR_INVALID_ARG, capi.ERR_CAPACITY
    assert dev_sim3(R=None) == INV and dev_sim3(m12=None) == INV and dev_sim3(th=0.0) == INV and dev_sim3(batch=0) == INV and dev_sim3(batch=65536) == INV
    assert dev_sim3(s1=capi.S3mSide(kf0, one, one, one, one, one)) == INV and dev_sim3(s2=capi.S3mSide(kf, one, None, one, one, one)) == INV
    assert dev_sim3(s1=capi.S3mSide(kf_big, one, one, one, one, one)) == CAPY
    assert dev_sim3(w=None) == INV and dev_sim3(bytes_=64) == INV and dev_sim3(w=C.c_void_p(4097)) == INV
    assert dev_proj(S=None) == INV and dev_proj(pcap=0) == INV and dev_proj(th=0.0) == INV and dev_proj(batch=0) == INV and dev_proj(batch=65536) == INV
    assert dev_proj(k=kf0) == INV and dev_proj(k=kf_null) == INV and dev_proj(k=kf_big) == CAPY and dev_proj(bytes_=64) == INV
    assert dev_fuse(S=None) == INV and dev_fuse(pcap=0) == INV and dev_fuse(npts=51) == INV and dev_fuse(npts=-1) == INV and dev_fuse(th=-2.0) == INV
    assert dev_fuse(batch=0) == INV and dev_fuse(k=kf0) == INV and dev_fuse(k=kf_big) == CAPY and dev_fuse(bytes_=64) == INV
    assert dev_grid(kps=None) == INV and dev_grid(cap=0) == INV and dev_grid(batch=0) == INV and dev_grid(batch=65536) == INV
    assert dev_grid(cap=M.MAX_FEATURES + 1) == CAPY
    if L.viorb_device_count() < 1:
        ND = capi.ERR_NO_DEVICE
        assert dev_sim3() == ND and dev_proj() == ND and dev_fuse() == ND and dev_grid() == ND
        assert _code(sim3) == ND and _code(proj) == ND and _code(fuse) == ND and _code(M.keyframe_grid, a["kps"], P["bounds4"]) == ND
