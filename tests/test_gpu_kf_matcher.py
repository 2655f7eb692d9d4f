"""GPU parity (bit-exact) of ORBmatcher::SearchForTriangulation and ORBmatcher::Fuse (csrc/bow_matcher.hip, frontend_kernels.hip)
against the oracle (oracle/kf_matcher.cpp)."""
import ctypes as C
import numpy as np
import pytest
from viorb_amd.synth import make_two_view_problem, local_points_f32
import kf_matcher_cases as K

pytestmark = pytest.mark.gpu


def _tri_args(p, only_stereo, ori):
    return K.tri_args(dict(p=p, only_stereo=only_stereo, ori=ori))


@pytest.mark.parametrize("seed,n1,n2,nc,stereo,only_stereo,ori", [(0, 900, 950, 500, 0.0, False, True), (1, 1000, 1000, 600, 0.4, False, False),
                                                                    (2, 2000, 1900, 1100, 0.6, True, True), (3, 40, 1200, 30, 0.0, False, True),
                                                                    (4, 700, 1, 1, 0.0, False, True)])
def test_search_for_triangulation_bit_exact(oracle, seed, n1, n2, nc, stereo, only_stereo, ori):
    from viorb_amd import SearchForTriangulation
    p = make_two_view_problem(seed, n1, n2, nc, stereo_frac=stereo)
    args = (p["k1"], p["d1"], p["hp1"], p["ur1"], p["node1"], p["k2"], p["d2"], p["hp2"], p["ur2"], p["node2"], p["F12"], p["Cw1"], p["pose2"], p["intr4"],
            p["sf"], p["level_sigma2"], only_stereo, ori)
    n_ref, m_ref = oracle.search_for_triangulation(*args)
    n, m = SearchForTriangulation(*args)
    assert n == n_ref and np.array_equal(m, m_ref)
    if nc >= 500:
        assert n > 50


def _fuse_problem(seed, stereo):
    p = make_two_view_problem(seed, 1000, 1100, 700, stereo_frac=stereo)
    rng = np.random.default_rng(seed)
    # map points: the common 3-D points (created from key frame 1) + random ones; descriptors = key frame 2's nearest keypoint's, with noise
    R2, t2 = p["pose2"][:9].reshape(3, 3).astype(np.float64), p["pose2"][9:].astype(np.float64)
    fx, fy, cx, cy = [float(v) for v in p["intr4"]]
    X = np.concatenate([p["X"], np.stack([rng.uniform(-4, 4, 300), rng.uniform(-3, 3, 300), rng.uniform(1, 15, 300)], 1)])
    uv2 = (R2 @ X.T).T + t2; uv2 = np.stack([fx * uv2[:, 0] / uv2[:, 2] + cx, fy * uv2[:, 1] / uv2[:, 2] + cy], 1)
    k2xy = np.stack([p["k2"]["x"], p["k2"]["y"]], 1).astype(np.float64)
    partner = np.array([int(np.argmin(((k2xy - q) ** 2).sum(1))) for q in uv2])
    pts_f = local_points_f32(p["k2"]["octave"][partner], p["pose1"].astype(np.float64), X.astype(np.float32), p["sf"])
    valid = (rng.random(len(X)) < 0.9).astype(np.uint8)
    desc = p["d2"][partner].copy()
    for _ in range(8):
        b = rng.integers(0, 256, len(X)); desc[np.arange(len(X)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    intr5 = np.concatenate([p["intr4"], [np.float32(40.0)]]).astype(np.float32)
    return p, pts_f, valid, desc, intr5


@pytest.mark.parametrize("seed,stereo,th", [(5, 0.0, 3.0), (6, 0.5, 3.0), (7, 0.0, 10.0)])
def test_fuse_bit_exact(oracle, seed, stereo, th):
    from viorb_amd import Fuse
    p, pts_f, valid, desc, intr5 = _fuse_problem(seed, stereo)
    log_sf = np.float32(np.log(np.float64(p["sf"][1])))
    bounds = (0.0, 752.0, 0.0, 480.0)
    n_ref, b_ref = oracle.fuse(p["k2"], p["d2"], p["ur2"], bounds, p["pose2"], intr5, p["sf"], p["inv_level_sigma2"], log_sf, pts_f, valid, desc, th)
    n, b = Fuse(p["k2"], p["d2"], p["ur2"], bounds, p["pose2"], intr5, p["sf"], p["inv_level_sigma2"], pts_f, valid, desc, th)
    assert n == n_ref and np.array_equal(b, b_ref)
    assert n > 100


# ---- hand-built cases (tests/kf_matcher_cases.py): each decides the rules it names, proved on the CPU by tests/test_kf_matcher_cases.py ------------
@pytest.mark.parametrize("ori", [False, True])
@pytest.mark.parametrize("name", sorted(K.TRI_CASES))
def test_search_for_triangulation_case(oracle, name, ori):
    from viorb_amd import SearchForTriangulation
    args = K.tri_args(K.TRI_CASES[name](), ori)
    n_ref, m_ref = oracle.search_for_triangulation(*args)
    n, m = SearchForTriangulation(*args)
    assert n == n_ref and np.array_equal(m, m_ref)


@pytest.mark.parametrize("name", sorted(K.FUSE_CASES))
def test_fuse_case(oracle, name):
    from viorb_amd import Fuse
    c = K.FUSE_CASES[name](); p = c["p"]
    n_ref, b_ref = K.fuse_oracle(oracle, c)
    n, b = Fuse(p["k2"], p["d2"], p["ur2"], c["bounds4"], p["pose2"], c["intr5"], p["sf"], p["inv_level_sigma2"], c["pts_f"], c["valid"], c["desc"], c["th"])
    assert n == n_ref and np.array_equal(b, b_ref)


# ---- batched device entry points ---------------------------------------------------------------------------------------------------------------
def test_search_for_triangulation_batched_device(oracle):
    """viorb_search_for_triangulation_device, 6 pairs of different sizes in one launch: the b * cap offsets, the per-pair F12 / Cw1 / pose2
    strides (one pair has F12 = 0 between pairs that match) and the -1 fill of the rows from a pair's count to cap."""
    import torch
    from viorb_amd import lib, KP_DTYPE
    from viorb_amd.capi import check, ptr, _torch_up as up
    cap, B = 1100, 6
    sizes = [(900, 1000), (cap, cap), (1, cap), (cap, 1), (0, 50), (50, 0)]
    shape = [(900, 1000, 500), (cap, cap, 600), (1, cap, 1), (cap, 1, 1), (50, 50, 20), (50, 50, 20)]
    k = [np.zeros((B, cap), KP_DTYPE) for _ in range(2)]; d = [np.zeros((B, cap, 32), np.uint8) for _ in range(2)]
    hp = [np.zeros((B, cap), np.uint8) for _ in range(2)]; ur = [np.full((B, cap), -1, np.float32) for _ in range(2)]
    node = [np.full((B, cap), -1, np.int32) for _ in range(2)]
    F, Cw, pose = np.zeros((B, 9), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 12), np.float32)
    refs = []
    for b, ((n1, n2), (m1, m2, nc)) in enumerate(zip(sizes, shape)):
        p = make_two_view_problem(60 + b, m1, m2, nc, stereo_frac=0.3)
        if nc == 1:                                                # the single planted pair is free to match: no map points, a node, mono
            i1, i2 = int(np.argmax(p["truth12"] >= 0)), int(p["truth12"].max())
            p["hp1"][i1] = p["hp2"][i2] = 0; p["node1"][i1] = p["node2"][i2] = 7; p["ur1"][i1] = p["ur2"][i2] = -1
        if (n1, n2) == (cap, 1):
            assert oracle.search_for_triangulation(*_tri_args(p, False, True))[0] == 1
            p["F12"] = np.zeros((3, 3), np.float32)                # den == 0: no match, whatever the neighbours' F12 say
        for s in (0, 1):
            m = (m1, m2)[s]; t = str(s + 1)
            k[s][b, :m], d[s][b, :m], hp[s][b, :m], ur[s][b, :m], node[s][b, :m] = p["k" + t], p["d" + t], p["hp" + t], p["ur" + t], p["node" + t]
        F[b], Cw[b], pose[b] = p["F12"].ravel(), p["Cw1"], p["pose2"]
        q = dict(p)
        for s, n in (("1", n1), ("2", n2)):
            for key in ("k", "d", "hp", "ur", "node"):
                q[key + s] = p[key + s][:n]
        refs.append(oracle.search_for_triangulation(*_tri_args(q, False, True)) if n1 and n2 else (0, np.full(n1, -1, np.int32)))
    assert refs[0][0] > 50 and refs[1][0] > 50 and refs[2][0] == 1 and refs[3][0] == 0
    t = [up(x) for x in (k[0], d[0], hp[0], ur[0], node[0])] + [torch.tensor([s[0] for s in sizes], dtype=torch.int32, device="cuda")] + \
        [up(x) for x in (k[1], d[1], hp[1], ur[1], node[1])] + [torch.tensor([s[1] for s in sizes], dtype=torch.int32, device="cuda")] + [up(F), up(Cw), up(pose)]
    match = torch.full((B, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    intr4, sf, sig2 = [np.ascontiguousarray(p[key], np.float32) for key in ("intr4", "sf", "level_sigma2")]
    check(lib().viorb_search_for_triangulation_device(*[ptr(x) for x in t], ptr(intr4), ptr(sf), ptr(sig2), len(sf), 0, 1, cap, B, ptr(match), ptr(nm),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    match, nm = match.cpu().numpy(), nm.cpu().numpy()
    for b, (n1, n2) in enumerate(sizes):
        assert nm[b] == refs[b][0] and np.array_equal(match[b, :n1], refs[b][1]) and (match[b, n1:] == -1).all(), b


def test_fuse_batched_device(oracle):
    """viorb_frontend_fuse_device, 4 key frames on one Frontend handle (lens bounds): the b * cap and b * pcap offsets, the per-key-frame pose
    and cell table, point counts 0, 1, pcap and an ordinary one, -1 beyond a count."""
    import torch
    from viorb_amd import lib, KP_DTYPE, Frontend
    from viorb_amd.capi import check, ptr, _torch_up as up
    B, cap, th = 4, 400, 2.0
    cases = [K.fuse_lens_bounds()] + [K._Fuse(30 + b, stereo=0.3 * (b % 2), th=th, bounds4=K.LENS_BOUNDS).case(()) for b in (1, 2, 3)]
    pcap = len(cases[0]["pts_f"])
    counts = [pcap, 0, 1, 150]
    p0 = cases[0]["p"]
    cam16 = np.zeros(16); cam16[:4] = p0["intr4"]
    fe = Frontend(cam16, [0, 0, -9.81], p0["sf"], p0["inv_level_sigma2"], bounds=K.LENS_BOUNDS, max_batch=B, cap=cap)
    kps = np.zeros((B, cap), KP_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); ur = np.full((B, cap), -1, np.float32)
    pose = np.zeros((B, 12), np.float32); pts = np.zeros((B, pcap, 8), np.float32); pv = np.zeros((B, pcap), np.uint8); pd = np.zeros((B, pcap, 32), np.uint8)
    refs = []
    for b, (c, npts) in enumerate(zip(cases, counts)):
        p = c["p"]; n = len(p["k2"]); m = len(c["pts_f"])
        assert n <= cap and npts <= m <= pcap
        kps[b, :n], desc[b, :n], ur[b, :n], pose[b] = p["k2"], p["d2"], p["ur2"], p["pose2"]
        order = np.arange(m)
        if npts == 1:                                              # the one point is one that fuses
            order[0] = int(np.argmax(K.fuse_oracle(oracle, c)[1] >= 0))
        pts[b, :m], pv[b, :m], pd[b, :m] = c["pts_f"][order], c["valid"][order], c["desc"][order]      # rows beyond the count hold live data that must be ignored
        cut = dict(c, pts_f=pts[b, :npts], valid=pv[b, :npts], desc=pd[b, :npts])
        refs.append(K.fuse_oracle(oracle, cut) if npts else (0, np.zeros(0, np.int32)))
    assert refs[0][0] > 100 and refs[2][0] == 1 and refs[3][0] > 30
    t = [up(x) for x in (kps, desc, ur)]
    cnt = torch.tensor([len(c["p"]["k2"]) for c in cases], dtype=torch.int32, device="cuda")
    cs = torch.zeros((B, 3073), dtype=torch.int32, device="cuda"); ci = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    fe.grid(t[0].data_ptr(), cnt.data_ptr(), B, cs, ci)
    e = [up(x) for x in (pose, pts, pv, pd)] + [torch.tensor(counts, dtype=torch.int32, device="cuda")]
    best = torch.full((B, pcap), -7, dtype=torch.int32, device="cuda"); nf = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    check(lib().viorb_frontend_fuse_device(fe.h, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(cnt), ptr(cs), ptr(ci), ptr(e[0]), ptr(e[1]), ptr(e[2]), ptr(e[3]), ptr(e[4]),
                                           pcap, th, float(cases[0]["intr5"][4]), B, ptr(best), ptr(nf), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    best, nf = best.cpu().numpy(), nf.cpu().numpy()
    for b, npts in enumerate(counts):
        assert nf[b] == refs[b][0] and np.array_equal(best[b, :npts], refs[b][1]) and (best[b, npts:] == -1).all(), b


# ---- LDS launch paths of k_search_triangulation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,nc", [(4100, 3000, 1500), (2500, 4100, 1500), (16384, 16384, 6000)])
def test_search_for_triangulation_large_lds(oracle, n1, n2, nc):
    """max(n1, n2) = 4100 is the smallest cap whose LDS plan (sort_n = 8192) exceeds 64 KB; 16384 is the API limit (147 712 B)."""
    from viorb_amd import SearchForTriangulation
    args = _tri_args(make_two_view_problem(8, n1, n2, nc, stereo_frac=0.3), False, True)
    n_ref, m_ref = oracle.search_for_triangulation(*args)
    n, m = SearchForTriangulation(*args)
    assert n == n_ref and np.array_equal(m, m_ref) and n > 100


def test_search_for_triangulation_refuses_more_than_the_limit():
    """16385 features: an error and match12 all -1, never a truncated result."""
    from viorb_amd import lib, ViorbError
    from viorb_amd.capi import check, ptr
    n = 16385
    p = make_two_view_problem(9, n, n, 4000)
    f32 = lambda a: np.ascontiguousarray(a, np.float32); i32 = lambda a: np.ascontiguousarray(a, np.int32)
    m = np.full(n, -7, np.int32); nm = C.c_int(-7)
    rc = lib().viorb_search_for_triangulation(ptr(p["k1"]), ptr(p["d1"]), ptr(p["hp1"]), ptr(f32(p["ur1"])), ptr(i32(p["node1"])), n, ptr(p["k2"]), ptr(p["d2"]),
                                              ptr(p["hp2"]), ptr(f32(p["ur2"])), ptr(i32(p["node2"])), n, ptr(f32(p["F12"])), ptr(p["Cw1"]), ptr(p["pose2"]),
                                              ptr(p["intr4"]), ptr(p["sf"]), ptr(p["level_sigma2"]), len(p["sf"]), 0, 1, ptr(m), C.byref(nm))
    with pytest.raises(ViorbError):
        check(rc)
    assert (m == -1).all() and nm.value == 0
