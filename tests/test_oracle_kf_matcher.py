"""Pins the oracle's SearchForTriangulation and Fuse restatements (oracle/kf_matcher.cpp) with literal numpy / pure-Python
re-derivations (no reference vectors exist: parity unpinned, see oracle/kf_matcher.h). The literals live in tests/kf_matcher_ref.py."""
import numpy as np
import pytest
from viorb_amd.synth import make_two_view_problem, local_points_f32
from kf_matcher_ref import literal_triangulation, literal_fuse


@pytest.mark.parametrize("seed,stereo,only_stereo,ori", [(0, 0.0, False, True), (1, 0.4, False, False), (2, 0.6, True, True)])
def test_search_for_triangulation_matches_literal(oracle, seed, stereo, only_stereo, ori):
    p = make_two_view_problem(seed, 400, 430, 220, stereo_frac=stereo)
    n, m = oracle.search_for_triangulation(p["k1"], p["d1"], p["hp1"], p["ur1"], p["node1"], p["k2"], p["d2"], p["hp2"], p["ur2"], p["node2"],
                                           p["F12"], p["Cw1"], p["pose2"], p["intr4"], p["sf"], p["level_sigma2"], only_stereo, ori)
    n2, m2 = literal_triangulation(p, only_stereo, ori)
    assert n == n2 and np.array_equal(m, m2)
    good = (m >= 0) & (m == p["truth12"])
    assert n > 20 and good.sum() >= 0.9 * n                       # the planted correspondences (free of map points) are what it finds


def test_fuse_finds_the_planted_points(oracle):
    """Map points = the 3-D points seen by key frame 1; fused into key frame 2 they must land on the keypoints that observe them."""
    p = make_two_view_problem(5, 600, 640, 400)
    nc = len(p["X"])
    inv = np.full(len(p["k2"]), -1); t12 = p["truth12"]
    # truth: point j (common index) <-> key frame 2 feature; recover from truth12 through key frame 1's permutation
    src1 = np.nonzero(t12 >= 0)[0]
    Pw = np.zeros((len(src1), 3), np.float32)
    # world points of the common features, in key frame 1 feature order: back-project with the known geometry is not needed — use X through the planted order
    # (make_two_view_problem keeps X in planted order; truth12[p1] pairs feature i1 with its key frame 2 partner, X index = rank in the unpermuted order)
    R2, tt2 = p["pose2"][:9].reshape(3, 3).astype(np.float64), p["pose2"][9:].astype(np.float64)
    fx, fy, cx, cy = [float(v) for v in p["intr4"]]
    # identify each common 3-D point's key frame 2 feature by projecting X and taking the nearest key frame 2 keypoint
    uv2 = (R2 @ p["X"].T).T + tt2; uv2 = np.stack([fx * uv2[:, 0] / uv2[:, 2] + cx, fy * uv2[:, 1] / uv2[:, 2] + cy], 1)
    k2xy = np.stack([p["k2"]["x"], p["k2"]["y"]], 1).astype(np.float64)
    partner = np.array([int(np.argmin(((k2xy - q) ** 2).sum(1))) for q in uv2])
    pose1_true = np.concatenate([p["pose1"][:9], p["pose1"][9:]]).astype(np.float64)
    octv = p["k2"]["octave"][partner]
    pts_f = local_points_f32(octv, pose1_true, p["X"].astype(np.float32), p["sf"])
    valid = np.ones(nc, np.uint8); valid[::17] = 0
    desc = p["d2"][partner].copy()
    rng = np.random.default_rng(1)
    for _ in range(6):
        b = rng.integers(0, 256, nc); desc[np.arange(nc), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    intr5 = np.concatenate([p["intr4"], [np.float32(40.0)]]).astype(np.float32)
    log_sf = np.float32(np.log(np.float64(p["sf"][1])))
    n, bi = oracle.fuse(p["k2"], p["d2"], p["ur2"], (0.0, 752.0, 0.0, 480.0), p["pose2"], intr5, p["sf"], p["inv_level_sigma2"], log_sf, pts_f,
                        valid, desc, 3.0)
    assert (bi[valid == 0] == -1).all()
    hit = bi[valid == 1] == partner[valid == 1]
    assert n == (bi >= 0).sum() and hit.mean() > 0.6, (n, hit.mean())     # level gate + chi gate reject some; none may land elsewhere
    assert ((bi[valid == 1] == -1) | hit).mean() > 0.97


@pytest.mark.parametrize("seed,stereo,th", [(11, 0.0, 3.0), (12, 0.5, 6.0)])
def test_fuse_matches_literal(oracle, seed, stereo, th):
    p = make_two_view_problem(seed, 300, 330, 200, stereo_frac=stereo)
    rng = np.random.default_rng(seed)
    R2, t2 = p["pose2"][:9].reshape(3, 3).astype(np.float64), p["pose2"][9:].astype(np.float64)
    fx, fy, cx, cy = [float(v) for v in p["intr4"]]
    X = np.concatenate([p["X"], np.stack([rng.uniform(-4, 4, 60), rng.uniform(-3, 3, 60), rng.uniform(1, 15, 60)], 1)])
    uv2 = (R2 @ X.T).T + t2; uv2 = np.stack([fx * uv2[:, 0] / uv2[:, 2] + cx, fy * uv2[:, 1] / uv2[:, 2] + cy], 1)
    k2xy = np.stack([p["k2"]["x"], p["k2"]["y"]], 1).astype(np.float64)
    partner = np.array([int(np.argmin(((k2xy - q) ** 2).sum(1))) for q in uv2])
    pts_f = local_points_f32(p["k2"]["octave"][partner], p["pose1"].astype(np.float64), X.astype(np.float32), p["sf"])
    valid = (rng.random(len(X)) < 0.9).astype(np.uint8)
    desc = p["d2"][partner].copy()
    for _ in range(8):
        b = rng.integers(0, 256, len(X)); desc[np.arange(len(X)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    intr5 = np.concatenate([p["intr4"], [np.float32(40.0)]]).astype(np.float32)
    log_sf = np.float32(np.log(np.float64(p["sf"][1])))
    n, bi = oracle.fuse(p["k2"], p["d2"], p["ur2"], (0.0, 752.0, 0.0, 480.0), p["pose2"], intr5, p["sf"], p["inv_level_sigma2"], log_sf, pts_f, valid, desc, th)
    n2, bi2 = literal_fuse(p, pts_f, valid, desc, intr5, th)
    assert n == n2 and np.array_equal(bi, bi2)
    assert n > 30
