"""numpy restatement of the Sim3 RANSAC solver, the checker of tests/test_sim3_ref.py and tests/test_gpu_sim3.py (never imported by
product code). Reference: Sim3Solver (src/Sim3Solver.cc:37-423).

Two modes, as tests/two_view_ref.py:
  mode "f32": the reference's own casts ("Sim3 solver" audit): float centroids and relative coordinates, M = Pr2 Pr1^T
              accumulated in double and stored to float, a float N, LAPACK's float32 symmetric eigen-solver in place of cv::eigen, the
              angle and cv::Rodrigues in double stored to float, float products in the reference's association for R Pr2, the
              projections and the translation, double only where OpenCV puts one (Mat::dot, the scale, the scalings by a double alpha).
  mode "f64": the definitional form: the same float inputs, everything after them in double.
The thresholds are the same in both modes: (size_t)(9.210 sigma2) is the reference's meaning, not a rounding.

Hypotheses are arrays over the sets; the errors are arrays [models, correspondences]."""
import numpy as np

FOUND, CONTINUE, NO_MORE, FEW = range(4)
SET_OK, SET_FEW, SET_BAD, SET_ZERO_ROTATION = range(4)
f32, f64 = np.float32, np.float64

# Measured by tests/test_sim3_ref.py::test_float32_restatement_against_float64 over PARAM_SETS (mode "f32" against mode "f64" of this
# file), rounded up; that test asserts that a fresh measurement does not exceed them and is not more than ten times below them.
#   R_DEV_F32     largest entry of |R_a - R_b| over the hypotheses whose set is not near-degenerate (gap() >= GAP_MIN)
#   T_DEV_F32     |t_a - t_b| relative to the distance of the set's centroid in camera 1 (the translation is a difference of centroids)
#   S_DEV_F32     |s_a - s_b| / s_b (0 with fix_scale: both are exactly 1)
#   ERR_DEV_F32   both squared reprojection errors per correspondence, |a - b| / max(b, threshold), both modes on the SAME float32 model
#                 (the best hypothesis of the f32 mode), over errors up to twice the threshold
R_DEV_F32 = 1.0e-5
T_DEV_F32 = 5.0e-6
S_DEV_F32 = 2.0e-7
ERR_DEV_F32 = 4.0e-5
GPU_FACTOR = 4                         # another float32-output eigen-solver: same order of backward error, other constants
BAND_FACTOR = 10                       # a flag may flip when its error is within 10 x the deviation of its threshold
MAX_BAND_SHARE_GPU, MAX_BAND_SHARE_CPU, MAX_SKIPPED_SETS = 0.02, 0.005, 0.10
# A set is near-degenerate when gap() = (lambda_1 - lambda_2) / max |lambda| of its N (f64) is below GAP_MIN: the top eigenvector of a
# perturbed N moves by about |dN| / (lambda_1 - lambda_2), so a float32 eigen-solver (|dN| of a few eps32 max |lambda|) is off by
# GAP_C eps32 / gap; the CPU suite measures deviation x gap / eps32 <= GAP_C over every hypothesis of PARAM_SETS (1.5 at most). GAP_MIN,
# derived as two_view_ref.GAP_MIN was, is the gap at which eps32 / gap reaches R_DEV_F32: below it a hypothesis cannot be compared at
# R_DEV_F32 at all. It skips 2 to 3.3 % of the sets of PARAM_SETS.
GAP_C = 2.0
GAP_MIN = float(np.finfo(np.float32).eps) / R_DEV_F32

# (seed, kind, n, outlier_frac, noise_px, noise_m) of synth.make_sim3_problem, shared by the CPU and GPU tests; 300 sets each
PARAM_SETS = [(0, "general", 300, 0.0, 0.5, 0.002), (1, "general", 300, 0.3, 0.5, 0.002), (2, "fix_scale", 300, 0.3, 0.5, 0.002),
              (3, "small_rotation", 300, 0.1, 0.5, 0.002), (4, "general", 130, 0.3, 1.0, 0.02), (5, "fix_scale", 65, 0.0, 0.3, 0.0)]
ITERATIONS = 300


def _ft(mode):
    return np.float32 if mode == "f32" else np.float64


def max_error(sigma2):
    """mvnMaxError: (size_t)(9.210 * sigma2), as the float it is compared in."""
    return np.floor(9.210 * np.asarray(sigma2, f32).astype(f64)).astype(f32)


def rodrigues(rv):
    """cv::Rodrigues of rotation vectors [..., 3], in double."""
    rv = np.asarray(rv, f64)
    th = np.linalg.norm(rv, axis=-1)
    small = th < np.finfo(f64).eps
    r = rv / np.where(small, 1.0, th)[..., None]
    c, s = np.cos(th)[..., None, None], np.sin(th)[..., None, None]
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    zero = np.zeros_like(x)
    K = np.stack([np.stack([zero, -z, y], -1), np.stack([z, zero, -x], -1), np.stack([-y, x, zero], -1)], -2)
    R = c * np.eye(3) + (1 - c) * (r[..., :, None] * r[..., None, :]) + s * K
    R[small] = np.eye(3)
    return R


def _mul3(R, X, FT):
    """(R[.., r, 0] X0 + R[.., r, 1] X1) + R[.., r, 2] X2 in FT, the small-matrix gemm association. R [..., 3, 3], X [..., 3] broadcast."""
    R, X = np.asarray(R, FT), np.asarray(X, FT)
    return (R[..., :, 0] * X[..., None, 0] + R[..., :, 1] * X[..., None, 1]) + R[..., :, 2] * X[..., None, 2]


def horn(P1, P2, fix_scale, mode):
    """ComputeSim3 for sets of three correspondences: P1, P2 [S, 3 points, 3]. dict of R [S,3,3], t [S,3], s [S], reason [S], gap [S]
    (f64 eigenvalue gap of this mode's N), O1n [S] (distance of the centroid in camera 1)."""
    FT = _ft(mode)
    P1, P2 = np.asarray(P1, f32).astype(FT).reshape(-1, 3, 3), np.asarray(P2, f32).astype(FT).reshape(-1, 3, 3)

    def centroid(P):
        ssum = (P[:, 0] + P[:, 1]) + P[:, 2]
        return (ssum.astype(f64) * (1.0 / 3)).astype(FT)
    O1, O2 = centroid(P1), centroid(P2)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = np.einsum("sir,sic->src", Pr2.astype(f64), Pr1.astype(f64)).astype(FT)
    N = np.empty((len(M), 4, 4), FT)
    m = lambda r, c: M[:, r, c]
    N[:, 0, 0] = m(0, 0) + m(1, 1) + m(2, 2)
    N[:, 0, 1] = N[:, 1, 0] = m(1, 2) - m(2, 1)
    N[:, 0, 2] = N[:, 2, 0] = m(2, 0) - m(0, 2)
    N[:, 0, 3] = N[:, 3, 0] = m(0, 1) - m(1, 0)
    N[:, 1, 1] = m(0, 0) - m(1, 1) - m(2, 2)
    N[:, 1, 2] = N[:, 2, 1] = m(0, 1) + m(1, 0)
    N[:, 1, 3] = N[:, 3, 1] = m(2, 0) + m(0, 2)
    N[:, 2, 2] = -m(0, 0) + m(1, 1) - m(2, 2)
    N[:, 2, 3] = N[:, 3, 2] = m(1, 2) + m(2, 1)
    N[:, 3, 3] = -m(0, 0) - m(1, 1) + m(2, 2)
    w, v = np.linalg.eigh(N)
    q = v[:, :, 3].astype(FT)
    w64 = np.linalg.eigvalsh(N.astype(f64))
    gap = (w64[:, 3] - w64[:, 2]) / np.maximum(np.abs(w64).max(1), np.finfo(f64).tiny)
    nv = np.sqrt((q[:, 1:].astype(f64) ** 2).sum(1))
    zero = nv == 0
    ang = np.arctan2(nv, q[:, 0].astype(f64))
    rv = ((2 * ang / np.where(zero, 1.0, nv))[:, None] * q[:, 1:].astype(f64)).astype(FT)
    R = rodrigues(rv).astype(FT)
    P3 = _mul3(R[:, None], Pr2, FT)                                  # [S, point, coord]
    if fix_scale:
        s = np.ones(len(R), FT)
    else:
        nom = (Pr1.astype(f64) * P3.astype(f64)).sum((1, 2))
        den = (P3 * P3).astype(f64).sum((1, 2))
        with np.errstate(all="ignore"):
            s = (nom / den).astype(FT)
    ro = _mul3(R, O2, FT)
    t = O1 - (ro.astype(f64) * s.astype(f64)[:, None]).astype(FT)
    reason = np.where(zero, SET_ZERO_ROTATION, SET_OK)
    R[zero], t[zero], s[zero] = 0, 0, 0
    return dict(R=R, t=t, s=s, reason=reason, gap=gap, O1n=np.linalg.norm(O1.astype(f64), axis=1))


def hypotheses(prob, sets, fix_scale, mode):
    sets = np.asarray(sets).reshape(-1, 3)
    return horn(np.asarray(prob["X1c"], f32)[sets], np.asarray(prob["X2c"], f32)[sets], fix_scale, mode)


def to_image(K, X, FT):
    """FromCameraToImage: 1 / z in FT, no depth test. X [..., 3] -> [..., 2]."""
    K, X = np.asarray(K, f32).astype(FT), np.asarray(X, FT)
    with np.errstate(all="ignore"):
        invz = FT(1) / X[..., 2]
        return np.stack([K[0] * (X[..., 0] * invz) + K[2], K[1] * (X[..., 1] * invz) + K[3]], -1)


def errors(R, t, s, prob, mode):
    """CheckInliers' err1, err2 [S, n] of models R [S,3,3], t [S,3], s [S] (float32 values) over the correspondences of prob."""
    FT = _ft(mode)
    R, t, s = np.asarray(R, f32).reshape(-1, 3, 3), np.asarray(t, f32).reshape(-1, 3), np.asarray(s, f32).reshape(-1)
    X1, X2 = np.asarray(prob["X1c"], f32).astype(FT), np.asarray(prob["X2c"], f32).astype(FT)
    p1, p2 = to_image(prob["K1"], X1, FT), to_image(prob["K2"], X2, FT)
    with np.errstate(all="ignore"):
        sR12 = (R.astype(f64) * s.astype(f64)[:, None, None]).astype(FT)
        sR21 = (np.swapaxes(R, 1, 2).astype(f64) * (1.0 / s.astype(f64))[:, None, None]).astype(FT)
        t12 = t.astype(FT)
        t21 = -_mul3(sR21, t12, FT)
        q1 = to_image(prob["K1"], _mul3(sR12[:, None], X2[None], FT) + t12[:, None], FT)        # X2 in image 1
        q2 = to_image(prob["K2"], _mul3(sR21[:, None], X1[None], FT) + t21[:, None], FT)        # X1 in image 2
        d1, d2 = p1[None] - q1, q2 - p2[None]
        e1 = (d1.astype(f64) ** 2).sum(-1).astype(FT)
        e2 = (d2.astype(f64) ** 2).sum(-1).astype(FT)
    return e1, e2


def flags_of(e1, e2, prob):
    """The inlier decision of :356 (a NaN error is no inlier)."""
    m1, m2 = max_error(prob["sigma2_1"]), max_error(prob["sigma2_2"])
    with np.errstate(invalid="ignore"):
        return (e1 < m1[None].astype(e1.dtype)) & (e2 < m2[None].astype(e2.dtype))


def err_band(e1, e2, prob, dev):
    """Correspondences whose decision may flip: an error within BAND_FACTOR x dev of its threshold (relative to the threshold)."""
    m1, m2 = max_error(prob["sigma2_1"]).astype(f64)[None], max_error(prob["sigma2_2"]).astype(f64)[None]
    with np.errstate(invalid="ignore"):
        return (np.abs(e1.astype(f64) - m1) <= BAND_FACTOR * dev * m1) | (np.abs(e2.astype(f64) - m2) <= BAND_FACTOR * dev * m2)


def ransac_iterations(n, probability, min_inliers, max_iterations):
    """SetRansacParameters; max_iterations where the formula has no value (n < min_inliers)."""
    eps = f32(min_inliers) / f32(n)
    if min_inliers == n:
        its = 1
    else:
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(1 - probability) / np.log(1 - np.power(f64(eps), 3)))
        its = int(v) if v < max_iterations else max_iterations
    return max(1, min(its, max_iterations))


def select(counts, N, min_inliers, max_its, first=0, best=0, per_call=5):
    """The loop of iterate over given counts: (status, iterations_done, best_inliers, best_iter)."""
    if N < min_inliers:
        return FEW, first, best, -1
    it, cur, best_iter = max(first, 0), 0, -1
    stop = min(max_its, len(counts))
    while it < stop and cur < per_call:
        c = int(counts[it])
        cur += 1; it += 1
        if c >= best:
            best, best_iter = c, it - 1
            if c > min_inliers:
                return FOUND, it, best, best_iter
    return (NO_MORE if it >= max_its else CONTINUE), it, best, best_iter


def ransac(prob, sets, mode, min_inliers=20, fix_scale=False, max_its=None, first=0, best=0, per_call=5):
    """Sim3Solver::iterate once: dict(status, iterations_done, best_inliers, best_iter, R12, t12, s12, n_inliers, inliers, hyp, counts)."""
    sets = np.asarray(sets).reshape(-1, 3)
    n = len(np.asarray(prob["X1c"]).reshape(-1, 3))
    max_its = len(sets) if max_its is None else max_its
    r = dict(status=FEW, iterations_done=first, best_inliers=best, best_iter=-1, n_inliers=0, inliers=np.zeros(n, np.uint8))
    if n < min_inliers:
        return r
    hyp = hypotheses(prob, sets, fix_scale, mode)
    e1, e2 = errors(hyp["R"].astype(f32), hyp["t"].astype(f32), hyp["s"].astype(f32), prob, mode)
    fl = flags_of(e1, e2, prob)
    counts = fl.sum(1)
    st, done, b, bi = select(counts, n, min_inliers, max_its, first, best, per_call)
    r.update(status=st, iterations_done=done, best_inliers=b, best_iter=bi, hyp=hyp, counts=counts, flags=fl)
    if bi >= 0:
        r.update(R12=hyp["R"][bi], t12=hyp["t"][bi], s12=hyp["s"][bi])
    if st == FOUND:
        r.update(n_inliers=int(counts[bi]), inliers=fl[bi].astype(np.uint8))
    return r


# ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:4589-4784), in double --------------------------------------------------------------------
# A Sim3 is (q = x y z w, t, s). Two Jacobian modes: "numeric", g2o's own (the Sim3 edges define no linearizeOplus: central differences
# with delta = 1e-9 through oplus, base_binary_edge.hpp:123-200), which is the reference form, and "analytic", used only to measure how
# far the rounding of the differences can move the result.
# Measured by tests/test_sim3_ref.py::test_optimiser_numeric_against_analytic over OPT_CASES and OPT_CASES_FLOOR, rounded up (the same rule as above):
#   OPT_S_DEV     largest entry of |S12_numeric - S12_analytic| (r, t, s as eight numbers; t is in metres at depths of 2 to 10)
#   OPT_CHI_DEV   |chi2_numeric - chi2_analytic| / chi2 after the second round
#   OPT_EDGE_DEV  |chi2_numeric - chi2_analytic| / th2 of one edge's stored chi2, over values up to twice th2 (the decision bands of keep)
OPT_S_DEV = 1.0e-8
OPT_CHI_DEV = 1.0e-9
OPT_EDGE_DEV = 1.0e-6
CHI2_TOL = 1e-5                        # the project's own bar for a solver's final chi2, relative (README)
OPT_DELTA = 1e-9
OPT_SIZES = (9, 10, 63, 64, 65, 257)


def _hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], f64)


def mat2q(m):
    """Eigen's Quaterniond(Matrix3d), coefficients x y z w."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        s = np.sqrt(t + 1.0); r = 0.5 / s
        return np.array([(m[2, 1] - m[1, 2]) * r, (m[0, 2] - m[2, 0]) * r, (m[1, 0] - m[0, 1]) * r, 0.5 * s])
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0); r = 0.5 / s
    q = np.zeros(4)
    q[i] = 0.5 * s; q[3] = (m[k, j] - m[j, k]) * r; q[j] = (m[j, i] + m[i, j]) * r; q[k] = (m[k, i] + m[i, k]) * r
    return q


def qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def qrot(q, v):
    """Eigen's quaternion * vector: v + w uv + qv x uv with uv = 2 qv x v. v [..., 3]."""
    qv = q[:3]
    uv = 2 * np.cross(qv, v)
    return v + q[3] * uv + np.cross(qv, uv)


def sim3_exp(u):
    """g2o::Sim3(Vector7d): (q, t, s) of update = omega, upsilon, sigma."""
    u = np.asarray(u, f64)
    om, ups, sigma = u[:3], u[3:6], u[6]
    th = np.sqrt(om @ om)
    Om = _hat(om); Om2 = Om @ Om
    s = np.exp(sigma); eps = 0.00001; I = np.eye(3)
    if abs(sigma) < eps:
        C = 1.0
        if th < eps:
            A, B, R = 0.5, 1.0 / 6, I + Om + Om2
        else:
            A = (1 - np.cos(th)) / (th * th); B = (th - np.sin(th)) / (th * th * th)
            R = I + np.sin(th) / th * Om + (1 - np.cos(th)) / (th * th) * Om2
    else:
        C = (s - 1) / sigma
        if th < eps:
            s2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / s2; B = ((0.5 * s2 - sigma + 1) * s) / (s2 * sigma)
            R = I + Om + Om2
        else:
            R = I + np.sin(th) / th * Om + (1 - np.cos(th)) / (th * th) * Om2
            a, b = s * np.sin(th), s * np.cos(th)
            c = th * th + sigma * sigma
            A = (a * sigma + (1 - b) * th) / (th * c); B = (C - ((b - 1) * sigma + a * th) / c) * 1.0 / (th * th)
    return mat2q(R), (A * Om + B * Om2 + C * I) @ ups, s


def sim3_mul(a, b):
    return qmul(a[0], b[0]), a[2] * qrot(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inv(a):
    qc = a[0] * np.array([-1, -1, -1, 1.0])
    return qc, qrot(qc, (-1.0 / a[2]) * a[1]), 1.0 / a[2]


def sim3_oplus(est, u, fix_scale):
    u = np.array(u, f64)
    if fix_scale:
        u[6] = 0
    return sim3_mul(sim3_exp(u), est)


def sim3_pack(S):
    return np.concatenate([S[0], S[1], [S[2]]])


def sim3_unpack(v):
    v = np.asarray(v, f64)
    return v[:4].copy(), v[4:7].copy(), float(v[7])


def edge_errors(S, X, K, obs):
    """obs - cam_map(project(S.map(X))) for points X [n,3]: [n,2]."""
    p = S[2] * qrot(S[0], X) + S[1]
    return np.stack([obs[:, 0] - (p[:, 0] / p[:, 2] * K[0] + K[2]), obs[:, 1] - (p[:, 1] / p[:, 2] * K[1] + K[3])], 1)


def edge_jacobians(S, X1, X2, K1, K2, o1, o2, fix_scale, mode):
    """(J12, J21) [n,2,7] of both edges with respect to the update of the Sim3 vertex."""
    n = len(X1)
    if mode == "numeric":
        J12, J21 = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
        scalar = 1 / (2 * OPT_DELTA)
        for d in range(7):
            u = np.zeros(7); u[d] = OPT_DELTA
            P = sim3_oplus(S, u, fix_scale); M = sim3_oplus(S, -u, fix_scale)
            J12[:, :, d] = scalar * (edge_errors(P, X2, K1, o1) - edge_errors(M, X2, K1, o1))
            J21[:, :, d] = scalar * (edge_errors(sim3_inv(P), X1, K2, o2) - edge_errors(sim3_inv(M), X1, K2, o2))
        return J12, J21

    def dproj(p, K):
        D = np.zeros((len(p), 2, 3))
        D[:, 0, 0] = K[0] / p[:, 2]; D[:, 0, 2] = -K[0] * p[:, 0] / p[:, 2] ** 2
        D[:, 1, 1] = K[1] / p[:, 2]; D[:, 1, 2] = -K[1] * p[:, 1] / p[:, 2] ** 2
        return D

    def gen(p):                                                     # d(exp(delta) p) / d delta = [-[p]x | I | p]
        G = np.zeros((len(p), 3, 7))
        G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = p[:, 2], -p[:, 1], -p[:, 2], p[:, 0], p[:, 1], -p[:, 0]
        G[:, :, 3:6] = np.eye(3)
        if not fix_scale:
            G[:, :, 6] = p
        return G
    p = S[2] * qrot(S[0], X2) + S[1]
    J12 = -dproj(p, K1) @ gen(p)
    Si = sim3_inv(S)
    q = Si[2] * qrot(Si[0], X1) + Si[1]
    G = gen(X1)
    lin = -Si[2] * np.stack([qrot(Si[0], G[:, :, d]) for d in range(7)], 2)          # S^-1 exp(-delta) X1
    J21 = -dproj(q, K2) @ lin
    return J12, J21


def _huber(e, delta):
    d2 = delta * delta
    sq = np.sqrt(np.maximum(e, 1e-300))
    return np.where(e <= d2, e, 2 * sq * delta - d2), np.where(e <= d2, 1.0, delta / sq)


def optimize_sim3(prob, S12, th2=10.0, fix_scale=False, valid=None, mode="numeric"):
    """dict(S12 [8], keep [n], n_in, info [8], trials: the accept / reject sequence of each round, last_rejected per round)."""
    X1, X2 = np.asarray(prob["X1c"], f32).astype(f64), np.asarray(prob["X2c"], f32).astype(f64)
    o1, o2 = np.asarray(prob["obs1"], f32).astype(f64), np.asarray(prob["obs2"], f32).astype(f64)
    w1 = (f32(1) / np.asarray(prob["sigma2_1"], f32)).astype(f64) if "inv_sigma2_1" not in prob else np.asarray(prob["inv_sigma2_1"], f32).astype(f64)
    w2 = (f32(1) / np.asarray(prob["sigma2_2"], f32)).astype(f64) if "inv_sigma2_2" not in prob else np.asarray(prob["inv_sigma2_2"], f32).astype(f64)
    K1, K2 = np.asarray(prob["K1"], f32).astype(f64), np.asarray(prob["K2"], f32).astype(f64)
    n = len(X1)
    keep = np.ones(n, bool) if valid is None else np.asarray(valid).astype(bool).copy()
    S0 = np.asarray(S12, f64).copy()
    est = sim3_unpack(S0)
    th2 = float(f32(th2)); delta = float(f32(np.sqrt(f32(th2))))
    ncorr = int(keep.sum())
    out = dict(S12=S0.copy(), keep=keep.astype(np.uint8), n_in=0, info=np.zeros(8), trials=[[], []], last_rejected=[False, False], margin=1.0)
    if ncorr == 0:
        return out

    def chi_of(S, k):
        e1, e2 = edge_errors(S, X2[k], K1, o1[k]), edge_errors(sim3_inv(S), X1[k], K2, o2[k])
        return w1[k] * (e1 ** 2).sum(1), w2[k] * (e2 ** 2).sum(1), e1, e2

    def robust_chi(S, k):
        c1, c2, _, _ = chi_of(S, k)
        return float(_huber(c1, delta)[0].sum() + _huber(c2, delta)[0].sum())
    nbad, its, chis, acc, rej = 0, [0, 0], [0.0, 0.0], 0, 0
    for rnd in range(2):
        k = keep.copy()
        lam, ni, nbadlm, ev = 0.0, 2.0, 0, est
        for it in range(5 if rnd == 0 else (10 if nbad > 0 else 5)):
            c1, c2, e1, e2 = chi_of(est, k)
            (r10, r11), (r20, r21) = _huber(c1, delta), _huber(c2, delta)
            cur = ini = float(r10.sum() + r20.sum())
            J12, J21 = edge_jacobians(est, X1[k], X2[k], K1, K2, o1[k], o2[k], fix_scale, mode)
            wa, wb = r11 * w1[k], r21 * w2[k]
            H = np.einsum("n,nri,nrj->ij", wa, J12, J12) + np.einsum("n,nri,nrj->ij", wb, J21, J21)
            g = -(np.einsum("n,nri,nr->i", wa, J12, e1) + np.einsum("n,nri,nr->i", wb, J21, e2))
            if it == 0:
                lam, ni, nbadlm = 1e-5 * np.abs(np.diag(H)).max(), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                bak = est
                try:
                    L = np.linalg.cholesky(H + lam * np.eye(7)); x = np.linalg.solve(L.T, np.linalg.solve(L, g)); ok = bool(np.isfinite(x).all())
                except np.linalg.LinAlgError:
                    x, ok = np.zeros(7), False
                if not ok:
                    x = np.zeros(7)
                if fix_scale:
                    x[6] = 0
                est = sim3_oplus(est, x, fix_scale); ev = est
                cur_before = cur
                tmp = robust_chi(est, k) if ok else np.finfo(f64).max
                scale = float((x * (lam * x + g)).sum()) + 1e-3
                rho = (cur - tmp) / scale
                rejected = not (rho > 0 and np.isfinite(tmp))
                if not rejected:
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3); lam *= max(1.0 / 3, alpha); ni = 2.0; cur = tmp; acc += 1
                else:
                    lam *= ni; ni *= 2; est = bak; rej += 1
                out["trials"][rnd].append(not rejected); out["last_rejected"][rnd] = rejected
                out["margin"] = min(out["margin"], abs(cur_before - tmp) / max(cur_before, 1e-300) if ok else 1.0)
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            its[rnd] += 1; chis[rnd] = cur
            if qmax == 10 or rho == 0:
                break
            nbadlm = nbadlm + 1 if (ini - cur) * 1e3 < ini else 0
            if nbadlm >= 3:
                break
        c1, c2, _, _ = chi_of(ev, k)                                # the stored errors: the last trial's state
        bad = (c1 > th2) | (c2 > th2)
        idx = np.nonzero(k)[0]
        keep[idx[bad]] = False
        out["chi_pairs_%d" % rnd] = (idx, c1, c2)
        if rnd == 0:
            nbad = int(bad.sum())
            if ncorr - nbad < 10:
                out.update(keep=keep.astype(np.uint8), n_in=0, info=np.array([ncorr, nbad, its[0], 0, chis[0], 0, acc, rej], f64))
                return out
        else:
            out["n_in"] = int((~bad).sum())
    out.update(S12=sim3_pack(est), keep=keep.astype(np.uint8), info=np.array([ncorr, nbad, its[0], its[1], chis[0], chis[1], acc, rej], f64))
    return out


def chi_band(res, th2, dev):
    """Correspondences whose keep flag may flip: a stored chi2 within BAND_FACTOR x dev of th2 in either round."""
    band = np.zeros(len(res["keep"]), bool)
    for rnd in (0, 1):
        if "chi_pairs_%d" % rnd in res:
            idx, c1, c2 = res["chi_pairs_%d" % rnd]
            band[idx[(np.abs(c1 - th2) <= BAND_FACTOR * dev * th2) | (np.abs(c2 - th2) <= BAND_FACTOR * dev * th2)]] = True
    return band


# The optimiser cases shared by the CPU and the GPU tests: (seed, fix_scale, valid correspondences, outlier_frac). Every case has `valid`
# holes in the middle of its arrays. g2o's Levenberg ends a round only after three iterations that gain less than 1e-3, so every round
# ends with trials at the rounding floor of chi2 (relative changes of 1e-13 and less), whose accept / reject decisions no two
# implementations share. OPT_CASES are the cases, found by a search over seeds with this checker, whose every decision is at least
# 1e-11 of chi2 away from zero and on which the numeric and the analytic mode agree in every count: the device is held to the counts
# there. OPT_CASES_FLOOR are cases without that property (with a fixed scale the six free dimensions converge a step earlier, and no
# seed of 440 per size met it; rounds that end on a rejected trial are floor decisions by construction): the device is held there to
# everything but the counts.
OPT_CASES = [(202, False, 9, 0.0), (200, False, 9, 0.2), (202, False, 10, 0.0), (304, False, 63, 0.0), (201, False, 63, 0.2), (203, False, 64, 0.0),
             (202, False, 64, 0.2), (286, False, 65, 0.0), (203, False, 65, 0.2), (225, False, 257, 0.0), (200, False, 257, 0.2), (201, True, 9, 0.2)]
OPT_CASES_FLOOR = [(211, False, 10, 0.2), (202, True, 9, 0.0), (212, True, 10, 0.0), (213, True, 10, 0.2), (222, True, 63, 0.0), (223, True, 63, 0.2),
                   (232, True, 64, 0.0), (233, True, 64, 0.2), (242, True, 65, 0.0), (243, True, 65, 0.2), (252, True, 257, 0.0), (253, True, 257, 0.2),
                   (230, False, 64, 0.0), (221, False, 63, 0.2)]


def opt_case(case):
    """(prob, S12 [8], valid [n], fix_scale, th2) of one optimiser case: the arrays hold size + size // 4 + 1 entries of which `size` are
    valid; the initial Sim3 is the truth moved by a few centimetres, half a degree and (with a free scale) one per cent."""
    from viorb_amd.synth import make_sim3_problem
    seed, fix, size, o = case
    n = size + size // 4 + 1
    p = make_sim3_problem(seed, "fix_scale" if fix else "general", n, o, 0.7, 0.003)
    valid = np.ones(n, np.uint8)
    valid[np.arange(1, n, 4)[:n - size]] = 0
    assert valid.sum() == size
    rng = np.random.default_rng(seed)
    dq = sim3_exp(np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.02, 3), [0.0 if fix else 0.01]]))
    S = sim3_mul(dq, (mat2q(np.asarray(p["R12"], f64)), np.asarray(p["t12"], f64), float(p["s12"])))
    return p, sim3_pack(S), valid, fix, 10.0
