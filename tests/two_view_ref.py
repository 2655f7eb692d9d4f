"""numpy restatement of the two-view initialiser, the checker of tests/test_two_view_ref.py and tests/test_gpu_two_view*.py (never
imported by product code). Reference: Initializer::Initialize and everything beneath it (src/Initializer.cc:44-929).

Two modes, as tests/mapping_ref.py:
  mode "f32": the reference's own casts ("two-view initialisation" audit): float A, LAPACK's float32 SVD in place of
              cv::SVD, float products in the reference's association, sequential float sums (Normalize, the scores), double only
              where OpenCV puts one (Mat::inv and determinant of a 3 x 3, cv::norm, Mat::dot, addWeighted, `1.0 / x`, acos).
  mode "f64": the definitional form: the same float inputs and the same float A, the SVDs and everything after them in double.

Matrices are compared after canon(): Frobenius norm 1, the largest-magnitude entry positive. Motion hypotheses are compared as a set
(match_hypotheses): their order depends on the signs an SVD happens to return, the accepted outcome does not."""
import numpy as np

FAILED, FROM_H, FROM_F = 0, 1, 2
OK, FEW_MATCHES, BAD_SET, NO_MODEL, H_DEGENERATE, NO_WINNER, FEW_GOOD, PARALLAX = range(8)
RT_NONE, RT_COUNTED, RT_TRIANGULATED = 0, 1, 2
TH_H, TH_F, TH_SCORE = 5.991, 3.841, 5.991
COS_GATE = 0.99998

# Measured by tests/test_two_view_ref.py::test_float32_restatement_against_float64 over PARAM_SETS (mode "f32" against mode "f64" of this
# file), rounded up; that test asserts that a fresh measurement does not exceed them and is not more than ten times below them.
#   HYP_DEV_F32     largest Frobenius distance of canon(H21i), canon(H12i), canon(F21i) between the modes, over the hypotheses whose
#                   set is not near-degenerate (gap() >= GAP_MIN)
#   CHI_DEV_F32     chi-square per match and direction, |a - b| / max(|b|, threshold), both modes on the SAME float32 matrix: the winner
#                   of the selected model (the flags that feed the reconstruction), over chi-squares up to twice the threshold
#   SCORE_DEV_F32   score of the winners of both searches, relative to max(score, 5.991), same matrix, where no flag flips
#   ROT_DEV_F32     angle of R_a^T R_b (radians), DIR_DEV_F32 angle between the unit t: the motions of the selected model's winner, same
#                   matrix, matched as a set
#   COS_DEV_F32     CheckRT's parallax cosine, absolute; REPROJ_DEV_F32 squared reprojection errors, relative to max(|e|, 4 sigma^2);
#   DEPTH_DEV_F32   the depths z1, z2, relative to the point's distance from the camera; POS_DEV_F32 |X_a - X_b| / |X_b|.
#                   All four on the same (R, t), over matches with a parallax cosine below COS_POS_MAX in f64 (beyond it the point is
#                   "at infinity": its position is ill-conditioned, and CheckRT itself stops testing its depth at 0.99998)
HYP_DEV_F32 = 2.0e-3
CHI_DEV_F32 = 2.5e-4
SCORE_DEV_F32 = 5.0e-6
ROT_DEV_F32 = 4.0e-3
DIR_DEV_F32 = 8.0e-5
COS_DEV_F32 = 2.5e-7
REPROJ_DEV_F32 = 5.0e-5
DEPTH_DEV_F32 = 2.0e-6
POS_DEV_F32 = 2.2e-6
COS_POS_MAX = 0.9999
GPU_FACTOR = 4                         # a different float32-output SVD: same order of backward error, other constants (as POS_TOL_GPU)
BAND_FACTOR = 10                       # a discrete result may flip when its quantity is within 10 x the deviation of its threshold
MAX_BAND_SHARE_GPU, MAX_BAND_SHARE_CPU, MAX_SKIPPED_SETS = 0.02, 0.005, 0.10
# A set is near-degenerate when gap() = (sigma_8 - sigma_9) / sigma_1 of its A (f64; sigma_9 = 0 for the 8 x 9 A of F) is below GAP_MIN. The
# null vector of a perturbed A moves by about |dA| / (sigma_8 - sigma_9), so a float32 SVD (|dA| of a few eps32 sigma_1) is off by
# GAP_C eps32 / gap; the CPU suite measures deviation x gap / eps32 <= GAP_C over every hypothesis of PARAM_SETS. GAP_MIN is then the gap
# below which that bound exceeds HYP_DEV_F32: such a hypothesis cannot be compared at HYP_DEV_F32 at all.
GAP_C = 16.0
GAP_MIN = float(np.finfo(np.float32).eps) / HYP_DEV_F32

# (seed, kind, n1, n2, n_matches, outlier_share, noise_px) of synth.make_two_view_init_problem, shared by the CPU and GPU tests
PARAM_SETS = [(0, "general", 400, 430, 300, 0.1, 0.5), (1, "planar", 400, 430, 300, 0.1, 0.5), (7, "forward", 400, 430, 300, 0.1, 0.5),
              (3, "low_parallax", 400, 430, 300, 0.1, 0.5), (4, "general", 1000, 1040, 300, 0.2, 1.0), (5, "planar", 200, 190, 130, 0.0, 0.3)]
f32, f64 = np.float32, np.float64


def _ft(mode):
    return np.float32 if mode == "f32" else np.float64


def _seqsum(a, mode):
    """Sum in order of appearance: float accumulator in f32 mode."""
    a = np.asarray(a)
    if a.size == 0:
        return _ft(mode)(0)
    return np.cumsum(a.astype(_ft(mode)))[-1]


def canon(M):
    M = np.asarray(M, np.float64)
    shp = M.shape
    M = M.reshape(shp[:-2] + (9,)) if len(shp) >= 2 and shp[-2:] == (3, 3) else M
    n = np.linalg.norm(M, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        M = M / n
    k = np.argmax(np.abs(M), axis=-1)
    s = np.sign(np.take_along_axis(M, k[..., None], -1))
    return (M * np.where(s == 0, 1, s)).reshape(shp)


def mat_dist(A, B):
    """Frobenius distance of canon(A), canon(B) (per matrix); the sign rule can pick different entries of near-equal magnitude, hence the min."""
    a, b = canon(A), canon(B)
    d1 = np.linalg.norm((a - b).reshape(a.shape[:-2] + (9,)), axis=-1)
    d2 = np.linalg.norm((a + b).reshape(a.shape[:-2] + (9,)), axis=-1)
    return np.minimum(d1, d2)


def rot_angle(Ra, Rb):
    c = (np.trace(np.asarray(Ra, f64).T @ np.asarray(Rb, f64)) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1)))


def dir_angle(ta, tb):
    ta, tb = np.asarray(ta, f64), np.asarray(tb, f64)
    c = ta @ tb / (np.linalg.norm(ta) * np.linalg.norm(tb))
    return float(np.arccos(np.clip(c, -1, 1)))


def match_hypotheses(Ra, ta, Rb, tb):
    """For each hypothesis of side a the nearest of side b by rotation angle + direction angle: (index, rot angle, dir angle) lists."""
    idx, ra, da = [], [], []
    for i in range(len(Ra)):
        cost = [rot_angle(Ra[i], Rb[j]) + dir_angle(ta[i], tb[j]) for j in range(len(Rb))]
        j = int(np.argmin(cost))
        idx.append(j); ra.append(rot_angle(Ra[i], Rb[j])); da.append(dir_angle(ta[i], tb[j]))
    return idx, ra, da


# ---- the match list and Normalize -----------------------------------------------------------------------------------------------------
def match_list(matches12, n2=None):
    m = np.asarray(matches12)
    ok = m >= 0 if n2 is None else (m >= 0) & (m < n2)
    i1 = np.nonzero(ok)[0]
    return i1, m[i1].astype(np.int64)


def compact(prob):
    """[N, 4] = u1 v1 u2 v2 (float32) of the match list, and i1."""
    i1, i2 = match_list(prob["matches12"], len(prob["xy2"]))
    return np.concatenate([f32(prob["xy1"]).reshape(-1, 2)[i1], f32(prob["xy2"]).reshape(-1, 2)[i2]], 1), i1


def normalise(xy, mode):
    """nrm4 = meanX meanY sX sY (:749-795). f32: float sums in key-point order as the reference; f64: double."""
    FT = _ft(mode)
    xy = f32(xy).reshape(-1, 2)
    n = len(xy)
    m = np.array([_seqsum(xy[:, 0], mode) / FT(n), _seqsum(xy[:, 1], mode) / FT(n)], FT)
    d = np.abs(xy.astype(FT) - m[None, :])
    md = np.array([_seqsum(d[:, 0], mode) / FT(n), _seqsum(d[:, 1], mode) / FT(n)], FT)
    s = (1.0 / md.astype(f64)).astype(FT)
    return np.array([m[0], m[1], s[0], s[1]], FT)


def T_of(nrm):
    T = np.eye(3, dtype=nrm.dtype)
    T[0, 0], T[1, 1], T[0, 2], T[1, 2] = nrm[2], nrm[3], -nrm[0] * nrm[2], -nrm[1] * nrm[3]
    return T


def _inv33(M, FT):
    with np.errstate(all="ignore"):
        try:
            return np.linalg.inv(np.asarray(M, f64)).astype(FT)
        except np.linalg.LinAlgError:
            return np.zeros(M.shape, FT)


# ---- hypotheses -------------------------------------------------------------------------------------------------------------------------
def build_A(model, pn1, pn2):
    """float32 A of ComputeH21 [.., 16, 9] / ComputeF21 [.., 8, 9] from normalised points [.., 8, 2] (float32 arithmetic in both modes)."""
    u1, v1, u2, v2 = f32(pn1[..., 0]), f32(pn1[..., 1]), f32(pn2[..., 0]), f32(pn2[..., 1])
    z, o = np.zeros_like(u1), np.ones_like(u1)
    if model == FROM_H:
        r0 = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
        r1 = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
        return np.stack([r0, r1], -2).reshape(u1.shape[:-1] + (16, 9)).astype(f32)
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], -1).astype(f32)


def gap(A):
    """(sigma_8 - sigma_9) / sigma_1 of A in double (sigma_9 = 0 for an 8 x 9 A)."""
    w = np.linalg.svd(np.asarray(A, f64), compute_uv=False)
    s9 = w[..., 8] if w.shape[-1] > 8 else 0.0
    with np.errstate(all="ignore"):
        return (w[..., 7] - s9) / w[..., 0]


def null_vector(A, mode):
    """vt.row(8) [.., 9] of the full SVD."""
    return np.linalg.svd(np.asarray(A, _ft(mode)), full_matrices=True)[2][..., 8, :]


def rank2(Fpre, mode):
    FT = _ft(mode)
    u, w, vt = np.linalg.svd(np.asarray(Fpre, FT).reshape(Fpre.shape[:-1] + (3, 3)))
    w = w.copy(); w[..., 2] = 0
    return ((u * w[..., None, :]) @ vt).astype(FT)                 # u * diag(w) * vt


def denorm_h(Hn, nrm1, nrm2, mode):
    FT = _ft(mode)
    T1, T2 = T_of(nrm1.astype(FT)), T_of(nrm2.astype(FT))
    H21 = ((_inv33(T2, FT) @ Hn.astype(FT)).astype(FT) @ T1).astype(FT)
    return H21, np.stack([_inv33(h, FT) for h in H21.reshape(-1, 3, 3)]).reshape(H21.shape)


def denorm_f(Fn, nrm1, nrm2, mode):
    FT = _ft(mode)
    T1, T2 = T_of(nrm1.astype(FT)), T_of(nrm2.astype(FT))
    return ((T2.T @ Fn.astype(FT)).astype(FT) @ T1).astype(FT)


def hypotheses(prob, sets, mode, nrm=None):
    """Per set: H21i, H12i, F21i [iterations, 3, 3] in the mode's type, and gapH, gapF [iterations]."""
    FT = _ft(mode)
    pm, _ = compact(prob)
    nrm1, nrm2 = nrm if nrm is not None else (normalise(prob["xy1"], mode), normalise(prob["xy2"], mode))
    sets = np.asarray(sets).reshape(-1, 8)
    p = pm[sets].astype(FT)                                           # [it, 8, 4]
    pn1 = (p[..., 0:2] - nrm1[None, None, 0:2].astype(FT)) * nrm1[None, None, 2:4].astype(FT)
    pn2 = (p[..., 2:4] - nrm2[None, None, 0:2].astype(FT)) * nrm2[None, None, 2:4].astype(FT)
    AH, AF = build_A(FROM_H, pn1, pn2), build_A(FROM_F, pn1, pn2)
    Hn = null_vector(AH, mode).reshape(-1, 3, 3)
    Fn = rank2(null_vector(AF, mode), mode)
    H21, H12 = denorm_h(Hn, nrm1, nrm2, mode)
    return dict(H21=H21, H12=H12, F21=denorm_f(Fn, nrm1, nrm2, mode), gapH=gap(AH), gapF=gap(AF), Hn=Hn, Fn=Fn, pn1=pn1, pn2=pn2)


# ---- scores -----------------------------------------------------------------------------------------------------------------------------
def chi2(model, M21, M12, pm, sigma, mode):
    """chi [N, 2] of CheckHomography (:352-374) / CheckFundamental (:428-454) for one matrix, in the mode's type."""
    FT = _ft(mode)
    M21 = np.asarray(M21, FT).reshape(9)
    u1, v1, u2, v2 = [np.asarray(pm[:, k], FT) for k in range(4)]
    inv_s2 = FT(1.0 / f64(FT(sigma) * FT(sigma)))
    with np.errstate(all="ignore"):
        if model == FROM_H:
            h, g = M21, np.asarray(M12, FT).reshape(9)
            w2 = (1.0 / (g[6] * u2 + g[7] * v2 + g[8]).astype(f64)).astype(FT)
            a, b = (g[0] * u2 + g[1] * v2 + g[2]) * w2, (g[3] * u2 + g[4] * v2 + g[5]) * w2
            c1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
            w1 = (1.0 / (h[6] * u1 + h[7] * v1 + h[8]).astype(f64)).astype(FT)
            a, b = (h[0] * u1 + h[1] * v1 + h[2]) * w1, (h[3] * u1 + h[4] * v1 + h[5]) * w1
            c2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
        else:
            f = M21
            a2, b2, c2_ = f[0] * u1 + f[1] * v1 + f[2], f[3] * u1 + f[4] * v1 + f[5], f[6] * u1 + f[7] * v1 + f[8]
            num2 = a2 * u2 + b2 * v2 + c2_
            c1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
            a1, b1, c1_ = f[0] * u2 + f[3] * v2 + f[6], f[1] * u2 + f[4] * v2 + f[7], f[2] * u2 + f[5] * v2 + f[8]
            num1 = a1 * u1 + b1 * v1 + c1_
            c2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
    return np.stack([c1, c2], 1).astype(FT)


def score(model, chi, mode):
    """(score, inlier flags [N], per-match contributions): each direction adds on its own, a match is an inlier only if both pass."""
    FT = _ft(mode)
    th = FT(TH_H if model == FROM_H else TH_F); ths = FT(TH_SCORE)
    passed = ~(chi > th)
    contrib = np.where(passed, ths - chi, FT(0)).astype(FT)
    return _seqsum(contrib.reshape(-1), mode), passed.all(1), contrib


def chi_threshold(model):
    return TH_H if model == FROM_H else TH_F


def chi_band(model, chi, dev):
    """Matches whose flag may flip: a chi-square within BAND_FACTOR * dev (relative to the threshold) of its threshold."""
    th = chi_threshold(model)
    return (np.abs(np.asarray(chi, f64) - th) <= BAND_FACTOR * dev * th).any(1)


def select(scores):
    """First-maximum argmax (strictly greater than the best so far, from 0) of [iterations, 2] float32 scores, RH in float, the model."""
    scores = f32(scores)
    best, S = [-1, -1], [f32(0), f32(0)]
    for m in range(2):
        for it in range(len(scores)):
            if scores[it, m] > S[m]:
                S[m], best[m] = scores[it, m], it
    with np.errstate(all="ignore"):
        RH = f32(S[0]) / (f32(S[0]) + f32(S[1]))
    model = FROM_H if f64(RH) > 0.40 else FROM_F
    reason = OK
    if best[model - 1] < 0:
        model, reason = FAILED, NO_MODEL
    return dict(best_iter=best, S=S, RH=RH, model=model, reason=reason)


# ---- motion hypotheses --------------------------------------------------------------------------------------------------------------------
def _K(K4, FT):
    fx, fy, cx, cy = [FT(f32(v)) for v in K4]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], FT)


def _unit(t, FT):
    return (t.astype(f64) / np.linalg.norm(t.astype(f64))).astype(FT)


def decompose_f(F21, K4, mode):
    FT = _ft(mode)
    K = _K(K4, FT)
    E = ((K.T @ np.asarray(F21, FT).reshape(3, 3)).astype(FT) @ K).astype(FT)
    u, w, vt = np.linalg.svd(E)
    t = _unit(u[:, 2], FT)
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], FT)
    R1 = ((u @ W) @ vt).astype(FT); R2 = ((u @ W.T) @ vt).astype(FT)
    if np.linalg.det(R1.astype(f64)) < 0: R1 = -R1
    if np.linalg.det(R2.astype(f64)) < 0: R2 = -R2
    return [R1, R2, R1, R2], [t, t, -t, -t]


def decompose_h(H21, K4, mode):
    """(ok, R [8], t [8], d [3], A): the eight motions of Faugeras (:584-686); ok False under the singular-value gate."""
    FT = _ft(mode)
    K = _K(K4, FT)
    A = ((_inv33(K, FT) @ np.asarray(H21, FT).reshape(3, 3)).astype(FT) @ K).astype(FT)
    U, w, Vt = np.linalg.svd(A)
    s = FT(np.linalg.det(U.astype(f64)) * np.linalg.det(Vt.astype(f64)))
    d1, d2, d3 = [FT(v) for v in w]
    with np.errstate(all="ignore"):
        if not (f64(d1 / d2) >= 1.00001) or not (f64(d2 / d3) >= 1.00001):
            return False, [], [], np.array([d1, d2, d3]), A
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)); aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]; x3 = [aux3, -aux3, aux3, -aux3]
        ast = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2); ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [ast, -ast, -ast, ast]
        asp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2); cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [asp, -asp, -asp, asp]
    R, t = [None] * 8, [None] * 8
    for i in range(4):
        Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]], FT)
        R[i] = (((s * U).astype(FT) @ Rp).astype(FT) @ Vt).astype(FT)
        t[i] = _unit((U @ (np.array([x1[i], 0, -x3[i]], FT) * (d1 - d3))).astype(FT), FT)
        Rq = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]], FT)
        R[4 + i] = (((s * U).astype(FT) @ Rq).astype(FT) @ Vt).astype(FT)
        t[4 + i] = _unit((U @ (np.array([x1[i], 0, x3[i]], FT) * (d1 + d3))).astype(FT), FT)
    return True, R, t, np.array([d1, d2, d3]), A


# ---- CheckRT ------------------------------------------------------------------------------------------------------------------------------
def check_rt(K4, R, t, pm, inliers, sigma, mode):
    """CheckRT (:798-907) over the inlier matches. code [N] (RT_*), X [N, 3], q = dict(cos, z1, z2, e1, e2, dist1, dist2) over all N
    (every quantity computed for every match with a finite point, whether or not the match reaches its gate), reached = dict of the
    gates each match actually reaches, n_good, parallax (degrees), cosines (of the counted matches)."""
    FT = _ft(mode)
    N = len(pm)
    fx, fy, cx, cy = [FT(f32(v)) for v in K4]
    K = _K(K4, FT)
    R = np.asarray(R, FT).reshape(3, 3); t = np.asarray(t, FT).reshape(3)
    P1 = np.concatenate([K, np.zeros((3, 1), FT)], 1)
    P2 = (K @ np.concatenate([R, t[:, None]], 1)).astype(FT)
    O2 = (-(R.T @ t)).astype(FT)
    th2 = FT(4.0 * f64(FT(sigma) * FT(sigma)))
    u1, v1, u2, v2 = [np.asarray(pm[:, k], FT) for k in range(4)]
    d = lambda a: np.asarray(a, f64)
    # A.row(0) = kp1.pt.x * P1.row(2) - P1.row(0): addWeighted in double, stored to float (both modes: the same float32 A)
    P1s, P2s = f32(P1), f32(P2)
    A = np.empty((N, 4, 4), f32)
    A[:, 0] = (d(P1s[2])[None] * d(f32(u1))[:, None] - d(P1s[0])[None]).astype(f32)
    A[:, 1] = (d(P1s[2])[None] * d(f32(v1))[:, None] - d(P1s[1])[None]).astype(f32)
    A[:, 2] = (d(P2s[2])[None] * d(f32(u2))[:, None] - d(P2s[0])[None]).astype(f32)
    A[:, 3] = (d(P2s[2])[None] * d(f32(v2))[:, None] - d(P2s[1])[None]).astype(f32)
    with np.errstate(all="ignore"):
        x = np.linalg.svd(A.astype(FT))[2][:, 3, :] if N else np.zeros((0, 4), FT)
        X = (d(x[:, :3]) / d(x[:, 3:4])).astype(FT)
        finite = np.isfinite(X).all(1)
        X = np.where(finite[:, None], X, FT(0))
        dist1 = np.sqrt((d(X) ** 2).sum(1)).astype(FT)
        n2 = (X - O2[None]).astype(FT)
        dist2 = np.sqrt((d(n2) ** 2).sum(1)).astype(FT)
        cos = ((d(X) * d(n2)).sum(1) / d(dist1 * dist2)).astype(FT)
        low = d(cos) < COS_GATE
        X2 = ((X @ R.T).astype(FT) + t[None]).astype(FT)
        z1, z2 = X[:, 2], X2[:, 2]
        iz1 = (1.0 / d(z1)).astype(FT); iz2 = (1.0 / d(z2)).astype(FT)
        e1 = (fx * X[:, 0] * iz1 + cx - u1) ** 2 + (fy * X[:, 1] * iz1 + cy - v1) ** 2
        e2 = (fx * X2[:, 0] * iz2 + cx - u2) ** 2 + (fy * X2[:, 1] * iz2 + cy - v2) ** 2
        inl = np.asarray(inliers, bool)[:N]
        g0 = inl & finite
        g1 = g0 & ~((z1 <= 0) & low)
        g2 = g1 & ~((z2 <= 0) & low)
        g3 = g2 & ~(e1 > th2)
        g4 = g3 & ~(e2 > th2)
    code = np.where(g4, np.where(low, RT_TRIANGULATED, RT_COUNTED), RT_NONE).astype(np.uint8)
    cosines = np.sort(cos[g4])
    n_good = int(g4.sum())
    par = FT(np.degrees(np.arccos(f64(cosines[min(50, n_good - 1)])))) if n_good else FT(0)
    return dict(code=code, X=X, q=dict(cos=cos, z1=z1, z2=z2, e1=e1, e2=e2, dist1=dist1, dist2=dist2), th2=th2, finite=finite,
                reached=dict(cos=g0, z1=g0 & low, z2=g1 & low, e1=g2, e2=g3), n_good=n_good, parallax=par, cosines=cosines)


def rt_band(r, devs=None):
    """Matches of a check_rt result whose verdict may flip: a gate quantity the match reaches within BAND_FACTOR x its deviation of its threshold."""
    cosd, rep, dep = devs or (COS_DEV_F32, REPROJ_DEV_F32, DEPTH_DEV_F32)
    q, g, th2 = r["q"], r["reached"], float(r["th2"])
    d = lambda a: np.asarray(a, f64)
    with np.errstate(all="ignore"):
        b = g["cos"] & (np.abs(d(q["cos"]) - COS_GATE) <= BAND_FACTOR * cosd)
        b |= g["z1"] & (np.abs(d(q["z1"])) <= BAND_FACTOR * dep * d(q["dist1"]))
        b |= g["z2"] & (np.abs(d(q["z2"])) <= BAND_FACTOR * dep * d(q["dist2"]))
        b |= g["e1"] & (np.abs(d(q["e1"]) - th2) <= BAND_FACTOR * rep * np.maximum(d(q["e1"]), th2))
        b |= g["e2"] & (np.abs(d(q["e2"]) - th2) <= BAND_FACTOR * rep * np.maximum(d(q["e2"]), th2))
    return b


def accept_h(n_good, parallax, n_inl, min_parallax=1.0, min_tri=50):
    best, second, idx, bp = 0, 0, -1, -1.0
    for i in range(8):
        if n_good[i] > best:
            second, best, idx, bp = best, n_good[i], i, parallax[i]
        elif n_good[i] > second:
            second = n_good[i]
    if not second < 0.75 * best: return -1, NO_WINNER
    if not (best > min_tri and best > 0.9 * n_inl): return -1, FEW_GOOD
    if not bp >= min_parallax: return -1, PARALLAX
    return idx, OK


def accept_f(n_good, parallax, n_inl, min_parallax=1.0, min_tri=50):
    mx = max(n_good[:4])
    nmin = max(int(0.9 * n_inl), min_tri)
    nsim = sum(1 for i in range(4) if n_good[i] > 0.7 * mx)
    if mx < nmin: return -1, FEW_GOOD
    if nsim > 1: return -1, NO_WINNER
    idx = [i for i in range(4) if n_good[i] == mx][0]
    if not parallax[idx] > min_parallax: return -1, PARALLAX
    return idx, OK


def reconstruct(model, M, inliers, prob, mode, sigma=1.0, min_parallax=1.0, min_tri=50):
    """ReconstructH / ReconstructF on a given matrix and inlier flags (over the match list)."""
    FT = _ft(mode)
    pm, i1 = compact(prob)
    n1 = len(f32(prob["xy1"]).reshape(-1, 2))
    out = dict(status=FAILED, reason=OK, R21=np.zeros((3, 3), FT), t21=np.zeros(3, FT), P3D=np.zeros((n1, 3), FT), triangulated=np.zeros(n1, np.uint8),
               hyp_R=[], hyp_t=[], rt=[], n_inliers=int(np.asarray(inliers, bool)[:len(pm)].sum()), win=-1)
    if model == FROM_H:
        ok, R, t, dd, _ = decompose_h(M, prob["K4"], mode)
        out["d"] = dd
        if not ok:
            out["reason"] = H_DEGENERATE
            return out
    elif model == FROM_F:
        R, t = decompose_f(M, prob["K4"], mode)
    else:
        out["reason"] = NO_MODEL
        return out
    out["hyp_R"], out["hyp_t"] = R, t
    out["rt"] = [check_rt(prob["K4"], R[h], t[h], pm, inliers, sigma, mode) for h in range(len(R))]
    ng = [r["n_good"] for r in out["rt"]]; par = [float(r["parallax"]) for r in out["rt"]]
    out["n_good"], out["parallax"] = ng, par
    win, reason = (accept_h if model == FROM_H else accept_f)(ng, [FT(p) for p in par], out["n_inliers"], FT(min_parallax), min_tri)
    out["win"], out["reason"] = win, reason
    if win >= 0:
        r = out["rt"][win]
        out["status"] = model; out["R21"], out["t21"] = R[win], t[win]
        c = r["code"] != RT_NONE
        out["P3D"][i1[c]] = r["X"][c]; out["triangulated"][i1[r["code"] == RT_TRIANGULATED]] = 1
    return out


def initialise(prob, sets, mode, sigma=1.0, min_parallax=1.0, min_tri=50):
    """Initializer::Initialize end to end in one mode (used against ground truth and for the timing note of DESIGN.md)."""
    pm, _ = compact(prob)
    if len(pm) < 8:
        return dict(status=FAILED, reason=FEW_MATCHES)
    hy = hypotheses(prob, sets, mode)
    it = len(hy["H21"])
    sc = np.zeros((it, 2), np.float32); fl = [[None, None] for _ in range(it)]
    for k in range(it):
        for m, (M21, M12) in enumerate(((hy["H21"][k], hy["H12"][k]), (hy["F21"][k], None))):
            s, inl, _ = score(m + 1, chi2(m + 1, M21, M12, pm, sigma, mode), mode)
            sc[k, m] = s; fl[k][m] = inl
    sel = select(sc)
    out = dict(select=sel, scores=sc, hyp=hy)
    if sel["model"] == FAILED:
        out.update(status=FAILED, reason=NO_MODEL)
        return out
    m = sel["model"]; k = sel["best_iter"][m - 1]
    M = hy["H21"][k] if m == FROM_H else hy["F21"][k]
    out.update(reconstruct(m, M, fl[k][m - 1], prob, mode, sigma, min_parallax, min_tri))
    out["M"], out["inliers"] = M, fl[k][m - 1]
    return out
