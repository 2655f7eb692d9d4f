"""Checker of the device vision-only global bundle adjustment (viorb_global_ba_se3, csrc/global_ba_se3.hip): numpy, float64, TEST
INFRASTRUCTURE ONLY. It restates Optimizer::BundleAdjustment (reference src/Optimizer.cc:3559-3747, BlockSolver_6_3) from the g2o sources:
a VertexSE3Expmap (6) per key frame, marginalised points, one EdgeSE3ProjectXYZ (uRight < 0) or EdgeStereoSE3ProjectXYZ per observation
(Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:103-234), SE3Quat::exp / operator* / map (types/se3quat.h) and one optimize(iterations) of
g2o's Levenberg on the Schur complement of the point block, solved densely. tests/test_global_ba_se3_ref.py pins it against the oracle's
vision-only window solve, the library's host edge hook, central differences and a solve of the un-eliminated normal equations.

Flat layouts are those of include/viorb.h: kfs [nk,7] = qx qy qz qw tx ty tz of Tcw, edge_obs [ne,4] = u v uRight invSigma2, intr5 = fx fy
cx cy bf. Unlike the C ABI, the Huber delta^2 of both edge types and the iteration count are arguments."""
import numpy as np
from global_ba_ref import _fsq, huber, qmat, qmul, mat2q, hat


# ---- g2o::SE3Quat on (quaternion x y z w, translation) ----------------------------------------------------------------------------------
def norm_rot(q):
    """SE3Quat::normalizeRotation: w >= 0, unit norm"""
    q = np.where(q[..., 3:4] < 0, -q, q)
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def qrot(q, v):
    """Eigen's quaternion * vector: v + w (2 qv x v) + qv x (2 qv x v)"""
    qv = q[..., :3]
    uv = np.cross(qv, v); uv = uv + uv
    return v + q[..., 3:4] * uv + np.cross(qv, uv)


def se3_map(k7, X):
    return qrot(k7[..., :4], X) + k7[..., 4:7]


def se3_exp(u):
    """SE3Quat::exp(update = [omega, upsilon]), se3quat.h:223-257 -> (q, t)"""
    om, ups = u[:3], u[3:]
    th = np.sqrt(om @ om)
    Om = hat(om); Om2 = Om @ Om
    if th < 0.00001:
        R = np.eye(3) + Om + Om2; V = R
    else:
        R = np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / (th * th) * Om2
        V = np.eye(3) + (1 - np.cos(th)) / (th * th) * Om + (th - np.sin(th)) / (th ** 3) * Om2
    return norm_rot(mat2q(R)), V @ ups


def se3_mul(qa, ta, qb, tb):
    """SE3Quat::operator*"""
    return norm_rot(qmul(qa, qb)), ta + qrot(qa, tb)


def retract(kfs, free_ids, xp):
    """VertexSE3Expmap::oplusImpl: estimate = SE3Quat::exp(update) * estimate"""
    out = kfs.copy()
    for r, i in enumerate(free_ids):
        q, t = se3_exp(xp[6 * r:6 * r + 6])
        out[i, :4], out[i, 4:7] = se3_mul(q, t, out[i, :4], out[i, 4:7])
    return out


# ---- edges -----------------------------------------------------------------------------------------------------------------------------
def edges(kfs, pts, intr5, e_idx, e_obs, jac=True):
    """Both edge types of every observation at once: e [ne,3], Jp [ne,3,3] (_jacobianOplusXi, the point), Jk [ne,3,6] (_jacobianOplusXj,
    the pose); the third rows are zero on a monocular edge."""
    fx, fy, cx, cy, bf = intr5
    K = kfs[e_idx[:, 1]]
    pc = se3_map(K, pts[e_idx[:, 0]])
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    st = ~(e_obs[:, 2] < 0)
    e = np.zeros((len(pc), 3))
    # EdgeSE3ProjectXYZ::cam_project: project2d then the intrinsics
    e[:, 0] = e_obs[:, 0] - (x / z * fx + cx); e[:, 1] = e_obs[:, 1] - (y / z * fy + cy)
    if st.any():
        # EdgeStereoSE3ProjectXYZ::cam_project: "const float invz = 1.0f/trans_xyz[2]", a double quotient rounded to float
        invz = np.float32(1.0 / z[st]).astype(np.float64)
        r0 = x[st] * invz * fx + cx
        e[st, 0] = e_obs[st, 0] - r0; e[st, 1] = e_obs[st, 1] - (y[st] * invz * fy + cy); e[st, 2] = e_obs[st, 2] - (r0 - bf * invz)
    if not jac:
        return e, None, None
    R = qmat(K[:, :4]); z_2 = z * z
    n = len(pc)
    Jp = np.zeros((n, 3, 3)); Jk = np.zeros((n, 3, 6))
    tmp = np.zeros((n, 2, 3))
    tmp[:, 0, 0] = fx; tmp[:, 0, 2] = -x / z * fx; tmp[:, 1, 1] = fy; tmp[:, 1, 2] = -y / z * fy
    Jp[:, :2, :] = np.einsum("nrk,nkc->nrc", (-1.0 / z)[:, None, None] * tmp, R)
    if st.any():
        Rs = R[st]; xs, ys, zs, z2s = x[st], y[st], z[st], z_2[st]
        J = np.zeros((st.sum(), 3, 3))
        J[:, 0, :] = -fx * Rs[:, 0, :] / zs[:, None] + fx * xs[:, None] * Rs[:, 2, :] / z2s[:, None]
        J[:, 1, :] = -fy * Rs[:, 1, :] / zs[:, None] + fy * ys[:, None] * Rs[:, 2, :] / z2s[:, None]
        J[:, 2, :] = J[:, 0, :] - bf * Rs[:, 2, :] / z2s[:, None]
        Jp[st] = J
    Jk[:, 0, 0] = x * y / z_2 * fx; Jk[:, 0, 1] = -(1 + (x * x / z_2)) * fx; Jk[:, 0, 2] = y / z * fx; Jk[:, 0, 3] = -1.0 / z * fx; Jk[:, 0, 5] = x / z_2 * fx
    Jk[:, 1, 0] = (1 + y * y / z_2) * fy; Jk[:, 1, 1] = -x * y / z_2 * fy; Jk[:, 1, 2] = -x / z * fy; Jk[:, 1, 4] = -1.0 / z * fy; Jk[:, 1, 5] = y / z_2 * fy
    Jk[st, 2, 0] = Jk[st, 0, 0] - bf * y[st] / z_2[st]; Jk[st, 2, 1] = Jk[st, 0, 1] + bf * x[st] / z_2[st]; Jk[st, 2, 2] = Jk[st, 0, 2]
    Jk[st, 2, 3] = Jk[st, 0, 3]; Jk[st, 2, 5] = Jk[st, 0, 5] - bf / z_2[st]
    return e, Jp, Jk


class Problem:
    def __init__(self, kfs, fixed, points, edge_idx, edge_obs, intr5):
        self.kfs = np.array(kfs, float).reshape(-1, 7); self.fixed = np.asarray(fixed).astype(bool)
        self.points = np.array(points, float).reshape(-1, 3)
        self.e_idx = np.asarray(edge_idx, np.int64).reshape(-1, 2); self.e_obs = np.asarray(edge_obs, float).reshape(-1, 4)
        self.intr5 = np.asarray(intr5, float)
        self.nk, self.np_, self.ne = len(self.kfs), len(self.points), len(self.e_idx)
        self.free_ids = np.flatnonzero(~self.fixed); self.fidx = np.full(self.nk, -1, np.int64); self.fidx[self.free_ids] = np.arange(len(self.free_ids))
        self.n = 6 * len(self.free_ids)
        self.included = np.zeros(self.np_, bool); self.included[self.e_idx[:, 0]] = True
        self.stereo = ~(self.e_obs[:, 2] < 0)
        # ordered pairs (a, b) of edges of one point whose key frames are both free
        self.ef = ef = self.fidx[self.e_idx[:, 1]]
        pa, pb = [], []
        bounds = np.flatnonzero(np.diff(self.e_idx[:, 0])) + 1
        for s, t in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [self.ne]])) if self.ne else []:
            ks = np.arange(s, t)[ef[s:t] >= 0]
            if len(ks):
                A, B = np.meshgrid(ks, ks, indexing="ij"); pa.append(A.ravel()); pb.append(B.ravel())
        self.pa = np.concatenate(pa) if pa else np.zeros(0, np.int64); self.pb = np.concatenate(pb) if pb else np.zeros(0, np.int64)
        self._pair_idx = None

    def pair_index(self):
        """flat index into S of every element of every pair's 6 x 6 block, in pair order (the graph is fixed over the solve)"""
        if self._pair_idx is None:
            ra = (6 * self.ef[self.pa])[:, None] + np.arange(6)[None, :]; cb = (6 * self.ef[self.pb])[:, None] + np.arange(6)[None, :]
            self._pair_idx = (ra[:, :, None] * self.n + cb[:, None, :]).ravel()
        return self._pair_idx


def _rho(P, chi_e, robust, d_mono, d_stereo):
    """(rho, rho') of every edge: RobustKernelHuber with the delta of the edge's type, or the identity"""
    if not robust:
        return chi_e, np.ones(P.ne)
    r0m, r1m = huber(chi_e, d_mono); r0s, r1s = huber(chi_e, d_stereo)
    return np.where(P.stereo, r0s, r0m), np.where(P.stereo, r1s, r1m)


def _errors(P, kfs, pts, robust, d_mono, d_stereo):
    """active errors + the (robust) chi2 of g2o's activeRobustChi2()"""
    if not P.ne:
        return np.zeros((0, 3)), np.zeros(0), 0.0
    e, _, _ = edges(kfs, pts, P.intr5, P.e_idx, P.e_obs, jac=False)
    chi_e = P.e_obs[:, 3] * (e * e).sum(-1)
    return e, chi_e, float(_rho(P, chi_e, robust, d_mono, d_stereo)[0].sum())


def _build(P, kfs, pts, e, chi_e, robust, d_mono, d_stereo, reverse):
    n = P.n
    Hpp = np.zeros((n, n)); bp = np.zeros(n)
    Hll = np.zeros((P.np_, 3, 3)); bl = np.zeros((P.np_, 3)); We = np.zeros((P.ne, 6, 3))
    if P.ne:
        _, Jp, Jk = edges(kfs, pts, P.intr5, P.e_idx, P.e_obs)
        w = _rho(P, chi_e, robust, d_mono, d_stereo)[1] * P.e_obs[:, 3]
        order = np.arange(P.ne)[::-1] if reverse else np.arange(P.ne)
        hl = w[:, None, None] * np.einsum("nra,nrb->nab", Jp, Jp); gl = -w[:, None] * np.einsum("nra,nr->na", Jp, e)
        pidx = P.e_idx[order, 0]
        for a in range(3):
            bl[:, a] = np.bincount(pidx, gl[order, a], P.np_)
            for b in range(3):
                Hll[:, a, b] = np.bincount(pidx, hl[order, a, b], P.np_)
        We = w[:, None, None] * np.einsum("nra,nrb->nab", Jk, Jp)
        fr = order[P.ef[order] >= 0]
        hk = w[:, None, None] * np.einsum("nra,nrb->nab", Jk, Jk); gk = -w[:, None] * np.einsum("nra,nr->na", Jk, e)
        rows = (6 * P.ef[fr])[:, None] + np.arange(6)[None, :]
        bp += np.bincount(rows.ravel(), gk[fr].ravel(), n)
        Hpp.ravel()[:] += np.bincount((rows[:, :, None] * n + rows[:, None, :]).ravel(), hk[fr].ravel(), n * n)
    return Hpp, bp, Hll, bl, We


def _solve_schur(P, Hpp, bp, Hll, bl, We, lam, linear, reverse):
    """BlockSolver::buildSystem's Schur complement + solve + back-substitution (block_solver.hpp:367-486)"""
    n = P.n
    inc = P.included
    D = Hll + lam * np.eye(3)
    D[~inc] = np.eye(3)
    Dinv = np.linalg.inv(D); Dinv[~inc] = 0.0
    db = np.einsum("pab,pb->pa", Dinv, bl)
    S = Hpp + lam * np.eye(n); bs = bp.copy()
    fr = np.flatnonzero(P.ef >= 0)
    if len(P.pa):
        pa, pb = (P.pa[::-1], P.pb[::-1]) if reverse else (P.pa, P.pb)
        blk = np.matmul(np.matmul(We[pa], Dinv[P.e_idx[pa, 0]]), We[pb].transpose(0, 2, 1))
        idx = P.pair_index()
        S.ravel()[:] -= np.bincount(idx.reshape(-1, 36)[::-1].ravel() if reverse else idx, blk.ravel(), n * n)
        fo = fr[::-1] if reverse else fr
        g = np.einsum("nab,nb->na", We[fo], db[P.e_idx[fo, 0]])
        bs -= np.bincount(((6 * P.ef[fo])[:, None] + np.arange(6)[None, :]).ravel(), g.ravel(), n)
    if n:
        if linear == "chol":
            try:
                L = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                return None, None
            import scipy.linalg
            xp = scipy.linalg.solve_triangular(L, scipy.linalg.solve_triangular(L, bs, lower=True), lower=True, trans=1)
        else:
            xp = np.linalg.solve(S, bs)
            if not np.all(np.isfinite(xp)):
                return None, None
    else:
        xp = np.zeros(0)
    cl = bl.copy()
    if len(fr):
        xk = xp.reshape(-1, 6)[P.ef[fr]]
        t = np.einsum("nab,na->nb", We[fr], xk)
        for c in range(3):
            cl[:, c] -= np.bincount(P.e_idx[fr, 0], t[:, c], P.np_)
    xl = np.einsum("pab,pb->pa", Dinv, cl)
    return xp, xl


def _solve_full(P, Hpp, bp, Hll, bl, We, lam):
    """the un-eliminated normal equations [[Hpp, Hpl], [Hpl^T, Hll]] + lambda I, included points only"""
    n = P.n; pts = np.flatnonzero(P.included); m = n + 3 * len(pts)
    col = {p: n + 3 * r for r, p in enumerate(pts)}
    H = np.zeros((m, m)); b = np.zeros(m)
    H[:n, :n] = Hpp; b[:n] = bp
    for p in pts:
        H[col[p]:col[p] + 3, col[p]:col[p] + 3] = Hll[p]; b[col[p]:col[p] + 3] = bl[p]
    for k in np.flatnonzero(P.ef >= 0):
        r = 6 * P.ef[k] + np.arange(6); c = col[P.e_idx[k, 0]]
        H[np.ix_(r, np.arange(c, c + 3))] += We[k]; H[np.ix_(np.arange(c, c + 3), r)] += We[k].T
    H += lam * np.eye(m)
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None, None
    x = np.linalg.solve(H, b)
    xl = np.zeros((P.np_, 3)); xl[pts] = x[n:].reshape(-1, 3)
    return x[:n], xl


def global_ba_se3(kfs, fixed, points, edge_idx, edge_obs, intr5, iterations=10, robust=True, delta2_mono=5.99, delta2_stereo=7.815,
                  stop=None, linear="chol", reverse=False):
    """One optimize(iterations) of g2o's Levenberg (optimization_algorithm_levenberg.cpp:61-189) with the termination rules of
    sparse_optimizer.cpp. stop: callable polled where g2o polls terminate(). linear: "chol" (Schur + Cholesky), "solve" (Schur +
    numpy.linalg.solve), "full" (no elimination). reverse: sum the edges in reverse order. Returns the poses, points, point_included,
    info[6] as the C ABI and `trials`: (iteration, lambda, ok, rho, accepted) per trial, `term`: (iniChi, currentChi) per iteration."""
    P = Problem(kfs, fixed, points, edge_idx, edge_obs, intr5)
    d_mono, d_stereo = _fsq(delta2_mono), _fsq(delta2_stereo)
    term = stop if stop is not None else (lambda: False)
    kf, pt = P.kfs.copy(), P.points.copy()
    res = dict(kfs=kf, points=pt, point_included=P.included.astype(np.uint8), info=np.zeros(6), trials=[], term=[], its=0)
    if term():
        return res
    lam, ni, nbad, its, ntrials, nfail = 0.0, 2.0, 0, 0, 0, 0
    e, chi_e, chi = _errors(P, kf, pt, robust, d_mono, d_stereo)
    chi_before = cur = chi
    for it in range(iterations):
        if term():
            break
        e, chi_e, cur = _errors(P, kf, pt, robust, d_mono, d_stereo)
        ini = cur
        Hpp, bp, Hll, bl, We = _build(P, kf, pt, e, chi_e, robust, d_mono, d_stereo, reverse)
        if it == 0:
            mx = max(np.abs(np.diag(Hpp)).max() if P.n else 0.0, np.abs(Hll[:, [0, 1, 2], [0, 1, 2]]).max() if P.np_ else 0.0)
            lam, ni, nbad = 1e-5 * mx, 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            kf_b, pt_b = kf, pt
            xp, xl = _solve_full(P, Hpp, bp, Hll, bl, We, lam) if linear == "full" else _solve_schur(P, Hpp, bp, Hll, bl, We, lam, linear, reverse)
            ok = xp is not None
            if ok:
                kf = retract(kf, P.free_ids, xp); pt = pt + xl
                _, _, tmp = _errors(P, kf, pt, robust, d_mono, d_stereo)
                scale = float(xp @ (lam * xp + bp) + (xl * (lam * xl + bl)).sum())
            else:
                tmp, scale, nfail = np.finfo(float).max, 0.0, nfail + 1
            scale += 1e-3
            rho = (cur - tmp) / scale
            acc = bool(rho > 0 and np.isfinite(tmp))
            res["trials"].append((it, lam, ok, rho, acc))
            if acc:
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0); lam *= max(1.0 / 3.0, alpha); ni = 2.0; cur = tmp
            else:
                lam *= ni; ni *= 2; kf, pt = kf_b, pt_b
            qmax += 1; ntrials += 1
            if not (rho < 0 and qmax < 10 and not term()):
                break
        its += 1
        res["term"].append((ini, cur))
        if qmax == 10 or rho == 0:
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            break
    res.update(kfs=kf, points=pt, its=its, info=np.array([chi_before, cur, its, ntrials, lam, nfail], float))
    return res
