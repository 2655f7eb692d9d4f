"""Checker of the device global bundle adjustment (viorb_global_ba_navstate, csrc/global_ba.hip): numpy, float64, TEST
INFRASTRUCTURE ONLY. It restates Optimizer::GlobalBundleAdjustmentNavState (reference src/Optimizer.cc:50-320): a PVR (9) + accelerometer
bias (3) block per key frame, marginalised points, one EdgeNavStatePVR + EdgeNavStateBias per key frame with a predecessor, one
EdgeNavStatePVRPointXYZ per observation, and one optimize(iterations) of g2o's Levenberg on the Schur complement of the point block,
solved densely. tests/test_global_ba_ref.py pins it against the oracle's window solve, the oracle's edge functions, central
differences and a solve of the full (un-eliminated) normal equations.

Flat layouts are those of include/viorb.h: navstate[22] = P3 V3 q4(x,y,z,w) bg3 ba3 dbg3 dba3, preint[142] = dP3 dV3 dR9 JPg9 JPa9 JVg9
JVa9 JRg9 cov81 dt, cam[16] = fx fy cx cy Rbc9 Pbc3. Unlike the C ABI, the Huber delta^2 of the mono edges and the iteration count
are arguments."""
import numpy as np

ACC_BIAS_RW2 = 5e-3 * 5e-3
LOC6 = np.array([0, 1, 2, 6, 7, 8])


def _fsq(v):
    return float(np.float32(np.sqrt(v)))          # "const float th = sqrt(...)": a float delta, squared in double


# ---- SO3 on quaternions (x, y, z, w) --------------------------------------------------------------------------------------------
def qnorm(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def qmul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0); bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def qconj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def qmat(q):
    x, y, z, w = np.moveaxis(q, -1, 0)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def mat2q(m):
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        s = np.sqrt(t + 1.0); r = 0.5 / s
        return np.array([(m[2, 1] - m[1, 2]) * r, (m[0, 2] - m[2, 0]) * r, (m[1, 0] - m[0, 1]) * r, 0.5 * s])
    if m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]:
        s = np.sqrt(m[0, 0] - m[1, 1] - m[2, 2] + 1.0); r = 0.5 / s
        return np.array([0.5 * s, (m[1, 0] + m[0, 1]) * r, (m[2, 0] + m[0, 2]) * r, (m[2, 1] - m[1, 2]) * r])
    if m[1, 1] > m[0, 0] and m[1, 1] >= m[2, 2]:
        s = np.sqrt(m[1, 1] - m[2, 2] - m[0, 0] + 1.0); r = 0.5 / s
        return np.array([(m[1, 0] + m[0, 1]) * r, 0.5 * s, (m[2, 1] + m[1, 2]) * r, (m[0, 2] - m[2, 0]) * r])
    s = np.sqrt(m[2, 2] - m[0, 0] - m[1, 1] + 1.0); r = 0.5 / s
    return np.array([(m[0, 2] + m[2, 0]) * r, (m[2, 1] + m[1, 2]) * r, 0.5 * s, (m[1, 0] - m[0, 1]) * r])


def so3_mul(a, b):
    return qnorm(qmul(qnorm(a), b))


def so3_exp(w):
    th = np.sqrt((w * w).sum(-1)); half = 0.5 * th
    small = th < 1e-10
    ths = np.where(small, 1.0, th)
    imag = np.where(small, 0.5 - 0.0208333 * th ** 2 + 0.000260417 * th ** 4, np.sin(half) / ths)
    return qnorm(np.concatenate([imag[..., None] * w, np.cos(half)[..., None]], -1))


def so3_log(q):
    n = np.sqrt((q[..., :3] ** 2).sum(-1)); w = q[..., 3]
    small = n < 1e-10
    ns = np.where(small, 1.0, n)
    f = np.where(small, 2.0 / w - 2.0 * n * n / (w * w * w), 2 * np.arctan(n / w) / ns)
    return f[..., None] * q[..., :3]


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], float)


def jr_inv(w):
    th = np.linalg.norm(w)
    if th < 0.00001:
        return np.eye(3)
    K = hat(w / th)
    return np.eye(3) + 0.5 * hat(w) + (1.0 - (1.0 + np.cos(th)) * th / (2.0 * np.sin(th))) * (K @ K)


# ---- edges ---------------------------------------------------------------------------------------------------------------------
def edge_pvr(ni, nj, preint, gw, jac=True):
    """EdgeNavStatePVR between key frame i (earlier; also the bias vertex) and j: e[9], J[9,21] = [d/d i(P V Phi) | d/d j | d/d dba_i]."""
    Pi, Vi, qi = ni[0:3], ni[3:6], qnorm(ni[6:10]); Pj, Vj, qj = nj[0:3], nj[3:6], qnorm(nj[6:10])
    dbg, dba = ni[16:19], ni[19:22]
    dP, dV, dR = preint[0:3], preint[3:6], preint[6:15].reshape(3, 3)
    JPg, JPa, JVg, JVa, JRg = (preint[15 + 9 * k:24 + 9 * k].reshape(3, 3) for k in range(5))
    dT = preint[141]; dT2 = dT * dT
    Ri, Rj = qmat(qi), qmat(qj)
    aP = Ri.T @ (Pj - Pi - Vi * dT - gw * (0.5 * dT2)); aV = Ri.T @ (Vj - Vi - gw * dT)
    rP = aP - (dP + JPg @ dbg + JPa @ dba); rV = aV - (dV + JVg @ dbg + JVa @ dba)
    corr = so3_mul(qnorm(mat2q(dR)), so3_exp(JRg @ dbg))
    rPhi = so3_log(so3_mul(so3_mul(qnorm(qconj(corr)), qnorm(qconj(qi))), qj))
    e = np.concatenate([rP, rV, rPhi])
    if not jac:
        return e, None
    J = np.zeros((9, 21)); Ji = jr_inv(rPhi)
    J[0:3, 0:3] = -np.eye(3); J[0:3, 3:6] = -dT * Ri.T; J[0:3, 6:9] = hat(aP)
    J[3:6, 3:6] = -Ri.T; J[3:6, 6:9] = hat(aV)
    J[6:9, 6:9] = -(Ji @ Rj.T @ Ri)
    J[0:3, 9:12] = Ri.T @ Rj; J[3:6, 12:15] = Ri.T; J[6:9, 15:18] = Ji
    J[0:3, 18:21] = -JPa; J[3:6, 18:21] = -JVa
    return e, J


def edge_proj(kfs, pts, cam, e_idx, e_obs, jac=True):
    """EdgeNavStatePVRPointXYZ of every observation at once: e [ne,2], Jp [ne,2,3] (point), Jk [ne,2,6] (dP | dPhi of the key frame)."""
    fx, fy, cx, cy = cam[:4]; Rcb = cam[4:13].reshape(3, 3).T; Pbc = cam[13:16]
    ns = kfs[e_idx[:, 1]]; Pw = pts[e_idx[:, 0]]
    Rwb = qmat(qnorm(ns[:, 6:10]))
    Paux = np.einsum("ab,nb->na", Rcb, np.einsum("nba,nb->na", Rwb, Pw - ns[:, 0:3]))
    Pc = Paux - Rcb @ Pbc
    x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
    e = np.stack([e_obs[:, 0] - (x / z * fx + cx), e_obs[:, 1] - (y / z * fy + cy)], -1)
    if not jac:
        return e, None, None, Pc
    Jpi = np.zeros((len(e), 2, 3))
    Jpi[:, 0, 0] = fx / z; Jpi[:, 0, 2] = -x / z * fx / z; Jpi[:, 1, 1] = fy / z; Jpi[:, 1, 2] = -y / z * fy / z
    RR = np.einsum("ab,ncb->nac", Rcb, Rwb)                           # Rcb Rwb^T
    H = np.zeros((len(e), 3, 3))
    H[:, 0, 1] = -Paux[:, 2]; H[:, 0, 2] = Paux[:, 1]; H[:, 1, 0] = Paux[:, 2]; H[:, 1, 2] = -Paux[:, 0]; H[:, 2, 0] = -Paux[:, 1]; H[:, 2, 1] = Paux[:, 0]
    Jp = -np.einsum("nrk,nkc->nrc", Jpi, RR)
    Jk = np.concatenate([np.einsum("nrk,kc->nrc", Jpi, Rcb), -np.einsum("nrk,nkc->nrc", Jpi, H @ Rcb)], -1)
    return e, Jp, Jk, Pc


def huber(chi, delta):
    """RobustKernelHuber: rho and rho' of an array of chi2."""
    chi = np.asarray(chi, float); d2 = delta * delta
    sq = np.sqrt(np.maximum(chi, 1e-300))
    inl = chi <= d2
    return np.where(inl, chi, 2 * sq * delta - d2), np.where(inl, 1.0, delta / sq)


def retract(kfs, free_ids, xp):
    out = kfs.copy()
    for r, i in enumerate(free_ids):
        u = xp[12 * r:12 * r + 12]
        q = qnorm(out[i, 6:10])
        out[i, 0:3] += qmat(q) @ u[0:3]; out[i, 3:6] += u[3:6]
        out[i, 6:10] = so3_mul(q, so3_exp(u[6:9])); out[i, 19:22] += u[9:12]
    return out


class Problem:
    def __init__(self, kfs, prev, fixed, preint, points, edge_idx, edge_obs, gw, cam):
        self.kfs = np.array(kfs, float).reshape(-1, 22); self.prev = np.asarray(prev, np.int64); self.fixed = np.asarray(fixed).astype(bool)
        self.preint = np.asarray(preint, float).reshape(-1, 142); self.points = np.array(points, float).reshape(-1, 3)
        self.e_idx = np.asarray(edge_idx, np.int64).reshape(-1, 2); self.e_obs = np.asarray(edge_obs, float).reshape(-1, 3)
        self.gw = np.asarray(gw, float); self.cam = np.asarray(cam, float)
        self.nk, self.np_, self.ne = len(self.kfs), len(self.points), len(self.e_idx)
        self.free_ids = np.flatnonzero(~self.fixed); self.fidx = np.full(self.nk, -1, np.int64); self.fidx[self.free_ids] = np.arange(len(self.free_ids))
        self.n = 12 * len(self.free_ids)
        self.included = np.zeros(self.np_, bool); self.included[self.e_idx[:, 0]] = True
        self.imu = [i for i in range(self.nk) if self.prev[i] >= 0]
        self.info_pvr = {i: np.linalg.inv(self.preint[i, 60:141].reshape(9, 9)) for i in self.imu}
        # ordered pairs (a, b) of edges of one point whose key frames are both free
        ef = self.fidx[self.e_idx[:, 1]]
        pa, pb = [], []
        k0 = 0
        pt = self.e_idx[:, 0]
        bounds = np.flatnonzero(np.diff(pt)) + 1
        for s, t in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [self.ne]])) if self.ne else []:
            ks = np.arange(s, t)[ef[s:t] >= 0]
            if len(ks):
                A, B = np.meshgrid(ks, ks, indexing="ij"); pa.append(A.ravel()); pb.append(B.ravel())
        self.pa = np.concatenate(pa) if pa else np.zeros(0, np.int64); self.pb = np.concatenate(pb) if pb else np.zeros(0, np.int64)
        self.ef = ef
        self._pair_idx = None

    def pair_index(self):
        """flat index into S of every element of every pair's 6 x 6 block, in pair order (the graph is fixed over the solve)"""
        if self._pair_idx is None:
            ra = (12 * self.ef[self.pa])[:, None] + LOC6[None, :]; cb = (12 * self.ef[self.pb])[:, None] + LOC6[None, :]
            self._pair_idx = (ra[:, :, None] * self.n + cb[:, None, :]).ravel()
        return self._pair_idx


def _errors(P, kfs, pts, robust, d_mono, d_pvr, d_bias):
    """active errors + the (robust) chi2 of g2o's activeRobustChi2()"""
    e, _, _, _ = edge_proj(kfs, pts, P.cam, P.e_idx, P.e_obs, jac=False) if P.ne else (np.zeros((0, 2)), 0, 0, 0)
    chi_e = P.e_obs[:, 2] * (e * e).sum(-1)
    c = (huber(chi_e, d_mono)[0] if robust else chi_e).sum() if P.ne else 0.0
    imu = {}
    for i in P.imu:
        j = P.prev[i]
        ep, _ = edge_pvr(kfs[j], kfs[i], P.preint[i], P.gw, jac=False)
        eb = (kfs[i, 13:16] + kfs[i, 19:22]) - (kfs[j, 13:16] + kfs[j, 19:22])
        chi_p = ep @ P.info_pvr[i] @ ep; chi_b = (eb @ eb) / ACC_BIAS_RW2 / P.preint[i, 141]
        imu[i] = (ep, eb, chi_p, chi_b)
        c += (float(huber(chi_p, d_pvr)[0]) + float(huber(chi_b, d_bias)[0])) if robust else (chi_p + chi_b)
    return e, chi_e, imu, float(c)


def _build(P, kfs, pts, e, chi_e, imu, robust, d_mono, d_pvr, d_bias, reverse):
    n = P.n
    Hpp = np.zeros((n, n)); bp = np.zeros(n)
    Hll = np.zeros((P.np_, 3, 3)); bl = np.zeros((P.np_, 3)); We = np.zeros((P.ne, 6, 3))
    if P.ne:
        _, Jp, Jk, _ = edge_proj(kfs, pts, P.cam, P.e_idx, P.e_obs)
        w = (huber(chi_e, d_mono)[1] if robust else np.ones(P.ne)) * P.e_obs[:, 2]
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
        rows = (12 * P.ef[fr])[:, None] + LOC6[None, :]
        bp += np.bincount(rows.ravel(), gk[fr].ravel(), n)
        Hpp.ravel()[:] += np.bincount((rows[:, :, None] * n + rows[:, None, :]).ravel(), hk[fr].ravel(), n * n)
    for i in (P.imu[::-1] if reverse else P.imu):
        j = P.prev[i]; ep, eb, chi_p, chi_b = imu[i]
        _, J = edge_pvr(kfs[j], kfs[i], P.preint[i], P.gw)
        wp = float(huber(chi_p, d_pvr)[1]) if robust else 1.0
        cols = np.full(21, -1, np.int64)
        if P.fidx[j] >= 0:
            cols[0:9] = 12 * P.fidx[j] + np.arange(9); cols[18:21] = 12 * P.fidx[j] + 9 + np.arange(3)
        if P.fidx[i] >= 0:
            cols[9:18] = 12 * P.fidx[i] + np.arange(9)
        m = cols >= 0
        OJ = P.info_pvr[i] @ J
        Hpp[np.ix_(cols[m], cols[m])] += wp * (J.T @ OJ)[np.ix_(m, m)]
        bp[cols[m]] -= wp * (OJ.T @ ep)[m]
        wb = (float(huber(chi_b, d_bias)[1]) if robust else 1.0) / ACC_BIAS_RW2 / P.preint[i, 141]
        for c in range(3):
            ic = 12 * P.fidx[i] + 9 + c if P.fidx[i] >= 0 else -1; jc = 12 * P.fidx[j] + 9 + c if P.fidx[j] >= 0 else -1
            if ic >= 0:
                Hpp[ic, ic] += wb; bp[ic] -= wb * eb[c]
            if jc >= 0:
                Hpp[jc, jc] += wb; bp[jc] += wb * eb[c]
            if ic >= 0 and jc >= 0:
                Hpp[ic, jc] -= wb; Hpp[jc, ic] -= wb
    return Hpp, bp, Hll, bl, We


def _solve_schur(P, Hpp, bp, Hll, bl, We, lam, linear, reverse):
    n = P.n
    inc = P.included
    D = Hll + lam * np.eye(3)
    D[~inc] = np.eye(3)
    Dinv = np.linalg.inv(D); Dinv[~inc] = 0.0
    db = np.einsum("pab,pb->pa", Dinv, bl)
    S = Hpp + lam * np.eye(n); bs = bp.copy()
    if len(P.pa):
        pa, pb = (P.pa[::-1], P.pb[::-1]) if reverse else (P.pa, P.pb)
        blk = np.matmul(np.matmul(We[pa], Dinv[P.e_idx[pa, 0]]), We[pb].transpose(0, 2, 1))
        idx = P.pair_index()
        S.ravel()[:] -= np.bincount(idx.reshape(-1, 36)[::-1].ravel() if reverse else idx, blk.ravel(), n * n)
        fr = np.flatnonzero(P.ef >= 0)
        if reverse:
            fr = fr[::-1]
        g = np.einsum("nab,nb->na", We[fr], db[P.e_idx[fr, 0]])
        bs -= np.bincount(((12 * P.ef[fr])[:, None] + LOC6[None, :]).ravel(), g.ravel(), n)
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
    fr = np.flatnonzero(P.ef >= 0)
    if len(fr):
        xk = xp.reshape(-1, 12)[P.ef[fr]][:, LOC6]
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
        r = 12 * P.ef[k] + LOC6; c = col[P.e_idx[k, 0]]
        H[np.ix_(r, np.arange(c, c + 3))] += We[k]; H[np.ix_(np.arange(c, c + 3), r)] += We[k].T
    H += lam * np.eye(m)
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None, None
    x = np.linalg.solve(H, b)
    xl = np.zeros((P.np_, 3)); xl[pts] = x[n:].reshape(-1, 3)
    return x[:n], xl


def global_ba(kfs, prev, fixed, preint, points, edge_idx, edge_obs, gw, cam, iterations=10, robust=True, delta2_mono=5.99,
              stop=None, linear="chol", reverse=False):
    """One optimize(iterations) of g2o's Levenberg (optimization_algorithm_levenberg.cpp:61-189) with the termination rules of
    sparse_optimizer.cpp. stop: callable polled where g2o polls terminate(). linear: "chol" (Schur + Cholesky), "solve" (Schur +
    numpy.linalg.solve), "full" (no elimination). reverse: sum the edges in reverse order. Returns the states, points, point_included,
    info[6] as the C ABI and `trials`: (iteration, lambda, ok, rho, accepted) per trial, `term`: (iniChi, currentChi) per iteration."""
    P = Problem(kfs, prev, fixed, preint, points, edge_idx, edge_obs, gw, cam)
    d_mono, d_pvr, d_bias = _fsq(delta2_mono), _fsq(21.666), _fsq(16.812)
    term = stop if stop is not None else (lambda: False)
    kf, pt = P.kfs.copy(), P.points.copy()
    res = dict(kfs=kf, points=pt, point_included=P.included.astype(np.uint8), info=np.zeros(6), trials=[], term=[], its=0)
    if term():
        return res
    lam, ni, nbad, its, ntrials, nfail = 0.0, 2.0, 0, 0, 0, 0
    e, chi_e, imu, chi = _errors(P, kf, pt, robust, d_mono, d_pvr, d_bias)
    chi_before = cur = chi
    for it in range(iterations):
        if term():
            break
        e, chi_e, imu, cur = _errors(P, kf, pt, robust, d_mono, d_pvr, d_bias)
        ini = cur
        Hpp, bp, Hll, bl, We = _build(P, kf, pt, e, chi_e, imu, robust, d_mono, d_pvr, d_bias, reverse)
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
                _, _, _, tmp = _errors(P, kf, pt, robust, d_mono, d_pvr, d_bias)
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
