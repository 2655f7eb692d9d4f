"""Numpy checker of the essential-graph solve (Optimizer::OptimizeEssentialGraph, reference src/Optimizer.cc:4313-4587), written from the
reference's text: g2o's Sim3::log (Thirdparty/g2o/g2o/types/sim3.h:148-230), EdgeSim3::computeError (types_seven_dof_expmap.h:106-114),
the numeric Jacobians of base_binary_edge.hpp:131-200, a dense solve of H + lambda I, and the Levenberg control of
optimization_algorithm_levenberg.cpp:61-164 with the iteration and stop rules of sparse_optimizer.cpp as the library's gba_run states
them. The Sim3 exponential, product, inverse and oplus are tests/sim3_ref.py's; the per-edge arithmetic is also written batched over
edges ([n, ...] arrays) so that a graph of a hundred key frames takes seconds.

Two Jacobian modes, as optimize_sim3 has: "numeric" is g2o's (error = (C * Si) * Sj^-1, column = scalar * (e+ - e-)); "numeric2" is the
same central difference with another evaluation order (error = C * (Si * Sj^-1), column = scalar * e+ - scalar * e-). The second exists
only to measure what the rounding of the differences moves: the quotient amplifies a rounding of 1e-16 |e| by 1 / (2 delta) = 5e8.

A Sim3 is 8 doubles r(x y z w) t s. A problem is what synth.make_essential_graph_problem returns."""
import numpy as np
from sim3_ref import sim3_exp, sim3_mul, sim3_inv, sim3_oplus, sim3_pack, sim3_unpack, GPU_FACTOR, BAND_FACTOR, CHI2_TOL  # noqa: F401

f64 = np.float64
EG_DELTA = 1e-9
LAMBDA_INIT = 1e-16                    # setUserLambdaInit (src/Optimizer.cc:4327)
ITERATIONS = 20
# What the rounding of the numeric differences moves, "numeric" against "numeric2", over tests/essential_graph_cases.py; measured by
# tests/test_essential_graph_ref.py on every run and set just above the largest value it sees:
#   EG_S_DEV    |difference| of the eight numbers of a Scw_out row, relative to max(1, |t|) of that row
#   EG_T_DEV    the same for the twelve numbers of a Tcw_out row
#   EG_P_DEV    |difference| of a points_out coordinate (float32) relative to max(1, |P|)
#   EG_CHI_DEV  |chi2_numeric - chi2_numeric2| / max(chi2, EG_CHI_ABS)
EG_S_DEV = 2.0e-5
EG_T_DEV = 2.0e-5
EG_P_DEV = 2.0e-5
EG_CHI_DEV = 3.0e-7
EG_CHI_ABS = 1e-18                     # a chi2 below it is zero: the squared rounding of a consistent graph's errors


# ---- batched g2o::Sim3 over [n] -----------------------------------------------------------------------------------------------------------
def _bq(S):
    return S[..., 0:4], S[..., 4:7], S[..., 7]


def bqmul(a, b):
    return np.stack([a[..., 3] * b[..., 0] + a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 3] * b[..., 1] + a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 3] * b[..., 2] + a[..., 2] * b[..., 3] + a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0],
                     a[..., 3] * b[..., 3] - a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2]], -1)


def bqrot(q, v):
    qv = q[..., :3]
    uv = 2 * np.cross(qv, v)
    return v + q[..., 3:4] * uv + np.cross(qv, uv)


def bmul(A, B):
    """Sim3 * Sim3 on [..., 8] rows: r = ra rb, t = sa (ra tb) + ta, s = sa sb."""
    ra, ta, sa = _bq(A); rb, tb, sb = _bq(B)
    return np.concatenate([bqmul(ra, rb), sa[..., None] * bqrot(ra, tb) + ta, (sa * sb)[..., None]], -1)


def binv(A):
    r, t, s = _bq(A)
    rc = r * np.array([-1, -1, -1, 1.0])
    return np.concatenate([rc, bqrot(rc, (-1.0 / s)[..., None] * t), (1.0 / s)[..., None]], -1)


def bmap(A, X):
    r, t, s = _bq(A)
    return s[..., None] * bqrot(r, X) + t


def brotmat(q):
    """Eigen's Quaterniond::toRotationMatrix (no normalisation) on [n, 4]: [n, 3, 3]."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def lu_solve3(W, t):
    """W.lu().solve(t) of [n, 3, 3], [n, 3]: Eigen's PartialPivLU (first largest |entry| at or below the diagonal, rows below divided by
    the pivot, trailing update) and the row-wise unit-lower / upper substitutions."""
    A = np.concatenate([W, t[..., None]], -1).astype(f64).copy()      # [n, 3, 4] rows with their right-hand side
    n = len(A); idx = np.arange(n)
    for k in range(2):
        p = k + np.argmax(np.abs(A[:, k:, k]), 1)                  # argmax returns the first maximum
        rows_k, rows_p = A[idx, k].copy(), A[idx, p].copy()
        A[idx, k], A[idx, p] = rows_p, rows_k
        piv = A[:, k, k]
        for r in range(k + 1, 3):
            with np.errstate(divide="ignore", invalid="ignore"):
                l = np.where(piv != 0, A[:, r, k] / piv, A[:, r, k])
            A[:, r, k] = l
            for c in range(k + 1, 3):
                A[:, r, c] = A[:, r, c] - l * A[:, k, c]
    b0 = A[:, 0, 3]
    y1 = A[:, 1, 3] - A[:, 1, 0] * b0
    y2 = A[:, 2, 3] - (A[:, 2, 0] * b0 + A[:, 2, 1] * y1)
    with np.errstate(divide="ignore", invalid="ignore"):
        x2 = y2 / A[:, 2, 2]
        x1 = (y1 - A[:, 1, 2] * x2) / A[:, 1, 1]
        x0 = (b0 - (A[:, 0, 1] * x1 + A[:, 0, 2] * x2)) / A[:, 0, 0]
    return np.stack([x0, x1, x2], -1)


def _skew(v):
    O = np.zeros(v.shape[:-1] + (3, 3))
    O[..., 0, 1], O[..., 0, 2], O[..., 1, 2] = -v[..., 2], v[..., 1], -v[..., 0]
    O[..., 1, 0], O[..., 2, 0], O[..., 2, 1] = v[..., 2], -v[..., 1], v[..., 0]
    return O


def blog(S):
    """Sim3::log of [n, 8]: [n, 7] = omega, upsilon, sigma, with its four branches at |sigma| < 1e-5 and d > 1 - 1e-5."""
    S = np.asarray(S, f64).reshape(-1, 8)
    r, t, s = _bq(S)
    with np.errstate(all="ignore"):
        sigma = np.log(s)
        R = brotmat(r)
        d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
        dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
        eps = 0.00001
        small_s, small_r = np.abs(sigma) < eps, d > 1 - eps
        theta = np.arccos(d)
        theta2 = theta * theta
        omega = np.where(small_r[:, None], 0.5 * dR, (theta / (2 * np.sqrt(1 - d * d)))[:, None] * dR)
        sigma2 = sigma * sigma
        C = np.where(small_s, 1.0, (s - 1) / sigma)
        a, b, c = s * np.sin(theta), s * np.cos(theta), theta2 + sigma * sigma
        A = np.where(small_s, np.where(small_r, 1. / 2., (1 - np.cos(theta)) / theta2),
                     np.where(small_r, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(small_s, np.where(small_r, 1. / 6., (theta - np.sin(theta)) / (theta2 * theta)),
                     np.where(small_r, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2))
        Om = _skew(omega)
        W = A[:, None, None] * Om + (B[:, None, None] * Om) @ Om + C[:, None, None] * np.eye(3)
        ups = lu_solve3(W, t)
    return np.concatenate([omega, ups, sigma[:, None]], -1)


def sim3_log(S8):
    return blog(np.asarray(S8, f64).reshape(1, 8))[0]


def log_branch(S8):
    """(|sigma| < eps, d > 1 - eps) of a Sim3: which of the four branches log takes."""
    S8 = np.asarray(S8, f64)
    R = brotmat(S8[None, :4])[0]
    return bool(abs(np.log(S8[7])) < 1e-5), bool(0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1) > 1 - 1e-5)


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------
def measurements(prob):
    """Sji = Sjw * Swi, both operands from Scw (edge_corrected) or from Smeas: [ne, 8]."""
    ei = prob["edge_idx"].reshape(-1, 2)
    if not len(ei):
        return np.zeros((0, 8))
    Sc, Sm = np.asarray(prob["Scw"], f64), np.asarray(prob["Smeas"], f64)
    return np.where(np.asarray(prob["edge_corrected"]).astype(bool)[:, None], bmul(Sc[ei[:, 1]], binv(Sc[ei[:, 0]])), bmul(Sm[ei[:, 1]], binv(Sm[ei[:, 0]])))


def edge_errors(C, Si, Sj, mode="numeric"):
    """log(C * Si * Sj^-1) of [n, 8] rows: [n, 7]."""
    if mode == "numeric2":
        return blog(bmul(C, bmul(Si, binv(Sj))))
    return blog(bmul(bmul(C, Si), binv(Sj)))


def _pack(S):
    return sim3_pack(S)


def edge_jacobians(C, Si, Sj, fix_scale, fixed_i, fixed_j, mode="numeric"):
    """(Ji, Jj) [n, 7, 7] (row = error row, column = increment) of g2o's central differences through oplusImpl; a fixed side: zeros."""
    n = len(C)
    Ji, Jj = np.zeros((n, 7, 7)), np.zeros((n, 7, 7))
    scalar = 1.0 / (2 * EG_DELTA)
    ident = (np.array([0, 0, 0, 1.0]), np.zeros(3), 1.0)
    for d in range(7):
        u = np.zeros(7); u[d] = EG_DELTA
        P = _pack(sim3_oplus(ident, u, fix_scale))[None]             # Sim3(update) itself: oplus is Sim3(update) * estimate
        M = _pack(sim3_oplus(ident, -u, fix_scale))[None]
        for J, side in ((Ji, 0), (Jj, 1)):
            free = ~(fixed_j if side else fixed_i)
            if not free.any():
                continue
            if side == 0:
                ep, em = edge_errors(C[free], bmul(P, Si[free]), Sj[free], mode), edge_errors(C[free], bmul(M, Si[free]), Sj[free], mode)
            else:
                ep, em = edge_errors(C[free], Si[free], bmul(P, Sj[free]), mode), edge_errors(C[free], Si[free], bmul(M, Sj[free]), mode)
            J[free, :, d] = scalar * (ep - em) if mode == "numeric" else scalar * ep - scalar * em
    return Ji, Jj


def one_edge(Si8, Sj8, C8, fix_scale, fixed_i, fixed_j, mode="numeric"):
    a = lambda v: np.asarray(v, f64).reshape(1, 8)
    e = edge_errors(a(C8), a(Si8), a(Sj8), mode)[0]
    Ji, Jj = edge_jacobians(a(C8), a(Si8), a(Sj8), fix_scale, np.array([bool(fixed_i)]), np.array([bool(fixed_j)]), mode)
    return e, Ji[0], Jj[0]


# ---- the solve ---------------------------------------------------------------------------------------------------------------------------
def recover(prob, S):
    """Tcw_out [nk, 12] = R row-major, t / s; points_out float32 = correctedSwr.map(Srw.map(P)), Srw the INPUT Scw of the reference."""
    R = brotmat(S[:, :4]).reshape(-1, 9)
    T = np.concatenate([R, S[:, 4:7] * (1. / S[:, 7])[:, None]], 1)
    pts = np.asarray(prob.get("points", np.zeros((0, 3), np.float32)), np.float32).reshape(-1, 3)
    out = pts.copy()
    if len(pts):
        ref = np.asarray(prob["point_ref"], np.int64)
        m = ref >= 0
        out[m] = bmap(binv(S[ref[m]]), bmap(prob["Scw"][ref[m]], pts[m].astype(f64))).astype(np.float32)
    return T, out


def optimize(prob, mode="numeric", iterations=ITERATIONS):
    """dict(Scw_out, Tcw_out, points_out, info [6]; per trial: accepted, rel_change = |chi2_before - chi2_trial| / max(chi2_before, tiny),
    iteration_of, chi2_before_trial)."""
    S = np.array(prob["Scw"], f64).reshape(-1, 8).copy()
    nk = len(S)
    fixed = np.asarray(prob["fixed"]).astype(bool)
    ei = np.asarray(prob["edge_idx"], np.int64).reshape(-1, 2)
    fs = bool(prob["fix_scale"])
    Cm = measurements(prob)
    deg = np.bincount(ei.ravel(), minlength=nk) if len(ei) else np.zeros(nk, int)
    fidx = np.where(~fixed, np.cumsum(~fixed) - 1, -1)
    n = 7 * int((~fixed).sum())
    active = (~fixed) & (deg > 0)                                   # a free vertex without an edge is not in g2o's active set

    def chi2(S):
        e = edge_errors(Cm, S[ei[:, 0]], S[ei[:, 1]]) if len(ei) else np.zeros((0, 7))
        return e, float((e * e).sum())

    def linearise(S, e):
        H, b = np.zeros((n, n)), np.zeros(n)
        if len(ei):
            Ji, Jj = edge_jacobians(Cm, S[ei[:, 0]], S[ei[:, 1]], fs, fixed[ei[:, 0]], fixed[ei[:, 1]], mode)
            for k, (i, j) in enumerate(ei):
                ri, rj = fidx[i], fidx[j]
                if ri >= 0:
                    H[7 * ri:7 * ri + 7, 7 * ri:7 * ri + 7] += Ji[k].T @ Ji[k]; b[7 * ri:7 * ri + 7] -= Ji[k].T @ e[k]
                if rj >= 0:
                    H[7 * rj:7 * rj + 7, 7 * rj:7 * rj + 7] += Jj[k].T @ Jj[k]; b[7 * rj:7 * rj + 7] -= Jj[k].T @ e[k]
                if ri >= 0 and rj >= 0:
                    H[7 * ri:7 * ri + 7, 7 * rj:7 * rj + 7] += Ji[k].T @ Jj[k]; H[7 * rj:7 * rj + 7, 7 * ri:7 * ri + 7] += Jj[k].T @ Ji[k]
        for v in np.nonzero((~fixed) & (deg == 0))[0]:
            H[7 * fidx[v]:7 * fidx[v] + 7, 7 * fidx[v]:7 * fidx[v] + 7] = np.eye(7)
        return H, b

    e, cur = chi2(S)
    chi_before = cur
    lam, ni = LAMBDA_INIT, 2.0
    its = trials = nfail = nbad = 0
    accepted, rel, it_of, chi_of = [], [], [], []
    for it in range(iterations):
        H, b = linearise(S, e)
        ini, bak = cur, S.copy()
        qmax, rho = 0, 0.0
        while True:
            A = H + lam * np.eye(n)
            for v in np.nonzero((~fixed) & (deg == 0))[0]:
                A[7 * fidx[v]:7 * fidx[v] + 7, 7 * fidx[v]:7 * fidx[v] + 7] = np.eye(7)
            ok = True
            try:
                L = np.linalg.cholesky(A)
                x = np.linalg.solve(L.T, np.linalg.solve(L, b))
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                scale = 0.0
                for v in np.nonzero(active)[0]:
                    xv, bv = x[7 * fidx[v]:7 * fidx[v] + 7], b[7 * fidx[v]:7 * fidx[v] + 7]
                    scale += float(xv @ (lam * xv + bv))
                    S[v] = _pack(sim3_oplus(sim3_unpack(S[v]), xv, fs))
                e_t, tmp = chi2(S)
            else:
                nfail += 1; tmp, scale = np.finfo(f64).max, 0.0
            scale += 1e-3
            rho = (cur - tmp) / scale
            acc = bool(rho > 0 and np.isfinite(tmp))
            rel.append(abs(cur - tmp) / max(cur, np.finfo(f64).tiny)); accepted.append(acc); it_of.append(it); chi_of.append(cur)
            if acc:
                alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                lam *= max(alpha, 1. / 3.); ni = 2.0; cur = tmp; e = e_t
            else:
                lam *= ni; ni *= 2; S = bak.copy()
            qmax += 1; trials += 1
            if not (rho < 0 and qmax < 10):
                break
        its += 1
        if qmax == 10 or rho == 0:
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            break
    T, P = recover(prob, S)
    return dict(Scw_out=S, Tcw_out=T, points_out=P, info=np.array([chi_before, cur, its, trials, lam, nfail], f64), accepted=accepted, rel_change=rel,
                iteration_of=it_of, chi2_before_trial=chi_of)


def decidable_prefix(res, floor):
    """The number of leading trials whose outcome is decided by more than rounding: up to, not including, the first trial whose relative
    chi2 change in the checker is below `floor`, or whose chi2 is itself zero (below EG_CHI_ABS, where the relative change is a quotient
    of two roundings)."""
    for k, r in enumerate(res["rel_change"]):
        if r < floor or res["chi2_before_trial"][k] < EG_CHI_ABS:
            return k
    return len(res["rel_change"])


def deviations(a, b):
    """(s_dev, t_dev, p_dev, chi_dev) between two results of one problem, in the units of EG_*_DEV."""
    sc = np.maximum(1.0, np.linalg.norm(a["Scw_out"][:, 4:7], axis=1))[:, None]
    s_dev = float((np.abs(a["Scw_out"] - b["Scw_out"]) / sc).max())
    tsc = np.maximum(1.0, np.linalg.norm(a["Tcw_out"][:, 9:12], axis=1))[:, None]
    t_dev = float((np.abs(a["Tcw_out"] - b["Tcw_out"]) / tsc).max())
    pa, pb = a["points_out"].astype(f64), b["points_out"].astype(f64)
    p_dev = float((np.abs(pa - pb) / np.maximum(1.0, np.linalg.norm(pa, axis=1))[:, None]).max()) if len(pa) else 0.0
    chi_dev = abs(a["info"][1] - b["info"][1]) / max(a["info"][1], EG_CHI_ABS)
    return s_dev, t_dev, p_dev, chi_dev
