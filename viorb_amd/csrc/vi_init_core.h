// viorb_amd/csrc/vi_init_core.h — FP64 arithmetic of the visual-inertial initialisation shared by the HIP kernels (vi_init.hip) and
// by the host-only hooks viorb_debug_vi_init_* that let the CPU suite compare it with tests/vi_init_ref.py without a GPU.
//
// What is restated (reference file:line):
//   EdgeGyrBias::computeError / linearizeOplus          src/IMU/g2otypes.cpp:1327-1351
//   Optimizer::OptimizeInitialGyroBias (one GN step)    src/Optimizer.cc:3138-3199
//   LocalMapping::TryInitVIO, rows of A|B and C|D       src/LocalMapping.cc:317-355, 422-463
//   Rwi from gw*, Rwi_ = Rwi Exp([dtheta_xy 0])         src/LocalMapping.cc:399-417, 498-504
//   NavState P, R, V of every key frame                 src/LocalMapping.cc:625-680, 737-784
// The reference builds the rows in CV_32F and solves with cv::SVDecomp in float; here everything is double (the audit of the initialisation), and the
// small systems are solved through their Gram matrices with a cyclic symmetric Jacobi that also yields the singular values.
// Flat layouts: twc12 = Rwc(9, row-major) twc(3) of KeyFrame::GetPoseInverse() as float; preint[142] as in vio_core.h.
#pragma once
#include "vio_core.h"

namespace viorb {

#define VI_EST_DOUBLES 48
// est[48] offsets
enum { VI_BG = 0, VI_SSTAR = 3, VI_GWSTAR = 4, VI_S = 7, VI_DTHETA = 8, VI_BA = 10, VI_RWI = 13, VI_RWI2 = 22, VI_GW = 31, VI_W4 = 34, VI_W6 = 38 };

// singular values under this fraction of the largest are not resolved by a Gram-matrix solve in double (eigenvalues of A^T A carry an
// absolute error of about 2^-53 |A|^2, i.e. singular values one of about 1.5e-8 |A|): such systems are reported, not solved
#define VI_REL_GUARD 1e-7
#define VI_ABS_GUARD 1e-10          // the reference's own guard on a singular value (src/LocalMapping.cc:372, 481)

VIO_HD m33 ldm_f(const float* p) { return mkm(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]); }
VIO_HD d3 ld3_f(const float* p) { return mk3(p[0], p[1], p[2]); }

// extrinsics as TryInitVIO derives them from Tbc (row-major 4 x 4): Rcb = Rbc^T, pcb = -Rcb pbc
struct vi_extr { m33 Rcb; d3 pcb; };
VIO_HD vi_extr vi_extrinsics(const double* Tbc16) {
    vi_extr x;
    x.Rcb = mkm(Tbc16[0], Tbc16[4], Tbc16[8], Tbc16[1], Tbc16[5], Tbc16[9], Tbc16[2], Tbc16[6], Tbc16[10]);
    x.pcb = mulv(scl(x.Rcb, -1.0), mk3(Tbc16[3], Tbc16[7], Tbc16[11]));
    return x;
}

// ---- step 1: one EdgeGyrBias at bg = 0. e = Log(dR^T Rwbi^T Rwbj), J = -JlInv(e) JRg, W = the rotation block of the pre-integration
// COVARIANCE, which is what the reference passes as the information matrix (src/Optimizer.cc:3187).
VIO_HD void vi_gyro_edge(const float* twc_i, const float* twc_j, const m33& Rcb, const double* preint, d3* e, m33* J, m33* W) {
    const m33 Rwbi = mul(ldm_f(twc_i), Rcb), Rwbj = mul(ldm_f(twc_j), Rcb);
    const m33 dR = ldm(preint + 6), JRg = ldm(preint + 51);
    const m33 E = mul(mul(tr(dR), tr(Rwbi)), Rwbj);
    *e = so3_log(qnorm(mat2q(E)));
    *J = scl(mul(so3_jr_inv(*e * -1.0), JRg), -1.0);          // JacobianLInv(w) = JacobianRInv(-w)
    const double* c = preint + 60;
    *W = mkm(c[6 * 9 + 6], c[6 * 9 + 7], c[6 * 9 + 8], c[7 * 9 + 6], c[7 * 9 + 7], c[7 * 9 + 8], c[8 * 9 + 6], c[8 * 9 + 7], c[8 * 9 + 8]);
}
// its contribution to the normal equations: H += J^T W J (9 entries, row-major), g += J^T W e
VIO_HD void vi_gyro_normal(d3 e, const m33& J, const m33& W, double* Hg12) {
    const m33 JtW = mul(tr(J), W);
    const m33 H = mul(JtW, J);
    const d3 g = mulv(JtW, e);
    Hg12[0] = H.a00; Hg12[1] = H.a01; Hg12[2] = H.a02; Hg12[3] = H.a10; Hg12[4] = H.a11; Hg12[5] = H.a12; Hg12[6] = H.a20; Hg12[7] = H.a21; Hg12[8] = H.a22;
    Hg12[9] = g.x; Hg12[10] = g.y; Hg12[11] = g.z;
}
// bg = -H^-1 g by the adjugate; false when H is singular to working precision
VIO_HD bool vi_gyro_solve(const double* Hg12, d3* bg) {
    const m33 H = ldm(Hg12);
    const d3 g = ld3(Hg12 + 9);
    const double c00 = H.a11 * H.a22 - H.a12 * H.a21, c01 = H.a12 * H.a20 - H.a10 * H.a22, c02 = H.a10 * H.a21 - H.a11 * H.a20;
    const double det = H.a00 * c00 + H.a01 * c01 + H.a02 * c02;
    const double mag = (fabs(H.a00) + fabs(H.a11) + fabs(H.a22));
    if (!(fabs(det) > 1e-30 * mag * mag * mag) || !(mag > 0)) { *bg = mk3(0, 0, 0); return false; }
    const m33 adj = mkm(c00, H.a02 * H.a21 - H.a01 * H.a22, H.a01 * H.a12 - H.a02 * H.a11,
                        c01, H.a00 * H.a22 - H.a02 * H.a20, H.a02 * H.a10 - H.a00 * H.a12,
                        c02, H.a01 * H.a20 - H.a00 * H.a21, H.a00 * H.a11 - H.a01 * H.a10);
    *bg = mulv(adj, g) * (-1.0 / det);
    return true;
}

// ---- steps 2 and 3: the three rows key frames (i, i+1, i+2) contribute. p2 / p3 = pre-integrations of key frames i+1 / i+2.
struct vi_triplet { d3 lambda, c1, c2, c3; double k, dt12, dt23; m33 R1b, R2b; };
VIO_HD vi_triplet vi_triplet_common(const float* t1, const float* t2, const float* t3, const vi_extr& X, const double* p2, const double* p3) {
    vi_triplet T;
    T.dt12 = p2[141]; T.dt23 = p3[141];
    const d3 pc1 = ld3_f(t1 + 9), pc2 = ld3_f(t2 + 9), pc3 = ld3_f(t3 + 9);
    const m33 R1 = ldm_f(t1), R2 = ldm_f(t2), R3 = ldm_f(t3);
    T.lambda = (pc2 - pc1) * T.dt23 + (pc2 - pc3) * T.dt12;
    T.k = T.dt12 * T.dt12 * T.dt23 + T.dt12 * T.dt23 * T.dt23;
    T.R1b = mul(R1, X.Rcb); T.R2b = mul(R2, X.Rcb);
    // the terms gamma and psi share: (Rc1 - Rc2) pcb dt23, (Rc3 - Rc2) pcb dt12 = -(Rc2 - Rc3) pcb dt12, and the three pre-integration terms
    T.c1 = mulv(sub(R1, R2), X.pcb) * T.dt23;
    T.c2 = mulv(sub(R3, R2), X.pcb) * T.dt12;
    T.c3 = mulv(T.R1b, ld3(p2)) * T.dt23 - mulv(T.R2b, ld3(p3)) * T.dt12 - mulv(T.R1b, ld3(p2 + 3)) * (T.dt12 * T.dt23);
    return T;
}
// rows [3][5] of A | B: lambda s + beta gw = gamma (src/LocalMapping.cc:345-347)
VIO_HD void vi_rows_ab(const vi_triplet& T, double* r15) {
    const d3 gamma = T.c2 + T.c1 + T.c3;
    const double beta = 0.5 * T.k;
    const double l[3] = {T.lambda.x, T.lambda.y, T.lambda.z}, g[3] = {gamma.x, gamma.y, gamma.z};
#pragma unroll
    for (int r = 0; r < 3; r++) {
        r15[5 * r] = l[r];
#pragma unroll
        for (int c = 0; c < 3; c++) r15[5 * r + 1 + c] = (r == c) ? beta : 0.0;
        r15[5 * r + 4] = g[r];
    }
}
// rows [3][7] of C | D: lambda s + phi dtheta_xy + zeta ba = psi (src/LocalMapping.cc:451-455, with the reference's two signs)
VIO_HD void vi_rows_cd(const vi_triplet& T, const double* p2, const double* p3, const m33& Rwi, double G, double* r21) {
    const m33 phi = scl(mul(Rwi, hat3(mk3(0, 0, G))), -0.5 * T.k);
    const m33 zeta = sub(add(scl(mul(T.R2b, ldm(p3 + 24)), T.dt12), scl(mul(T.R1b, ldm(p2 + 42)), T.dt12 * T.dt23)), scl(mul(T.R1b, ldm(p2 + 24)), T.dt23));
    const d3 psi = T.c1 + T.c2 + T.c3 - mulv(Rwi, mk3(0, 0, G)) * (0.5 * T.k);
    const double l[3] = {T.lambda.x, T.lambda.y, T.lambda.z}, ps[3] = {psi.x, psi.y, psi.z};
    const double ph[9] = {phi.a00, phi.a01, phi.a02, phi.a10, phi.a11, phi.a12, phi.a20, phi.a21, phi.a22};
    const double ze[9] = {zeta.a00, zeta.a01, zeta.a02, zeta.a10, zeta.a11, zeta.a12, zeta.a20, zeta.a21, zeta.a22};
#pragma unroll
    for (int r = 0; r < 3; r++) {
        r21[7 * r] = l[r]; r21[7 * r + 1] = ph[3 * r]; r21[7 * r + 2] = ph[3 * r + 1];
#pragma unroll
        for (int c = 0; c < 3; c++) r21[7 * r + 3 + c] = ze[3 * r + c];
        r21[7 * r + 6] = ps[r];
    }
}
// packed upper triangle of [M | v]^T [M | v] restricted to what the solve needs: G = M^T M (N (N + 1) / 2 entries, row by row) then M^T v (N)
template <int N> VIO_HD void vi_gram_add(const double* rows /* 3 x (N + 1) */, double* acc /* N (N + 1) / 2 + N */) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        int o = 0;
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = i; j < N; j++) acc[o++] += rows[(N + 1) * r + i] * rows[(N + 1) * r + j];
#pragma unroll
        for (int i = 0; i < N; i++) acc[o++] += rows[(N + 1) * r + i] * rows[(N + 1) * r + N];
    }
}

// Least squares through the Gram matrix: eigen-decomposition of G by cyclic Jacobi (every index static: registers on the device),
// w = sqrt(eigenvalues) sorted descending (the singular values of M), x = V diag(1 / lambda) V^T (M^T v).
// Returns 0, or 1 when the smallest singular value is under VI_ABS_GUARD or under VI_REL_GUARD of the largest (x and w are still written
// where they are finite; callers zero them).
template <int N> VIO_HD int vi_gram_solve(const double* acc, double* x, double* w) {
    double a[N][N], v[N][N];
    {
        int o = 0;
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = i; j < N; j++) { a[i][j] = acc[o]; a[j][i] = acc[o]; o++; }
    }
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) v[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; sweep++) {
        double off = 0, dia = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            dia += a[i][i] * a[i][i];
#pragma unroll
            for (int j = i + 1; j < N; j++) off += a[i][j] * a[i][j];
        }
        if (!(off > 1e-36 * dia)) break;
#pragma unroll
        for (int p = 0; p < N - 1; p++) {
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (fabs(theta) > 1e150) ? 0.5 / theta : ((theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                a[p][p] -= t * apq; a[q][q] += t * apq; a[p][q] = 0.0; a[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    if (k != p && k != q) {
                        const double akp = a[k][p], akq = a[k][q];
                        a[k][p] = c * akp - s * akq; a[p][k] = a[k][p];
                        a[k][q] = s * akp + c * akq; a[q][k] = a[k][q];
                    }
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
    double lam[N], lmax = 0, lmin = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        lam[i] = a[i][i] > 0 ? a[i][i] : 0.0;
        lmax = (i == 0 || lam[i] > lmax) ? lam[i] : lmax;
        lmin = (i == 0 || lam[i] < lmin) ? lam[i] : lmin;
    }
    const double wmax = sqrt(lmax), wmin = sqrt(lmin);
    const bool bad = !(wmin >= VI_ABS_GUARD) || !(wmin >= VI_REL_GUARD * wmax);
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
        double d = 0;
#pragma unroll
        for (int i = 0; i < N; i++) d += v[i][k] * acc[N * (N + 1) / 2 + i];
        d = lam[k] > 0 ? d / lam[k] : 0.0;
#pragma unroll
        for (int i = 0; i < N; i++) x[i] += v[i][k] * d;
    }
    // singular values, descending (a fixed compare-exchange network over static indices)
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = sqrt(lam[i]);
#pragma unroll
    for (int pass = 0; pass < N - 1; pass++)
#pragma unroll
        for (int i = 0; i < N - 1 - pass; i++) {
            const double hi = w[i] > w[i + 1] ? w[i] : w[i + 1], lo = w[i] > w[i + 1] ? w[i + 1] : w[i];
            w[i] = hi; w[i + 1] = lo;
        }
    return bad ? 1 : 0;
}

// Rwi from the approximate gravity gw* (src/LocalMapping.cc:399-416): gI = [0 0 1], vhat = gI x gwn / |gI x gwn|, theta = atan2(|gI x gwn|, gI . gwn).
// false when gw* is zero or parallel to gI (the reference divides by zero there).
VIO_HD bool vi_rwi_from_gravity(d3 gwstar, m33* Rwi) {
    const double n = norm3(gwstar);
    if (!(n > 0)) return false;
    const d3 gwn = gwstar * (1.0 / n);
    const d3 c = mk3(-gwn.y, gwn.x, 0.0);
    const double nc = norm3(c);
    if (!(nc > 0)) return false;
    const double theta = atan2(nc, gwn.z);
    *Rwi = qmat(so3_exp((c * (1.0 / nc)) * theta));
    return true;
}

// ---- writing the estimate back (src/LocalMapping.cc:625-680, 737-784) ---------------------------------------------------------------
// NavState position and rotation of a key frame: P = s wPc + Rwc pcb, R = Rwc Rcb as the unit quaternion SetNavStateRot stores
VIO_HD void vi_kf_pose(const float* twc, const vi_extr& X, double s, d3* P, quat* q) {
    const m33 Rwc = ldm_f(twc);
    *P = ld3_f(twc + 9) * s + mulv(Rwc, X.pcb);
    *q = qnorm(mat2q(mul(Rwc, X.Rcb)));
}
// velocity from the pre-integration of the NEXT interval (:659, :765); zero when that interval has no duration
VIO_HD d3 vi_vel_forward(const float* twc, const float* twc_next, const vi_extr& X, double s, const double* preint_next, d3 ba, d3 gw) {
    const double dt = preint_next[141];
    if (!(dt > 0)) return mk3(0, 0, 0);
    const m33 Rwc = ldm_f(twc), Rn = ldm_f(twc_next);
    const d3 sum = (ld3_f(twc + 9) - ld3_f(twc_next + 9)) * s + mulv(sub(Rwc, Rn), X.pcb)
                 + mulv(mul(Rwc, X.Rcb), ld3(preint_next) + mulv(ldm(preint_next + 24), ba)) + ((gw * 0.5) * dt) * dt;
    return sum * (-1.0 / dt);
}
// velocity of the newest key frame from its predecessor's (:677, :780): V = Vprev + gw dt + Rprev (dv + Jvba ba)
VIO_HD d3 vi_vel_backward(d3 Vprev, quat qprev, const double* preint_cur, d3 ba, d3 gw) {
    const double dt = preint_cur[141];
    return Vprev + gw * dt + mulv(qmat(qprev), ld3(preint_cur + 3) + mulv(ldm(preint_cur + 42), ba));
}
// V of key frame i of a stream with N key frames in the estimate and K >= N in all. Pv: the pre-integrations the reference reads for
// the key frames of the estimate (i + 1 < N, and N - 1's own); Pf: the final ones, read for the key frames inserted afterwards.
VIO_HD d3 vi_kf_velocity(int i, int N, int K, const float* T, const vi_extr& X, double s, const double* Pv, const double* Pf, d3 ba, d3 gw) {
    d3 Pd; quat qp;
    if (i != N - 1 && i < K - 1) return vi_vel_forward(T + 12 * i, T + 12 * (i + 1), X, s, (i + 1 < N ? Pv : Pf) + (size_t)142 * (i + 1), ba, gw);
    // the newest key frame of the estimate, from N - 2
    vi_kf_pose(T + 12 * (N - 2), X, s, &Pd, &qp);
    const d3 Vset = vi_vel_backward(vi_vel_forward(T + 12 * (N - 2), T + 12 * (N - 1), X, s, Pv + (size_t)142 * (N - 1), ba, gw), qp, Pv + (size_t)142 * (N - 1), ba, gw);
    if (i == N - 1) return Vset;
    // the newest key frame of all (i = K - 1 > N - 1), from K - 2
    const d3 Vprev = (K - 2 == N - 1) ? Vset : vi_vel_forward(T + 12 * (K - 2), T + 12 * (K - 1), X, s, Pf + (size_t)142 * (K - 1), ba, gw);
    vi_kf_pose(T + 12 * (K - 2), X, s, &Pd, &qp);
    return vi_vel_backward(Vprev, qp, Pf + (size_t)142 * (K - 1), ba, gw);
}

} // namespace viorb
