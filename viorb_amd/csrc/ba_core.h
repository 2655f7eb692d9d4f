// viorb_amd/csrc/ba_core.h — the per-edge and per-block arithmetic of the four bundle adjustments, written once: the window solves
// viorb_local_ba_navstate / viorb_local_ba_se3 (local_ba.hip) and the map solves viorb_global_ba_navstate (global_ba.hip) /
// viorb_global_ba_se3 (global_ba_se3.hip). Host and device (VIO_HD) except the three device-only reduction helpers at the end. The library is built with
// -ffp-contract=off and everything here is inlined, so an expression rounds here exactly as it did where it was copied from; a change here
// changes all solves that use the function ("where each edge's arithmetic lives").
//
// Deliberately NOT shared, because the solves differ there on purpose:
//   * the two Cholesky designs (one-workgroup MFMA solve of the window, blocked launch chain of the map)
//   * where the Levenberg control runs (device-side ctl of the window, the host for the map); its rule is lm_core.h's
//   * the window's pair-gathered Schur complement, and the window's back-substitution: it subtracts term by term where the map's
//     subtracts a finished sum — a different rounding, hence two functions
//   * pose_opt_mp.inc and proj_edge / se3_edge of vio_core.h: the only-pose edges, which divide by z differently
//   * BaSolve, the batch drivers, the C ABI and everything above it
//
// What is restated (reference file:line):
//   EdgeNavStatePVRPointXYZ error + Jacobians           src/IMU/g2otypes.h:129-203, g2otypes.cpp:299-354
//   EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ          Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:103-234
//   VertexSE3Expmap::oplusImpl                           Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:73-76
//   BlockSolver::buildSystem / solve (Hll, Hpl, Hpp)     Thirdparty/g2o/g2o/core/block_solver.hpp:367-486
#pragma once
#include "vio_core.h"

namespace viorb {

// ---- Huber deltas: "const float th = sqrt(...)", squared in double by RobustKernelHuber. The monocular delta of the window solves is
// sqrt(5.991) (src/Optimizer.cc:1959, :4096), that of the map solves sqrt(5.99) (:174, :3595); stereo :3596 / :4097; IMU and bias
// factors :105-106 / :1877-1878. The chi2 gates of the window solves compare with the unrounded thresholds (:2045, :4207, :4223).
VIO_HD double ba_delta_mono_window() { return (double)(float)sqrt(5.991); }
VIO_HD double ba_delta_mono_map() { return (double)(float)sqrt(5.99); }
VIO_HD double ba_delta_stereo() { return (double)(float)sqrt(7.815); }
VIO_HD double ba_delta_pvr() { return (double)(float)sqrt(21.666); }
VIO_HD double ba_delta_bias() { return (double)(float)sqrt(16.812); }
#define BA_GATE_CHI2_MONO 5.991
#define BA_GATE_CHI2_STEREO 7.815
// chi2 -> (rho, rho') with or without the robust kernel
VIO_HD void ba_robust(int robust, double chi, double delta, double* r0, double* r1) {
    if (robust) huber(chi, delta, r0, r1); else { *r0 = chi; *r1 = 1.0; }
}

// position, inside a key frame's block of blk unknowns, of the r-th of the six coordinates a reprojection edge depends on:
// NavState block (12) = [P V Phi | bias] -> P at 0..2, Phi at 6..8; SE3 block (6) = [omega upsilon] -> 0..5
VIO_HD int loc6(int blk, int r) { return blk == 12 ? (r < 3 ? r : r + 3) : r; }

// ---- EdgeNavStatePVRPointXYZ: e = obs - proj(Pc); Jp[2][3] = -Jpi Rcb Rwb^T (point), Jk[2][6] = Jpi Rcb | -Jpi hat(Paux) Rcb (dP | dPhi)
struct nav_geom { d3 Pc, Paux; m33 RwbT; };
VIO_HD nav_geom ba_nav_geom(const cam_t& K, const double* kf22, const double* pt3) {
    nav_geom g;
    const pvr s = ld_pvr(kf22);
    g.RwbT = tr(qmat(s.q));
    g.Paux = mulv(K.Rcb, mulv(g.RwbT, ld3(pt3) - s.P));
    g.Pc = g.Paux - K.RcbPbc;
    return g;
}
VIO_HD void ba_nav_error(const cam_t& K, d3 Pc, const double* obs, double* e) {
    e[0] = obs[0] - (Pc.x / Pc.z * K.fx + K.cx); e[1] = obs[1] - (Pc.y / Pc.z * K.fy + K.cy);
}
VIO_HD void ba_nav_jac(const cam_t& K, const nav_geom& g, double* Jp, double* Jk) {
    const double x = g.Pc.x, y = g.Pc.y, z = g.Pc.z;
    const double j00 = K.fx / z, j02 = -x / z * K.fx / z, j11 = K.fy / z, j12 = -y / z * K.fy / z;
    const m33 RR = mul(K.Rcb, g.RwbT), HR = mul(hat3(g.Paux), K.Rcb);
    Jp[0] = -(j00 * RR.a00 + j02 * RR.a20); Jp[1] = -(j00 * RR.a01 + j02 * RR.a21); Jp[2] = -(j00 * RR.a02 + j02 * RR.a22);
    Jp[3] = -(j11 * RR.a10 + j12 * RR.a20); Jp[4] = -(j11 * RR.a11 + j12 * RR.a21); Jp[5] = -(j11 * RR.a12 + j12 * RR.a22);
    Jk[0] = j00 * K.Rcb.a00 + j02 * K.Rcb.a20; Jk[1] = j00 * K.Rcb.a01 + j02 * K.Rcb.a21; Jk[2] = j00 * K.Rcb.a02 + j02 * K.Rcb.a22;
    Jk[3] = -(j00 * HR.a00 + j02 * HR.a20); Jk[4] = -(j00 * HR.a01 + j02 * HR.a21); Jk[5] = -(j00 * HR.a02 + j02 * HR.a22);
    Jk[6] = j11 * K.Rcb.a10 + j12 * K.Rcb.a20; Jk[7] = j11 * K.Rcb.a11 + j12 * K.Rcb.a21; Jk[8] = j11 * K.Rcb.a12 + j12 * K.Rcb.a22;
    Jk[9] = -(j11 * HR.a10 + j12 * HR.a20); Jk[10] = -(j11 * HR.a11 + j12 * HR.a21); Jk[11] = -(j11 * HR.a12 + j12 * HR.a22);
}

// ---- EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ. A key frame is qx qy qz qw tx ty tz of Tcw; an observation u v uRight invSigma2
// (uRight < 0: monocular). The error is se3_edge's (vio_core.h; its Jacobian is the only-pose edges', which divide by z differently).
VIO_HD se3q se3_ld7(const double* k) { se3q s; s.r = mkq(k[0], k[1], k[2], k[3]); s.t = mk3(k[4], k[5], k[6]); return s; }
VIO_HD void se3_st7(double* k, const se3q& s) { k[0] = s.r.x; k[1] = s.r.y; k[2] = s.r.z; k[3] = s.r.w; k[4] = s.t.x; k[5] = s.t.y; k[6] = s.t.z; }
VIO_HD void se3_oplus7(double* k7, const double* u) { se3_st7(k7, se3_mul(se3_exp(u), se3_ld7(k7))); }      // VertexSE3Expmap::oplusImpl: T <- exp(u) T
VIO_HD bool ba_se3_stereo(const double* obs4) { return !(obs4[2] < 0); }
// Jp[3][3] = d e / d point (_jacobianOplusXi), Jk[3][6] = d e / d (omega, upsilon) (_jacobianOplusXj); the third rows are zero on a
// monocular edge. The point Jacobian is written as the reference writes it for each edge type: -1/z * tmp * R with the product summed
// over tmp's three columns (monocular), the closed form element by element (stereo).
VIO_HD void ba_se3_jac(const se3q& T, d3 Xw, bool stereo, double fx, double fy, double bf, double* Jp, double* Jk) {
    const d3 pc = se3_map(T, Xw);
    const m33 R = qmat(T.r);
    const double x = pc.x, y = pc.y, z = pc.z, z_2 = z * z;
    const double Rr[9] = {R.a00, R.a01, R.a02, R.a10, R.a11, R.a12, R.a20, R.a21, R.a22};
    if (!stereo) {
        const double t0[3] = {fx, 0, -x / z * fx}, t1[3] = {0, fy, -y / z * fy};
        for (int c = 0; c < 3; c++) {
            double s0 = 0, s1 = 0;
            for (int q = 0; q < 3; q++) { s0 += (-1. / z * t0[q]) * Rr[3 * q + c]; s1 += (-1. / z * t1[q]) * Rr[3 * q + c]; }
            Jp[c] = s0; Jp[3 + c] = s1; Jp[6 + c] = 0;
        }
    } else {
        for (int c = 0; c < 3; c++) {
            Jp[c] = -fx * Rr[c] / z + fx * x * Rr[6 + c] / z_2;
            Jp[3 + c] = -fy * Rr[3 + c] / z + fy * y * Rr[6 + c] / z_2;
            Jp[6 + c] = Jp[c] - bf * Rr[6 + c] / z_2;
        }
    }
    Jk[0] = x * y / z_2 * fx; Jk[1] = -(1 + (x * x / z_2)) * fx; Jk[2] = y / z * fx; Jk[3] = -1. / z * fx; Jk[4] = 0; Jk[5] = x / z_2 * fx;
    Jk[6] = (1 + y * y / z_2) * fy; Jk[7] = -x * y / z_2 * fy; Jk[8] = -x / z * fy; Jk[9] = 0; Jk[10] = -1. / z * fy; Jk[11] = y / z_2 * fy;
    if (stereo) { Jk[12] = Jk[0] - bf * y / z_2; Jk[13] = Jk[1] + bf * x / z_2; Jk[14] = Jk[2]; Jk[15] = Jk[3]; Jk[16] = 0; Jk[17] = Jk[5] - bf / z_2; }
    else { for (int q = 12; q < 18; q++) Jk[q] = 0; }
}

// ---- blocks of the normal equations from one edge with ROWS residual rows (Jp[ROWS][3], Jk[ROWS][6], weight w = rho' invSigma2)
// the edge's block of W (block_solver.hpp's Hpl): We[6][3] = w Jk^T Jp
template <int ROWS> VIO_HD void ba_w_block(double w, const double* Jk, const double* Jp, double* We) {
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = Jk[r] * Jp[c];
#pragma unroll
            for (int row = 1; row < ROWS; row++) s += Jk[6 * row + r] * Jp[3 * row + c];
            We[3 * r + c] = w * s;
        }
}
// a point's Hll (upper triangle H[6] = 00 01 02 11 12 22) += w Jp^T Jp and bl -= w Jp^T e
template <int ROWS> VIO_HD void ba_point_add(double* H, double* b, double w, const double* Jp, const double* e) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) {
            double s = Jp[i] * Jp[j];
#pragma unroll
            for (int row = 1; row < ROWS; row++) s += Jp[3 * row + i] * Jp[3 * row + j];
            H[k++] += w * s;
        }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double s = Jp[a] * e[0];
#pragma unroll
        for (int row = 1; row < ROWS; row++) s += Jp[3 * row + a] * e[row];
        b[a] -= w * s;
    }
}
VIO_HD void ba_point_store(double* Hll9, double* bl3, const double* H, const double* b) {
    Hll9[0] = H[0]; Hll9[1] = H[1]; Hll9[2] = H[2]; Hll9[3] = H[1]; Hll9[4] = H[3]; Hll9[5] = H[4]; Hll9[6] = H[2]; Hll9[7] = H[4]; Hll9[8] = H[5];
    for (int a = 0; a < 3; a++) bl3[a] = b[a];
}
// Dinv = (Hll + lambda I)^-1 by cofactors and db = Dinv bl
VIO_HD void ba_point_inverse(const double* H, double lambda, const double* bl3, double* Di, double* db3) {
    const double a = H[0] + lambda, b = H[1], c = H[2], d = H[4] + lambda, e = H[5], f = H[8] + lambda;
    const double det = a * (d * f - e * e) - b * (b * f - c * e) + c * (b * e - c * d), id = 1.0 / det;
    const double i00 = (d * f - e * e) * id, i01 = (c * e - b * f) * id, i02 = (b * e - c * d) * id, i11 = (a * f - c * c) * id, i12 = (b * c - a * e) * id, i22 = (a * d - b * b) * id;
    Di[0] = i00; Di[1] = i01; Di[2] = i02; Di[3] = i01; Di[4] = i11; Di[5] = i12; Di[6] = i02; Di[7] = i12; Di[8] = i22;
    const double b0 = bl3[0], b1 = bl3[1], b2 = bl3[2];
    db3[0] = i00 * b0 + i01 * b1 + i02 * b2; db3[1] = i01 * b0 + i11 * b1 + i12 * b2; db3[2] = i02 * b0 + i12 * b1 + i22 * b2;
}
// a key frame's 21 + 6 sums: the upper triangle of its 6 x 6 block += w Jr^T Jr, a[21..26] -= w Jr^T e, one residual row at a time
// (the window solves take the row count from BaDev at run time) or all ROWS rows of an edge
VIO_HD void ba_kf_add_row(double* a, double w, const double* Jr, double er) {
    int c = 0;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int cc = r; cc < 6; cc++) a[c++] += w * (Jr[r] * Jr[cc]);
#pragma unroll
    for (int r = 0; r < 6; r++) a[21 + r] -= w * (Jr[r] * er);
}
template <int ROWS> VIO_HD void ba_kf_add(double* a, double w, const double* Jk, const double* e) {
#pragma unroll
    for (int row = 0; row < ROWS; row++) ba_kf_add_row(a, w, Jk + 6 * row, e[row]);
}
// index in a[0..20] of element (r, c) of the 6 x 6 block
VIO_HD int ba_kf_tri(int r, int c) { const int lo = r < c ? r : c, hi = r < c ? c : r; return lo * 6 - lo * (lo - 1) / 2 + (hi - lo); }

// ---- IMU factor (EdgeNavStatePVR, pvr_edge of vio_core.h) and bias factor (EdgeNavStateBias) between key frame i and its predecessor j
VIO_HD double ba_chi9(const double* info, const double* e) {
    double chi = 0;
    for (int a = 0; a < 9; a++) { double t = 0; for (int b = 0; b < 9; b++) t += info[a * 9 + b] * e[b]; chi += e[a] * t; }
    return chi;
}
VIO_HD d3 ba_bias_error(const double* ki22, const double* kj22) { return (ld3(ki22 + 13) + ld3(ki22 + 19)) - (ld3(kj22 + 13) + ld3(kj22 + 19)); }
// robust chi2 of both factors for the error pass: rho[0] IMU, rho[1] bias; e9 / *eb receive the errors. The bias chi2 divides here and
// multiplies by the information in ba_imu_weights, as both always did: the two round differently.
VIO_HD void ba_imu_chi2(const double* ki22, const double* kj22, const double* preint_i, const double* info, d3 gw, double acc_bias_rw2, int robust,
                        double* e9, d3* eb, double* rho) {
    double r1;
    pvr_edge(ld_pvr(kj22), ld_pvr(ki22), ld3(kj22 + 16), ld3(kj22 + 19), preint_i, gw, e9, nullptr);
    ba_robust(robust, ba_chi9(info, e9), ba_delta_pvr(), &rho[0], &r1);
    *eb = ba_bias_error(ki22, kj22);
    ba_robust(robust, dot3(*eb, *eb) / acc_bias_rw2 / preint_i[141], ba_delta_bias(), &rho[1], &r1);
}
// linearisation of both factors: e9, J[9][21], the IMU factor's Huber weight, the bias error and wb = rho' / (accBiasRW2 dt)
VIO_HD void ba_imu_weights(const double* ki22, const double* kj22, const double* preint_i, const double* info, d3 gw, double acc_bias_rw2, int robust,
                           double* e9, double* J, double* w_pvr, d3* eb, double* wb) {
    double r0, r1;
    pvr_edge(ld_pvr(kj22), ld_pvr(ki22), ld3(kj22 + 16), ld3(kj22 + 19), preint_i, gw, e9, J);
    ba_robust(robust, ba_chi9(info, e9), ba_delta_pvr(), &r0, &r1); *w_pvr = r1;
    *eb = ba_bias_error(ki22, kj22);
    const double binfo = 1.0 / acc_bias_rw2 / preint_i[141];
    ba_robust(robust, binfo * dot3(*eb, *eb), ba_delta_bias(), &r0, &r1);
    *wb = r1 * binfo;
}
// OJ[9][21] = Omega J, element q of every nthreads-th by thread t
VIO_HD void ba_omega_j(const double* info, const double* J, double* OJ, int t, int nthreads) {
    for (int q = t; q < 189; q += nthreads) { const int r = q / 21, c = q % 21; double s = 0; for (int k = 0; k < 9; k++) s += info[r * 9 + k] * J[k * 21 + c]; OJ[q] = s; }
}

#if defined(__HIPCC__)
// ---- reductions over a workgroup of EXACTLY 256 threads (s_red has one slot per wavefront, four): the wave's butterfly, then the four
// partial sums in wave order. Neither ends with a barrier: a second reduction in the same kernel needs its own s_red or a
// __syncthreads() first (every call site makes one call).
__device__ __forceinline__ double ba_block_sum(double v, double* s_red) {      // s_red[4]; the result is the same in every thread
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}
__device__ __forceinline__ void ba_kf_reduce(const double* a, double (*s_red)[27]) {      // s_red[4][27]; read with ba_kf_sum after it
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 27; k++) {
        double v = a[k];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
        if ((t & 63) == 0) s_red[t >> 6][k] = v;
    }
    __syncthreads();
}
__device__ __forceinline__ double ba_kf_sum(const double (*s_red)[27], int k) { return s_red[0][k] + s_red[1][k] + s_red[2][k] + s_red[3][k]; }
#endif

} // namespace viorb
