// viorb_amd/csrc/global_ba_core.h — what the global bundle adjustment (global_ba.hip) shares between host and device: sizes, the
// argument predicates both the host form (before any GPU call) and the device form (in a kernel) apply, the reprojection edge's
// linearisation, the 9 x 9 inverse behind the IMU factor's information matrix and the Levenberg step of g2o.
//
// What is restated (reference file:line):
//   Optimizer::GlobalBundleAdjustmentNavState           src/Optimizer.cc:50-320
//   EdgeNavStatePVRPointXYZ error + Jacobians           src/IMU/g2otypes.h:129-203, g2otypes.cpp:299-354
//   OptimizationAlgorithmLevenberg::solve               Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-164
// The IMU factor, the retraction and the Huber kernel are those of vio_core.h.
#pragma once
#include <float.h>
#include <cmath>
#include "vio_core.h"

#define GBA_NB 64                      // block order of the Cholesky: tile factor, panel solve and trailing update work on 64 x 64 tiles
#define GBA_MAX_FREE_KF 2048           // documented limit: a reduced system of order 24576 (4.8 GB); more returns VIORB_ERR_CAPACITY
#define GBA_ACC_BIAS_RW2 (5e-3 * 5e-3) // IMUData::_accBiasRW2 (src/IMU/imudata.cpp)

namespace viorb {

// position, inside a key frame's [P V Phi | bias] block, of the r-th coordinate a reprojection edge depends on (P 0..2, Phi 6..8)
VIO_HD int gba_loc(int r) { return r < 3 ? r : r + 3; }
VIO_HD int gba_ld(int n) { return ((n > 0 ? n : 1) + GBA_NB - 1) / GBA_NB * GBA_NB; }

// argument predicates (include/viorb.h: VIORB_ERR_INVALID_ARG)
VIO_HD bool gba_prev_ok(int prev_i, int i) { return prev_i >= -1 && prev_i < i; }
VIO_HD bool gba_edge_ok(int pt, int kf, int pt_before, int np, int nk) { return pt >= 0 && pt < np && kf >= 0 && kf < nk && pt >= pt_before; }

// Gauss-Jordan with partial pivoting; false when a pivot is exactly zero
VIO_HD bool gba_inverse9(const double* a_in, double* inv) {
    double a[81];
    for (int i = 0; i < 81; i++) { a[i] = a_in[i]; inv[i] = (i / 9 == i % 9) ? 1.0 : 0.0; }
    for (int col = 0; col < 9; col++) {
        int p = col; double best = fabs(a[col * 9 + col]);
        for (int i = col + 1; i < 9; i++) if (fabs(a[i * 9 + col]) > best) { best = fabs(a[i * 9 + col]); p = i; }
        if (!(best > 0.0)) return false;
        if (p != col) for (int j = 0; j < 9; j++) { double t = a[p * 9 + j]; a[p * 9 + j] = a[col * 9 + j]; a[col * 9 + j] = t; t = inv[p * 9 + j]; inv[p * 9 + j] = inv[col * 9 + j]; inv[col * 9 + j] = t; }
        const double iv = 1.0 / a[col * 9 + col];
        for (int j = 0; j < 9; j++) { a[col * 9 + j] *= iv; inv[col * 9 + j] *= iv; }
        for (int i = 0; i < 9; i++) if (i != col) { const double f = a[i * 9 + col]; if (f == 0) continue; for (int j = 0; j < 9; j++) { a[i * 9 + j] -= f * a[col * 9 + j]; inv[i * 9 + j] -= f * inv[col * 9 + j]; } }
    }
    return true;
}

// EdgeNavStatePVRPointXYZ: e = obs - proj(Pc); Jp[2][3] = -Jpi Rcb Rwb^T (point), Jk[2][6] = Jpi Rcb | -Jpi hat(Paux) Rcb (dP | dPhi)
VIO_HD void gba_proj_error(const cam_t& K, const double* kf22, const double* pt3, const double* obs, double* e) {
    const pvr s = ld_pvr(kf22);
    const d3 Pc = mulv(K.Rcb, mulv(tr(qmat(s.q)), ld3(pt3) - s.P)) - K.RcbPbc;
    e[0] = obs[0] - (Pc.x / Pc.z * K.fx + K.cx); e[1] = obs[1] - (Pc.y / Pc.z * K.fy + K.cy);
}
VIO_HD void gba_proj_lin(const cam_t& K, const double* kf22, const double* pt3, double* Jp, double* Jk) {
    const pvr s = ld_pvr(kf22);
    const m33 RT = tr(qmat(s.q));
    const d3 Paux = mulv(K.Rcb, mulv(RT, ld3(pt3) - s.P)), Pc = Paux - K.RcbPbc;
    const double x = Pc.x, y = Pc.y, z = Pc.z;
    const double j00 = K.fx / z, j02 = -x / z * K.fx / z, j11 = K.fy / z, j12 = -y / z * K.fy / z;
    const m33 RR = mul(K.Rcb, RT), HR = mul(hat3(Paux), K.Rcb);
    Jp[0] = -(j00 * RR.a00 + j02 * RR.a20); Jp[1] = -(j00 * RR.a01 + j02 * RR.a21); Jp[2] = -(j00 * RR.a02 + j02 * RR.a22);
    Jp[3] = -(j11 * RR.a10 + j12 * RR.a20); Jp[4] = -(j11 * RR.a11 + j12 * RR.a21); Jp[5] = -(j11 * RR.a12 + j12 * RR.a22);
    Jk[0] = j00 * K.Rcb.a00 + j02 * K.Rcb.a20; Jk[1] = j00 * K.Rcb.a01 + j02 * K.Rcb.a21; Jk[2] = j00 * K.Rcb.a02 + j02 * K.Rcb.a22;
    Jk[3] = -(j00 * HR.a00 + j02 * HR.a20); Jk[4] = -(j00 * HR.a01 + j02 * HR.a21); Jk[5] = -(j00 * HR.a02 + j02 * HR.a22);
    Jk[6] = j11 * K.Rcb.a10 + j12 * K.Rcb.a20; Jk[7] = j11 * K.Rcb.a11 + j12 * K.Rcb.a21; Jk[8] = j11 * K.Rcb.a12 + j12 * K.Rcb.a22;
    Jk[9] = -(j11 * HR.a10 + j12 * HR.a20); Jk[10] = -(j11 * HR.a11 + j12 * HR.a21); Jk[11] = -(j11 * HR.a12 + j12 * HR.a22);
}

// Huber deltas: "const float th = sqrt(...)", squared in double by the kernel. The mono edges use 5.99 here (src/Optimizer.cc:198),
// not the window solve's 5.991.
VIO_HD double gba_delta_mono() { return (double)(float)sqrt(5.99); }
VIO_HD double gba_delta_pvr() { return (double)(float)sqrt(21.666); }
VIO_HD double gba_delta_bias() { return (double)(float)sqrt(16.812); }
// chi2 -> (rho, rho') with or without the robust kernel
VIO_HD void gba_robust(int robust, double chi, double delta, double* r0, double* r1) {
    if (robust) huber(chi, delta, r0, r1); else { *r0 = chi; *r1 = 1.0; }
}

// One Levenberg trial's decision (optimization_algorithm_levenberg.cpp:104-141). In: the chi2 before the trial, the trial's chi2
// (DBL_MAX after a failed factorisation), sum x (lambda x + b). Updates lambda / ni; returns rho; *accepted tells whether the state stays.
struct gba_lm { double lambda, ni, cur; };
inline double gba_lm_trial(gba_lm& L, double tmp, double scale, bool* accepted) {
    scale += 1e-3;
    const double rho = (L.cur - tmp) / scale;
    *accepted = rho > 0 && std::isfinite(tmp);
    if (*accepted) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
        L.lambda *= (alpha > 1. / 3. ? alpha : 1. / 3.); L.ni = 2; L.cur = tmp;
    } else { L.lambda *= L.ni; L.ni *= 2; }
    return rho;
}

} // namespace viorb
