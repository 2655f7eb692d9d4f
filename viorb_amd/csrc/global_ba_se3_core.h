// viorb_amd/csrc/global_ba_se3_core.h — what the vision-only global bundle adjustment (global_ba_se3.hip) shares between host and
// device: its limit, the argument predicates both forms apply, and the two binary edges with both Jacobians.
//
// What is restated (reference file:line):
//   Optimizer::BundleAdjustment                          src/Optimizer.cc:3559-3747
//   EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ          Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:103-234
// The SE3Quat algebra and the error of both edges (with the stereo projection's float reciprocal depth) are those of vio_core.h
// (se3_edge; its Jacobian is the only-pose edges', which divide by z differently, so the binary edges' is written out here); the Levenberg step and the Huber kernel those of global_ba_core.h.
#pragma once
#include "global_ba_core.h"

#define GBA_SE3_MAX_FREE_KF 4096       // documented limit: a reduced system of order 24576, as the NavState solve's

namespace viorb {

VIO_HD se3q gba_ld_se3(const double* k) { se3q s; s.r = mkq(k[0], k[1], k[2], k[3]); s.t = mk3(k[4], k[5], k[6]); return s; }
VIO_HD void gba_st_se3(double* k, const se3q& s) { k[0] = s.r.x; k[1] = s.r.y; k[2] = s.r.z; k[3] = s.r.w; k[4] = s.t.x; k[5] = s.t.y; k[6] = s.t.z; }

// "const float thHuber3D = sqrt(7.815)" (src/Optimizer.cc:3596), squared in double by the kernel; the monocular delta is gba_delta_mono()
VIO_HD double gba_delta_stereo() { return (double)(float)sqrt(7.815); }
VIO_HD bool gba_se3_stereo(const double* obs4) { return !(obs4[2] < 0); }
VIO_HD double gba_se3_delta(const double* obs4) { return gba_se3_stereo(obs4) ? gba_delta_stereo() : gba_delta_mono(); }
// a stereo edge needs a baseline (VIORB_ERR_INVALID_ARG otherwise)
VIO_HD bool gba_se3_obs_ok(const double* obs4, double bf) { return !gba_se3_stereo(obs4) || bf > 0.0; }

// error e[3] (e[2] = 0 on a monocular edge); returns the edge's dimension
VIO_HD int gba_se3_error(const double* kf7, const double* pt3, const double* obs4, const double* intr5, double* e) {
    return se3_edge(gba_ld_se3(kf7), ld3(pt3), obs4[0], obs4[1], obs4[2], intr5[0], intr5[1], intr5[2], intr5[3], intr5[4], false, e, nullptr);
}
// error and both Jacobians: Jp[3][3] = d e / d point (_jacobianOplusXi), Jk[3][6] = d e / d (omega, upsilon) (_jacobianOplusXj); the third
// rows are zero on a monocular edge. The point Jacobian is written as the reference writes it for each edge type: -1/z * tmp * R with
// the product summed over tmp's three columns (monocular), the closed form element by element (stereo).
VIO_HD int gba_se3_lin(const double* kf7, const double* pt3, const double* obs4, const double* intr5, double* e, double* Jp, double* Jk) {
    const se3q T = gba_ld_se3(kf7);
    const double fx = intr5[0], fy = intr5[1], bf = intr5[4];
    const int dim = se3_edge(T, ld3(pt3), obs4[0], obs4[1], obs4[2], fx, fy, intr5[2], intr5[3], bf, false, e, nullptr);
    const d3 pc = se3_map(T, ld3(pt3));
    const m33 R = qmat(T.r);
    const double x = pc.x, y = pc.y, z = pc.z, z_2 = z * z;
    const double Rr[9] = {R.a00, R.a01, R.a02, R.a10, R.a11, R.a12, R.a20, R.a21, R.a22};
    if (dim == 2) {
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
    if (dim == 3) { Jk[12] = Jk[0] - bf * y / z_2; Jk[13] = Jk[1] + bf * x / z_2; Jk[14] = Jk[2]; Jk[15] = Jk[3]; Jk[16] = 0; Jk[17] = Jk[5] - bf / z_2; }
    else for (int c = 12; c < 18; c++) Jk[c] = 0;
    return dim;
}

} // namespace viorb
