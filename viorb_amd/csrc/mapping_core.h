// viorb_amd/csrc/mapping_core.h — the per-pair and per-point arithmetic of map-point creation, shared by the HIP kernels of mapping.hip
// and by the host-only hooks viorb_debug_triangulate_pair / viorb_debug_map_point_update (the CPU test-suite compares them with
// tests/mapping_ref.py without a GPU). Fixed-size values live in registers: every array below is indexed by compile-time constants only.
//
// What is restated (reference file:line):
//   LocalMapping::CreateNewMapPoints, per-pair loop     src/LocalMapping.cc:1319-1464
//   KeyFrame::UnprojectStereo                           src/KeyFrame.cc:952-968
//   MapPoint::UpdateNormalAndDepth                      src/MapPoint.cc:337-378
// Float / double placement is the audit table of DESIGN.md §2 ("map-point creation"): cv::norm and Mat::dot accumulate in double,
// the small-matrix gemm sums float products in float, `s*row - row` is OpenCV's addWeighted (double), `1.0/z` is double.
// The 4 x 4 SVD is a one-sided Jacobi on the lane, held in double registers (see jacobi_rot).
#pragma once
#include <float.h>
#include "orb_math.h"               // VIORB_HD, hamming256

#define MAP_HD VIORB_HD

namespace viorb {

// reason codes of viorb_triangulate_pairs (include/viorb.h VIORB_TRI_*)
enum { TRI_ACCEPT = 0, TRI_NO_POINT = 1, TRI_BEHIND_1 = 2, TRI_BEHIND_2 = 3, TRI_REPROJ_1 = 4, TRI_REPROJ_2 = 5, TRI_SCALE = 6, TRI_NO_PAIR = 255 };

struct MapCam {
    float fx, fy, cx, cy, invfx, invfy, mb, mbf, ratio_factor;
    int nlevels;
    float sf[16], sigma2[16];
};

// One key point as the per-pair loop reads it: mvKeysUn[i].pt / .octave, mvuRight[i], mvDepth[i], mvKeys[i].pt (distorted).
struct MapKey { float u, v, ur, depth, ud, vd; int octave; };

// double-accumulated 3-vector products (cv::Mat::dot, cv::norm of CV_32F)
MAP_HD double map_dot3d(float a0, float a1, float a2, float b0, float b1, float b2) {
    return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}
MAP_HD double map_norm3d(float a0, float a1, float a2) { return sqrt(map_dot3d(a0, a1, a2, a0, a1, a2)); }

// One rotation of the one-sided (Hestenes) Jacobi on rows I < J of At (= columns of A) and of Vt: the scheme cv::SVD runs for a
// 4 x 4 matrix (inner products, rotation angle and column norms in double). cv::SVD stores the rotated CV_32F columns as float; here
// they stay in double registers until the singular vector is rounded to float at the end: with float storage every rotation perturbs
// A by eps_32 * sigma_1 and the low-parallax pairs (sigma_1 / sigma_3 of 100 and more) land 6e-5 from the definitional position, a
// hundred times outside the tolerance the tests derive from LAPACK's float32 SVD (map-point creation audit, row 9).
template <int I, int J> MAP_HD bool jacobi_rot(double (&at)[4][4], double (&vt)[4][4], double (&w)[4]) {
    const double a = w[I], b = w[J];
    double p = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) p += at[I][k] * at[J][k];
    if (fabs(p) <= (DBL_EPSILON * 2) * sqrt(a * b)) return false;
    p *= 2;
    const double beta = a - b, gamma = sqrt(p * p + beta * beta);
    double c, s;
    if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = sqrt(delta / gamma); c = p / (gamma * s * 2); }
    else { c = sqrt((gamma + beta) / (gamma * 2)); s = p / (gamma * c * 2); }
    double na = 0, nb = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double t0 = c * at[I][k] + s * at[J][k];
        const double t1 = c * at[J][k] - s * at[I][k];
        at[I][k] = t0; at[J][k] = t1;
        na += t0 * t0; nb += t1 * t1;
    }
    w[I] = na; w[J] = nb;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double t0 = c * vt[I][k] + s * vt[J][k];
        const double t1 = c * vt[J][k] - s * vt[I][k];
        vt[I][k] = t0; vt[J][k] = t1;
    }
    return true;
}

// Right singular vector of the smallest singular value of the 4 x 4 float matrix A (row-major), rounded to float into x[4] (the
// CV_32F vt.row(3) of src/LocalMapping.cc:1357-1360). All indices are compile-time constants: At, Vt and W live in registers.
MAP_HD void smallest_right_singular_vector(const float (&A)[4][4], float (&x)[4]) {
    double at[4][4], vt[4][4], w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { at[i][k] = (double)A[k][i]; vt[i][k] = (i == k) ? 1.0 : 0.0; sd += (double)A[k][i] * (double)A[k][i]; }
        w[i] = sd;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        changed |= jacobi_rot<0, 1>(at, vt, w); changed |= jacobi_rot<0, 2>(at, vt, w); changed |= jacobi_rot<0, 3>(at, vt, w);
        changed |= jacobi_rot<1, 2>(at, vt, w); changed |= jacobi_rot<1, 3>(at, vt, w); changed |= jacobi_rot<2, 3>(at, vt, w);
        if (!changed) break;
    }
    double best = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) sd += at[i][k] * at[i][k];
        const bool take = (i == 0) || sd < best;
        if (take) { best = sd; x[0] = (float)vt[i][0]; x[1] = (float)vt[i][1]; x[2] = (float)vt[i][2]; x[3] = (float)vt[i][3]; }
    }
}

// pose12 = Rcw (row-major 9) tcw (3). Twc's rotation is its transpose, its translation the camera centre Ow.
MAP_HD bool unproject_stereo(const MapCam& c, const float* T, const float* Ow, const MapKey& k, float (&X)[3]) {
    const float z = k.depth;
    if (!(z > 0)) return false;
    const float x = (k.ud - c.cx) * z * c.invfx, y = (k.vd - c.cy) * z * c.invfy;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float t = T[r] * x + T[3 + r] * y + T[6 + r] * z;
        X[r] = (float)((double)t + (double)Ow[r]);
    }
    return true;
}

// x, y, z of Rcw * X + tcw as `Rcw.row(r).dot(x3Dt) + tcw.at<float>(r)`: double dot, double add, stored to float.
MAP_HD float cam_coord(const float* T, int r, const float (&X)[3]) {
    return (float)(map_dot3d(T[3 * r], T[3 * r + 1], T[3 * r + 2], X[0], X[1], X[2]) + (double)T[9 + r]);
}

MAP_HD bool reproj_rejects(const MapCam& c, const float* T, const MapKey& k, float z, const float (&X)[3]) {
    const int oct = k.octave < 0 ? 0 : (k.octave > 15 ? 15 : k.octave);
    const float sigma2 = c.sigma2[oct];
    const float x = cam_coord(T, 0, X), y = cam_coord(T, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = c.fx * x * invz + c.cx, v = c.fy * y * invz + c.cy;
    const float ex = u - k.u, ey = v - k.v;
    if (!(k.ur >= 0)) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float u_r = u - c.mbf * invz;                      // the current key frame's mbf in both views (src/LocalMapping.cc:1439)
    const float er = u_r - k.ur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// src/LocalMapping.cc:1319-1464 for one (idx1, idx2) pair. Returns the reason code; Pw is written for TRI_ACCEPT and for every
// rejection after a point exists (reasons >= TRI_BEHIND_1), zeros otherwise.
MAP_HD int triangulate_pair(const MapCam& c, const float* T1, const float* Ow1, const float* T2, const float* Ow2, const MapKey& k1,
                            const MapKey& k2, float (&X)[3]) {
    X[0] = X[1] = X[2] = 0.0f;
    const bool st1 = k1.ur >= 0, st2 = k2.ur >= 0;
    const float xn1[3] = {(k1.u - c.cx) * c.invfx, (k1.v - c.cy) * c.invfy, 1.0f};
    const float xn2[3] = {(k2.u - c.cx) * c.invfx, (k2.v - c.cy) * c.invfy, 1.0f};
    float ray1[3], ray2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ray1[r] = T1[r] * xn1[0] + T1[3 + r] * xn1[1] + T1[6 + r] * xn1[2];
        ray2[r] = T2[r] * xn2[0] + T2[3 + r] * xn2[1] + T2[6 + r] * xn2[2];
    }
    const float cosRays = (float)(map_dot3d(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) /
                                  (map_norm3d(ray1[0], ray1[1], ray1[2]) * map_norm3d(ray2[0], ray2[1], ray2[2])));
    float cs1 = cosRays + 1.0f, cs2 = cs1;
    if (st1) cs1 = (float)cos(2.0 * atan2((double)(c.mb / 2.0f), (double)k1.depth));
    else if (st2) cs2 = (float)cos(2.0 * atan2((double)(c.mb / 2.0f), (double)k2.depth));
    const float cs = cs1 < cs2 ? cs1 : cs2;

    if (cosRays < cs && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
        float A[4][4], x[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float a0 = k < 3 ? T1[k] : T1[9], a1 = k < 3 ? T1[3 + k] : T1[10], a2 = k < 3 ? T1[6 + k] : T1[11];
            const float b0 = k < 3 ? T2[k] : T2[9], b1 = k < 3 ? T2[3 + k] : T2[10], b2 = k < 3 ? T2[6 + k] : T2[11];
            A[0][k] = (float)((double)a2 * (double)xn1[0] - (double)a0);
            A[1][k] = (float)((double)a2 * (double)xn1[1] - (double)a1);
            A[2][k] = (float)((double)b2 * (double)xn2[0] - (double)b0);
            A[3][k] = (float)((double)b2 * (double)xn2[1] - (double)b1);
        }
        smallest_right_singular_vector(A, x);
        if (x[3] == 0) return TRI_NO_POINT;
#pragma unroll
        for (int r = 0; r < 3; r++) X[r] = (float)((double)x[r] / (double)x[3]);
    } else if (st1 && cs1 < cs2) {
        if (!unproject_stereo(c, T1, Ow1, k1, X)) return TRI_NO_POINT;
    } else if (st2 && cs2 < cs1) {
        if (!unproject_stereo(c, T2, Ow2, k2, X)) return TRI_NO_POINT;
    } else
        return TRI_NO_POINT;

    const float z1 = cam_coord(T1, 2, X);
    if (!(z1 > 0)) return TRI_BEHIND_1;
    const float z2 = cam_coord(T2, 2, X);
    if (!(z2 > 0)) return TRI_BEHIND_2;
    if (reproj_rejects(c, T1, k1, z1, X)) return TRI_REPROJ_1;
    if (reproj_rejects(c, T2, k2, z2, X)) return TRI_REPROJ_2;
    const float dist1 = (float)map_norm3d(X[0] - Ow1[0], X[1] - Ow1[1], X[2] - Ow1[2]);
    const float dist2 = (float)map_norm3d(X[0] - Ow2[0], X[1] - Ow2[1], X[2] - Ow2[2]);
    if (dist1 == 0 || dist2 == 0) return TRI_SCALE;
    const int o1 = k1.octave < 0 ? 0 : (k1.octave > 15 ? 15 : k1.octave), o2 = k2.octave < 0 ? 0 : (k2.octave > 15 ? 15 : k2.octave);
    const float ratioDist = dist2 / dist1, ratioOctave = c.sf[o1] / c.sf[o2];
    if (ratioDist * c.ratio_factor < ratioOctave || ratioDist > ratioOctave * c.ratio_factor) return TRI_SCALE;
    return TRI_ACCEPT;
}

// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:354-377), one observation's term: normal += (Pw - Ow_i) / cv::norm(..)
// (float difference, double norm, float-by-double division stored to float, float sum in observation order).
MAP_HD void normal_add(const float* Pw, const float* Ow, float (&n)[3]) {
    const float d0 = Pw[0] - Ow[0], d1 = Pw[1] - Ow[1], d2 = Pw[2] - Ow[2];
    const double nrm = map_norm3d(d0, d1, d2);
    n[0] = n[0] + (float)((double)d0 / nrm); n[1] = n[1] + (float)((double)d1 / nrm); n[2] = n[2] + (float)((double)d2 / nrm);
}
// pts_f[8] = Pw3 normal3 minDist maxDist from the summed normal, the observation count and the reference key frame's data.
MAP_HD void finish_point(const float* Pw, const float (&nsum)[3], int nobs, const float* Ow_ref, float sf_level, float sf_last, float* out8) {
    const float dist = (float)map_norm3d(Pw[0] - Ow_ref[0], Pw[1] - Ow_ref[1], Pw[2] - Ow_ref[2]);
    const float maxd = dist * sf_level, mind = maxd / sf_last;
    out8[0] = Pw[0]; out8[1] = Pw[1]; out8[2] = Pw[2];
    out8[3] = (float)((double)nsum[0] / (double)nobs); out8[4] = (float)((double)nsum[1] / (double)nobs); out8[5] = (float)((double)nsum[2] / (double)nobs);
    out8[6] = mind; out8[7] = maxd;
}

} // namespace viorb
