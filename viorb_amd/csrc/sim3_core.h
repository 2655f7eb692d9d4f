// viorb_amd/csrc/sim3_core.h — the arithmetic of the Sim3 RANSAC solver, shared by the HIP kernels of sim3.hip and by the host-only
// hooks viorb_debug_sim3_* (the CPU test-suite compares them with tests/sim3_ref.py without a GPU; tests/cpp/sim3_core_host_test.cpp
// runs them under the address and undefined-behaviour sanitizers).
//
// What is restated (reference file:line):
//   Sim3Solver::Sim3Solver (the thresholds)                src/Sim3Solver.cc:84-88, include/Sim3Solver.h:78-79
//   Sim3Solver::iterate (the acceptance rule)              src/Sim3Solver.cc:140-207
//   Sim3Solver::ComputeCentroid / ComputeSim3              src/Sim3Solver.cc:215-337
//   Sim3Solver::CheckInliers / Project / FromCameraToImage src/Sim3Solver.cc:340-423 (one correspondence)
//   g2o::Sim3 (exp, product, inverse, map)                 Thirdparty/g2o/g2o/types/sim3.h:70-146, 233-272
//   VertexSim3Expmap::oplusImpl, both projection edges     Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:60-69, 130-171
//   the numeric Jacobian of an edge without linearizeOplus Thirdparty/g2o/g2o/core/base_binary_edge.hpp:123-200
// Float / double placement is the audit table of DESIGN.md §2 ("Sim3 solver"). The eigenvector of the 4 x 4 N is a cyclic two-sided
// Jacobi in double whose indices are all compile-time constants, so that the matrix and the vectors stay in registers.
#pragma once
#include "mapping_core.h"
#include "vio_core.h"

namespace viorb {

enum { SIM3_FOUND = 0, SIM3_CONTINUE = 1, SIM3_NO_MORE = 2, SIM3_FEW = 3 };
enum { SIM3_SET_OK = 0, SIM3_SET_FEW = 1, SIM3_SET_BAD = 2, SIM3_SET_ZERO_ROTATION = 3 };

struct Sim3K { float fx, fy, cx, cy; };

// mvnMaxError is a std::vector<size_t>: 9.210 * sigma2 (double) is truncated to an integer, and `err < mvnMaxError[i]` (:356) converts
// that integer to float. A product that no size_t holds (negative, NaN, 2^64 and more) is undefined in the reference; here it is a
// threshold of 0, under which nothing is an inlier.
MAP_HD float sim3_max_error(float sigma2) {
    const double v = 9.210 * (double)sigma2;
    return v >= 0 && v < 1.8e19 ? (float)(unsigned long long)v : 0.0f;
}

// One rotation of the two-sided Jacobi on the symmetric a (both triangles kept) and the eigenvector columns v.
template <int P, int Q> MAP_HD void sim3_jacobi_rot(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2 * apq);
    const double tt = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1));
    const double c = 1 / sqrt(tt * tt + 1), s = tt * c;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k == P || k == Q) continue;
        const double akp = c * a[k][P] - s * a[k][Q], akq = s * a[k][P] + c * a[k][Q];
        a[k][P] = akp; a[P][k] = akp; a[k][Q] = akq; a[Q][k] = akq;
    }
    a[P][P] -= tt * apq; a[Q][Q] += tt * apq;
    a[P][Q] = 0; a[Q][P] = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double vkp = c * v[k][P] - s * v[k][Q], vkq = s * v[k][P] + c * v[k][Q];
        v[k][P] = vkp; v[k][Q] = vkq;
    }
}

// Eigenvector of the largest eigenvalue of the symmetric 4 x 4 float matrix n (its upper triangle n11 n12 n13 n14 n22 n23 n24 n33 n34
// n44), rounded to float: evec.row(0) of cv::eigen (:272). Its sign is free: q and -q are the same rotation.
MAP_HD void sim3_top_eigenvector(const float (&n)[10], float (&q)[4]) {
    double a[4][4], v[4][4];
    a[0][0] = n[0]; a[0][1] = a[1][0] = n[1]; a[0][2] = a[2][0] = n[2]; a[0][3] = a[3][0] = n[3];
    a[1][1] = n[4]; a[1][2] = a[2][1] = n[5]; a[1][3] = a[3][1] = n[6];
    a[2][2] = n[7]; a[2][3] = a[3][2] = n[8]; a[3][3] = n[9];
    double fro = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) { v[i][k] = i == k ? 1.0 : 0.0; fro += a[i][k] * a[i][k]; }
    for (int sweep = 0; sweep < 30; sweep++) {
        const double off = ((a[0][1] * a[0][1] + a[0][2] * a[0][2]) + (a[0][3] * a[0][3] + a[1][2] * a[1][2])) + (a[1][3] * a[1][3] + a[2][3] * a[2][3]);
        if (off <= (DBL_EPSILON * DBL_EPSILON) * fro) break;
        sim3_jacobi_rot<0, 1>(a, v); sim3_jacobi_rot<0, 2>(a, v); sim3_jacobi_rot<0, 3>(a, v);
        sim3_jacobi_rot<1, 2>(a, v); sim3_jacobi_rot<1, 3>(a, v); sim3_jacobi_rot<2, 3>(a, v);
    }
    double best = a[0][0];
    q[0] = (float)v[0][0]; q[1] = (float)v[1][0]; q[2] = (float)v[2][0]; q[3] = (float)v[3][0];
#pragma unroll
    for (int i = 1; i < 4; i++) {
        if (a[i][i] > best) { best = a[i][i]; q[0] = (float)v[0][i]; q[1] = (float)v[1][i]; q[2] = (float)v[2][i]; q[3] = (float)v[3][i]; }
    }
}

// cv::Rodrigues of a float rotation vector: the matrix in double, stored to float.
MAP_HD void sim3_rodrigues(const float (&r)[3], float (&R)[9]) {
    const double rx0 = r[0], ry0 = r[1], rz0 = r[2];
    const double theta = sqrt((rx0 * rx0 + ry0 * ry0) + rz0 * rz0);
    if (theta < DBL_EPSILON) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
    const double rx = rx0 * it, ry = ry0 * it, rz = rz0 * it;
    R[0] = (float)(c + c1 * rx * rx);      R[1] = (float)(c1 * rx * ry - s * rz); R[2] = (float)(c1 * rx * rz + s * ry);
    R[3] = (float)(c1 * rx * ry + s * rz); R[4] = (float)(c + c1 * ry * ry);      R[5] = (float)(c1 * ry * rz - s * rx);
    R[6] = (float)(c1 * rx * rz - s * ry); R[7] = (float)(c1 * ry * rz + s * rx); R[8] = (float)(c + c1 * rz * rz);
}

// ComputeSim3 (:226-316) from three correspondences: P1[i], P2[i] = point i in camera 1 / camera 2. Returns SIM3_SET_OK, or
// SIM3_SET_ZERO_ROTATION (zero outputs) where the reference divides 0 / 0 at :280 and every comparison of :356 then fails.
MAP_HD int sim3_horn(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, float (&R)[9], float (&t)[3], float& s) {
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];       // Pr[i][k]: coordinate k of point i
#pragma unroll
    for (int k = 0; k < 3; k++) {
        // cv::reduce sums in float; C / P.cols scales by the double 1. / 3
        O1[k] = (float)((double)((P1[0][k] + P1[1][k]) + P1[2][k]) * (1.0 / 3));
        O2[k] = (float)((double)((P2[0][k] + P2[1][k]) + P2[2][k]) * (1.0 / 3));
#pragma unroll
        for (int i = 0; i < 3; i++) { Pr1[i][k] = P1[i][k] - O1[k]; Pr2[i][k] = P2[i][k] - O2[k]; }
    }
    // M = Pr2 * Pr1^T: the transposed operand takes gemm's general path, which accumulates CV_32F products in double
    float M[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            M[r][c] = (float)(((double)Pr2[0][r] * (double)Pr1[0][c] + (double)Pr2[1][r] * (double)Pr1[1][c]) + (double)Pr2[2][r] * (double)Pr1[2][c]);
    // N11 .. N44 are doubles assigned from float expressions, then stored into a CV_32F matrix (:247-265)
    float n[10];
    n[0] = M[0][0] + M[1][1] + M[2][2]; n[1] = M[1][2] - M[2][1]; n[2] = M[2][0] - M[0][2]; n[3] = M[0][1] - M[1][0];
    n[4] = M[0][0] - M[1][1] - M[2][2]; n[5] = M[0][1] + M[1][0]; n[6] = M[2][0] + M[0][2];
    n[7] = -M[0][0] + M[1][1] - M[2][2]; n[8] = M[1][2] + M[2][1]; n[9] = -M[0][0] - M[1][1] + M[2][2];
    float q[4];
    sim3_top_eigenvector(n, q);
    const double nv = sqrt(((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2]) + (double)q[3] * (double)q[3]);
    if (!(nv > 0)) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = 0.0f;
        t[0] = t[1] = t[2] = 0.0f; s = 0.0f;
        return SIM3_SET_ZERO_ROTATION;
    }
    const double ang = atan2(nv, (double)q[0]);
    const double k2 = 2 * ang / nv;
    const float rv[3] = {(float)(k2 * (double)q[1]), (float)(k2 * (double)q[2]), (float)(k2 * (double)q[3])};
    sim3_rodrigues(rv, R);
    // P3 = R * Pr2 (gemm small-matrix path: float products summed left to right in float)
    float P3[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int r = 0; r < 3; r++) P3[i][r] = (R[3 * r] * Pr2[i][0] + R[3 * r + 1] * Pr2[i][1]) + R[3 * r + 2] * Pr2[i][2];
    if (!fix_scale) {
        double nom = 0, den = 0;                   // Mat::dot in double; cv::pow(P3, 2) in float, summed in double (rows, then columns)
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int i = 0; i < 3; i++) { nom += (double)Pr1[i][r] * (double)P3[i][r]; den += (double)(P3[i][r] * P3[i][r]); }
        s = (float)(nom / den);
    } else s = 1.0f;
    // t = O1 - s * R * O2: gemm with alpha = s (the float sum scaled in double), float subtraction
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float ro = (R[3 * r] * O2[0] + R[3 * r + 1] * O2[1]) + R[3 * r + 2] * O2[2];
        t[r] = O1[r] - (float)((double)ro * (double)s);
    }
    return SIM3_SET_OK;
}

// T12 = [s R | t] and T21 = [(1 / s) R^T | -(1 / s) R^T t] (:321-336) as sR12, t12, sR21, t21.
struct Sim3Pair { float sR12[9], t12[3], sR21[9], t21[3]; };
MAP_HD void sim3_transforms(const float* R, const float* t, float s, Sim3Pair& T) {
    const double is = 1.0 / (double)s;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) { T.sR12[3 * r + c] = (float)((double)R[3 * r + c] * (double)s); T.sR21[3 * r + c] = (float)((double)R[3 * c + r] * is); }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        T.t12[r] = t[r];
        T.t21[r] = -((T.sR21[3 * r] * t[0] + T.sR21[3 * r + 1] * t[1]) + T.sR21[3 * r + 2] * t[2]);
    }
}
MAP_HD void sim3_T12(const float* R, const float* t, float s, float* T16) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) T16[4 * r + c] = (float)((double)R[3 * r + c] * (double)s);
        T16[4 * r + 3] = t[r];
    }
    T16[12] = 0.0f; T16[13] = 0.0f; T16[14] = 0.0f; T16[15] = 1.0f;
}

// FromCameraToImage (:405-423): no depth test, 1 / z in float.
MAP_HD void sim3_to_image(const Sim3K& k, float X, float Y, float Z, float& u, float& v) {
    const float invz = 1 / Z;
    const float x = X * invz, y = Y * invz;
    u = k.fx * x + k.cx; v = k.fy * y + k.cy;
}
// Project (:382-403): Rcw * X + tcw through the small-matrix gemm, then the above.
MAP_HD void sim3_project(const Sim3K& k, const float* sR, const float* t, float X, float Y, float Z, float& u, float& v) {
    const float x = ((sR[0] * X + sR[1] * Y) + sR[2] * Z) + t[0];
    const float y = ((sR[3] * X + sR[4] * Y) + sR[5] * Z) + t[1];
    const float z = ((sR[6] * X + sR[7] * Y) + sR[8] * Z) + t[2];
    sim3_to_image(k, x, y, z, u, v);
}
// One correspondence of CheckInliers (:348-363): p1 = its projection in image 1 (from X1c), p2 in image 2 (from X2c). Mat::dot is a
// double sum stored to float.
MAP_HD bool sim3_is_inlier(const Sim3K& k1, const Sim3K& k2, const Sim3Pair& T, const float* X1, const float* X2, float p1u, float p1v, float p2u,
                           float p2v, float max1, float max2, float& err1, float& err2) {
    float u, v;
    sim3_project(k1, T.sR12, T.t12, X2[0], X2[1], X2[2], u, v);
    const float a0 = p1u - u, a1 = p1v - v;
    sim3_project(k2, T.sR21, T.t21, X1[0], X1[1], X1[2], u, v);
    const float b0 = u - p2u, b1 = v - p2v;
    err1 = (float)((double)a0 * (double)a0 + (double)a1 * (double)a1);
    err2 = (float)((double)b0 * (double)b0 + (double)b1 * (double)b1);
    return err1 < max1 && err2 < max2;
}

// The loop of iterate (:158-206) over given inlier counts, from the carried state (mnIterations, mnBestInliers) = (first, best):
// counts[i] is the count of iteration i, n_counts of them exist. The kernel k_sim3_select evaluates the same rule by ballot.
struct Sim3Select { int status, iterations_done, best_inliers, best_iter; };
MAP_HD Sim3Select sim3_select(const int* counts, int n_counts, int N, int min_inliers, int max_its, int first, int best, int per_call) {
    Sim3Select r; r.status = SIM3_FEW; r.iterations_done = first; r.best_inliers = best; r.best_iter = -1;
    if (N < min_inliers) return r;
    int it = first < 0 ? 0 : first, cur = 0;
    const int stop = max_its < n_counts ? max_its : n_counts;
    while (it < stop && cur < per_call) {
        const int c = counts[it];
        cur++; it++;
        if (c >= best) {
            best = c; r.best_iter = it - 1;
            if (c > min_inliers) { r.status = SIM3_FOUND; r.iterations_done = it; r.best_inliers = best; return r; }
        }
    }
    r.iterations_done = it > first ? it : first; r.best_inliers = best;
    r.status = r.iterations_done >= max_its ? SIM3_NO_MORE : SIM3_CONTINUE;
    return r;
}

// ---- g2o::Sim3 for OptimizeSim3, all in double; the value types and the Huber routine are vio_core.h's -----------------------------
struct sim3d { quat r; d3 t; double s; };
VIO_HD d3 sim3_map(const sim3d& a, d3 p) { return qrot(a.r, p) * a.s + a.t; }
VIO_HD sim3d sim3_mul(const sim3d& a, const sim3d& b) { sim3d o; o.r = qmul(a.r, b.r); o.t = qrot(a.r, b.t) * a.s + a.t; o.s = a.s * b.s; return o; }
VIO_HD sim3d sim3_inv(const sim3d& a) { sim3d o; o.r = qconj(a.r); o.t = qrot(o.r, a.t * (-1. / a.s)); o.s = 1. / a.s; return o; }
VIO_HD sim3d sim3_ld(const double* p) { sim3d o; o.r = mkq(p[0], p[1], p[2], p[3]); o.t = mk3(p[4], p[5], p[6]); o.s = p[7]; return o; }
VIO_HD void sim3_st(double* p, const sim3d& a) { p[0] = a.r.x; p[1] = a.r.y; p[2] = a.r.z; p[3] = a.r.w; p[4] = a.t.x; p[5] = a.t.y; p[6] = a.t.z; p[7] = a.s; }
// Sim3(update = [omega, upsilon, sigma]) (sim3.h:70-142) with its four branches at |sigma|, theta < 1e-5
VIO_HD sim3d sim3_exp(const double* u) {
    const d3 om = mk3(u[0], u[1], u[2]), ups = mk3(u[3], u[4], u[5]);
    const double sigma = u[6], th = norm3(om), eps = 0.00001;
    const m33 Om = hat3(om), Om2 = mul(Om, Om);
    sim3d o; o.s = exp(sigma);
    double A, B, C;
    m33 R;
    if (fabs(sigma) < eps) {
        C = 1;
        if (th < eps) { A = 1. / 2.; B = 1. / 6.; R = add(add(eye3(), Om), Om2); }
        else {
            const double th2 = th * th;
            A = (1 - cos(th)) / th2; B = (th - sin(th)) / (th2 * th);
            R = add(add(eye3(), scl(Om, sin(th) / th)), scl(Om2, (1 - cos(th)) / (th * th)));
        }
    } else {
        C = (o.s - 1) / sigma;
        if (th < eps) {
            const double s2 = sigma * sigma;
            A = ((sigma - 1) * o.s + 1) / s2; B = ((0.5 * s2 - sigma + 1) * o.s) / (s2 * sigma);
            R = add(add(eye3(), Om), Om2);
        } else {
            R = add(add(eye3(), scl(Om, sin(th) / th)), scl(Om2, (1 - cos(th)) / (th * th)));
            const double a = o.s * sin(th), b = o.s * cos(th), th2 = th * th, s2 = sigma * sigma, c = th2 + s2;
            A = (a * sigma + (1 - b) * th) / (th * c);
            B = (C - ((b - 1) * sigma + a * th) / c) * 1. / th2;
        }
    }
    o.r = mat2q(R);
    o.t = mulv(add(add(scl(Om, A), scl(Om2, B)), scl(eye3(), C)), ups);
    return o;
}
// oplusImpl: update[6] = 0 with _fix_scale, then Sim3(update) * estimate
VIO_HD sim3d sim3_oplus(const sim3d& est, const double* u, bool fix_scale) {
    double v[7];
#pragma unroll
    for (int k = 0; k < 7; k++) v[k] = u[k];
    if (fix_scale) v[6] = 0;
    return sim3_mul(sim3_exp(v), est);
}
// the estimate after oplus of +delta (k even) / -delta (k odd) on dimension k / 2, delta = 1e-9 (base_binary_edge.hpp:150-175)
VIO_HD sim3d sim3_perturbed(const sim3d& est, int k, bool fix_scale) {
    double u[7];
#pragma unroll
    for (int d = 0; d < 7; d++) u[d] = (d == k / 2) ? ((k & 1) ? -1e-9 : 1e-9) : 0.0;
    return sim3_oplus(est, u, fix_scale);
}
// EdgeSim3ProjectXYZ (S = the estimate, X = the point of camera 2, K = camera 1) and EdgeInverseSim3ProjectXYZ (S = the INVERSE of
// the estimate, X = the point of camera 1, K = camera 2): obs - cam_map(project(S.map(X)))
VIO_HD void sim3_edge_error(const sim3d& S, d3 X, const double* K4, double u, double v, double* e) {
    const d3 p = sim3_map(S, X);
    e[0] = u - (p.x / p.z * K4[0] + K4[2]); e[1] = v - (p.y / p.z * K4[1] + K4[3]);
}

} // namespace viorb
