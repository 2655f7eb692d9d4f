// viorb_amd/csrc/two_view_core.h — the arithmetic of the two-view initialiser, shared by the HIP kernels of two_view.hip and by the
// host-only hooks viorb_debug_two_view_* (the CPU test-suite compares them with tests/two_view_ref.py without a GPU; tests/cpp/
// two_view_core_host_test.cpp runs them under the address and undefined-behaviour sanitizers).
//
// What is restated (reference file:line):
//   Initializer::Normalize                                src/Initializer.cc:749-795
//   Initializer::ComputeH21 / ComputeF21                  src/Initializer.cc:226-303
//   Initializer::CheckHomography / CheckFundamental       src/Initializer.cc:305-468 (one match)
//   Initializer::ReconstructH (the eight motions)         src/Initializer.cc:584-686
//   Initializer::DecomposeE                               src/Initializer.cc:909-929
//   Initializer::CheckRT / Triangulate (one match)        src/Initializer.cc:734-747, 798-894
// Float / double placement is the audit table of DESIGN.md §2 ("two-view initialisation"). The 9-column null-space solve is a
// one-sided Jacobi whose columns are spread over nine lanes (TvCol is one lane's share, all in double registers); the host form
// walks the same rotation schedule over an array of nine TvCol, so both give the same bits. The 3 x 3 SVDs are a one-sided
// Jacobi in double on one lane; the 4 x 4 of the triangulation is mapping_core.h's.
#pragma once
#include "mapping_core.h"

namespace viorb {

enum { TV_FAILED = 0, TV_FROM_H = 1, TV_FROM_F = 2 };
enum { TV_REASON_OK = 0, TV_REASON_FEW_MATCHES = 1, TV_REASON_BAD_SET = 2, TV_REASON_NO_MODEL = 3, TV_REASON_H_DEGENERATE = 4,
       TV_REASON_NO_WINNER = 5, TV_REASON_FEW_GOOD = 6, TV_REASON_PARALLAX = 7 };
// CheckRT verdict of one match: not counted, counted (in nGood, point stored), counted and flagged in vbGood (cosParallax < 0.99998)
enum { TV_RT_NONE = 0, TV_RT_COUNTED = 1, TV_RT_TRIANGULATED = 2 };

// ---- 3 x 3 helpers (row-major) -----------------------------------------------------------------------------------------------
// cv::gemm on CV_32F 3 x 3: float products summed in float, left to right
MAP_HD void tv_mul33(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
MAP_HD void tv_mul33_tn(const float* A, const float* B, float* C) {           // A^T * B
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}
MAP_HD double tv_det33(const float* M) {                                     // cv::determinant of CV_32F: double
    return (double)M[0] * ((double)M[4] * M[8] - (double)M[5] * M[7]) - (double)M[1] * ((double)M[3] * M[8] - (double)M[5] * M[6]) +
           (double)M[2] * ((double)M[3] * M[7] - (double)M[4] * M[6]);
}
// cv::Mat::inv() of a 3 x 3 CV_32F: cofactors and determinant in double, stored to float. False (and zeros) for det == 0.
MAP_HD bool tv_inv33(const float* M, float* R) {
    const double d = tv_det33(M);
    if (d == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = 0.0f;
        return false;
    }
    const double id = 1.0 / d;
    R[0] = (float)(((double)M[4] * M[8] - (double)M[5] * M[7]) * id);
    R[1] = (float)(((double)M[2] * M[7] - (double)M[1] * M[8]) * id);
    R[2] = (float)(((double)M[1] * M[5] - (double)M[2] * M[4]) * id);
    R[3] = (float)(((double)M[5] * M[6] - (double)M[3] * M[8]) * id);
    R[4] = (float)(((double)M[0] * M[8] - (double)M[2] * M[6]) * id);
    R[5] = (float)(((double)M[2] * M[3] - (double)M[0] * M[5]) * id);
    R[6] = (float)(((double)M[3] * M[7] - (double)M[4] * M[6]) * id);
    R[7] = (float)(((double)M[1] * M[6] - (double)M[0] * M[7]) * id);
    R[8] = (float)(((double)M[0] * M[4] - (double)M[1] * M[3]) * id);
    return true;
}

// ---- Normalize ---------------------------------------------------------------------------------------------------------------
// nrm4 = meanX meanY sX sY of one frame (sums in double, DESIGN.md audit row 1). T = [sX 0 -meanX sX; 0 sY -meanY sY; 0 0 1].
MAP_HD void tv_norm_finish_mean(double sx, double sy, int n, float* nrm4) { nrm4[0] = (float)(sx / n); nrm4[1] = (float)(sy / n); }
MAP_HD void tv_norm_finish_dev(double dx, double dy, int n, float* nrm4) {
    const float mdx = (float)(dx / n), mdy = (float)(dy / n);
    nrm4[2] = (float)(1.0 / (double)mdx); nrm4[3] = (float)(1.0 / (double)mdy);
}
MAP_HD void tv_norm_T(const float* nrm4, float* T) {
    T[0] = nrm4[2]; T[1] = 0.0f; T[2] = -nrm4[0] * nrm4[2];
    T[3] = 0.0f; T[4] = nrm4[3]; T[5] = -nrm4[1] * nrm4[3];
    T[6] = 0.0f; T[7] = 0.0f; T[8] = 1.0f;
}
MAP_HD void tv_norm_point(const float* nrm4, float x, float y, float& xn, float& yn) { xn = (x - nrm4[0]) * nrm4[2]; yn = (y - nrm4[1]) * nrm4[3]; }

// ---- entries of A ------------------------------------------------------------------------------------------------------------
// Column c of the two rows one pair contributes to ComputeH21's A (:239-257) and of its row of ComputeF21's A (:281-289), as selects on
// scalars: a lane picks its column without an addressed array.
MAP_HD void tv_entry_h(int c, float u1, float v1, float u2, float v2, float& e0, float& e1) {
    const int m = c % 3;
    const float b = m == 0 ? u1 : (m == 1 ? v1 : 1.0f);
    e0 = c < 3 ? 0.0f : (c < 6 ? -b : v2 * b);
    e1 = c < 3 ? b : (c < 6 ? 0.0f : -u2 * b);
}
MAP_HD float tv_entry_f(int c, float u1, float v1, float u2, float v2) {
    const int m = c % 3;
    const float b = m == 0 ? u1 : (m == 1 ? v1 : 1.0f);
    return c < 3 ? u2 * b : (c < 6 ? v2 * b : b);
}
MAP_HD void tv_rows_h(float u1, float v1, float u2, float v2, float (&r0)[9], float (&r1)[9]) {
    for (int c = 0; c < 9; c++) tv_entry_h(c, u1, v1, u2, v2, r0[c], r1[c]);
}
MAP_HD void tv_row_f(float u1, float v1, float u2, float v2, float (&r)[9]) {
    for (int c = 0; c < 9; c++) r[c] = tv_entry_f(c, u1, v1, u2, v2);
}

// ---- the 9-column one-sided Jacobi, one column per lane ------------------------------------------------------------------------
// One lane's share: column c of A (M rows, M = 16 for H and 8 for F), row c of Vt and the column's squared norm.
template <int M> struct TvCol { double a[M]; double v[9]; double w; };

// Round-robin schedule over ten players (nine columns and a bye): in round r (0..8) column l meets tv_partner(l, r); column r rests.
MAP_HD int tv_partner(int l, int r) { return l == r ? -1 : (2 * r - l + 18) % 9; }

// The rotation of columns I < J (mapping_core.h's jacobi_rot, the scheme of cv::SVD): false when the pair is already orthogonal.
MAP_HD bool tv_rot_cs(double wI, double wJ, double p, double& c, double& s) {
    if (fabs(p) <= (DBL_EPSILON * 2) * sqrt(wI * wJ)) return false;
    p *= 2;
    const double beta = wI - wJ, gamma = sqrt(p * p + beta * beta);
    // jacobi_rot's two branches as selects (the same operations on either side): nothing here is addressed, so nothing goes to scratch
    const bool neg = beta < 0;
    const double first = neg ? sqrt(((gamma - beta) * 0.5) / gamma) : sqrt((gamma + beta) / (gamma * 2));
    const double second = p / (gamma * first * 2);
    c = neg ? second : first; s = neg ? first : second;
    return true;
}
template <int M> MAP_HD double tv_col_dot(const TvCol<M>& x, const TvCol<M>& y) {
    double p = 0;
#pragma unroll
    for (int k = 0; k < M; k++) p += x.a[k] * y.a[k];
    return p;
}
// mine <- its side of the rotation with `other`; lower: mine is column I (the smaller index)
template <int M> MAP_HD void tv_col_rotate(TvCol<M>& mine, const TvCol<M>& other, double c, double s, bool lower) {
    double n = 0;
#pragma unroll
    for (int k = 0; k < M; k++) {
        const double t = lower ? c * mine.a[k] + s * other.a[k] : c * mine.a[k] - s * other.a[k];
        mine.a[k] = t; n += t * t;
    }
    mine.w = n;
#pragma unroll
    for (int k = 0; k < 9; k++) mine.v[k] = lower ? c * mine.v[k] + s * other.v[k] : c * mine.v[k] - s * other.v[k];
}
template <int M> MAP_HD void tv_col_init(TvCol<M>& col, int c) {
    double n = 0;
#pragma unroll
    for (int k = 0; k < M; k++) n += col.a[k] * col.a[k];
    col.w = n;
#pragma unroll
    for (int k = 0; k < 9; k++) col.v[k] = (k == c) ? 1.0 : 0.0;
}
enum { TV_MAX_SWEEPS = 30 };

// The host form: A [M][9] float (row-major) -> vt.row(8) rounded to float. The same rounds, pairs and arithmetic as the nine lanes.
template <int M> inline void tv_null9_host(const float (*A)[9], float* x9) {
    TvCol<M> col[9];
    for (int c = 0; c < 9; c++) { for (int k = 0; k < M; k++) col[c].a[k] = (double)A[k][c]; tv_col_init(col[c], c); }
    for (int sweep = 0; sweep < TV_MAX_SWEEPS; sweep++) {
        bool changed = false;
        for (int r = 0; r < 9; r++) {
            TvCol<M> next[9];
            for (int l = 0; l < 9; l++) {
                next[l] = col[l];
                const int q = tv_partner(l, r);
                if (q < 0) continue;
                const bool lower = l < q;
                const double p = tv_col_dot(col[l], col[q]);
                double c = 1, s = 0;
                if (!tv_rot_cs(lower ? col[l].w : col[q].w, lower ? col[q].w : col[l].w, p, c, s)) continue;
                tv_col_rotate(next[l], col[q], c, s, lower);
                changed = true;
            }
            for (int l = 0; l < 9; l++) col[l] = next[l];
        }
        if (!changed) break;
    }
    int best = 0;
    for (int c = 1; c < 9; c++) if (col[c].w < col[best].w) best = c;
    for (int k = 0; k < 9; k++) x9[k] = (float)col[best].v[k];
}

// ---- 3 x 3 SVD, one-sided Jacobi in double on one lane ---------------------------------------------------------------------------
// A = U diag(w) Vt, w descending. at[i] = column i of A (rotated in place to sigma_i u_i), vt[i] = row i of Vt.
template <int I, int J> MAP_HD bool tv_rot3(double (&at)[3][3], double (&vt)[3][3], double (&w)[3]) {
    const double p = (at[I][0] * at[J][0] + at[I][1] * at[J][1]) + at[I][2] * at[J][2];
    double c, s;
    if (!tv_rot_cs(w[I], w[J], p, c, s)) return false;
    double na = 0, nb = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double t0 = c * at[I][k] + s * at[J][k], t1 = c * at[J][k] - s * at[I][k];
        at[I][k] = t0; at[J][k] = t1; na += t0 * t0; nb += t1 * t1;
        const double v0 = c * vt[I][k] + s * vt[J][k], v1 = c * vt[J][k] - s * vt[I][k];
        vt[I][k] = v0; vt[J][k] = v1;
    }
    w[I] = na; w[J] = nb;
    return true;
}
template <int I, int J> MAP_HD void tv_sort3(double (&at)[3][3], double (&vt)[3][3], double (&w)[3]) {
    if (w[I] < w[J]) {
        double t = w[I]; w[I] = w[J]; w[J] = t;
#pragma unroll
        for (int k = 0; k < 3; k++) { t = at[I][k]; at[I][k] = at[J][k]; at[J][k] = t; t = vt[I][k]; vt[I][k] = vt[J][k]; vt[J][k] = t; }
    }
}
// U (row-major), w, Vt (row-major) in double. A third singular value below 1e-9 of the first leaves its left vector to the cross
// product of the other two (an essential matrix built from a rank-2 F).
MAP_HD void tv_svd33(const float* A, double (&U)[9], double (&w)[3], double (&Vt)[9]) {
    double at[3][3], vt[3][3], n[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int k = 0; k < 3; k++) { at[i][k] = (double)A[3 * k + i]; vt[i][k] = (i == k) ? 1.0 : 0.0; }
        n[i] = (at[i][0] * at[i][0] + at[i][1] * at[i][1]) + at[i][2] * at[i][2];
    }
    for (int sweep = 0; sweep < TV_MAX_SWEEPS; sweep++) {
        bool changed = false;
        changed |= tv_rot3<0, 1>(at, vt, n); changed |= tv_rot3<0, 2>(at, vt, n); changed |= tv_rot3<1, 2>(at, vt, n);
        if (!changed) break;
    }
    tv_sort3<0, 1>(at, vt, n); tv_sort3<0, 2>(at, vt, n); tv_sort3<1, 2>(at, vt, n);
#pragma unroll
    for (int i = 0; i < 3; i++) { w[i] = sqrt(n[i]); Vt[3 * i] = vt[i][0]; Vt[3 * i + 1] = vt[i][1]; Vt[3 * i + 2] = vt[i][2]; }
    double u[3][3];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const double inv = w[i] > 0 ? 1.0 / w[i] : 0.0;
        u[i][0] = at[i][0] * inv; u[i][1] = at[i][1] * inv; u[i][2] = at[i][2] * inv;
    }
    if (w[2] > 1e-9 * w[0]) { const double inv = 1.0 / w[2]; u[2][0] = at[2][0] * inv; u[2][1] = at[2][1] * inv; u[2][2] = at[2][2] * inv; }
    else { u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1]; u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2]; u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0]; }
#pragma unroll
    for (int i = 0; i < 3; i++) { U[i] = u[i][0]; U[3 + i] = u[i][1]; U[6 + i] = u[i][2]; }      // U[3 r + i] = component r of left vector i
}

// ---- hypotheses from the null vector --------------------------------------------------------------------------------------------
// ComputeF21's second half: SVD of Fpre, smallest singular value zeroed, recomposed (src/Initializer.cc:296-302).
MAP_HD void tv_f_rank2(const float* Fpre, float* Fn) {
    double U[9], w[3], Vt[9];
    tv_svd33(Fpre, U, w, Vt);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Fn[3 * i + j] = (float)(U[3 * i] * w[0] * Vt[j] + U[3 * i + 1] * w[1] * Vt[3 + j]);
}
// H21i = T2inv * Hn * T1, H12i = H21i.inv() (:160-161)
MAP_HD void tv_h_denorm(const float* Hn, const float* nrm1, const float* nrm2, float* H21, float* H12) {
    float T1[9], T2[9], T2inv[9], tmp[9];
    tv_norm_T(nrm1, T1); tv_norm_T(nrm2, T2); tv_inv33(T2, T2inv);
    tv_mul33(T2inv, Hn, tmp); tv_mul33(tmp, T1, H21);
    tv_inv33(H21, H12);
}
// F21i = T2^T * Fn * T1 (:212)
MAP_HD void tv_f_denorm(const float* Fn, const float* nrm1, const float* nrm2, float* F21) {
    float T1[9], T2[9], tmp[9];
    tv_norm_T(nrm1, T1); tv_norm_T(nrm2, T2);
    tv_mul33_tn(T2, Fn, tmp); tv_mul33(tmp, T1, F21);
}

// ---- scores: one match -----------------------------------------------------------------------------------------------------------
// chi2[0] = chiSquare1, chi2[1] = chiSquare2 of CheckHomography (:352-374). Returns the score contribution; inlier: both pass.
MAP_HD float tv_score_h(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float invSigmaSquare, float (&chi2)[2], bool& inlier) {
    const float th = 5.991f;
    float score = 0.0f;
    const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float sd1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    chi2[0] = sd1 * invSigmaSquare;
    const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float sd2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    chi2[1] = sd2 * invSigmaSquare;
    inlier = true;
    if (chi2[0] > th) inlier = false; else score += th - chi2[0];
    if (chi2[1] > th) inlier = false; else score += th - chi2[1];
    return score;
}
// CheckFundamental (:428-454)
MAP_HD float tv_score_f(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare, float (&chi2)[2], bool& inlier) {
    const float th = 3.841f, thScore = 5.991f;
    float score = 0.0f;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2], b2 = F[3] * u1 + F[4] * v1 + F[5], c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    chi2[0] = (num2 * num2 / (a2 * a2 + b2 * b2)) * invSigmaSquare;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6], b1 = F[1] * u2 + F[4] * v2 + F[7], c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    chi2[1] = (num1 * num1 / (a1 * a1 + b1 * b1)) * invSigmaSquare;
    inlier = true;
    if (chi2[0] > th) inlier = false; else score += thScore - chi2[0];
    if (chi2[1] > th) inlier = false; else score += thScore - chi2[1];
    return score;
}
MAP_HD float tv_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// ---- motion hypotheses -----------------------------------------------------------------------------------------------------------
struct TvK { float fx, fy, cx, cy; };
MAP_HD void tv_K(const TvK& k, float* K) { K[0] = k.fx; K[1] = 0.0f; K[2] = k.cx; K[3] = 0.0f; K[4] = k.fy; K[5] = k.cy; K[6] = 0.0f; K[7] = 0.0f; K[8] = 1.0f; }

MAP_HD void tv_unit3(const float* t, float* out) {                            // t / cv::norm(t)
    const double n = map_norm3d(t[0], t[1], t[2]);
    out[0] = (float)((double)t[0] / n); out[1] = (float)((double)t[1] / n); out[2] = (float)((double)t[2] / n);
}

// DecomposeE after E = K^T F K (:479-486, 909-929): the four motions in the order (R1, t) (R2, t) (R1, -t) (R2, -t).
MAP_HD void tv_decompose_f(const float* F21, const TvK& k, float (&R)[8][9], float (&t)[8][3]) {
    float K[9], tmp[9], E[9];
    tv_K(k, K); tv_mul33_tn(K, F21, tmp); tv_mul33(tmp, K, E);
    double Ud[9], w[3], Vd[9];
    tv_svd33(E, Ud, w, Vd);
    float U[9], Vt[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { U[i] = (float)Ud[i]; Vt[i] = (float)Vd[i]; }
    const float tc[3] = {U[2], U[5], U[8]};
    float tu[3];
    tv_unit3(tc, tu);
    float UW[9], UWt[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        UW[3 * i] = U[3 * i + 1]; UW[3 * i + 1] = -U[3 * i]; UW[3 * i + 2] = U[3 * i + 2];
        UWt[3 * i] = -U[3 * i + 1]; UWt[3 * i + 1] = U[3 * i]; UWt[3 * i + 2] = U[3 * i + 2];
    }
    float R1[9], R2[9];
    tv_mul33(UW, Vt, R1); tv_mul33(UWt, Vt, R2);
    const bool n1 = tv_det33(R1) < 0, n2 = tv_det33(R2) < 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const float a = n1 ? -R1[i] : R1[i], b = n2 ? -R2[i] : R2[i];
        R[0][i] = a; R[1][i] = b; R[2][i] = a; R[3][i] = b; R[4][i] = 0.0f; R[5][i] = 0.0f; R[6][i] = 0.0f; R[7][i] = 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        t[0][i] = tu[i]; t[1][i] = tu[i]; t[2][i] = -tu[i]; t[3][i] = -tu[i]; t[4][i] = 0.0f; t[5][i] = 0.0f; t[6][i] = 0.0f; t[7][i] = 0.0f;
    }
}

// One motion of ReconstructH: R = s U Rp Vt, t = U tp / |U tp| (:621-637, 658-675)
MAP_HD void tv_h_motion(const float* U, const float* Vt, float s, const float* Rp, const float* tp, float* R, float* t) {
    float sU[9], tmp[9];
#pragma unroll
    for (int i = 0; i < 9; i++) sU[i] = s * U[i];
    tv_mul33(sU, Rp, tmp); tv_mul33(tmp, Vt, R);
    float tt[3];
#pragma unroll
    for (int i = 0; i < 3; i++) tt[i] = (U[3 * i] * tp[0] + U[3 * i + 1] * tp[1]) + U[3 * i + 2] * tp[2];
    tv_unit3(tt, t);
}
// ReconstructH up to the eight (R, t) of Faugeras (:584-686). False: the singular-value gate d1/d2 < 1.00001 || d2/d3 < 1.00001
// (or a singular K). d3 = (d1, d2, d3) for the tests.
MAP_HD bool tv_decompose_h(const float* H21, const TvK& k, float (&R)[8][9], float (&t)[8][3], float (&d3)[3]) {
    float K[9], invK[9], tmp[9], A[9];
    tv_K(k, K);
    const bool kok = tv_inv33(K, invK);
    tv_mul33(invK, H21, tmp); tv_mul33(tmp, K, A);
    double Ud[9], wd[3], Vd[9];
    tv_svd33(A, Ud, wd, Vd);
    float U[9], Vt[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { U[i] = (float)Ud[i]; Vt[i] = (float)Vd[i]; }
    const float s = (float)(tv_det33(U) * tv_det33(Vt));
    const float d1 = (float)wd[0], d2 = (float)wd[1], d3v = (float)wd[2];
    d3[0] = d1; d3[1] = d2; d3[2] = d3v;
#pragma unroll
    for (int h = 0; h < 8; h++) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[h][i] = 0.0f;
        t[h][0] = 0.0f; t[h][1] = 0.0f; t[h][2] = 0.0f;
    }
    if (!kok || !((double)(d1 / d2) >= 1.00001) || !((double)(d2 / d3v) >= 1.00001)) return false;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3v * d3v));
    const float aux3 = sqrtf((d2 * d2 - d3v * d3v) / (d1 * d1 - d3v * d3v));
    const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3v * d3v)) / ((d1 + d3v) * d2);
    const float ctheta = (d2 * d2 + d1 * d3v) / ((d1 + d3v) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3v * d3v)) / ((d1 - d3v) * d2);
    const float cphi = (d1 * d3v - d2 * d2) / ((d1 - d3v) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float Rp[9] = {ctheta, 0.0f, -stheta[i], 0.0f, 1.0f, 0.0f, stheta[i], 0.0f, ctheta};
        const float tp[3] = {x1[i] * (d1 - d3v), 0.0f * (d1 - d3v), -x3[i] * (d1 - d3v)};
        tv_h_motion(U, Vt, s, Rp, tp, R[i], t[i]);
        const float Rq[9] = {cphi, 0.0f, sphi[i], 0.0f, -1.0f, 0.0f, sphi[i], 0.0f, -cphi};
        const float tq[3] = {x1[i] * (d1 + d3v), 0.0f * (d1 + d3v), x3[i] * (d1 + d3v)};
        tv_h_motion(U, Vt, s, Rq, tq, R[4 + i], t[4 + i]);
    }
    return true;
}

// ---- CheckRT: one match ------------------------------------------------------------------------------------------------------------
// What CheckRT prepares once per motion (:814-826): P2 = K [R | t] (3 x 4 row-major), O2 = -R^T t.
struct TvPose { float R[9], t[3], P2[12], O2[3]; };
MAP_HD void tv_pose(const TvK& k, const float* R, const float* t, TvPose& p) {
    float K[9];
    tv_K(k, K);
#pragma unroll
    for (int i = 0; i < 9; i++) p.R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) p.t[i] = t[i];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) p.P2[4 * i + j] = (K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j]) + K[3 * i + 2] * R[6 + j];
        p.P2[4 * i + 3] = (K[3 * i] * t[0] + K[3 * i + 1] * t[1]) + K[3 * i + 2] * t[2];
        p.O2[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
    }
}
// q6 = cosParallax, z1, z2, squareError1, squareError2, dist2: the gate quantities (cos and z1 once a finite point exists, the rest as far as
// the match gets; untouched entries are 0). X is the triangulated point whenever it is finite.
MAP_HD int tv_check_rt_match(const TvK& k, const TvPose& p, float u1, float v1, float u2, float v2, float th2, float (&X)[3], float (&q6)[6]) {
#pragma unroll
    for (int i = 0; i < 6; i++) q6[i] = 0.0f;
    X[0] = X[1] = X[2] = 0.0f;
    // Triangulate: A.row(0) = kp1.pt.x * P1.row(2) - P1.row(0) .. with P1 = K [I | 0] (cv::addWeighted: double, stored to float)
    const float P1[12] = {k.fx, 0.0f, k.cx, 0.0f, 0.0f, k.fy, k.cy, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    float A[4][4], x[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        A[0][c] = (float)((double)P1[8 + c] * (double)u1 - (double)P1[c]);
        A[1][c] = (float)((double)P1[8 + c] * (double)v1 - (double)P1[4 + c]);
        A[2][c] = (float)((double)p.P2[8 + c] * (double)u2 - (double)p.P2[c]);
        A[3][c] = (float)((double)p.P2[8 + c] * (double)v2 - (double)p.P2[4 + c]);
    }
    smallest_right_singular_vector(A, x);
    float Y[3];
#pragma unroll
    for (int r = 0; r < 3; r++) Y[r] = (float)((double)x[r] / (double)x[3]);
    if (!isfinite(Y[0]) || !isfinite(Y[1]) || !isfinite(Y[2])) return TV_RT_NONE;
    X[0] = Y[0]; X[1] = Y[1]; X[2] = Y[2];
    const float dist1 = (float)map_norm3d(X[0], X[1], X[2]);
    const float n2[3] = {X[0] - p.O2[0], X[1] - p.O2[1], X[2] - p.O2[2]};
    const float dist2 = (float)map_norm3d(n2[0], n2[1], n2[2]);
    const float cosParallax = (float)(map_dot3d(X[0], X[1], X[2], n2[0], n2[1], n2[2]) / (double)(dist1 * dist2));
    q6[0] = cosParallax; q6[1] = X[2]; q6[5] = dist2;
    const bool low = (double)cosParallax < 0.99998;
    if (X[2] <= 0 && low) return TV_RT_NONE;
    float X2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) X2[r] = ((p.R[3 * r] * X[0] + p.R[3 * r + 1] * X[1]) + p.R[3 * r + 2] * X[2]) + p.t[r];
    q6[2] = X2[2];
    if (X2[2] <= 0 && low) return TV_RT_NONE;
    const float invZ1 = (float)(1.0 / (double)X[2]);
    const float im1x = k.fx * X[0] * invZ1 + k.cx, im1y = k.fy * X[1] * invZ1 + k.cy;
    const float e1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    q6[3] = e1;
    if (e1 > th2) return TV_RT_NONE;
    const float invZ2 = (float)(1.0 / (double)X2[2]);
    const float im2x = k.fx * X2[0] * invZ2 + k.cx, im2y = k.fy * X2[1] * invZ2 + k.cy;
    const float e2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    q6[4] = e2;
    if (e2 > th2) return TV_RT_NONE;
    return low ? TV_RT_TRIANGULATED : TV_RT_COUNTED;
}
MAP_HD float tv_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }
// parallax = acos(cos) * 180 / CV_PI (:901), in double, stored to float
MAP_HD float tv_parallax_deg(float c) { return (float)(acos((double)c) * 180 / 3.1415926535897932384626433832795); }

// order-preserving map of a float onto unsigned integers (the radix select of the parallax cosines)
MAP_HD uint32_t tv_float_key(float f) {
    union { float f; uint32_t u; } c; c.f = f;
    return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
MAP_HD float tv_key_float(uint32_t k) {
    union { float f; uint32_t u; } c; c.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return c.f;
}

// ---- the accept rules ----------------------------------------------------------------------------------------------------------------
// ReconstructH :689-731. Returns the winning hypothesis or -1 with `reason`.
MAP_HD int tv_accept_h(const int* n_good, const float* parallax, int n_inliers, float min_parallax, int min_tri, int& reason) {
    int best = 0, second = 0, idx = -1;
    float bestPar = -1.0f;
    for (int i = 0; i < 8; i++) {
        if (n_good[i] > best) { second = best; best = n_good[i]; idx = i; bestPar = parallax[i]; }
        else if (n_good[i] > second) second = n_good[i];
    }
    reason = TV_REASON_OK;
    if (!((double)second < 0.75 * (double)best)) reason = TV_REASON_NO_WINNER;
    else if (!(best > min_tri && (double)best > 0.9 * (double)n_inliers)) reason = TV_REASON_FEW_GOOD;
    else if (!(bestPar >= min_parallax)) reason = TV_REASON_PARALLAX;
    return reason == TV_REASON_OK ? idx : -1;
}
// ReconstructF :499-569
MAP_HD int tv_accept_f(const int* n_good, const float* parallax, int n_inliers, float min_parallax, int min_tri, int& reason) {
    int maxGood = n_good[0];
    for (int i = 1; i < 4; i++) maxGood = n_good[i] > maxGood ? n_good[i] : maxGood;
    const int n09 = (int)(0.9 * (double)n_inliers), nMinGood = n09 > min_tri ? n09 : min_tri;
    int nsimilar = 0;
    for (int i = 0; i < 4; i++) nsimilar += (double)n_good[i] > 0.7 * (double)maxGood;
    reason = TV_REASON_OK;
    if (maxGood < nMinGood) { reason = TV_REASON_FEW_GOOD; return -1; }
    if (nsimilar > 1) { reason = TV_REASON_NO_WINNER; return -1; }
    int idx = 0;
    for (int i = 3; i >= 0; i--) if (n_good[i] == maxGood) idx = i;
    if (!(parallax[idx] > min_parallax)) { reason = TV_REASON_PARALLAX; return -1; }
    return idx;
}

} // namespace viorb
