// viorb_amd/csrc/sim3_match_core.h — the arithmetic of the three projection matchers that take a similarity instead of a pose, shared by
// the HIP kernels of sim3_match.hip and by the host-only hooks viorb_debug_sim3_decompose / _pair / _project / viorb_debug_claim_in_order
// (the CPU test-suite compares them with tests/sim3_match_ref.py without a GPU).
//
// What is restated (reference file:line):
//   ORBmatcher::SearchByProjection(KeyFrame*, Scw, ...)   src/ORBmatcher.cc:290-403   (decomposition :298-303, gates :320-365, claim :370-398)
//   ORBmatcher::Fuse(KeyFrame*, Scw, ...)                  src/ORBmatcher.cc:977-1100  (decomposition :985-990, gates :1008-1054)
//   ORBmatcher::SearchBySim3                               src/ORBmatcher.cc:1102-1326 (transforms :1119-1121, gates :1158-1194 and :1238-1274)
//   KeyFrame::IsInImage, MapPoint::PredictScale            src/KeyFrame.cc:947-950, src/MapPoint.cc (ceil(log(max / dist) / log(factor)), clamped)
// Float / double placement is the audit table of DESIGN.md §2 ("Sim3 matchers"). The cell rectangle of KeyFrame::GetFeaturesInArea, the
// guarded float-to-int conversion and the thresholds are match_core.h; k_fuse (frontend_kernels.hip) predicts its level with
// s3m_predict_level too. Nothing here depends on contraction (-ffp-contract=off).
#pragma once
#include <limits.h>
#include "match_core.h"

namespace viorb {

// reason[i]: which statement of the reference ended the point (VIORB_S3M_* of include/viorb_sim3_match.h)
enum { S3M_MATCHED = 0, S3M_NOT_CANDIDATE = 1, S3M_BEHIND = 2, S3M_OUT_OF_IMAGE = 3, S3M_OUT_OF_RANGE = 4, S3M_VIEW_ANGLE = 5,
       S3M_NO_FEATURE_IN_WINDOW = 6, S3M_ABOVE_THRESHOLD = 7, S3M_NOT_MUTUAL = 8 };
// which function a projection belongs to (viorb_debug_sim3_project)
enum { S3M_FN_SEARCH_BY_SIM3 = 0, S3M_FN_SEARCH_BY_PROJECTION = 1, S3M_FN_FUSE = 2 };

// The camera, the image bounds and the search radius of one call. log_sf = (float)log((double)mfScaleFactor), taken on the host.
struct S3mCam {
    float fx, fy, cx, cy;
    GridCam g;
    float th, log_sf;
    int nlevels;
    float scale[16];
};

// Scw decomposed (:298-303): scw = sqrt(row0 . row0) with the dot and the root in double (Mat::dot, sqrt(double)), stored to float;
// Rcw = sRcw / scw and tcw = t / scw are MatExpr scalings by the double alpha = 1.0 / scw, rounded per element; Ow = -Rcw^T tcw.
struct S3mScw { float scw, R[9], t[3], Ow[3]; };

// The transforms of SearchBySim3 (:1119-1121): sR12 = s12 * R12 and sR21 = (1.0 / s12) * R12^T by a double alpha, t21 = -sR21 * t12.
struct S3mPair { float sR12[9], sR21[9], t21[3]; };

// One point after the gates: reason is the gate that ended it, or S3M_MATCHED when it reaches the window scan; the cell rectangle is
// GetFeaturesInArea's (not empty whenever reason == S3M_MATCHED).
struct S3mProj { float u, v, dist3D, radius; int level, reason; GridRect rect; };

// M X of a row-major 3 x 3 in float: (m0 x0 + m1 x1) + m2 x2, the small-matrix gemm association
VIORB_HD void s3m_mul3(const float* M, const float* X, float* out) {
#pragma unroll
    for (int r = 0; r < 3; r++) { const float tt = M[3 * r] * X[0] + M[3 * r + 1] * X[1] + M[3 * r + 2] * X[2]; out[r] = tt; }
}

VIORB_HD void s3m_decompose(const float* S, S3mScw& D) {          // S [12]: the top three rows of the 4 x 4, row-major
    const double dot = ((double)S[0] * (double)S[0] + (double)S[1] * (double)S[1]) + (double)S[2] * (double)S[2];
    D.scw = (float)sqrt(dot);
    const double alpha = 1.0 / (double)D.scw;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) D.R[3 * r + c] = (float)((double)S[4 * r + c] * alpha);
        D.t[r] = (float)((double)S[4 * r + 3] * alpha);
    }
#pragma unroll
    for (int r = 0; r < 3; r++) { const float tt = D.R[r] * D.t[0] + D.R[3 + r] * D.t[1] + D.R[6 + r] * D.t[2]; D.Ow[r] = -tt; }
}

VIORB_HD void s3m_pair(const float* R12, const float* t12, float s12, S3mPair& T) {
    const double a12 = (double)s12, a21 = 1.0 / (double)s12;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            T.sR12[3 * r + c] = (float)((double)R12[3 * r + c] * a12);
            T.sR21[3 * r + c] = (float)((double)R12[3 * c + r] * a21);
        }
    float m[3];
    s3m_mul3(T.sR21, t12, m);
    T.t21[0] = -m[0]; T.t21[1] = -m[1]; T.t21[2] = -m[2];
}

// cv::norm of a float 3-vector: squares summed in double, the root in double, rounded to float
VIORB_HD float s3m_norm3(float a, float b, float c) { return (float)sqrt(((double)a * a + (double)b * b) + (double)c * c); }

// MapPoint::PredictScale: ratio = mfMaxDistance / dist in float, ceil(log(ratio) / mfLogScaleFactor) converted to int, clamped into
// 0..nlevels-1. A quotient no int holds (non-finite: dist == 0, or a scale factor of 1 whose logarithm is 0) goes through float_to_int
// and so clamps to level 0 on the host and on the device alike.
VIORB_HD int s3m_predict_level(float max_distance, float dist, float log_sf, int nlevels) {
    const float ratio = max_distance / dist;
    const int lvl = float_to_int(ceilf(viorb_logf(ratio) / log_sf));
    return lvl < 0 ? 0 : (lvl >= nlevels ? nlevels - 1 : lvl);
}

// From the point in the camera frame to the window: depth (rejected on z < 0, so z == 0 goes on with an infinite invz and fails the image
// gate), projection, IsInImage, the 0.8 / 1.2 distance gate, with VIEW the viewing-angle gate PO . Pn < 0.5 dist (the dot in double, as
// Mat::dot), PredictScale, radius = th * scale[level], the cell rectangle. X = pts_f[8]; PO is read with VIEW only.
template <bool VIEW> VIORB_HD void s3m_gates(const S3mCam& C, const float* pc, float dist3D, const float* X, const float* PO, S3mProj& P) {
    P.u = P.v = P.radius = 0.0f; P.dist3D = dist3D; P.level = 0; P.rect.x0 = P.rect.y0 = 0; P.rect.x1 = P.rect.y1 = -1; P.rect.empty = true;
    if (pc[2] < 0.0f) { P.reason = S3M_BEHIND; return; }
    const float invz = 1.0f / pc[2];                         // 1.0 / z in double rounded to float is the float quotient
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = C.fx * x + C.cx, v = C.fy * y + C.cy;
    P.u = u; P.v = v;
    if (!(u >= C.g.minX && u < C.g.maxX && v >= C.g.minY && v < C.g.maxY)) { P.reason = S3M_OUT_OF_IMAGE; return; }
    const float maxD = 1.2f * X[7], minD = 0.8f * X[6];
    if (dist3D < minD || dist3D > maxD) { P.reason = S3M_OUT_OF_RANGE; return; }
    if (VIEW) {
        const double dotp = ((double)PO[0] * X[3] + (double)PO[1] * X[4]) + (double)PO[2] * X[5];
        if (dotp < 0.5 * (double)dist3D) { P.reason = S3M_VIEW_ANGLE; return; }
    }
    const int lvl = s3m_predict_level(X[7], dist3D, C.log_sf, C.nlevels);
    const float radius = C.th * C.scale[lvl];
    P.level = lvl; P.radius = radius;
    grid_window(C.g, u, v, radius, P.rect);
    P.reason = P.rect.empty ? S3M_NO_FEATURE_IN_WINDOW : S3M_MATCHED;
}

// SearchByProjection(KF, Scw) and Fuse(KF, Scw): p3Dc = Rcw Pw + tcw, dist = |Pw - Ow|
VIORB_HD void s3m_project_scw(const S3mCam& C, const S3mScw& D, const float* X, S3mProj& P) {
    float pc[3];
    s3m_mul3(D.R, X, pc);
    pc[0] = pc[0] + D.t[0]; pc[1] = pc[1] + D.t[1]; pc[2] = pc[2] + D.t[2];
    const float PO[3] = {X[0] - D.Ow[0], X[1] - D.Ow[1], X[2] - D.Ow[2]};
    s3m_gates<true>(C, pc, s3m_norm3(PO[0], PO[1], PO[2]), X, PO, P);
}

// SearchBySim3, one direction: X in its own camera (Rw Pw + tw, rounded), then in the other one (sR X + t, rounded); dist3D is the norm of
// the point in the other camera's frame. No viewing-angle gate.
VIORB_HD void s3m_project_pair(const S3mCam& C, const float* pose12_own, const float* sR, const float* t, const float* X, S3mProj& P) {
    float pa[3], pb[3];
    s3m_mul3(pose12_own, X, pa);
    pa[0] = pa[0] + pose12_own[9]; pa[1] = pa[1] + pose12_own[10]; pa[2] = pa[2] + pose12_own[11];
    s3m_mul3(sR, pa, pb);
    pb[0] = pb[0] + t[0]; pb[1] = pb[1] + t[1]; pb[2] = pb[2] + t[2];
    s3m_gates<false>(C, pb, s3m_norm3(pb[0], pb[1], pb[2]), X, nullptr, P);
}

// The ordered phase of SearchByProjection(KF, Scw) (:370-398). A candidate is dist << 16 | feature; a point's list holds its candidates
// that are free on entry, in GetFeaturesInArea visiting order. s3m_pick is the reference's inner loop over the candidates `is_free`
// admits: the first minimum; -1 when there is none at a distance <= gate (TH_LOW for the Scw matcher, ORBdist for the relocalisation one).
template <class Free> VIORB_HD int s3m_pick(const uint32_t* list, int n, size_t stride, Free&& is_free, int gate = TH_LOW) {
    int best = -1, best_dist = 256;
    for (int k = 0; k < n; k++) {
        const uint32_t e = list[(size_t)k * stride];
        const int idx = (int)(e & 0xffffu), d = (int)(e >> 16);
        if (d < best_dist && is_free(idx)) { best_dist = d; best = idx; }
    }
    return best_dist <= gate ? best : -1;
}

// The point-order loop as a fixed-point iteration: choice[p] = s3m_pick over the features no earlier point chose in the previous sweep.
// After k sweeps the choices of points 0..k-1 are those of the literal loop (point p only depends on earlier points), and a sweep that
// changes nothing is the loop's result, so the iteration ends after at most npts + 1 sweeps. The device kernel runs the same sweeps with a
// workgroup; this is the serial form. owner [nfeat] is scratch. Returns the number of sweeps.
inline int s3m_claim_in_order(const uint32_t* cand, const int32_t* cand_n, int npts, int lcap, const uint8_t* taken_in, int nfeat, int32_t* choice,
                              int32_t* owner, int gate = TH_LOW) {
    for (int p = 0; p < npts; p++) choice[p] = -1;
    int sweeps = 0;
    for (;;) {
        sweeps++;
        for (int f = 0; f < nfeat; f++) owner[f] = INT_MAX;
        for (int p = npts - 1; p >= 0; p--) if (choice[p] >= 0) owner[choice[p]] = p;      // the lowest point that holds the feature
        bool changed = false;
        for (int p = 0; p < npts; p++) {
            const int n = cand_n[p] < lcap ? cand_n[p] : lcap;
            const int c = s3m_pick(cand + (size_t)p * lcap, n, 1, [&](int idx) { return idx < nfeat && !taken_in[idx] && owner[idx] >= p; }, gate);
            if (c != choice[p]) { choice[p] = c; changed = true; }
        }
        if (!changed) return sweeps;
    }
}

#if defined(__HIPCC__)
// The same sweeps with a workgroup, the points of a sweep in parallel; every thread of the workgroup calls it. s_owner [n] (LDS): the
// lowest point that chose feature f in the previous sweep (LDS atomics on scratch). choice [npts] is -1 on entry and holds the loop's
// result on return. cand: entry k of point p at cand[k * stride + p], cand_n [npts] counts on past list_cap; a point whose candidates
// exceeded its list is served by rescan(p) = the first minimum of its window among the features that are free on entry and whose
// s_owner is >= p, or -1 above the gate. Shared by k_s3m_claim (sim3_match.hip) and k_reloc_claim (relocalization.hip).
template <class Rescan>
__device__ __forceinline__ void s3m_claim_sweeps(int* s_owner, int n, int npts, int* choice, const int* __restrict__ cand_n,
                                                 const uint32_t* __restrict__ cand, size_t stride, int list_cap, int gate, Rescan&& rescan) {
    for (;;) {
        for (int f = threadIdx.x; f < n; f += blockDim.x) s_owner[f] = INT_MAX;
        __syncthreads();
        for (int p = threadIdx.x; p < npts; p += blockDim.x) { const int c = choice[p]; if (c >= 0) atomicMin(&s_owner[c], p); }
        __syncthreads();
        int changed = 0;
        for (int p = threadIdx.x; p < npts; p += blockDim.x) {
            const int nc = cand_n[p];
            if (nc == 0) continue;
            const int c = nc <= list_cap ? s3m_pick(cand + p, nc, stride, [&](int idx) { return s_owner[idx] >= p; }, gate) : rescan(p);
            if (c != choice[p]) { choice[p] = c; changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }
}
#endif

} // namespace viorb
