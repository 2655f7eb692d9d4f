// viorb_amd/csrc/reloc_core.h — the arithmetic of the relocalisation matcher ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound,
// th, ORBdist) and the decisions of the refine cascade of Tracking::Relocalization, shared by the HIP kernels of relocalization.hip and by
// the host (tests/cpp/reloc_core_host_test.cpp runs it under the address and undefined-behaviour sanitizers).
//
// What is restated (reference file:line):
//   the projection and its gates                         src/ORBmatcher.cc:1477-1479, :1498-1532
//   MapPoint::Get{Min,Max}DistanceInvariance             src/MapPoint.cc:380-390
//   MapPoint::PredictScale(dist, Frame*)                 src/MapPoint.cc:409-424 (s3m_predict_level: the KeyFrame* overload is the same text)
//   Frame::GetFeaturesInArea with level limits           src/Frame.cc:507-560 (grid_window / grid_scan of match_core.h; reloc_level_ok)
//   the claim loop and the rotation histogram            src/ORBmatcher.cc:1536-1597 (reloc_match_serial: the serial form of k_reloc_claim)
//   the thresholds of the cascade                        src/Tracking.cc:2226-2273 (reloc_after_solve1 / _search1 / _solve2 / _search2)
// Float / double placement is the audit table of DESIGN.md ("Relocalisation"). Nothing here depends on contraction.
#pragma once
#include "sim3_match_core.h"

namespace viorb {

// reason code of a match the rotation histogram removed (:1586-1596); the others are the S3M_* of sim3_match_core.h
enum { RELOC_ROTATION = 9 };

// Two properties differ from every other matcher of the library: there is no z < 0 gate and no viewing-angle gate, and the image test is
// `u < min || u > max` (:1508-1511), which a NaN coordinate and a coordinate on either bound pass. pose12 = Rcw(9) tcw(3); X = pts_f[8].
//   x3Dc = Rcw x3Dw + tcw        the float gemm (m0 x0 + m1 x1) + m2 x2, then the float add
//   Ow = -Rcw^T tcw              the same product, negated
//   invzc = 1.0 / z              the double quotient rounded to float is the float quotient
//   u = fx*xc*invzc + cx         (fx * xc) * invzc + cx, every operation rounded to float
//   dist3D = cv::norm(PO)        squares and sum in double, sqrt in double, rounded to float
VIORB_HD void reloc_project(const S3mCam& C, const float* pose12, const float* X, S3mProj& P) {
    P.u = P.v = P.radius = 0.0f; P.dist3D = 0.0f; P.level = 0; P.rect.x0 = P.rect.y0 = 0; P.rect.x1 = P.rect.y1 = -1; P.rect.empty = true;
    float pc[3], Ow[3];
    s3m_mul3(pose12, X, pc);
    pc[0] = pc[0] + pose12[9]; pc[1] = pc[1] + pose12[10]; pc[2] = pc[2] + pose12[11];
#pragma unroll
    for (int r = 0; r < 3; r++) { const float tt = pose12[r] * pose12[9] + pose12[3 + r] * pose12[10] + pose12[6 + r] * pose12[11]; Ow[r] = -tt; }
    const float invz = 1.0f / pc[2];
    const float ux = C.fx * pc[0], vy = C.fy * pc[1];
    const float uz = ux * invz, vz = vy * invz;
    const float u = uz + C.cx, v = vz + C.cy;
    P.u = u; P.v = v;
    if (u < C.g.minX || u > C.g.maxX) { P.reason = S3M_OUT_OF_IMAGE; return; }
    if (v < C.g.minY || v > C.g.maxY) { P.reason = S3M_OUT_OF_IMAGE; return; }
    const float dist3D = s3m_norm3(X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]);
    P.dist3D = dist3D;
    const float maxD = 1.2f * X[7], minD = 0.8f * X[6];
    if (dist3D < minD || dist3D > maxD) { P.reason = S3M_OUT_OF_RANGE; return; }
    const int lvl = s3m_predict_level(X[7], dist3D, C.log_sf, C.nlevels);
    const float radius = C.th * C.scale[lvl];
    P.level = lvl; P.radius = radius;
    grid_window(C.g, u, v, radius, P.rect);
    P.reason = P.rect.empty ? S3M_NO_FEATURE_IN_WINDOW : S3M_MATCHED;
}

// Frame::GetFeaturesInArea(u, v, r, nPredictedLevel - 1, nPredictedLevel + 1): maxLevel >= 0 always, so bCheckLevels is true
VIORB_HD bool reloc_level_ok(int octave, int lvl) { return !(octave < lvl - 1) && !(octave > lvl + 1); }

// Frame::GetFeaturesInArea (src/Frame.cc:530-557) over the CSR grid of a frame with n features in arrays of cap: visit(idx) for every
// feature of the cell rectangle whose octave is inside nPredictedLevel - 1 .. nPredictedLevel + 1 and, then, with |dx| < r and |dy| < r, in
// the reference's order (grid_scan, which keeps every read inside the arrays whatever the grid holds). KP: viorb_keypoint (x, y, octave).
template <class KP, class Visit>
VIORB_HD void reloc_scan(const S3mProj& P, const KP* kp, const int* cs, const int* ci, int n, int cap, Visit&& visit) {
    grid_scan(P.rect, cs, ci, n, cap, [&](int idx) {
        const KP k = kp[idx];
        if (!reloc_level_ok(k.octave, P.level)) return;
        const float dx = k.x - P.u, dy = k.y - P.v;
        if (fabsf(dx) < P.radius && fabsf(dy) < P.radius) visit(idx);
    });
}

// The claim loop plus the rotation histogram over given candidate lists, serially: the fixed point of s3m_claim_in_order under the gate
// orb_dist, then :1578-1597. cand / cand_n / taken_in as for s3m_claim_in_order; angle_kf [npts] = pKF->mvKeysUn[i].angle, angle_f [nfeat] =
// CurrentFrame.mvKeysUn[i2].angle. best_idx [npts]: what point i keeps; removed [npts]: matched in the loop, then taken away by the
// histogram (its feature stayed claimed during the loop). owner [max(nfeat, 1)] is scratch. Returns nmatches.
inline int reloc_match_serial(const uint32_t* cand, const int32_t* cand_n, int npts, int lcap, const uint8_t* taken_in, int nfeat, int orb_dist,
                              int check_orientation, const float* angle_kf, const float* angle_f, int32_t* best_idx, uint8_t* removed,
                              int32_t* owner) {
    s3m_claim_in_order(cand, cand_n, npts, lcap, taken_in, nfeat, best_idx, owner, orb_dist);
    int hist[HISTO_LENGTH], keep[HISTO_LENGTH], nmatches = 0;
    for (int i = 0; i < HISTO_LENGTH; i++) { hist[i] = 0; keep[i] = 1; }
    for (int p = 0; p < npts; p++) {
        removed[p] = 0;
        if (best_idx[p] < 0) continue;
        nmatches++;
        if (check_orientation) hist[rot_bin(angle_kf[p], angle_f[best_idx[p]])]++;
    }
    if (!check_orientation) return nmatches;
    nmatches -= three_maxima(hist, keep);
    for (int p = 0; p < npts; p++)
        if (best_idx[p] >= 0 && !keep[rot_bin(angle_kf[p], angle_f[best_idx[p]])]) { best_idx[p] = -1; removed[p] = 1; }
    return nmatches;
}

// ---- the cascade (src/Tracking.cc:2226-2273) --------------------------------------------------------------------------------------------
// stage[b]: where hypothesis b left the cascade (VIORB_RELOC_* of include/viorb_relocalization.h), or RELOC_RUNNING until it has
enum { RELOC_RUNNING = 0, RELOC_FEW_INLIERS = 1, RELOC_ACCEPTED_FIRST = 2, RELOC_COARSE_SHORT = 3, RELOC_SECOND_WEAK = 4, RELOC_ACCEPTED_SECOND = 5,
       RELOC_NARROW_SHORT = 6, RELOC_THIRD_REJECTED = 7, RELOC_ACCEPTED_THIRD = 8 };

struct RelocThresholds { int min_good, accept, narrow_above; };     // 10, 50, 30 (the narrow search runs for narrow_above < nGood < accept)

// after the first solve: :2228 (stop, nothing nulled), :2236 (enough already), else the coarse search runs
VIORB_HD int reloc_after_solve1(const RelocThresholds& T, int n_good) {
    if (n_good < T.min_good) return RELOC_FEW_INLIERS;
    if (!(n_good < T.accept)) return RELOC_ACCEPTED_FIRST;
    return RELOC_RUNNING;
}
// after the coarse search: :2240
VIORB_HD int reloc_after_search1(const RelocThresholds& T, int n_good, int n_additional) {
    return (n_additional + n_good >= T.accept) ? RELOC_RUNNING : RELOC_COARSE_SHORT;
}
// after the second solve: :2246 decides whether the narrow search runs; without it :2269 decides
VIORB_HD int reloc_after_solve2(const RelocThresholds& T, int n_good) {
    if (n_good > T.narrow_above && n_good < T.accept) return RELOC_RUNNING;
    return n_good >= T.accept ? RELOC_ACCEPTED_SECOND : RELOC_SECOND_WEAK;
}
// after the narrow search: :2255
VIORB_HD int reloc_after_search2(const RelocThresholds& T, int n_good, int n_additional) {
    return (n_good + n_additional >= T.accept) ? RELOC_RUNNING : RELOC_NARROW_SHORT;
}
// after the third solve: :2269
VIORB_HD int reloc_after_solve3(const RelocThresholds& T, int n_good) { return n_good >= T.accept ? RELOC_ACCEPTED_THIRD : RELOC_THIRD_REJECTED; }

} // namespace viorb
