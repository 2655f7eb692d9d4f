// viorb_amd/shim/Initializer_shim.h — the reference's Initializer (include/Initializer.h, src/Initializer.cc) as a class template over
// the reference's own Frame, backed by viorb_two_view_init of include/viorb_two_view.h. Included in the reference tree after its headers
// (INTEGRATION.md §4f): `typedef viorb_shim::Initializer<Frame> Initializer;` in place of the reference's class leaves
// Tracking::MonocularInitialization untouched.
//
//   Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200)                     src/Initializer.cc:32-42
//   bool Initialize(const Frame& CurrentFrame, const vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
//                   vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated)                                src/Initializer.cc:44-121
//
// The reference draws its RANSAC sets from a process-wide rand() seeded once per process; here they come from
// viorb_two_view_draw_sets(N, iterations, mSeed): set mSeed (0 by default) for another draw. A pair of frames with fewer than eight
// matches returns false without a call (the reference indexes an empty list there). mLastStatus / mLastReason report
// VIORB_TWO_VIEW_FROM_H / _FROM_F / _FAILED and the failure gate. A failure of the GPU library is an exception carrying viorb_last_error().
#ifndef VIORB_INITIALIZER_SHIM_H
#define VIORB_INITIALIZER_SHIM_H

#include <cstdint>
#include <vector>
#include "viorb_tracking_shim.h"

namespace viorb_shim {

template <class FrameT, class Point3T = cv::Point3f> class Initializer {
public:
    Initializer(const FrameT& ReferenceFrame, float sigma = 1.0, int iterations = 200)
        : mSeed(0), mLastStatus(VIORB_TWO_VIEW_FAILED), mLastReason(VIORB_TWO_VIEW_REASON_OK), mSigma(sigma), mMaxIterations(iterations) {
        mxy1.resize(2 * ReferenceFrame.mvKeysUn.size() + 2);
        mN1 = (int)ReferenceFrame.mvKeysUn.size();
        for (int i = 0; i < mN1; i++) { mxy1[2 * i] = ReferenceFrame.mvKeysUn[i].pt.x; mxy1[2 * i + 1] = ReferenceFrame.mvKeysUn[i].pt.y; }
        mFx = ReferenceFrame.mK.template at<float>(0, 0); mFy = ReferenceFrame.mK.template at<float>(1, 1);
        mCx = ReferenceFrame.mK.template at<float>(0, 2); mCy = ReferenceFrame.mK.template at<float>(1, 2);
    }

    bool Initialize(const FrameT& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<Point3T>& vP3D,
                    std::vector<bool>& vbTriangulated) {
        const int n2 = (int)CurrentFrame.mvKeysUn.size();
        std::vector<float> xy2(2 * (size_t)n2 + 2);
        for (int i = 0; i < n2; i++) { xy2[2 * i] = CurrentFrame.mvKeysUn[i].pt.x; xy2[2 * i + 1] = CurrentFrame.mvKeysUn[i].pt.y; }
        std::vector<int32_t> m((size_t)mN1 + 1, -1);
        int N = 0;
        for (int i = 0; i < mN1 && i < (int)vMatches12.size(); i++) { m[i] = vMatches12[i]; N += vMatches12[i] >= 0; }
        mLastStatus = VIORB_TWO_VIEW_FAILED; mLastReason = VIORB_TWO_VIEW_REASON_FEW_MATCHES;
        if (N < 8) return false;
        std::vector<int32_t> sets((size_t)mMaxIterations * 8);
        check(viorb_two_view_draw_sets(N, mMaxIterations, mSeed, &sets[0]), "Initializer::Initialize (sets)");
        viorb_two_view_config cfg;
        cfg.sigma = mSigma; cfg.iterations = mMaxIterations; cfg.min_parallax_deg = 1.0f; cfg.min_triangulated = 50;
        cfg.fx = mFx; cfg.fy = mFy; cfg.cx = mCx; cfg.cy = mCy;
        const size_t cap = (size_t)(mN1 > n2 ? mN1 : n2) + 1;
        std::vector<float> P(3 * cap); std::vector<uint8_t> tri(cap);
        float R[9], t[3]; int32_t status = 0, reason = 0;
        viorb_two_view_outputs out = viorb_two_view_outputs();
        out.status = &status; out.reason = &reason; out.R21 = R; out.t21 = t; out.P3D = &P[0]; out.triangulated = &tri[0];
        check(viorb_two_view_init(&cfg, &mxy1[0], mN1, &xy2[0], n2, &m[0], &sets[0], &out), "Initializer::Initialize");
        mLastStatus = status; mLastReason = reason;
        if (status == VIORB_TWO_VIEW_FAILED) return false;
        R21.create(3, 3, CV_32F); t21.create(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R21.template at<float>(r, c) = R[3 * r + c]; t21.template at<float>(r) = t[r]; }
        vP3D.resize(mN1); vbTriangulated.assign(mN1, false);
        for (int i = 0; i < mN1; i++) { vP3D[i] = Point3T(P[3 * i], P[3 * i + 1], P[3 * i + 2]); vbTriangulated[i] = tri[i] != 0; }
        return true;
    }

    uint64_t mSeed;                    // seed of viorb_two_view_draw_sets
    int mLastStatus, mLastReason;

private:
    std::vector<float> mxy1;           // mvKeys1 (Reference Frame: 1)
    int mN1;
    float mFx, mFy, mCx, mCy;          // mK
    float mSigma;
    int mMaxIterations;
};

} // namespace viorb_shim

#endif // VIORB_INITIALIZER_SHIM_H
