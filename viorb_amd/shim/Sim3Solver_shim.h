// viorb_amd/shim/Sim3Solver_shim.h — the reference's Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) as a class template over the
// reference's own KeyFrame and MapPoint, backed by viorb_sim3_ransac of include/viorb_sim3.h. Included in the reference tree after its
// headers ("Loop verification"): `typedef viorb_shim::Sim3Solver<KeyFrame, MapPoint> Sim3Solver;` in place of the reference's class
// leaves LoopClosing::ComputeSim3 untouched.
//
//   Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12, bool bFixScale = true)   src/Sim3Solver.cc:37-112
//   void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)             :114-138
//   cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)                      :140-207
//   cv::Mat find(vector<bool>& vbInliers12, int& nInliers)                                                       :209-213
//   cv::Mat GetEstimatedRotation(); cv::Mat GetEstimatedTranslation(); float GetEstimatedScale();               :367-380
//
// The constructor keeps the reference's filtering (a match, a map point of key frame 1 at the same index, neither bad, both still
// indexed by their key frame), its mvnIndices1 mapping and its own expression for the points in camera coordinates. The reference draws
// its RANSAC sets from a process-wide generator; here they come from viorb_sim3_draw_sets(N, mRansacMaxIts, seed) with the seed given
// to the constructor (0 by default), drawn by SetRansacParameters. iterate carries (mnIterations, mnBestInliers) between calls, as
// LoopClosing needs when it resumes a solver whose model failed the optimisation, and scatters the flags to
// vbInliers[mvnIndices1[i]]. With N < minInliers it sets bNoMore and returns an empty matrix without a call. A failure of the GPU
// library is an exception carrying viorb_last_error().
#ifndef VIORB_SIM3SOLVER_SHIM_H
#define VIORB_SIM3SOLVER_SHIM_H

#include <cstdint>
#include <vector>
#include "viorb_tracking_shim.h"

namespace viorb_shim {

template <class KeyFrameT, class MapPointT> class Sim3Solver {
public:
    Sim3Solver(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true, uint64_t seed = 0)
        : mSeed(seed), mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale), mBestScale(0.0f) {
        std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
        for (int i1 = 0; i1 < mN1; i1++) {
            // a match, a map point of key frame 1 at the same index, neither bad, both still indexed by their key frame (:64-79)
            MapPointT* pMP2 = vpMatched12[i1];
            MapPointT* pMP1 = pMP2 ? vpKeyFrameMP1[i1] : (MapPointT*)0;
            if (!pMP1 || pMP1->isBad() || pMP2->isBad()) continue;
            const int k1 = pMP1->GetIndexInKeyFrame(pKF1), k2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (k1 < 0 || k2 < 0) continue;
            mvSigma2_1.push_back(pKF1->mvLevelSigma2[pKF1->mvKeysUn[k1].octave]);
            mvSigma2_2.push_back(pKF2->mvLevelSigma2[pKF2->mvKeysUn[k2].octave]);
            mvnIndices1.push_back(i1);
            cv::Mat X3D1w = pMP1->GetWorldPos(), X3D2w = pMP2->GetWorldPos();
            cv::Mat X1c = Rcw1 * X3D1w + tcw1, X2c = Rcw2 * X3D2w + tcw2;
            for (int r = 0; r < 3; r++) { mvX1c.push_back(X1c.template at<float>(r)); mvX2c.push_back(X2c.template at<float>(r)); }
        }
        N = (int)mvnIndices1.size();
        intrinsics(pKF1->mK, mK1); intrinsics(pKF2->mK, mK2);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        if (N >= 1) {
            const int its = viorb_sim3_ransac_iterations(N, probability, minInliers, maxIterations);
            if (its < 0) check(its, "Sim3Solver::SetRansacParameters");
            mRansacMaxIts = its;
        }
        mvSets.clear();
        if (N >= 3 && N >= mRansacMinInliers) {
            mvSets.resize((size_t)mRansacMaxIts * 3);
            check(viorb_sim3_draw_sets(N, mRansacMaxIts, mSeed, &mvSets[0]), "Sim3Solver::SetRansacParameters (sets)");
        }
        mnIterations = 0;
    }

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        vbInliers.assign(mN1, false);
        nInliers = 0;
        bNoMore = N < mRansacMinInliers;                                 // :146-150: nothing is indexed
        if (bNoMore) return cv::Mat();
        viorb_sim3_config cfg;
        cfg.iterations = mRansacMaxIts; cfg.min_inliers = mRansacMinInliers; cfg.fix_scale = mbFixScale ? 1 : 0; cfg.iterations_per_call = nIterations;
        int32_t status = 0, done = 0, best = 0, best_iter = -1, n_in = 0;
        float R[9], t[3], s = 0, T12[16];
        std::vector<uint8_t> flags((size_t)N + 1);
        viorb_sim3_outputs out = viorb_sim3_outputs();
        out.status = &status; out.iterations_done = &done; out.best_inliers = &best; out.best_iter = &best_iter; out.R12 = R; out.t12 = t; out.s12 = &s;
        out.T12 = T12; out.n_inliers = &n_in; out.inliers = &flags[0];
        check(viorb_sim3_ransac(&cfg, &mvX1c[0], &mvX2c[0], &mvSigma2_1[0], &mvSigma2_2[0], mK1, mK2, N, mvSets.empty() ? (const int32_t*)0 : &mvSets[0],
                                mRansacMaxIts, mnIterations, mnBestInliers, &out), "Sim3Solver::iterate");
        mnIterations = done; mnBestInliers = best;
        if (best_iter >= 0) {
            mBestRotation.create(3, 3, CV_32F); mBestTranslation.create(3, 1, CV_32F); mBestT12.create(4, 4, CV_32F);
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) mBestRotation.template at<float>(r, c) = R[3 * r + c]; mBestTranslation.template at<float>(r) = t[r]; }
            for (int k = 0; k < 16; k++) mBestT12.template at<float>(k / 4, k % 4) = T12[k];
            mBestScale = s;
        }
        if (status == VIORB_SIM3_FOUND) {
            nInliers = n_in;
            for (int i = 0; i < N; i++) if (flags[i]) vbInliers[mvnIndices1[i]] = true;
            return mBestT12;
        }
        if (status == VIORB_SIM3_NO_MORE || status == VIORB_SIM3_FEW) bNoMore = true;
        return cv::Mat();
    }

    cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool no_more = false;
        return iterate(mRansacMaxIts, no_more, vbInliers12, nInliers);
    }

    cv::Mat GetEstimatedRotation() { return mBestRotation; }
    cv::Mat GetEstimatedTranslation() { return mBestTranslation; }
    float GetEstimatedScale() { return mBestScale; }

    uint64_t mSeed;                    // seed of viorb_sim3_draw_sets
    int N, mN1;                        // correspondences after the filtering; vpMatched12.size()
    int mnIterations, mnBestInliers;   // the state iterate carries
    int mRansacMinInliers, mRansacMaxIts;
    std::vector<size_t> mvnIndices1;

private:
    static void intrinsics(const cv::Mat& K, float* k4) {
        k4[0] = K.template at<float>(0, 0); k4[1] = K.template at<float>(1, 1); k4[2] = K.template at<float>(0, 2); k4[3] = K.template at<float>(1, 2);
    }
    bool mbFixScale;
    std::vector<float> mvX1c, mvX2c, mvSigma2_1, mvSigma2_2;      // mvX3Dc1, mvX3Dc2, mvLevelSigma2[octave] of both key points
    std::vector<int32_t> mvSets;
    float mK1[4], mK2[4];
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale;
};

} // namespace viorb_shim

#endif // VIORB_SIM3SOLVER_SHIM_H
