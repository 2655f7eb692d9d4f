// tests/cpp/shim_sim3_test.cpp — compile / link / run test of viorb_shim::Sim3Solver (viorb_amd/shim/Sim3Solver_shim.h) with the
// stand-ins of sim3_standin.h. Usage: shim_sim3_test problem.bin out.bin. The problem file (written by tests/test_gpu_sim3_shim.py)
// holds n1 (the key points of key frame 1), the seed, fix_scale, min_inliers, K4, and per key point: the state of its match (0: no
// match, 1: a match, 2: key frame 1 has no map point there, 3: a bad map point, 4: a match key frame 2 no longer indexes), the octaves
// of both key points, the two map points and the key points' positions (x1 y1 x2 y2). Both key frames sit at the origin, so the points in camera coordinates are the world
// points. The program runs the solver the way LoopClosing::ComputeSim3 does, iterate(5, ...) until a model or bNoMore, and writes what
// it returned. Exit code 0: it ran (whatever it returned), 3: the library reported an error (printed), 2: usage.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "sim3_standin.h"
#include "Sim3Solver_shim.h"
#include "Optimizer_shim.h"

typedef viorb_shim::Sim3Solver<standin::KeyFrame, standin::MapPoint> Sim3Solver;

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: shim_sim3_test problem.bin out.bin\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int hdr[4]; float K4[4];
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(K4, 4, 4, f) != 4) return 2;
    const int n1 = hdr[0];
    std::vector<int> state(n1 + 1), o1(n1 + 1), o2(n1 + 1); std::vector<float> X1(3 * n1 + 1), X2(3 * n1 + 1), obs(4 * n1 + 1);
    if ((int)std::fread(&state[0], 4, n1, f) != n1 || (int)std::fread(&o1[0], 4, n1, f) != n1 || (int)std::fread(&o2[0], 4, n1, f) != n1 ||
        (int)std::fread(&X1[0], 4, 3 * n1, f) != 3 * n1 || (int)std::fread(&X2[0], 4, 3 * n1, f) != 3 * n1 || (int)std::fread(&obs[0], 4, 4 * n1, f) != 4 * n1) return 2;
    std::fclose(f);
    standin::KeyFrame KF1, KF2;
    for (standin::KeyFrame* kf : {&KF1, &KF2}) {
        kf->mK.create(3, 3, CV_32F); kf->mK.at<float>(0, 0) = K4[0]; kf->mK.at<float>(1, 1) = K4[1]; kf->mK.at<float>(0, 2) = K4[2]; kf->mK.at<float>(1, 2) = K4[3]; kf->mK.at<float>(2, 2) = 1.f;
        kf->mRcw.create(3, 3, CV_32F); for (int i = 0; i < 3; i++) kf->mRcw.at<float>(i, i) = 1.f;
        kf->mtcw.create(3, 1, CV_32F);
        float s = 1.f;
        for (int l = 0; l < 8; l++) { kf->mvLevelSigma2.push_back(s * s); kf->mvInvLevelSigma2.push_back(1.0f / (s * s)); s *= 1.2f; }
    }
    std::vector<standin::MapPoint> mp1(n1), mp2(n1);
    std::vector<standin::MapPoint*> vpMatched12(n1, (standin::MapPoint*)0);
    KF1.mvpMapPoints.assign(n1, (standin::MapPoint*)0);
    for (int i = 0; i < n1; i++) {
        KF1.mvKeysUn.push_back(cv::KeyPoint(obs[4 * i], obs[4 * i + 1], 0, -1, 0, o1[i])); KF2.mvKeysUn.push_back(cv::KeyPoint(obs[4 * i + 2], obs[4 * i + 3], 0, -1, 0, o2[i]));
        mp1[i].mWorldPos.create(3, 1, CV_32F); mp2[i].mWorldPos.create(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) { mp1[i].mWorldPos.at<float>(r) = X1[3 * i + r]; mp2[i].mWorldPos.at<float>(r) = X2[3 * i + r]; }
        mp1[i].mObservations[&KF1] = i;
        if (state[i] != 4) mp2[i].mObservations[&KF2] = i;
        if (state[i] == 3) mp2[i].mbBad = true;
        if (state[i] != 2) KF1.mvpMapPoints[i] = &mp1[i];
        if (state[i] != 0) vpMatched12[i] = &mp2[i];
    }
    cv::Mat T12; std::vector<bool> vbInliers; int nInliers = 0, calls = 0; bool bNoMore = false;
    int N = 0, maxIts = 0, its = 0, best = 0, nOpt = -1; float R[9] = {0}, t[3] = {0}, s = 0; standin::Sim3 gS = standin::Sim3();
    try {
        Sim3Solver solver(&KF1, &KF2, vpMatched12, hdr[2] != 0, (unsigned)hdr[1]);
        solver.SetRansacParameters(0.99, hdr[3], 300);
        N = solver.N; maxIts = solver.mRansacMaxIts;
        while (T12.empty() && !bNoMore) { T12 = solver.iterate(5, bNoMore, vbInliers, nInliers); calls++; }
        its = solver.mnIterations; best = solver.mnBestInliers;
        if (!T12.empty()) {
            const cv::Mat Rm = solver.GetEstimatedRotation(), tm = solver.GetEstimatedTranslation();
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[3 * r + c] = Rm.at<float>(r, c); t[r] = tm.at<float>(r); }
            s = solver.GetEstimatedScale();
            // LoopClosing.cc:349-350 (without SearchBySim3): the inliers as matches, g2o::Sim3 from the getters, OptimizeSim3
            for (int i = 0; i < n1; i++) if (!vbInliers[i]) vpMatched12[i] = 0;
            const double Rd[9] = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]};
            const double tr = Rd[0] + Rd[4] + Rd[8];                 // a rotation of less than 120 degrees: the first branch of Quaterniond(R)
            const double sq = std::sqrt(tr + 1.0), rq = 0.5 / sq;
            gS.v[0] = (Rd[7] - Rd[5]) * rq; gS.v[1] = (Rd[2] - Rd[6]) * rq; gS.v[2] = (Rd[3] - Rd[1]) * rq; gS.v[3] = 0.5 * sq;
            gS.v[4] = t[0]; gS.v[5] = t[1]; gS.v[6] = t[2]; gS.v[7] = s;
            nOpt = viorb_shim::optimize_sim3(&KF1, &KF2, vpMatched12, gS, 10.0f, hdr[2] != 0,
                                             [](const standin::Sim3& a, double* o) { for (int k = 0; k < 8; k++) o[k] = a.v[k]; },
                                             [](standin::Sim3& a, const double* o) { for (int k = 0; k < 8; k++) a.v[k] = o[k]; });
        }
    } catch (const std::runtime_error& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int head[8] = {T12.empty() ? 0 : 1, bNoMore ? 1 : 0, nInliers, calls, N, maxIts, its, best};
    std::fwrite(head, 4, 8, o);
    float T16[16] = {0};
    if (!T12.empty()) for (int k = 0; k < 16; k++) T16[k] = T12.at<float>(k / 4, k % 4);
    std::fwrite(T16, 4, 16, o); std::fwrite(R, 4, 9, o); std::fwrite(t, 4, 3, o); std::fwrite(&s, 4, 1, o);
    for (int i = 0; i < n1; i++) { const unsigned char b = i < (int)vbInliers.size() && vbInliers[i]; std::fwrite(&b, 1, 1, o); }
    std::fwrite(&nOpt, 4, 1, o); std::fwrite(gS.v, 8, 8, o);
    for (int i = 0; i < n1; i++) { const unsigned char b = vpMatched12[i] != 0; std::fwrite(&b, 1, 1, o); }
    std::fclose(o);
    std::printf("iterate returned %s after %d calls (N %d, max its %d, iterations %d, inliers %d, bNoMore %d)\n", T12.empty() ? "nothing" : "a model", calls, N, maxIts, its,
                nInliers, (int)bNoMore);
    return 0;
}
