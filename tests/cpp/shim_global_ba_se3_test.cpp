// tests/cpp/shim_global_ba_se3_test.cpp — compile / link / run test of viorb_shim::global_bundle_adjustment and bundle_adjustment
// (viorb_amd/shim/Optimizer_shim.h) against stand-ins that carry the reference's member names (global_ba_se3_standin.h).
//   shim_global_ba_se3_test                              no device needed: a tiny map; an observer outside vpKFs throws, and without a device
//                                                        the call throws with the library's error text and leaves the map untouched
//   shim_global_ba_se3_test problem.bin out.bin nLoopKF  reads a map written by tests/test_gpu_global_ba_se3_shim.py (with one bad key frame
//                                                        and one bad point the template has to skip), runs the template, writes what it left
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>
#include "global_ba_se3_standin.h"
#include "Optimizer_shim.h"

using namespace standin;

// Converter::toSE3Quat: Eigen's matrix -> quaternion, then SE3Quat's normalizeRotation
static void pose_to_qt(const cv::Mat& T, double qt[7]) {
    double m[3][3];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) m[r][c] = T.at<float>(r, c); qt[4 + r] = T.at<float>(r, 3); }
    double q[4];                                                              // x y z w
    const double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) { const double s = std::sqrt(t + 1.0), r = 0.5 / s; q[3] = 0.5 * s; q[0] = (m[2][1] - m[1][2]) * r; q[1] = (m[0][2] - m[2][0]) * r; q[2] = (m[1][0] - m[0][1]) * r; }
    else {
        int i = 0; if (m[1][1] > m[0][0]) i = 1; if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[i] = 0.5 * s; s = 0.5 / s; q[3] = (m[k][j] - m[j][k]) * s; q[j] = (m[j][i] + m[i][j]) * s; q[k] = (m[k][i] + m[i][k]) * s;
    }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), sg = q[3] < 0 ? -1.0 : 1.0;
    for (int c = 0; c < 4; c++) qt[c] = sg * q[c] / n;
}
// Converter::toCvMat(g2o::SE3Quat)
static cv::Mat qt_to_pose(const double* qt) {
    const double x = qt[0], y = qt[1], z = qt[2], w = qt[3];
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)}, {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T.at<float>(r, c) = (float)R[r][c]; T.at<float>(r, 3) = (float)qt[4 + r]; }
    T.at<float>(3, 3) = 1.f;
    return T;
}
static cv::Mat pose_mat(const double* p12) {
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T.at<float>(r, c) = (float)p12[3 * r + c]; T.at<float>(r, 3) = (float)p12[9 + r]; }
    T.at<float>(3, 3) = 1.f;
    return T;
}
static cv::Mat point_mat(const double* p) { cv::Mat m(3, 1, CV_32F); for (int c = 0; c < 3; c++) m.at<float>(c) = (float)p[c]; return m; }
// a key frame's keypoint table grows with its observations: keypoint i has octave i and mvInvLevelSigma2[i] is that observation's weight
static void observe(MapPoint& mp, KeyFrame& kf, double u, double v, double uright, double inv_sigma2) {
    const int i = (int)kf.mvKeysUn.size();
    kf.mvKeysUn.push_back(cv::KeyPoint((float)u, (float)v, 31.f, -1.f, 0.f, i, -1)); kf.mvuRight.push_back((float)uright); kf.mvInvLevelSigma2.push_back((float)inv_sigma2);
    mp.obs[&kf] = (size_t)i;
}

int main(int argc, char** argv) {
    double intr[5] = {450, 450, 376, 240, 45};
    std::vector<KeyFrame> kf; std::vector<MapPoint> mp; Map map;
    unsigned long nLoopKF = 0; int iterations = 10, robust = 1;
    std::vector<double> in;
    if (argc >= 4) {
        FILE* f = fopen(argv[1], "rb"); if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
        fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
        in.resize(bytes / sizeof(double)); if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2; fclose(f);
        nLoopKF = strtoul(argv[3], nullptr, 10);
        // header: nk np ne iterations robust bad_kf bad_pt 0 | intr5 | poses [nk][12] = R row-major, t | points [np][3] | edges [ne][6] = point kf u v uRight invSigma2
        const double* h = in.data();
        const int nk = (int)h[0], np = (int)h[1], ne = (int)h[2], bad_kf = (int)h[5], bad_pt = (int)h[6];
        iterations = (int)h[3]; robust = (int)h[4];
        const double* q = h + 8;
        for (int k = 0; k < 5; k++) intr[k] = q[k];
        q += 5;
        kf.resize(nk); mp.resize(np);
        for (int k = 0; k < nk; k++) { kf[k].Tcw = pose_mat(q + 12 * (size_t)k); kf[k].mnId = (unsigned long)k; kf[k].bad = k == bad_kf; }
        q += 12 * (size_t)nk;
        for (int p = 0; p < np; p++) { mp[p].Pw = point_mat(q + 3 * (size_t)p); mp[p].mnId = (unsigned long)p; mp[p].bad = p == bad_pt; }
        q += 3 * (size_t)np;
        for (int e = 0; e < ne; e++) { const double* r = q + 6 * (size_t)e; observe(mp[(int)r[0]], kf[(int)r[1]], r[2], r[3], r[4], r[5]); }
    } else {
        kf.resize(3); mp.resize(4);
        for (int k = 0; k < 3; k++) { const double p12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -0.1 * k, 0, 0}; kf[k].Tcw = pose_mat(p12); kf[k].mnId = (unsigned long)k; }
        const double P[4][3] = {{0.5, 0.2, 4}, {-0.4, 0.3, 5}, {0.1, -0.5, 6}, {-0.2, -0.1, 3}};
        for (int p = 0; p < 4; p++) {
            mp[p].Pw = point_mat(P[p]); mp[p].mnId = (unsigned long)p;
            for (int k = 0; k < 3; k++) {
                const double u = 450 * (P[p][0] - 0.1 * k) / P[p][2] + 376;
                observe(mp[p], kf[k], u, 450 * P[p][1] / P[p][2] + 240, (p + k) % 2 ? u - 45 / P[p][2] : -1.0, 1.0);
            }
        }
    }
    for (size_t k = 0; k < kf.size(); k++) { kf[k].fx = (float)intr[0]; kf[k].fy = (float)intr[1]; kf[k].cx = (float)intr[2]; kf[k].cy = (float)intr[3]; kf[k].mbf = (float)intr[4]; }
    for (size_t k = kf.size(); k-- > 0;) map.kfs.push_back(&kf[k]);              // GetAllKeyFrames promises no order
    for (size_t p = 0; p < mp.size(); p++) map.pts.push_back(&mp[p]);
    volatile int stop = 0; bool bstop = false;
    double info[6] = {0, 0, 0, 0, 0, 0};
    if (argc < 4) {
        // an observer that is not among the key frames has no vertex: rejected before the library is called
        std::vector<KeyFrame*> two(map.kfs.begin() + 1, map.kfs.end());          // key frames 1 and 0; key frame 2 observes but is left out, and 2 > maxKFid = 1 skips it
        std::vector<KeyFrame*> gap; gap.push_back(&kf[2]); gap.push_back(&kf[0]);  // key frame 1 (<= maxKFid = 2) observes and is missing
        bool threw = false;
        try { viorb_shim::bundle_adjustment(gap, map.pts, 10, &bstop, &stop, 0ul, true, pose_to_qt, qt_to_pose); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("not among the key frames") != std::string::npos; }
        if (!threw) { printf("FAIL: an observer without a vertex did not throw\n"); return 1; }
        if (viorb_device_count() < 1) {
            threw = false;
            try { viorb_shim::global_bundle_adjustment(&map, 10, &bstop, &stop, 0ul, true, pose_to_qt, qt_to_pose); }
            catch (const std::runtime_error& e) { threw = true; printf("OK threw: %s\n", e.what()); }
            if (!threw || kf[1].pose_sets || mp[0].pos_sets) { printf("FAIL: no device, but the template did not throw or touched the map\n"); return 1; }
            return 0;
        }
        try { viorb_shim::bundle_adjustment(two, map.pts, 5, &bstop, &stop, 0ul, true, pose_to_qt, qt_to_pose, info); }
        catch (const std::runtime_error& e) { printf("FAIL: %s\n", e.what()); return 1; }
        if (kf[2].pose_sets || !kf[1].pose_sets) { printf("FAIL: an observer above maxKFid was not skipped\n"); return 1; }
    }
    try { viorb_shim::global_bundle_adjustment(&map, iterations, &bstop, &stop, nLoopKF, robust != 0, pose_to_qt, qt_to_pose, info); }
    catch (const std::runtime_error& e) { printf("FAIL: %s\n", e.what()); return 1; }
    printf("OK iterations %d trials %d chi2 %.10g -> %.10g\n", (int)info[2], (int)info[3], info[0], info[1]);
    if (argc < 4) return 0;
    // out: info6 | per key frame: Tcw16 (GetPose), mTcwGBA16 (or zeros), pose_sets, mnBAGlobalForKF | per point: Pw3, mPosGBA3 (or zeros), pos_sets,
    //            normal_updates, mnBAGlobalForKF
    std::vector<double> out(info, info + 6);
    for (size_t k = 0; k < kf.size(); k++) {
        for (int i = 0; i < 16; i++) out.push_back((double)kf[k].Tcw.at<float>(i / 4, i % 4));
        for (int i = 0; i < 16; i++) out.push_back(kf[k].mTcwGBA.empty() ? 0.0 : (double)kf[k].mTcwGBA.at<float>(i / 4, i % 4));
        out.push_back(kf[k].pose_sets); out.push_back((double)kf[k].mnBAGlobalForKF);
    }
    for (size_t p = 0; p < mp.size(); p++) {
        for (int c = 0; c < 3; c++) out.push_back(mp[p].Pw.at<float>(c));
        for (int c = 0; c < 3; c++) out.push_back(mp[p].mPosGBA.empty() ? 0.0 : (double)mp[p].mPosGBA.at<float>(c));
        out.push_back(mp[p].pos_sets); out.push_back(mp[p].normal_updates); out.push_back((double)mp[p].mnBAGlobalForKF);
    }
    FILE* f = fopen(argv[2], "wb"); if (!f) return 2;
    fwrite(out.data(), sizeof(double), out.size(), f); fclose(f);
    return 0;
}
