// tests/cpp/shim_global_ba_test.cpp — compile / link / run test of viorb_shim::global_bundle_adjustment_navstate (viorb_amd/shim/Optimizer_shim.h)
// against stand-ins that carry the reference's member names (global_ba_standin.h).
//   shim_global_ba_test                              no device needed: a tiny map; a stereo observation throws, and without a device the
//                                                    call throws with the library's error text and leaves the map untouched
//   shim_global_ba_test problem.bin out.bin nLoopKF  reads a map written by tests/test_gpu_global_ba_shim.py (with one bad key frame and one
//                                                    bad point the template has to skip), runs the template, writes what it left in the objects
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>
#include "global_ba_standin.h"
#include "Optimizer_shim.h"

using namespace standin;

static void unpack(const double* o, NavState& ns) { viorb_shim::unpack_navstate<NavState, Vec3, Quat, SO3>(o, ns); }
static void fill_preint(const double* o, IMUPreintegrator& M) {
    M.dP = Vec3(o[0], o[1], o[2]); M.dV = Vec3(o[3], o[4], o[5]);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) {
        M.dR(r, c) = o[6 + 3 * r + c]; M.JPg(r, c) = o[15 + 3 * r + c]; M.JPa(r, c) = o[24 + 3 * r + c];
        M.JVg(r, c) = o[33 + 3 * r + c]; M.JVa(r, c) = o[42 + 3 * r + c]; M.JRg(r, c) = o[51 + 3 * r + c];
    }
    for (int r = 0; r < 9; r++) for (int c = 0; c < 9; c++) M.cov(r, c) = o[60 + 9 * r + c];
    M.dt = o[141];
}
static cv::Mat point_mat(const double* p) { cv::Mat m(3, 1, CV_32F); for (int c = 0; c < 3; c++) m.at<float>(c) = (float)p[c]; return m; }
// a key frame's keypoint table grows with its observations: keypoint i has octave i and mvInvLevelSigma2[i] is that observation's weight
static void observe(MapPoint& mp, KeyFrame& kf, double u, double v, double inv_sigma2, float uright = -1.f) {
    const int i = (int)kf.mvKeysUn.size();
    kf.mvKeysUn.push_back(cv::KeyPoint((float)u, (float)v, 31.f, -1.f, 0.f, i, -1)); kf.mvuRight.push_back(uright); kf.mvInvLevelSigma2.push_back((float)inv_sigma2);
    mp.obs[&kf] = (size_t)i;
}

int main(int argc, char** argv) {
    Mat<4, 4> Tbc; cv::Mat MatTbc(4, 4, CV_32F);
    double gw[3] = {0, 0, 9.81}, cam[16] = {450, 450, 376, 240, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    std::vector<KeyFrame> kf; std::vector<MapPoint> mp; Map map;
    unsigned long nLoopKF = 0; int iterations = 10, robust = 1;
    std::vector<double> in;
    if (argc >= 4) {
        FILE* f = fopen(argv[1], "rb"); if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
        fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
        in.resize(bytes / sizeof(double)); if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2; fclose(f);
        nLoopKF = strtoul(argv[3], nullptr, 10);
        // header: nk np ne iterations robust bad_kf bad_pt 0 | gw3 cam16 | kfs [nk][22] | preint [nk][142] | points [np][3] | edges [ne][5] = point kf u v invSigma2
        const double* h = in.data();
        const int nk = (int)h[0], np = (int)h[1], ne = (int)h[2], bad_kf = (int)h[5], bad_pt = (int)h[6];
        iterations = (int)h[3]; robust = (int)h[4];
        const double* q = h + 8;
        for (int k = 0; k < 3; k++) gw[k] = q[k];
        for (int k = 0; k < 16; k++) cam[k] = q[3 + k];
        q += 19;
        kf.resize(nk); mp.resize(np);
        for (int k = 0; k < nk; k++) {
            unpack(q + 22 * (size_t)k, kf[k].ns); kf[k].mnId = (unsigned long)k; kf[k].prev = k ? &kf[k - 1] : nullptr; kf[k].bad = k == bad_kf;
            kf[k].fx = (float)cam[0]; kf[k].fy = (float)cam[1]; kf[k].cx = (float)cam[2]; kf[k].cy = (float)cam[3];
        }
        q += 22 * (size_t)nk;
        for (int k = 0; k < nk; k++) fill_preint(q + 142 * (size_t)k, kf[k].pre);
        q += 142 * (size_t)nk;
        for (int p = 0; p < np; p++) { mp[p].Pw = point_mat(q + 3 * (size_t)p); mp[p].mnId = (unsigned long)p; mp[p].bad = p == bad_pt; }
        q += 3 * (size_t)np;
        for (int e = 0; e < ne; e++) observe(mp[(int)q[5 * (size_t)e]], kf[(int)q[5 * (size_t)e + 1]], q[5 * (size_t)e + 2], q[5 * (size_t)e + 3], q[5 * (size_t)e + 4]);
        for (int k = nk - 1; k >= 0; k--) map.kfs.push_back(&kf[k]);          // GetAllKeyFrames promises no order
    } else {
        kf.resize(3); mp.resize(4);
        for (int k = 0; k < 3; k++) {
            double ns[22] = {0}; ns[0] = 0.1 * k; ns[9] = 1.0; unpack(ns, kf[k].ns); kf[k].mnId = (unsigned long)k; kf[k].prev = k ? &kf[k - 1] : nullptr;
            kf[k].fx = kf[k].fy = 450; kf[k].cx = 376; kf[k].cy = 240;
            double pre[142] = {0}; pre[0] = 0.1; pre[6] = pre[10] = pre[14] = 1.0; for (int d = 0; d < 9; d++) pre[60 + 10 * d] = 1e-4; pre[141] = 0.05;
            fill_preint(pre, kf[k].pre);
            map.kfs.push_back(&kf[k]);
        }
        const double P[4][3] = {{0.5, 0.2, 4}, {-0.4, 0.3, 5}, {0.1, -0.5, 6}, {-0.2, -0.1, 3}};
        for (int p = 0; p < 4; p++) {
            mp[p].Pw = point_mat(P[p]); mp[p].mnId = (unsigned long)p;
            for (int k = 0; k < 3; k++) observe(mp[p], kf[k], 450 * (P[p][0] - 0.1 * k) / P[p][2] + 376, 450 * P[p][1] / P[p][2] + 240, 1.0);
        }
    }
    for (size_t p = 0; p < mp.size(); p++) map.pts.push_back(&mp[p]);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Tbc(r, c) = cam[4 + 3 * r + c]; Tbc(r, 3) = cam[13 + r]; }
    Tbc(3, 3) = 1.0;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) MatTbc.at<float>(r, c) = (float)Tbc(r, c);
    volatile int stop = 0; bool bstop = false;
    double info[6] = {0, 0, 0, 0, 0, 0};
    if (argc < 4) {
        // a stereo observation is rejected before the library is called
        KeyFrame extra = kf[2]; MapPoint sp = mp[0]; sp.obs.clear(); observe(sp, extra, 300, 200, 1.0, 290.f);
        Map m2 = map; m2.pts.push_back(&sp);
        bool threw = false;
        try { viorb_shim::global_bundle_adjustment_navstate<Vec3, Quat, SO3>(&m2, gw, 10, &bstop, &stop, 0ul, true, Tbc, MatTbc); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("Stereo") != std::string::npos; }
        if (!threw) { printf("FAIL: a stereo observation did not throw\n"); return 1; }
        if (viorb_device_count() < 1) {
            threw = false;
            try { viorb_shim::global_bundle_adjustment_navstate<Vec3, Quat, SO3>(&map, gw, 10, &bstop, &stop, 0ul, true, Tbc, MatTbc); }
            catch (const std::runtime_error& e) { threw = true; printf("OK threw: %s\n", e.what()); }
            if (!threw || kf[1].ns_sets || mp[0].pos_sets) { printf("FAIL: no device, but the template did not throw or touched the map\n"); return 1; }
            return 0;
        }
    }
    try { viorb_shim::global_bundle_adjustment_navstate<Vec3, Quat, SO3>(&map, gw, iterations, &bstop, &stop, nLoopKF, robust != 0, Tbc, MatTbc, info); }
    catch (const std::runtime_error& e) { printf("FAIL: %s\n", e.what()); return 1; }
    printf("OK iterations %d trials %d chi2 %.10g -> %.10g\n", (int)info[2], (int)info[3], info[0], info[1]);
    if (argc < 4) return 0;
    // out: info6 | per key frame: ns22 (GetNavState), gba22 (mNavStateGBA), Tcw16 (mTcwGBA or zeros), ns_sets, pose_updates, mnBAGlobalForKF
    //            | per point: Pw3, mPosGBA3 (or zeros), pos_sets, normal_updates, mnBAGlobalForKF
    std::vector<double> out(info, info + 6);
    for (size_t k = 0; k < kf.size(); k++) {
        double a[22], b[22];
        viorb_shim::pack_navstate(kf[k].ns, a); viorb_shim::pack_navstate(kf[k].mNavStateGBA, b);
        out.insert(out.end(), a, a + 22); out.insert(out.end(), b, b + 22);
        for (int i = 0; i < 16; i++) out.push_back(kf[k].mTcwGBA.empty() ? 0.0 : (double)kf[k].mTcwGBA.at<float>(i / 4, i % 4));
        out.push_back(kf[k].ns_sets); out.push_back(kf[k].pose_updates); out.push_back((double)kf[k].mnBAGlobalForKF);
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
