// tests/cpp/shim_map_correction_test.cpp — drives viorb_shim::correct_loop_propagate and viorb_shim::apply_global_ba
// (viorb_amd/shim/LoopClosing_shim.h) with the stand-in types of map_correction_standin.h, from problem files that
// tests/test_gpu_map_correction_shim.py writes (mode 0: one scene of viorb_correct_loop; mode 1: one map of viorb_apply_global_ba; the key
// frame of slot kf_by_key[j] is stored at position j, so pointer order is the scene's key order), and writes what the templates left in
// the objects, every number as a double, for the test to compare with the checker tests/map_correction_ref.py.
// usage: shim_map_correction_test problem.bin out.bin [problem.bin out.bin ...]   (one process for all: the device is opened once)
//        exit 0 ok, 2 usage / io, 3 a template threw (printed as "exception: ...")
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "map_correction_standin.h"
#include "LoopClosing_shim.h"

typedef mcs::KeyFrame KeyFrame;
typedef mcs::MapPoint MapPoint;

static std::vector<unsigned char> g_blob;
static size_t g_pos = 0;
template <class T> static const T* take(size_t n) {
    const T* p = reinterpret_cast<const T*>(g_blob.data() + g_pos);
    g_pos += n * sizeof(T);
    if (g_pos > g_blob.size()) { std::printf("problem file too short\n"); std::exit(2); }
    return p;
}
static cv::Mat pose_mat(const float* T12) {
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T.at<float>(r, c) = T12[3 * r + c]; T.at<float>(r, 3) = T12[9 + r]; }
    T.at<float>(3, 3) = 1.0f;
    return T;
}
static cv::Mat vec3(const float* v) { cv::Mat P(3, 1, CV_32F); for (int c = 0; c < 3; c++) P.at<float>(c) = v[c]; return P; }
static void put_pose(std::vector<double>& out, const cv::Mat& T) {
    for (int i = 0; i < 12; i++) out.push_back(T.empty() ? 0.0 : (double)(i < 9 ? T.at<float>(i / 3, i % 3) : T.at<float>(i - 9, 3)));
}
static standin::NavState ns_of(const double* o) {
    standin::NavState n;
    viorb_shim::unpack_navstate<standin::NavState, standin::Vec3, standin::Quat, standin::SO3>(o, n);
    return n;
}
static void put_ns(std::vector<double>& out, const standin::NavState& n) { double o[22]; viorb_shim::pack_navstate(n, o); out.insert(out.end(), o, o + 22); }

static int correct_loop(const int32_t* h, std::vector<double>& out) {
    const int nk = h[1], nkp = h[2], np = h[3], no = h[4], nc = h[5], cur = h[6], cur_id = h[7];
    const int32_t *by_key = take<int32_t>(nk), *kp_start = take<int32_t>(nk + 1), *kp_point = take<int32_t>(nkp), *pt_bad = take<int32_t>(np), *obs_start = take<int32_t>(np + 1),
                  *obs = take<int32_t>(no), *pt_ref = take<int32_t>(np), *pt_by = take<int32_t>(np), *conn = take<int32_t>(nc);
    const float *pose12 = take<float>((size_t)nk * 12), *pts_f = take<float>((size_t)np * 8);
    const double* Scw8 = take<double>(8);
    std::vector<KeyFrame> store(nk); std::vector<MapPoint> pts(np); std::vector<KeyFrame*> kfs(nk);
    for (int j = 0; j < nk; j++) kfs[by_key[j]] = &store[j];            // ascending addresses in key order
    for (int k = 0; k < nk; k++) {
        KeyFrame& K = *kfs[k];
        K.mnId = k == cur ? (long unsigned int)cur_id : 1000u + k;
        K.Tcw = pose_mat(pose12 + 12 * (size_t)k);
        float sf = 1.0f;
        for (int i = 0; i < 8; i++) { K.mvScaleFactors.push_back(sf); sf *= 1.2f; }
        for (int i = kp_start[k]; i < kp_start[k + 1]; i++) K.mvpMapPoints.push_back(kp_point[i] >= 0 ? &pts[kp_point[i]] : nullptr);
    }
    for (int p = 0; p < np; p++) {
        MapPoint& P = pts[p];
        P.bad = pt_bad[p] != 0; P.Pw = vec3(pts_f + 8 * (size_t)p); P.normal = vec3(pts_f + 8 * (size_t)p + 3); P.mind = pts_f[8 * p + 6]; P.maxd = pts_f[8 * p + 7];
        P.mnCorrectedByKF = (long unsigned int)pt_by[p]; P.ref = pt_ref[p] >= 0 ? kfs[pt_ref[p]] : nullptr;
        for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
            KeyFrame* K = kfs[obs[o] & 0xffff];
            K->mvKeysUn.push_back(cv::KeyPoint(0, 0, 0, -1, 0, (obs[o] >> 16) & 0xff));
            P.mObservations[K] = K->mvKeysUn.size() - 1;
        }
    }
    std::vector<KeyFrame*> connected;
    for (int i = 0; i < nc; i++) connected.push_back(kfs[conn[i]]);
    connected.push_back(kfs[cur]);                                      // :462
    mcs::Sim3 Scw; std::memcpy(Scw.v, Scw8, sizeof(Scw.v));
    std::map<KeyFrame*, mcs::Sim3> Corrected, NonCorrected;
    viorb_shim::correct_loop_propagate<KeyFrame, MapPoint>(kfs[cur], connected, Scw, Corrected, NonCorrected,
        [](const mcs::Sim3& s, double* o) { std::memcpy(o, s.v, sizeof(s.v)); }, [](const double* o) { mcs::Sim3 s; std::memcpy(s.v, o, sizeof(s.v)); return s; }, pose_mat);
    for (int k = 0; k < nk; k++) { put_pose(out, kfs[k]->Tcw); out.push_back(kfs[k]->pose_sets); }
    for (int p = 0; p < np; p++) {
        const MapPoint& P = pts[p];
        for (int c = 0; c < 3; c++) out.push_back(P.Pw.at<float>(c));
        for (int c = 0; c < 3; c++) out.push_back(P.normal.at<float>(c));
        out.push_back(P.mind); out.push_back(P.maxd); out.push_back((double)P.mnCorrectedByKF);
        out.push_back(P.mnCorrectedReference == (long unsigned int)cur_id ? cur : (double)P.mnCorrectedReference - 1000.0);
        out.push_back(P.pos_sets); out.push_back(P.normal_sets);
    }
    out.push_back((double)Corrected.size());
    for (auto& kv : Corrected) {
        out.push_back(kv.first == kfs[cur] ? cur : (double)kv.first->mnId - 1000.0);
        for (int c = 0; c < 8; c++) out.push_back(kv.second.v[c]);
        for (int c = 0; c < 8; c++) out.push_back(NonCorrected[kv.first].v[c]);
    }
    return 0;
}

static int apply_gba(const int32_t* h, std::vector<double>& out) {
    const int nk = h[1], nchild = h[2], norigin = h[3], np = h[4];
    const unsigned long nLoopKF = 5;
    const int32_t *child_start = take<int32_t>(nk + 1), *child_kf = take<int32_t>(nchild), *origins = take<int32_t>(norigin), *in_gba = take<int32_t>(nk), *pt_bad = take<int32_t>(np),
                  *pt_in = take<int32_t>(np), *pt_ref = take<int32_t>(np);
    const float *pose12 = take<float>((size_t)nk * 12), *gba12 = take<float>((size_t)nk * 12), *Pw = take<float>((size_t)np * 3), *PosGBA = take<float>((size_t)np * 3), *Tbc12 = take<float>(12);
    const double *ns22 = take<double>((size_t)nk * 22), *nsg22 = take<double>((size_t)nk * 22);
    std::vector<KeyFrame> kfs(nk); std::vector<MapPoint> pts(np);
    mcs::Map map;
    for (int k = 0; k < nk; k++) {
        KeyFrame& K = kfs[k];
        K.mnId = k; K.mnBAGlobalForKF = in_gba[k] ? nLoopKF : 0; K.Tcw = pose_mat(pose12 + 12 * (size_t)k); K.mTcwGBA = pose_mat(gba12 + 12 * (size_t)k);
        K.ns = ns_of(ns22 + 22 * (size_t)k); K.mNavStateGBA = ns_of(nsg22 + 22 * (size_t)k);
        for (int i = child_start[k]; i < child_start[k + 1]; i++) K.children.insert(&kfs[child_kf[i]]);
        map.kfs.push_back(&K);
    }
    for (int i = 0; i < norigin; i++) map.mvpKeyFrameOrigins.push_back(&kfs[origins[i]]);
    for (int p = 0; p < np; p++) {
        MapPoint& P = pts[p];
        P.bad = pt_bad[p] != 0; P.mnBAGlobalForKF = pt_in[p] ? nLoopKF : 0; P.Pw = vec3(Pw + 3 * (size_t)p); P.mPosGBA = vec3(PosGBA + 3 * (size_t)p); P.ref = &kfs[pt_ref[p]];
        map.pts.push_back(&P);
    }
    viorb_shim::apply_global_ba<KeyFrame, MapPoint, standin::NavState, standin::Vec3, standin::Quat, standin::SO3>(&map, nLoopKF, pose_mat(Tbc12), pose_mat);
    for (int k = 0; k < nk; k++) {
        const KeyFrame& K = kfs[k];
        put_pose(out, K.Tcw); put_ns(out, K.ns); put_pose(out, K.mTcwBefGBA); put_ns(out, K.mNavStateBefGBA); put_pose(out, K.mTcwGBA); put_ns(out, K.mNavStateGBA);
        out.push_back(K.mnBAGlobalForKF == nLoopKF); out.push_back(K.pose_sets);
    }
    for (int p = 0; p < np; p++) { for (int c = 0; c < 3; c++) out.push_back(pts[p].Pw.at<float>(c)); out.push_back(pts[p].pos_sets); }
    return 0;
}

static int run_one(const char* problem, const char* result) {
    g_pos = 0;
    FILE* f = std::fopen(problem, "rb");
    if (!f) { std::printf("cannot open %s\n", problem); return 2; }
    std::fseek(f, 0, SEEK_END); const long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    g_blob.resize((size_t)sz);
    if (std::fread(g_blob.data(), 1, (size_t)sz, f) != (size_t)sz) { std::printf("short read\n"); return 2; }
    std::fclose(f);
    const int32_t* h = take<int32_t>(8);
    std::vector<double> out;
    try {
        if (h[0] == 0) correct_loop(h, out); else apply_gba(h, out);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    FILE* o = std::fopen(result, "wb");
    if (!o) return 2;
    std::fwrite(out.data(), 8, out.size(), o);
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3 || argc % 2 != 1) { std::printf("usage: %s problem.bin out.bin [problem.bin out.bin ...]\n", argv[0]); return 2; }
    for (int a = 1; a + 1 < argc; a += 2) {
        const int rc = run_one(argv[a], argv[a + 1]);
        if (rc != 0) { std::printf("failed at %s\n", argv[a]); return rc; }
    }
    return 0;
}
