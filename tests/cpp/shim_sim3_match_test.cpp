// tests/cpp/shim_sim3_match_test.cpp — drives the three Sim3 matcher templates of viorb_amd/shim/ORBmatcher_shim.h (search_by_sim3,
// search_by_projection_sim3, fuse_sim3) with stand-in KeyFrame / MapPoint / cv types from a problem file that
// tests/test_gpu_sim3_match_shim.py writes, and writes what they leave in vpMatches12, vpMatched, vpReplacePoint and the observations.
// usage: shim_sim3_match_test problem.bin out.bin     exit 0 ok, 2 usage / io, 3 the shim threw (printed as "exception: ...")
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "sim3_match_standin.h"
#include "ORBmatcher_shim.h"

using standin::KeyFrame;
using standin::MapPoint;

static std::vector<unsigned char> g_blob;
static size_t g_pos = 0;
template <class T> static const T* take(size_t n) {
    const T* p = reinterpret_cast<const T*>(g_blob.data() + g_pos);
    g_pos += n * sizeof(T);
    if (g_pos > g_blob.size()) { std::printf("problem file too short\n"); std::exit(2); }
    return p;
}

static void fill_point(MapPoint& m, const float* f8, const unsigned char* d32, bool bad, int id) {
    for (int c = 0; c < 3; c++) { m.mWorldPos.at<float>(c) = f8[c]; m.mNormalVector.at<float>(c) = f8[3 + c]; }
    m.mfMinDistance = f8[6]; m.mfMaxDistance = f8[7]; m.mbBad = bad; m.id = id;
    std::memcpy(m.mDescriptor.data, d32, 32);
}

struct Side { KeyFrame kf; std::vector<MapPoint> pts; };
static void read_side(Side& S, int n, const float* intr, const float* bounds, const float* sf, int nlevels, int id0) {
    const viorb_keypoint* k = take<viorb_keypoint>(n);
    const unsigned char* desc = take<unsigned char>((size_t)n * 32);
    const float* pose = take<float>(12);
    const unsigned char* has = take<unsigned char>(n);
    const unsigned char* bad = take<unsigned char>(n);
    const float* pf = take<float>((size_t)n * 8);
    const unsigned char* pd = take<unsigned char>((size_t)n * 32);
    KeyFrame& K = S.kf;
    K.N = n; K.fx = intr[0]; K.fy = intr[1]; K.cx = intr[2]; K.cy = intr[3];
    K.mnMinX = bounds[0]; K.mnMaxX = bounds[1]; K.mnMinY = bounds[2]; K.mnMaxY = bounds[3];
    K.mnScaleLevels = nlevels; K.mvScaleFactors.assign(sf, sf + nlevels);
    K.mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
    if (n) std::memcpy(K.mDescriptors.data, desc, (size_t)n * 32);
    K.mRcw.create(3, 3, CV_32F); K.mtcw.create(3, 1, CV_32F);
    for (int i = 0; i < 9; i++) K.mRcw.at<float>(i) = pose[i];
    for (int i = 0; i < 3; i++) K.mtcw.at<float>(i) = pose[9 + i];
    S.pts.resize(n);
    K.mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; i++) {
        K.mvKeysUn.push_back(cv::KeyPoint(k[i].x, k[i].y, k[i].size, k[i].angle, k[i].response, k[i].octave, k[i].class_id));
        if (!has[i]) continue;
        fill_point(S.pts[i], pf + (size_t)i * 8, pd + (size_t)i * 32, bad[i] != 0, id0 + i);
        S.pts[i].mObservations[&K] = (size_t)i;
        K.mvpMapPoints[i] = &S.pts[i];
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: shim_sim3_match_test problem.bin out.bin\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END); g_blob.resize((size_t)std::ftell(f)); std::fseek(f, 0, SEEK_SET);
    if (std::fread(g_blob.data(), 1, g_blob.size(), f) != g_blob.size()) return 2;
    std::fclose(f);
    const int32_t* head = take<int32_t>(4);
    const int n1 = head[0], n2 = head[1], np = head[2], nlevels = head[3];
    const float* intr = take<float>(4); const float* bounds = take<float>(4); const float* sf = take<float>(16);
    const float* model = take<float>(13);                 // R12 t12 s12
    const float* scw = take<float>(12);
    const float* th = take<float>(3);                     // SearchBySim3, SearchByProjection, Fuse
    Side S1, S2;
    read_side(S1, n1, intr, bounds, sf, nlevels, 0);
    read_side(S2, n2, intr, bounds, sf, nlevels, 100000);
    const int32_t* partner1 = take<int32_t>(n1);          // vpMatches12 on entry: the feature of key frame 2 whose point it holds, or -1
    const float* lpf = take<float>((size_t)np * 8); const unsigned char* lpd = take<unsigned char>((size_t)np * 32);
    const unsigned char* lbad = take<unsigned char>(np);
    const int32_t* matched_init = take<int32_t>(n1);      // vpMatched on entry: a loop point, -2 another point, -1 NULL
    const int32_t* in_kf = take<int32_t>(np);             // Fuse: the feature of key frame 1 that already holds loop point p, or -1
    std::vector<MapPoint> loop(np); MapPoint other;
    other.id = -2;
    std::vector<MapPoint*> vpPoints(np);
    for (int p = 0; p < np; p++) { fill_point(loop[p], lpf + (size_t)p * 8, lpd + (size_t)p * 32, lbad[p] != 0, 1000000 + p); vpPoints[p] = &loop[p]; }

    cv::Mat R12(3, 3, CV_32F), t12(3, 1, CV_32F), Scw(4, 4, CV_32F);
    for (int i = 0; i < 9; i++) R12.at<float>(i) = model[i];
    for (int i = 0; i < 3; i++) t12.at<float>(i) = model[9 + i];
    for (int i = 0; i < 12; i++) Scw.at<float>(i) = scw[i];
    Scw.at<float>(15) = 1.f;
    std::vector<MapPoint*> vpMatches12(n1, nullptr), vpMatched(n1, nullptr), vpReplacePoint(np, nullptr);
    for (int i = 0; i < n1; i++) if (partner1[i] >= 0) vpMatches12[i] = S2.kf.mvpMapPoints[partner1[i]];
    for (int i = 0; i < n1; i++) vpMatched[i] = matched_init[i] >= 0 ? &loop[matched_init[i]] : (matched_init[i] == -2 ? &other : nullptr);
    int nFound = 0, nMatches = 0, nFused = 0;
    try {
        nFound = viorb_shim::search_by_sim3<KeyFrame, MapPoint>(&S1.kf, &S2.kf, vpMatches12, model[12], R12, t12, th[0]);
        nMatches = viorb_shim::search_by_projection_sim3<KeyFrame, MapPoint>(&S1.kf, Scw, vpPoints, vpMatched, (int)th[1]);
        for (int p = 0; p < np; p++) if (in_kf[p] >= 0) S1.kf.mvpMapPoints[in_kf[p]] = &loop[p];
        nFused = viorb_shim::fuse_sim3<KeyFrame, MapPoint>(&S1.kf, Scw, vpPoints, th[2], vpReplacePoint);
    } catch (const std::runtime_error& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    std::vector<int32_t> out;
    out.push_back(nFound); out.push_back(nMatches); out.push_back(nFused);
    for (int i = 0; i < n1; i++) out.push_back(vpMatches12[i] ? vpMatches12[i]->id : -1);
    for (int i = 0; i < n1; i++) out.push_back(vpMatched[i] ? vpMatched[i]->id : -1);
    for (int p = 0; p < np; p++) out.push_back(vpReplacePoint[p] ? vpReplacePoint[p]->id : -1);
    for (int p = 0; p < np; p++) out.push_back(loop[p].added.empty() ? -1 : (int32_t)loop[p].added[0].second);
    for (int p = 0; p < np; p++) out.push_back((int32_t)loop[p].added.size());
    for (int i = 0; i < n1; i++) out.push_back(S1.kf.mvpMapPoints[i] ? S1.kf.mvpMapPoints[i]->id : -1);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(out.data(), sizeof(int32_t), out.size(), o);
    std::fclose(o);
    std::printf("nFound %d nMatches %d nFused %d\n", nFound, nMatches, nFused);
    return 0;
}
