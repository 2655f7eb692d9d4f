// tests/cpp/shim_reloc_test.cpp — drives the relocalisation templates of viorb_amd/shim (relocalization_refine of viorb_tracking_shim.h,
// search_by_projection_reloc of ORBmatcher_shim.h) with stand-in Frame / KeyFrame / MapPoint / cv types from a problem file that
// tests/test_gpu_relocalization_shim.py writes, and writes what they leave in mvpMapPoints, mvbOutlier and mTcw.
// usage: shim_reloc_test problem.bin out.bin     exit 0 ok, 2 usage / io, 3 the shim threw (printed as "exception: ...")
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>
#include "reloc_standin.h"
#include "ORBmatcher_shim.h"

using standin::Frame;
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

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: shim_reloc_test problem.bin out.bin\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END); g_blob.resize((size_t)std::ftell(f)); std::fseek(f, 0, SEEK_SET);
    if (std::fread(g_blob.data(), 1, g_blob.size(), f) != g_blob.size()) return 2;
    std::fclose(f);
    const int32_t* head = take<int32_t>(4);
    const int n = head[0], np = head[1], nlevels = head[2], repeat = head[3];     // repeat: a map point held by two key-frame features
    const float* intr = take<float>(5); const float* bounds = take<float>(4); const float* sf = take<float>(16);
    const viorb_keypoint* k = take<viorb_keypoint>(n);
    const unsigned char* desc = take<unsigned char>((size_t)n * 32);
    const float* uright = take<float>(n);
    const float* pose = take<float>(12);
    const float* angle = take<float>(np); const unsigned char* valid = take<unsigned char>(np); const unsigned char* bad = take<unsigned char>(np);
    const float* pf = take<float>((size_t)np * 8); const unsigned char* pd = take<unsigned char>((size_t)np * 32);
    const int32_t* bow = take<int32_t>(n); const unsigned char* inl = take<unsigned char>(n);
    const unsigned char* found = take<unsigned char>(np); const unsigned char* taken = take<unsigned char>(n);

    Frame F;
    F.N = n; F.fx = intr[0]; F.fy = intr[1]; F.cx = intr[2]; F.cy = intr[3]; F.mbf = intr[4];
    F.mnMinX = bounds[0]; F.mnMaxX = bounds[1]; F.mnMinY = bounds[2]; F.mnMaxY = bounds[3];
    F.mnScaleLevels = nlevels; F.mvScaleFactors.assign(sf, sf + nlevels);
    for (int l = 0; l < nlevels; l++) F.mvLevelSigma2.push_back(sf[l] * sf[l]);
    F.mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
    if (n) std::memcpy(F.mDescriptors.data, desc, (size_t)n * 32);
    for (int j = 0; j < n; j++) F.mvKeysUn.push_back(cv::KeyPoint(k[j].x, k[j].y, k[j].size, k[j].angle, k[j].response, k[j].octave, k[j].class_id));
    F.mvuRight.assign(uright, uright + n);
    F.mvpMapPoints.assign(n, nullptr); F.mvbOutlier.assign(n, false);
    std::vector<MapPoint> pts(np); MapPoint other; other.id = -2;
    KeyFrame KF;
    KF.mvpMapPoints.assign(np, nullptr);
    for (int i = 0; i < np; i++) {
        KF.mvKeysUn.push_back(cv::KeyPoint(0, 0, 31, angle[i], 1, 0, -1));
        if (!valid[i] && !bad[i]) continue;
        MapPoint& m = pts[i];
        for (int c = 0; c < 3; c++) m.mWorldPos.at<float>(c) = pf[(size_t)i * 8 + c];
        m.mfMinDistance = pf[(size_t)i * 8 + 6]; m.mfMaxDistance = pf[(size_t)i * 8 + 7]; m.mbBad = bad[i] != 0; m.id = i;
        std::memcpy(m.mDescriptor.data, pd + (size_t)i * 32, 32);
        KF.mvpMapPoints[i] = &m;
    }
    if (repeat && np >= 2 && KF.mvpMapPoints[0]) KF.mvpMapPoints[1] = KF.mvpMapPoints[0];
    cv::Mat Tcw(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw.at<float>(r, c) = r < 3 ? (c < 3 ? pose[3 * r + c] : pose[9 + r]) : (c == 3 ? 1.f : 0.f);
    std::vector<bool> vbInliers(n); std::vector<MapPoint*> vpMapPointMatches(n, nullptr);
    for (int j = 0; j < n; j++) { vbInliers[j] = inl[j] != 0; if (bow[j] >= 0) vpMapPointMatches[j] = KF.mvpMapPoints[bow[j]]; }

    int nGood = 0, stage = 0, nmatches = 0;
    std::vector<int32_t> out;
    try {
        nGood = viorb_shim::relocalization_refine<Frame, KeyFrame, MapPoint>(F, &KF, Tcw, vbInliers, vpMapPointMatches, true, &stage);
        out.push_back(nGood); out.push_back(stage);
        for (int j = 0; j < n; j++) out.push_back(F.mvpMapPoints[j] ? F.mvpMapPoints[j]->id : -1);
        for (int j = 0; j < n; j++) out.push_back(F.mvbOutlier[j] ? 1 : 0);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { float v = F.mTcw.at<float>(r, c); int32_t w; std::memcpy(&w, &v, 4); out.push_back(w); }
        for (int r = 0; r < 3; r++) { float v = F.mTcw.at<float>(r, 3); int32_t w; std::memcpy(&w, &v, 4); out.push_back(w); }
        // the matcher alone, as ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) at the hypothesis' pose
        Frame G = F;
        G.mTcw = Tcw;
        std::set<MapPoint*> sAlreadyFound;
        for (int i = 0; i < np; i++) if (found[i] && KF.mvpMapPoints[i]) sAlreadyFound.insert(KF.mvpMapPoints[i]);
        for (int j = 0; j < n; j++) G.mvpMapPoints[j] = taken[j] ? &other : nullptr;
        nmatches = viorb_shim::search_by_projection_reloc<Frame, KeyFrame, MapPoint>(G, &KF, sAlreadyFound, 10.f, 100, true);
        out.push_back(nmatches);
        for (int j = 0; j < n; j++) out.push_back(G.mvpMapPoints[j] ? G.mvpMapPoints[j]->id : -1);
    } catch (const std::runtime_error& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(out.data(), sizeof(int32_t), out.size(), o);
    std::fclose(o);
    std::printf("nGood %d stage %d nmatches %d\n", nGood, stage, nmatches);
    return 0;
}
