// tests/cpp/shim_mapping_test.cpp — compile / link / run test of viorb_amd/shim/LocalMapping_shim.h with the stand-ins of
// mapping_standin.h. Usage: shim_mapping_test problem.bin out.bin. The problem file (written by tests/test_gpu_mapping_shim.py) holds
// one current key frame and J neighbours; the program builds KeyFrame objects whose addresses order as the file's kf2_first flags
// say, runs viorb_shim::create_new_map_points, performs the reference's `new MapPoint` / AddObservation block on the result, runs
// viorb_shim::update_map_points on the new points (it must reproduce the descriptor, normal and depth range create returned) and
// writes the accepted list for the Python side to compare with the direct C-ABI call. Without a device both templates must THROW.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "mapping_standin.h"
#include "LocalMapping_shim.h"

using namespace standin;

static std::vector<unsigned char> g_blob; static size_t g_at = 0;
template <class T> static void rd(T* dst, size_t n) { std::memcpy(dst, &g_blob[g_at], n * sizeof(T)); g_at += n * sizeof(T); }
static int rdi() { int v; rd(&v, 1); return v; }
static float rdf() { float v; rd(&v, 1); return v; }

static void read_kf(KeyFrame& K, cv::Mat* F12, float* median, const float* cam8, const std::vector<float>& sf, const std::vector<float>& s2) {
    const int n = rdi();
    K.N = n; K.mvKeysUn.resize(n); K.mvKeys.resize(n); K.mvuRight.resize(n); K.mvDepth.resize(n); K.mps.assign(n, nullptr);
    std::vector<viorb_keypoint> kp(n); rd(kp.data(), n);
    for (int i = 0; i < n; i++) K.mvKeysUn[i] = cv::KeyPoint(kp[i].x, kp[i].y, kp[i].size, kp[i].angle, kp[i].response, kp[i].octave, kp[i].class_id);
    K.mDescriptors.create(n, 32, CV_8U); rd(K.mDescriptors.data, (size_t)n * 32);
    std::vector<unsigned char> hp(n); rd(hp.data(), n);
    static MapPoint some_point;
    for (int i = 0; i < n; i++) if (hp[i]) K.mps[i] = &some_point;
    rd(K.mvuRight.data(), n); rd(K.mvDepth.data(), n);
    std::vector<float> xy(2 * (size_t)n); rd(xy.data(), xy.size());
    for (int i = 0; i < n; i++) K.mvKeys[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1]);
    std::vector<int> node(n); rd(node.data(), n);
    for (int i = 0; i < n; i++) if (node[i] >= 0) K.mFeatVec.addFeature((unsigned)node[i], (unsigned)i);
    float pose[12]; rd(pose, 12);
    K.Tcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) K.Tcw.at<float>(r, c) = pose[3 * r + c]; K.Tcw.at<float>(r, 3) = pose[9 + r]; }
    K.Tcw.at<float>(3, 3) = 1.f;
    K.Ow = cv::Mat(3, 1, CV_32F); for (int c = 0; c < 3; c++) K.Ow.at<float>(c) = rdf();
    float F[9]; rd(F, 9); *median = rdf();
    if (F12) { *F12 = cv::Mat(3, 3, CV_32F); for (int k = 0; k < 9; k++) F12->at<float>(k / 3, k % 3) = F[k]; }
    K.fx = cam8[0]; K.fy = cam8[1]; K.cx = cam8[2]; K.cy = cam8[3]; K.mb = cam8[4]; K.mbf = cam8[5]; K.mfScaleFactor = cam8[6];
    K.mvScaleFactors = sf; K.mvLevelSigma2 = s2; K.mnScaleLevels = (int)sf.size();
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: shim_mapping_test problem.bin out.bin\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END); g_blob.resize((size_t)std::ftell(f)); std::fseek(f, 0, SEEK_SET);
    if (std::fread(g_blob.data(), 1, g_blob.size(), f) != g_blob.size()) return 2;
    std::fclose(f);
    const int J = rdi(), mono = rdi(), nlev = rdi();
    float cam8[8]; rd(cam8, 8);
    std::vector<float> sf(nlev), s2(nlev); rd(sf.data(), nlev); rd(s2.data(), nlev);
    std::vector<unsigned char> first(J); rd(first.data(), J);
    // one array of key frames: neighbours whose KeyFrame* must order before the current key frame's, the current one, the others
    int n_before = 0; for (int j = 0; j < J; j++) n_before += first[j] ? 1 : 0;
    std::vector<KeyFrame> store(J + 1);
    KeyFrame* cur = &store[n_before];
    std::vector<KeyFrame*> neigh(J); int lo = 0, hi = n_before + 1;
    for (int j = 0; j < J; j++) neigh[j] = first[j] ? &store[lo++] : &store[hi++];
    std::vector<cv::Mat> vF(J); std::vector<float> vMed(J);
    float dummy;
    read_kf(*cur, nullptr, &dummy, cam8, sf, s2);
    for (int j = 0; j < J; j++) read_kf(*neigh[j], &vF[j], &vMed[j], cam8, sf, s2);

    std::vector<viorb_shim::NewMapPoint> vNew;
    const bool have_device = viorb_device_count() > 0;
    try {
        viorb_shim::create_new_map_points(cur, neigh, vF, vMed, mono != 0, vNew);
        if (!have_device) { std::printf("FAIL create_new_map_points did not throw without a device\n"); return 1; }
    } catch (const std::runtime_error& e) {
        if (have_device) { std::printf("FAIL create_new_map_points threw: %s\n", e.what()); return 1; }
        if (std::string(e.what()).find("no HIP device") == std::string::npos) { std::printf("FAIL wrong error text: %s\n", e.what()); return 1; }
    }
    // the caller's part, src/LocalMapping.cc:1466-1481
    std::vector<MapPoint> pts(vNew.size() + 1); std::vector<MapPoint*> vp;
    for (size_t p = 0; p < vNew.size(); p++) {
        MapPoint& M = pts[p]; const viorb_shim::NewMapPoint& q = vNew[p];
        M.Pw = q.x3D; M.ref = cur;
        M.AddObservation(cur, q.idx1); M.AddObservation(neigh[q.neighbour], q.idx2);
        cur->AddMapPoint(&M, q.idx1); neigh[q.neighbour]->AddMapPoint(&M, q.idx2);
        vp.push_back(&M);
    }
    if (!have_device) {                                       // update_map_points on one hand-made point must throw as well
        MapPoint& M = pts[0]; M.ref = cur; M.Pw.at<float>(2) = 5.f; M.AddObservation(cur, 0); M.AddObservation(neigh[0], 0); vp.assign(1, &M);
        try { viorb_shim::update_map_points<KeyFrame, MapPoint>(vp); std::printf("FAIL update_map_points did not throw without a device\n"); return 1; }
        catch (const std::runtime_error&) {}
        std::printf("OK no device: both templates threw\n");
        return 0;
    }
    viorb_shim::update_map_points<KeyFrame, MapPoint>(vp);
    int bad = 0;
    for (size_t p = 0; p < vNew.size(); p++) {
        const MapPoint& M = pts[p]; const viorb_shim::NewMapPoint& q = vNew[p];
        if (M.updates != 1 || std::memcmp(M.desc.data, q.descriptor.data, 32) != 0 || M.minD != q.minDistance || M.maxD != q.maxDistance) bad++;
        for (int c = 0; c < 3; c++) if (M.Pn.at<float>(c) != q.normal.at<float>(c)) bad++;
    }
    if (bad) { std::printf("FAIL update_map_points differs from what create_new_map_points returned on %d values\n", bad); return 1; }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int n = (int)vNew.size(); std::fwrite(&n, 4, 1, o);
    for (int p = 0; p < n; p++) {
        const viorb_shim::NewMapPoint& q = vNew[p];
        const int idx[3] = {(int)q.idx1, (int)q.neighbour, (int)q.idx2}; std::fwrite(idx, 4, 3, o);
        const float v[8] = {q.x3D.at<float>(0), q.x3D.at<float>(1), q.x3D.at<float>(2), q.normal.at<float>(0), q.normal.at<float>(1), q.normal.at<float>(2),
                            q.minDistance, q.maxDistance};
        std::fwrite(v, 4, 8, o); std::fwrite(q.descriptor.data, 1, 32, o);
    }
    std::fclose(o);
    std::printf("OK %d new points through the shim, update_map_points reproduces them\n", n);
    return 0;
}
