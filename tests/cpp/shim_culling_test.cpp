// tests/cpp/shim_culling_test.cpp — drives viorb_shim::key_frame_culling and viorb_shim::map_point_culling
// (viorb_amd/shim/LocalMapping_shim.h) with the stand-in KeyFrame / MapPoint of culling_standin.h, from a problem file that
// tests/test_gpu_culling_shim.py writes (one scene of viorb_amd/culling.py and one list of recent map points). It writes the reasons,
// the map the stand-ins hold after the shim's SetBadFlag calls, and the state the library reported, all in the scene's numbering.
// usage: shim_culling_test problem.bin out.bin     exit 0 ok, 2 usage / io, 3 the shim threw (printed as "exception: ...")
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <stdexcept>
#include <string>
#include <vector>
#include "culling_standin.h"
#include "LocalMapping_shim.h"

typedef standin::CullKeyFrame KeyFrame;
typedef standin::CullMapPoint MapPoint;

static std::vector<unsigned char> g_blob;
static size_t g_pos = 0;
template <class T> static const T* take(size_t n) {
    const T* p = reinterpret_cast<const T*>(g_blob.data() + g_pos);
    g_pos += n * sizeof(T);
    if (g_pos > g_blob.size()) { std::printf("problem file too short\n"); std::exit(2); }
    return p;
}
static void put(FILE* o, const std::vector<int32_t>& v) { if (!v.empty()) std::fwrite(v.data(), 4, v.size(), o); }

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: %s problem.bin out.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END); const long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    g_blob.resize((size_t)sz);
    if (std::fread(g_blob.data(), 1, (size_t)sz, f) != (size_t)sz) { std::printf("short read\n"); return 2; }
    std::fclose(f);
    // nk nc nkp np nobs cur monocular vins_inited n_recent cur_kf_id, then th_depth
    const int32_t* h = take<int32_t>(10);
    const int nk = h[0], nc = h[1], nkp = h[2], np = h[3], no = h[4], cur = h[5], n_recent = h[8];
    const bool mono = h[6] != 0, vins = h[7] != 0;
    const float th = *take<float>(1);
    const double* kf_time = take<double>(nk);
    const int32_t* kf_prev = take<int32_t>(nk); const int32_t* kf_next = take<int32_t>(nk); const int32_t* cand_kf = take<int32_t>(nc);
    const int32_t* kp_start = take<int32_t>(nc + 1); const int32_t* kp_point = take<int32_t>(nkp); const float* kp_depth = take<float>(nkp);
    const int32_t* pt_nobs = take<int32_t>(np); const int32_t* obs_start = take<int32_t>(np + 1); const uint32_t* obs = take<uint32_t>(no);
    const int32_t* r_found = take<int32_t>(n_recent); const int32_t* r_visible = take<int32_t>(n_recent); const int32_t* r_first = take<int32_t>(n_recent);
    const int32_t* r_nobs = take<int32_t>(n_recent);
    const unsigned char* kf_flags = take<unsigned char>(nk); const unsigned char* kp_octave = take<unsigned char>(nkp); const unsigned char* pt_bad = take<unsigned char>(np);
    const unsigned char* r_bad = take<unsigned char>(n_recent);

    std::vector<KeyFrame> kfs(nk); std::vector<MapPoint> pts(np);
    for (int k = 0; k < nk; k++) {
        kfs[k].id = k; kfs[k].mnId = (kf_flags[k] & 1) ? 0 : (unsigned long)(k + 1); kfs[k].mbNotErase = (kf_flags[k] & 2) != 0; kfs[k].mTimeStamp = kf_time[k]; kfs[k].mThDepth = th;
        kfs[k].mpPrevKeyFrame = kf_prev[k] >= 0 ? &kfs[kf_prev[k]] : nullptr; kfs[k].mpNextKeyFrame = kf_next[k] >= 0 ? &kfs[kf_next[k]] : nullptr;
    }
    for (int j = 0; j < nc; j++) {                                   // the candidates' keypoint tables
        KeyFrame& K = kfs[cand_kf[j]];
        kfs[cur].covisible.push_back(&K);
        for (int i = kp_start[j]; i < kp_start[j + 1]; i++) {
            K.mvKeysUn.push_back(cv::KeyPoint(0, 0, 31, 0, 0, kp_octave[i])); K.mvuRight.push_back(-1.f); K.mvDepth.push_back(kp_depth[i]);
            K.mvpMapPoints.push_back(kp_point[i] >= 0 ? &pts[kp_point[i]] : nullptr);
        }
    }
    for (int p = 0; p < np; p++) {                                   // an observation points at a keypoint of its own behind the table
        pts[p].id = p; pts[p].nObs = pt_nobs[p]; pts[p].mbBad = pt_bad[p] != 0;
        for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
            KeyFrame& K = kfs[obs[o] & 0xffffu];
            pts[p].mObservations[&K] = K.mvKeysUn.size();
            K.mvKeysUn.push_back(cv::KeyPoint(0, 0, 31, 0, 0, (int)((obs[o] >> 16) & 0xffu))); K.mvuRight.push_back((obs[o] & (1u << 24)) ? 10.f : -1.f); K.mvDepth.push_back(1.f);
            K.mvpMapPoints.push_back(nullptr);
        }
    }
    std::vector<MapPoint> recent(n_recent); std::list<MapPoint*> mlpRecentAddedMapPoints;
    for (int i = 0; i < n_recent; i++) {
        recent[i].id = i; recent[i].mbBad = r_bad[i] != 0; recent[i].mnFound = r_found[i]; recent[i].mnVisible = r_visible[i]; recent[i].mnFirstKFid = r_first[i]; recent[i].nObs = r_nobs[i];
        mlpRecentAddedMapPoints.push_back(&recent[i]);
    }

    viorb_shim::CullingReport<KeyFrame, MapPoint> R;
    int n_culled = 0, n_bad = 0;
    try {
        n_culled = viorb_shim::key_frame_culling<KeyFrame, MapPoint>(&kfs[cur], mono, vins, &R);
        n_bad = viorb_shim::map_point_culling(mlpRecentAddedMapPoints, (unsigned long)h[9], mono);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    const int32_t none = -99;
    std::vector<int32_t> head(2), culled(nc, -1), kf_state((size_t)nk * 8, none), pt_state((size_t)np * 4, none), rec((size_t)n_recent * 2, 0);
    head[0] = n_culled; head[1] = n_bad;
    for (size_t k = 0; k < R.culled.size(); k++) culled[k] = R.culled[k]->id;
    for (int k = 0; k < nk; k++) {
        int32_t* s = &kf_state[(size_t)k * 8];
        s[0] = kfs[k].mbBad; s[1] = kfs[k].mbToBeErased; s[2] = kfs[k].mpPrevKeyFrame ? kfs[k].mpPrevKeyFrame->id : -1; s[3] = kfs[k].mpNextKeyFrame ? kfs[k].mpNextKeyFrame->id : -1;
        s[4] = kfs[k].preint_calls;
    }
    for (size_t k = 0; k < R.kfs.size(); k++) {                      // what the library reported, in the scene's numbering
        int32_t* s = &kf_state[(size_t)R.kfs[k]->id * 8];
        s[5] = R.kf_prev_out[k] >= 0 ? R.kfs[R.kf_prev_out[k]]->id : -1; s[6] = R.kf_next_out[k] >= 0 ? R.kfs[R.kf_next_out[k]]->id : -1; s[7] = R.kf_repreint[k];
    }
    for (int p = 0; p < np; p++) { pt_state[(size_t)p * 4] = pts[p].nObs; pt_state[(size_t)p * 4 + 1] = pts[p].mbBad; }
    for (size_t p = 0; p < R.pts.size(); p++) { pt_state[(size_t)R.pts[p]->id * 4 + 2] = R.pt_nobs_out[p]; pt_state[(size_t)R.pts[p]->id * 4 + 3] = R.pt_bad_out[p]; }
    for (int i = 0; i < n_recent; i++) rec[(size_t)i * 2] = recent[i].mbBad;
    for (std::list<MapPoint*>::iterator it = mlpRecentAddedMapPoints.begin(); it != mlpRecentAddedMapPoints.end(); ++it) rec[(size_t)(*it)->id * 2 + 1] = 1;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    put(o, head); put(o, R.reason); put(o, R.redundant); put(o, R.mps); put(o, culled); put(o, kf_state); put(o, pt_state); put(o, rec);
    std::fclose(o);
    std::printf("culled %d, %d recent points set bad\n", n_culled, n_bad);
    return 0;
}
