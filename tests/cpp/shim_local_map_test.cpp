// tests/cpp/shim_local_map_test.cpp — drives viorb_shim::update_local_map (viorb_amd/shim/viorb_tracking_shim.h) with the stand-in Frame /
// KeyFrame / MapPoint of local_map_standin.h, from a problem file that tests/test_gpu_local_map_shim.py writes (one scene of
// viorb_amd/local_map.py; the key frame of slot kf_by_key[j] is stored at position j, so pointer order is the scene's key order). It then
// works out the expected members over the same objects from the same starting state (expected_local_map, a restatement in this project's
// own words), requires the written-back members to be equal, and writes them out in the scene's numbering.
// usage: shim_local_map_test problem.bin out.bin [problem.bin out.bin ...]   (one process for all: the device is opened once)
//        exit 0 ok, 2 usage / io, 3 the shim threw (printed as "exception: ..."), 4 the members differ; it stops at the first problem that fails
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "local_map_standin.h"
#include "viorb_tracking_shim.h"

typedef standin::LmKeyFrame KeyFrame;
typedef standin::LmMapPoint MapPoint;
typedef standin::LmFrame Frame;
using std::map; using std::set; using std::vector;

static std::vector<unsigned char> g_blob;
static size_t g_pos = 0;
static const int32_t* take(size_t n) {
    const int32_t* p = reinterpret_cast<const int32_t*>(g_blob.data() + g_pos);
    g_pos += n * 4;
    if (g_pos > g_blob.size()) { std::printf("problem file too short\n"); std::exit(2); }
    return p;
}

// What the tracking thread holds around the call, and what the call must leave there.
struct State {
    Frame frame; vector<KeyFrame*> local_kfs; KeyFrame* ref_kf = nullptr; vector<MapPoint*> local_pts;
};

// The expected result, restated over the stand-in objects in this project's own words (the rules are those of DESIGN.md "Local map" and of
// tests/local_map_ref.py; nothing here comes from the library or the shim). Sets of pointers stand for the per-frame marks.
static void expected_local_map(State& s) {
    // votes: one per observation of every good point the frame holds; a bad point leaves the frame
    map<KeyFrame*, int> votes;                                       // ordered by address, as the counter of the tracking thread is
    for (size_t i = 0; i < s.frame.mvpMapPoints.size(); i++) {
        MapPoint* p = s.frame.mvpMapPoints[i];
        if (!p) continue;
        if (p->isBad()) { s.frame.mvpMapPoints[i] = nullptr; continue; }
        const map<KeyFrame*, size_t> seen_by = p->GetObservations();
        for (const auto& o : seen_by) votes[o.first] += 1;
    }
    if (!votes.empty()) {                                            // otherwise the list and the reference key frame stay
        set<KeyFrame*> listed;
        vector<KeyFrame*> list;
        auto append_if_new = [&](KeyFrame* k) { if (k && listed.insert(k).second) { list.push_back(k); return true; } return false; };
        KeyFrame* winner = nullptr; int most = 0;
        for (const auto& v : votes) {                                // address order; bad key frames are passed over, a later one needs MORE votes to win
            if (v.first->isBad()) continue;
            if (v.second > most) { most = v.second; winner = v.first; }
            append_if_new(v.first);
        }
        const size_t n_voted = list.size();                          // only these are visited
        for (size_t j = 0; j < n_voted && list.size() <= 80; j++) {
            KeyFrame* k = list[j];
            const vector<KeyFrame*> best10 = k->GetBestCovisibilityKeyFrames(10);
            for (size_t q = 0; q < best10.size(); q++) if (!best10[q]->isBad() && append_if_new(best10[q])) break;     // one neighbour
            const set<KeyFrame*> children = k->GetChilds();
            for (KeyFrame* c : children) if (!c->isBad() && append_if_new(c)) break;                                   // one child
            append_if_new(k->GetParent()); append_if_new(k->GetPrevKeyFrame()); append_if_new(k->GetNextKeyFrame());   // bad or not
        }
        s.local_kfs = list;
        if (winner) { s.ref_kf = winner; s.frame.mpReferenceKF = winner; }
    }
    // points: every good point of the listed key frames, once, where it first appears
    set<MapPoint*> taken;
    s.local_pts.clear();
    for (KeyFrame* k : s.local_kfs)
        for (MapPoint* p : k->GetMapPointMatches())
            if (p && !p->isBad() && taken.insert(p).second) s.local_pts.push_back(p);
}

static int run_one(const char* problem, const char* result) {
    g_pos = 0;
    FILE* f = std::fopen(problem, "rb");
    if (!f) { std::printf("cannot open %s\n", problem); return 2; }
    std::fseek(f, 0, SEEK_END); const long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    g_blob.resize((size_t)sz);
    if (std::fread(g_blob.data(), 1, (size_t)sz, f) != (size_t)sz) { std::printf("short read\n"); return 2; }
    std::fclose(f);
    // nk n_child n_kp np n_obs n_frame n_prev prev_ref
    const int32_t* h = take(8);
    const int nk = h[0], nch = h[1], nkp = h[2], np = h[3], no = h[4], nf = h[5], npv = h[6], prev_ref = h[7];
    const int32_t *kf_bad = take(nk), *parent = take(nk), *prev = take(nk), *next = take(nk), *covis = take((size_t)nk * 10), *child_start = take(nk + 1), *child_kf = take(nch);
    const int32_t *by_key = take(nk), *kp_start = take(nk + 1), *kp_point = take(nkp), *pt_bad = take(np), *obs_start = take(np + 1), *obs = take(no);
    const int32_t *frame_point = take(nf), *prev_lkf = take(npv);

    std::vector<KeyFrame> store(nk); std::vector<MapPoint> pts(np); std::vector<KeyFrame*> kfs(nk);
    for (int j = 0; j < nk; j++) kfs[by_key[j]] = &store[j];             // ascending addresses in key order
    for (int p = 0; p < np; p++) {
        pts[p].id = p; pts[p].mbBad = pt_bad[p] != 0;
        for (int o = obs_start[p]; o < obs_start[p + 1]; o++) pts[p].mObservations[kfs[obs[o] & 0xffff]] = 0;
    }
    for (int k = 0; k < nk; k++) {
        KeyFrame& K = *kfs[k];
        K.id = k; K.mbBad = kf_bad[k] != 0;
        K.mpParent = parent[k] >= 0 ? kfs[parent[k]] : nullptr; K.mpPrevKeyFrame = prev[k] >= 0 ? kfs[prev[k]] : nullptr; K.mpNextKeyFrame = next[k] >= 0 ? kfs[next[k]] : nullptr;
        for (int i = 0; i < 10; i++) if (covis[k * 10 + i] >= 0) K.mvpOrderedConnectedKeyFrames.push_back(kfs[covis[k * 10 + i]]);
        for (int c = child_start[k]; c < child_start[k + 1]; c++) K.mspChildrens.insert(kfs[child_kf[c]]);
        for (int i = kp_start[k]; i < kp_start[k + 1]; i++) K.mvpMapPoints.push_back(kp_point[i] >= 0 ? &pts[kp_point[i]] : nullptr);
    }
    State start;
    start.frame.N = nf; start.frame.mnId = 1234;
    for (int i = 0; i < nf; i++) start.frame.mvpMapPoints.push_back(frame_point[i] >= 0 ? &pts[frame_point[i]] : nullptr);
    for (int j = 0; j < npv; j++) start.local_kfs.push_back(kfs[prev_lkf[j]]);
    start.ref_kf = prev_ref >= 0 ? kfs[prev_ref] : nullptr;

    State lib = start, want = start;
    int status = 0;
    try {
        status = viorb_shim::update_local_map<KeyFrame, MapPoint>(lib.frame, lib.local_kfs, lib.ref_kf, lib.local_pts);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    expected_local_map(want);
    if (lib.local_kfs != want.local_kfs) { std::printf("mvpLocalKeyFrames differs from the restatement\n"); return 4; }
    if (lib.ref_kf != want.ref_kf || lib.frame.mpReferenceKF != want.frame.mpReferenceKF) { std::printf("mpReferenceKF differs from the restatement\n"); return 4; }
    if (lib.local_pts != want.local_pts) { std::printf("mvpLocalMapPoints differs from the restatement\n"); return 4; }
    if (lib.frame.mvpMapPoints != want.frame.mvpMapPoints) { std::printf("mCurrentFrame.mvpMapPoints differs from the restatement\n"); return 4; }

    std::vector<int32_t> out;
    out.push_back(status); out.push_back((int32_t)lib.local_kfs.size()); out.push_back((int32_t)lib.local_pts.size());
    out.push_back(lib.ref_kf ? lib.ref_kf->id : -1); out.push_back(lib.frame.mpReferenceKF ? lib.frame.mpReferenceKF->id : -1);
    for (size_t j = 0; j < lib.local_kfs.size(); j++) out.push_back(lib.local_kfs[j]->id);
    for (size_t j = 0; j < lib.local_pts.size(); j++) out.push_back(lib.local_pts[j]->id);
    for (int i = 0; i < nf; i++) out.push_back(lib.frame.mvpMapPoints[i] ? lib.frame.mvpMapPoints[i]->id : -1);
    FILE* o = std::fopen(result, "wb");
    if (!o) return 2;
    std::fwrite(out.data(), 4, out.size(), o);
    std::fclose(o);
    std::printf("%zu local key frames, %zu local points, status %d\n", lib.local_kfs.size(), lib.local_pts.size(), status);
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
