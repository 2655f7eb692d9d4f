// tests/cpp/shim_covis_test.cpp — drives viorb_shim::update_connections and viorb_shim::update_connections_loop
// (viorb_amd/shim/KeyFrame_shim.h) with the stand-in KeyFrame / MapPoint of covis_standin.h, from a problem file that
// tests/test_gpu_covis_shim.py writes (one scene of viorb_amd/covisibility.py and a mode; the key frame of slot kf_by_key[j] is stored at
// position j, so pointer order is the scene's key order). Mode 0: update_connections on every target, one call each, in order. Mode 1:
// update_connections_loop on the targets as the group, with the LoopConnections map. It then works out the expected members over a
// second set of the same objects (expected_connections, a restatement in this project's own words), requires the written-back members to
// be equal, and writes them out in the scene's numbering.
// usage: shim_covis_test problem.bin out.bin [problem.bin out.bin ...]   (one process for all: the device is opened once)
//        exit 0 ok, 2 usage / io, 3 the shim threw (printed as "exception: ..."), 4 the members differ; it stops at the first problem that fails
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "covis_standin.h"
#include "KeyFrame_shim.h"

typedef standin::CvKeyFrame KeyFrame;
typedef standin::CvMapPoint MapPoint;
using std::map; using std::set; using std::vector;

static std::vector<unsigned char> g_blob;
static size_t g_pos = 0;
static const int32_t* take(size_t n) {
    const int32_t* p = reinterpret_cast<const int32_t*>(g_blob.data() + g_pos);
    g_pos += n * 4;
    if (g_pos > g_blob.size()) { std::printf("problem file too short\n"); std::exit(2); }
    return p;
}

// The graph members of every key frame, held outside the objects for the restatement
struct Node { map<KeyFrame*, int> weight; vector<KeyFrame*> best; vector<int> best_w; bool first; KeyFrame* parent; set<KeyFrame*> children; };
typedef map<KeyFrame*, Node> Graph;

// heaviest first; among equal weights the higher address first
static void sort_best(Node& n, const vector<std::pair<KeyFrame*, int> >& entries) {
    vector<std::pair<KeyFrame*, int> > e = entries;
    std::sort(e.begin(), e.end(), [](const std::pair<KeyFrame*, int>& a, const std::pair<KeyFrame*, int>& b) { return a.second != b.second ? a.second > b.second : std::less<KeyFrame*>()(b.first, a.first); });
    n.best.clear(); n.best_w.clear();
    for (const auto& x : e) { n.best.push_back(x.first); n.best_w.push_back(x.second); }
}

// The expected result of one key frame's update, restated over the stand-in objects in this project's own words (the rules are those of
// DESIGN.md "Covisibility graph" and of tests/covis_ref.py; nothing here comes from the library or the shim).
static void expected_connections(Graph& G, KeyFrame* target) {
    map<KeyFrame*, int> shared;                                      // how many of the target's keypoints each other key frame also sees, by address
    for (MapPoint* p : target->GetMapPointMatches()) {
        if (!p || p->isBad()) continue;
        for (const auto& o : p->GetObservations()) if (o.first->mnId != target->mnId) shared[o.first] += 1;
    }
    if (shared.empty()) return;                                      // nothing at all changes
    KeyFrame* strongest = nullptr; int most = 0;
    vector<std::pair<KeyFrame*, int> > linked;
    for (const auto& s : shared) {                                   // address order; a later one needs MORE to be the strongest
        if (s.second > most) { most = s.second; strongest = s.first; }
        if (s.second >= 15) linked.push_back(s);
    }
    if (linked.empty()) linked.push_back(std::make_pair(strongest, most));
    for (const auto& l : linked) {                                   // the other side learns the weight; its list is rebuilt from its WHOLE map, unless nothing changed
        Node& other = G[l.first];
        auto it = other.weight.find(target);
        if (it != other.weight.end() && it->second == l.second) continue;
        other.weight[target] = l.second;
        sort_best(other, vector<std::pair<KeyFrame*, int> >(other.weight.begin(), other.weight.end()));
    }
    Node& me = G[target];
    me.weight = shared;                                              // everything seen together, below the threshold too; old entries go
    sort_best(me, linked);                                           // but the list holds the linked ones only
    if (me.first && target->mnId != 0) { me.parent = me.best.front(); G[me.parent].children.insert(target); me.first = false; }
}

static int run_one(const char* problem, const char* result) {
    g_pos = 0;
    FILE* f = std::fopen(problem, "rb");
    if (!f) { std::printf("cannot open %s\n", problem); return 2; }
    std::fseek(f, 0, SEEK_END); const long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    g_blob.resize((size_t)sz);
    if (std::fread(g_blob.data(), 1, (size_t)sz, f) != (size_t)sz) { std::printf("short read\n"); return 2; }
    std::fclose(f);
    // mode nk n_kp np n_obs n_conn n_ord n_target
    const int32_t* h = take(8);
    const int mode = h[0], nk = h[1], nkp = h[2], np = h[3], no = h[4], nc = h[5], nr = h[6], nt = h[7];
    const int32_t *by_key = take(nk), *flags = take(nk), *parent = take(nk), *kp_start = take(nk + 1), *kp_point = take(nkp), *pt_bad = take(np), *obs_start = take(np + 1), *obs = take(no);
    const int32_t *conn_start = take(nk + 1), *conn_kf = take(nc), *conn_w = take(nc), *ord_start = take(nk + 1), *ord_kf = take(nr), *ord_w = take(nr), *targets = take(nt);

    std::vector<KeyFrame> store(nk); std::vector<MapPoint> pts(np); std::vector<KeyFrame*> kfs(nk);      // never resized: the key frames hold a mutex and stay in place
    for (int j = 0; j < nk; j++) kfs[by_key[j]] = &store[j];             // ascending addresses in key order
    for (int p = 0; p < np; p++) {
        pts[p].id = p; pts[p].mbBad = pt_bad[p] != 0;
        for (int o = obs_start[p]; o < obs_start[p + 1]; o++) pts[p].mObservations[kfs[obs[o] & 0xffff]] = 0;
    }
    Graph G;
    for (int k = 0; k < nk; k++) {
        KeyFrame& K = *kfs[k];
        K.id = k; K.mnId = (flags[k] & 1) ? 0 : (long unsigned int)k + 1;
        for (int i = kp_start[k]; i < kp_start[k + 1]; i++) K.mvpMapPoints.push_back(kp_point[i] >= 0 ? &pts[kp_point[i]] : nullptr);
        Node& n = G[&K];
        for (int i = conn_start[k]; i < conn_start[k + 1]; i++) n.weight[kfs[conn_kf[i]]] = conn_w[i];
        for (int i = ord_start[k]; i < ord_start[k + 1]; i++) { n.best.push_back(kfs[ord_kf[i]]); n.best_w.push_back(ord_w[i]); }
        n.first = (flags[k] & 2) != 0; n.parent = parent[k] >= 0 ? kfs[parent[k]] : nullptr;
        K.set_graph(n.weight, n.best, n.best_w, n.first, n.parent);
    }
    vector<KeyFrame*> group;
    for (int t = 0; t < nt; t++) group.push_back(kfs[targets[t]]);

    map<KeyFrame*, set<KeyFrame*> > loop_lib, loop_want;
    try {
        if (mode == 0) for (KeyFrame* k : group) viorb_shim::update_connections<MapPoint>(k);
        else viorb_shim::update_connections_loop<MapPoint>(group, loop_lib);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    for (KeyFrame* k : group) {                                      // the new links of every member of the group: not a neighbour before, not in the group
        const vector<KeyFrame*> before = G[k].best;
        expected_connections(G, k);
        set<KeyFrame*> fresh;
        for (const auto& w : G[k].weight) fresh.insert(w.first);
        for (KeyFrame* b : before) fresh.erase(b);
        for (KeyFrame* g : group) fresh.erase(g);
        loop_want[k] = fresh;
    }
    for (int k = 0; k < nk; k++) {
        const KeyFrame& K = *kfs[k]; const Node& n = G[kfs[k]];
        if (K.weights() != n.weight) { std::printf("mConnectedKeyFrameWeights of key frame %d differs from the restatement\n", k); return 4; }
        if (K.ordered() != n.best || K.ordered_weights() != n.best_w) { std::printf("the ordered list of key frame %d differs from the restatement\n", k); return 4; }
        if (K.parent() != n.parent || K.first_connection() != n.first) { std::printf("mpParent / mbFirstConnection of key frame %d differs from the restatement\n", k); return 4; }
        if (K.children() != n.children) { std::printf("mspChildrens of key frame %d differs from the restatement\n", k); return 4; }
    }
    if (mode == 1 && loop_lib != loop_want) { std::printf("LoopConnections differs from the restatement\n"); return 4; }

    std::vector<int32_t> out;
    for (int k = 0; k < nk; k++) {
        const KeyFrame& K = *kfs[k];
        out.push_back((int32_t)K.weights().size());
        for (const auto& w : K.weights()) { out.push_back(w.first->id); out.push_back(w.second); }
        out.push_back((int32_t)K.ordered().size());
        for (size_t i = 0; i < K.ordered().size(); i++) { out.push_back(K.ordered()[i]->id); out.push_back(K.ordered_weights()[i]); }
        out.push_back(K.parent() ? K.parent()->id : -1); out.push_back(K.first_connection() ? 1 : 0);
        out.push_back((int32_t)K.children().size());
        for (KeyFrame* c : K.children()) out.push_back(c->id);
    }
    out.push_back((int32_t)loop_lib.size());
    for (const auto& l : loop_lib) { out.push_back(l.first->id); out.push_back((int32_t)l.second.size()); for (KeyFrame* c : l.second) out.push_back(c->id); }
    FILE* o = std::fopen(result, "wb");
    if (!o) return 2;
    std::fwrite(out.data(), 4, out.size(), o);
    std::fclose(o);
    std::printf("mode %d: %d key frames, %d targets, %zu loop sets\n", mode, nk, nt, loop_lib.size());
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
