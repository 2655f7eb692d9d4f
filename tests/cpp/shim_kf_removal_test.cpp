// tests/cpp/shim_kf_removal_test.cpp — drives viorb_shim::set_bad_flag, set_erase and remove_key_frames (viorb_amd/shim/KeyFrame_shim.h) with
// the stand-in objects of kf_removal_standin.h, from a problem file that tests/test_gpu_kf_removal_shim.py writes (one scene of
// viorb_amd/kf_removal.py and a mode; the key frame of slot kf_by_key[j] is stored at position j, so pointer order is the scene's key
// order). Mode 0: set_bad_flag / set_erase on every operation's key frame, one call of the library each, in order. Mode 1:
// remove_key_frames on all of them in one call. It then works out the expected state over a second description of the same map
// (expected_removal, a restatement in this project's own words), requires the members the shim left in the objects to be equal, and writes
// them out in the scene's numbering.
// usage: shim_kf_removal_test problem.bin out.bin [problem.bin out.bin ...]   (one process for all: the device is opened once)
//        exit 0 ok, 2 usage / io, 3 the shim threw (printed as "exception: ..."), 4 the members differ; it stops at the first problem that fails
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "kf_removal_standin.h"
#include "KeyFrame_shim.h"

typedef standin::RmKeyFrame KeyFrame;
typedef standin::RmMapPoint MapPoint;
using std::map; using std::set; using std::vector;

static std::vector<unsigned char> g_blob;
static size_t g_pos = 0;
static const int32_t* take(size_t n) {
    const int32_t* p = reinterpret_cast<const int32_t*>(g_blob.data() + g_pos);
    g_pos += n * 4;
    if (g_pos > g_blob.size()) { std::printf("problem file too short\n"); std::exit(2); }
    return p;
}

// The map, described outside the objects, for the restatement
struct Node {
    map<KeyFrame*, int> weight; vector<KeyFrame*> best; vector<int> best_w; KeyFrame* parent = nullptr; KeyFrame* prev = nullptr; KeyFrame* next = nullptr;
    bool first = false, gone = false, keep = false, pending = false, loop = false; float pose[12]; bool has_rel = false; float rel[12]; vector<MapPoint*> table;
};
struct Spot { map<KeyFrame*, size_t> seen_by; map<KeyFrame*, bool> stereo; int count = 0; KeyFrame* ref = nullptr; bool gone = false; };
struct World {
    map<KeyFrame*, Node> kf; map<MapPoint*, Spot> pt;
    vector<KeyFrame*> left_map, left_db; vector<MapPoint*> pts_left_map; vector<std::pair<KeyFrame*, KeyFrame*> > imu;
};

static void sort_best(Node& n) {                                     // heaviest first; among equal weights the higher address first
    vector<std::pair<KeyFrame*, int> > e(n.weight.begin(), n.weight.end());
    std::sort(e.begin(), e.end(), [](const std::pair<KeyFrame*, int>& a, const std::pair<KeyFrame*, int>& b) { return a.second != b.second ? a.second > b.second : std::less<KeyFrame*>()(b.first, a.first); });
    n.best.clear(); n.best_w.clear();
    for (const auto& x : e) { n.best.push_back(x.first); n.best_w.push_back(x.second); }
}

// What one operation leaves, restated in this project's own words (the rules are those of DESIGN.md "Key-frame removal" and of
// tests/kf_removal_ref.py; nothing here comes from the library or the shim). Returns whether the key frame left the map.
static bool expected_removal(World& W, KeyFrame* x, int kind) {
    Node& me = W.kf[x];
    if (kind == 1) {                                                 // a release: only a pending removal goes on
        if (!me.loop) me.keep = false;
        if (!me.pending) return false;
    }
    if (me.gone) { W.left_map.push_back(x); W.left_db.push_back(x); return false; }
    if (me.first) return false;
    if (me.keep) { me.pending = true; return false; }
    for (const auto& w : me.weight) {                                // whoever I list and who lists me back forgets me and re-sorts its whole map
        Node& other = W.kf[w.first];
        if (other.weight.erase(x)) sort_best(other);
    }
    for (size_t i = 0; i < me.table.size(); i++) {                   // my points lose me
        MapPoint* p = me.table[i];
        if (!p) continue;
        Spot& s = W.pt[p];
        if (!s.seen_by.count(x)) continue;
        s.count -= s.stereo[x] ? 2 : 1;
        s.seen_by.erase(x);
        if (s.ref == x) s.ref = s.seen_by.empty() ? nullptr : s.seen_by.begin()->first;
        if (s.count <= 2) {                                          // too few left: the point goes, and its remaining observers drop it from their tables
            s.gone = true;
            for (const auto& o : s.seen_by) W.kf[o.first].table[o.second] = nullptr;
            s.seen_by.clear();
            W.pts_left_map.push_back(p);
        }
    }
    me.weight.clear(); me.best.clear(); me.best_w.clear();
    set<KeyFrame*> orphans, hosts;                                   // my children look for a new parent among my parent and those of them already placed
    for (auto& k : W.kf) if (k.second.parent == x && !k.second.gone) orphans.insert(k.first);
    hosts.insert(me.parent);
    while (!orphans.empty()) {
        int top = -1; KeyFrame* who = nullptr; KeyFrame* to = nullptr;
        for (KeyFrame* c : orphans) {
            Node& n = W.kf[c];
            for (KeyFrame* b : n.best) {
                if (!hosts.count(b)) continue;
                const auto it = n.weight.find(b);
                const int w = it == n.weight.end() ? 0 : it->second;
                if (w > top) { top = w; who = c; to = b; }
            }
        }
        if (!who) break;
        W.kf[who].parent = to; hosts.insert(who); orphans.erase(who);
    }
    for (KeyFrame* c : orphans) W.kf[c].parent = me.parent;
    const float* T = me.pose; const float* P = W.kf[me.parent].pose;      // my pose relative to my parent: Tcw * [Rpw^T | -Rpw^T tpw], float, left to right
    float O[3];
    for (int r = 0; r < 3; r++) O[r] = ((-P[r]) * P[9] + (-P[3 + r]) * P[10]) + (-P[6 + r]) * P[11];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) me.rel[3 * r + c] = ((T[3 * r] * P[c * 3] + T[3 * r + 1] * P[c * 3 + 1]) + T[3 * r + 2] * P[c * 3 + 2]) + T[9 + r] * 0.0f;
        me.rel[9 + r] = ((T[3 * r] * O[0] + T[3 * r + 1] * O[1]) + T[3 * r + 2] * O[2]) + T[9 + r] * 1.0f;
    }
    me.has_rel = true; me.gone = true;
    if (me.prev) W.kf[me.prev].next = me.next;
    if (me.next) W.kf[me.next].prev = me.prev;
    if (me.prev && me.next) W.imu.push_back(std::make_pair(me.next, x));
    me.prev = me.next = nullptr;
    W.left_map.push_back(x); W.left_db.push_back(x);
    return true;
}

static int run_one(const char* problem, const char* result) {
    g_pos = 0;
    FILE* f = std::fopen(problem, "rb");
    if (!f) { std::printf("cannot open %s\n", problem); return 2; }
    std::fseek(f, 0, SEEK_END); const long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    g_blob.resize((size_t)sz);
    if (std::fread(g_blob.data(), 1, (size_t)sz, f) != (size_t)sz) { std::printf("short read\n"); return 2; }
    std::fclose(f);
    // mode nk n_kp np n_obs n_conn n_ord n_op
    const int32_t* h = take(8);
    const int mode = h[0], nk = h[1], nkp = h[2], np = h[3], no = h[4], nc = h[5], nr = h[6], nop = h[7];
    const int32_t *by_key = take(nk), *flags = take(nk), *parent = take(nk), *prev = take(nk), *next = take(nk);
    const float* pose = reinterpret_cast<const float*>(take((size_t)nk * 12));
    const int32_t *kp_start = take(nk + 1), *kp_point = take(nkp), *pt_bad = take(np), *pt_nobs = take(np), *pt_ref = take(np), *obs_start = take(np + 1), *obs = take(no);
    const int32_t *conn_start = take(nk + 1), *conn_kf = take(nc), *conn_w = take(nc), *ord_start = take(nk + 1), *ord_kf = take(nr), *ord_w = take(nr), *op_kf = take(nop), *op_kind = take(nop);

    std::vector<KeyFrame> store(nk); std::vector<MapPoint> pts(np); std::vector<KeyFrame*> kfs(nk);      // never resized: the objects hold a mutex and stay in place
    standin::RmMap the_map; standin::RmKeyFrameDatabase the_db;
    std::vector<std::pair<KeyFrame*, KeyFrame*> > imu_log;
    for (int j = 0; j < nk; j++) kfs[by_key[j]] = &store[j];             // ascending addresses in key order
    World W;
    for (int k = 0; k < nk; k++) {
        KeyFrame& K = *kfs[k];
        K.id = k; K.mnId = (flags[k] & 1) ? 0 : (long unsigned int)k + 1; K.imu_log = &imu_log;
        Node& n = W.kf[&K];
        for (int i = kp_start[k]; i < kp_start[k + 1]; i++) n.table.push_back(kp_point[i] >= 0 ? &pts[kp_point[i]] : nullptr);
        K.mvuRight.assign(n.table.size(), -1.f);
        for (int i = conn_start[k]; i < conn_start[k + 1]; i++) n.weight[kfs[conn_kf[i]]] = conn_w[i];
        for (int i = ord_start[k]; i < ord_start[k + 1]; i++) { n.best.push_back(kfs[ord_kf[i]]); n.best_w.push_back(ord_w[i]); }
        n.parent = parent[k] >= 0 ? kfs[parent[k]] : nullptr; n.prev = prev[k] >= 0 ? kfs[prev[k]] : nullptr; n.next = next[k] >= 0 ? kfs[next[k]] : nullptr;
        n.first = (flags[k] & 1) != 0; n.gone = (flags[k] & 2) != 0; n.keep = (flags[k] & 4) != 0; n.pending = (flags[k] & 8) != 0; n.loop = (flags[k] & 16) != 0;
        std::memcpy(n.pose, pose + 12 * k, sizeof(n.pose));
    }
    for (int p = 0; p < np; p++) {
        pts[p].id = p;
        Spot& s = W.pt[&pts[p]];
        s.count = pt_nobs[p]; s.gone = pt_bad[p] != 0; s.ref = pt_ref[p] >= 0 ? kfs[pt_ref[p]] : nullptr;
        for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
            KeyFrame* K = kfs[obs[o] & 0xffff];
            const vector<MapPoint*>& t = W.kf[K].table;
            const size_t idx = (size_t)(std::find(t.begin(), t.end(), &pts[p]) - t.begin());
            if (idx == t.size()) { std::printf("the scene lists an observer whose table does not hold the point\n"); return 2; }
            s.seen_by[K] = idx; s.stereo[K] = (obs[o] >> 24) & 1;
            if (s.stereo[K]) K->mvuRight[idx] = 1.f;
        }
        pts[p].set_up(s.seen_by, s.count, s.ref, s.gone, &the_map);
    }
    for (int k = 0; k < nk; k++) {
        const Node& n = W.kf[kfs[k]];
        set<KeyFrame*> children;
        if (!n.gone) for (int c = 0; c < nk; c++) if (parent[c] == k && !(flags[c] & 2)) children.insert(kfs[c]);
        kfs[k]->set_up(n.table, n.weight, n.best, n.best_w, n.parent, children, n.gone, n.keep, n.pending, n.loop, n.pose, &the_map, &the_db);
        kfs[k]->SetPrevKeyFrame(n.prev); kfs[k]->SetNextKeyFrame(n.next);
    }
    vector<KeyFrame*> list; vector<int> kinds;
    for (int j = 0; j < nop; j++) { list.push_back(kfs[op_kf[j]]); kinds.push_back(op_kind[j]); }
    try {
        if (mode == 0) for (int j = 0; j < nop; j++) { if (kinds[j]) viorb_shim::set_erase<MapPoint>(list[j]); else viorb_shim::set_bad_flag<MapPoint>(list[j]); }
        else viorb_shim::remove_key_frames<KeyFrame, MapPoint>(list, kinds);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    int removed = 0;
    for (int j = 0; j < nop; j++) removed += expected_removal(W, list[j], kinds[j]) ? 1 : 0;

    for (int k = 0; k < nk; k++) {
        const KeyFrame& K = *kfs[k]; const Node& n = W.kf[kfs[k]];
        if (K.weights() != n.weight) { std::printf("mConnectedKeyFrameWeights of key frame %d differs from the restatement\n", k); return 4; }
        if (K.ordered() != n.best || K.ordered_weights() != n.best_w) { std::printf("the ordered list of key frame %d differs from the restatement\n", k); return 4; }
        if (K.GetParent() != n.parent) { std::printf("mpParent of key frame %d differs from the restatement\n", k); return 4; }
        if (K.isBad() != n.gone || K.not_erase() != n.keep || K.to_be_erased() != n.pending) { std::printf("the flags of key frame %d differ from the restatement\n", k); return 4; }
        if (K.GetPrevKeyFrame() != n.prev || K.GetNextKeyFrame() != n.next) { std::printf("the links of key frame %d differ from the restatement\n", k); return 4; }
        if (K.GetMapPointMatches() != n.table) { std::printf("mvpMapPoints of key frame %d differs from the restatement\n", k); return 4; }
        if (!n.gone) {
            set<KeyFrame*> children;
            for (const auto& c : W.kf) if (c.second.parent == kfs[k] && !c.second.gone) children.insert(c.first);
            if (K.children() != children) { std::printf("mspChildrens of key frame %d differs from the restatement\n", k); return 4; }
        }
        if (n.has_rel) for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) {
            const float want = c < 3 ? n.rel[3 * r + c] : n.rel[9 + r], got = K.Tcp().at<float>(r, c);
            if (std::memcmp(&want, &got, 4) != 0) { std::printf("mTcp of key frame %d differs from the restatement\n", k); return 4; }
        }
    }
    for (int p = 0; p < np; p++) {
        const Spot& s = W.pt[&pts[p]];
        if (pts[p].GetObservations() != s.seen_by || pts[p].Observations() != s.count || pts[p].isBad() != s.gone || pts[p].GetReferenceKeyFrame() != s.ref) {
            std::printf("map point %d differs from the restatement\n", p); return 4;
        }
    }
    vector<MapPoint*> a = the_map.erased_pts, b = W.pts_left_map;
    std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
    if (the_map.erased_kfs != W.left_map || the_db.erased != W.left_db || a != b || imu_log != W.imu) { std::printf("the map, the database or the IMU appends differ from the restatement\n"); return 4; }

    std::vector<int32_t> out;
    for (int k = 0; k < nk; k++) {
        const KeyFrame& K = *kfs[k];
        out.push_back((int32_t)K.weights().size());
        for (const auto& w : K.weights()) { out.push_back(w.first->id); out.push_back(w.second); }
        out.push_back((int32_t)K.ordered().size());
        for (size_t i = 0; i < K.ordered().size(); i++) { out.push_back(K.ordered()[i]->id); out.push_back(K.ordered_weights()[i]); }
        out.push_back(K.GetParent() ? K.GetParent()->id : -1);
        out.push_back((K.mnId == 0 ? 1 : 0) | (K.isBad() ? 2 : 0) | (K.not_erase() ? 4 : 0) | (K.to_be_erased() ? 8 : 0) | (K.loop_edges() ? 16 : 0));
        out.push_back(K.GetPrevKeyFrame() ? K.GetPrevKeyFrame()->id : -1); out.push_back(K.GetNextKeyFrame() ? K.GetNextKeyFrame()->id : -1);
        out.push_back(K.isBad() ? -1 : (int32_t)K.children().size());
        if (!K.isBad()) for (KeyFrame* c : K.children()) out.push_back(c->id);
        const bool has = W.kf[kfs[k]].has_rel;
        out.push_back(has ? 1 : 0);
        if (has) for (int i = 0; i < 12; i++) { const float v = i < 9 ? K.Tcp().at<float>(i / 3, i % 3) : K.Tcp().at<float>(i - 9, 3); int32_t bits; std::memcpy(&bits, &v, 4); out.push_back(bits); }
        const vector<MapPoint*> t = K.GetMapPointMatches();
        out.push_back((int32_t)t.size());
        for (MapPoint* p : t) out.push_back(p ? p->id : -1);
    }
    for (int p = 0; p < np; p++) {
        out.push_back(pts[p].Observations()); out.push_back(pts[p].isBad() ? 1 : 0); out.push_back(pts[p].GetReferenceKeyFrame() ? pts[p].GetReferenceKeyFrame()->id : -1);
        const map<KeyFrame*, size_t> o = pts[p].GetObservations();
        out.push_back((int32_t)o.size());
        for (const auto& x : o) out.push_back(x.first->id);
    }
    out.push_back((int32_t)the_map.erased_kfs.size()); for (KeyFrame* k : the_map.erased_kfs) out.push_back(k->id);
    out.push_back((int32_t)the_db.erased.size()); for (KeyFrame* k : the_db.erased) out.push_back(k->id);
    out.push_back((int32_t)a.size()); for (MapPoint* p : a) out.push_back(p->id);
    out.push_back((int32_t)imu_log.size()); for (const auto& x : imu_log) { out.push_back(x.first->id); out.push_back(x.second->id); }
    FILE* o = std::fopen(result, "wb");
    if (!o) return 2;
    std::fwrite(out.data(), 4, out.size(), o);
    std::fclose(o);
    std::printf("mode %d: %d key frames, %d operations, %d removed\n", mode, nk, nop, removed);
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
