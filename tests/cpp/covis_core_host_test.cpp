// tests/cpp/covis_core_host_test.cpp — the host build of viorb_amd/csrc/covis_core.h as a stand-alone program. No GPU, no library: only
// the header.
//   covis_core_host_test                    the self-test that tests/test_covis_host_sanitized.py compiles with -fsanitize=address,undefined
//                                           and runs as a child process: cov_run_host (validate, counters, AddConnection, the target's own
//                                           members, the first connection, LoopConnections) against the literal loop below on a few thousand
//                                           random small streams, every kind of broken snapshot, which the validator must refuse without
//                                           reading through it, and the overflow by one. The program counts the situations the random set
//                                           must hold (the fallback to pKFmax, a tie for nmax, an equal-weight pair in a sorted list, an
//                                           AddConnection early return, a rebuild that brings a sub-threshold entry into a list, a
//                                           first-connection parent, a stale entry, a non-empty and an empty LoopConnections set) and prints
//                                           them on one checksum line.
//   covis_core_host_test time FILE [reps]   the literal loop (one thread) timed on a packed snapshot that tools/covis_time.py writes: 8
//                                           totals, ccap and erase_targets as int32, then the arrays of viorb_covis_map in their order (the
//                                           two byte arrays as bytes).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <vector>
#include "covis_core.h"

using namespace viorb;

static long long sum = 0;
static unsigned rng_state = 97531u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rint_(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }
static void fail(const char* what) { std::printf("FAILED: %s\n", what); std::exit(2); }

// a packed batch with exactly sized arrays, so that the address sanitizer sees any read past an end
struct Packed {
    int batch = 0, ccap = 1, erase = 0;
    std::vector<int32_t> kf_start, kf_by_key, kf_parent, kp_start, kp_point, pt_start, obs_start, conn_start, conn_kf, conn_w, ord_start, ord_kf, ord_w, target_start, target_kf;
    std::vector<uint8_t> kf_flags, pt_bad;
    std::vector<uint32_t> obs;
    CovMap map() const {
        CovMap M;
        M.batch = batch; M.n_kf = (int)kf_flags.size(); M.n_kp = (int)kp_point.size(); M.n_pt = (int)pt_bad.size(); M.n_obs = (int)obs.size();
        M.n_conn = (int)conn_kf.size(); M.n_ord = (int)ord_kf.size(); M.n_target = (int)target_kf.size();
        M.kf_start = kf_start.data(); M.kf_by_key = kf_by_key.data(); M.kf_flags = kf_flags.data(); M.kf_parent = kf_parent.data(); M.kp_start = kp_start.data();
        M.kp_point = kp_point.data(); M.pt_start = pt_start.data(); M.pt_bad = pt_bad.data(); M.obs_start = obs_start.data(); M.obs = obs.data();
        M.conn_start = conn_start.data(); M.conn_kf = conn_kf.data(); M.conn_w = conn_w.data(); M.ord_start = ord_start.data(); M.ord_kf = ord_kf.data(); M.ord_w = ord_w.data();
        M.target_start = target_start.data(); M.target_kf = target_kf.data();
        M.ccap = ccap; M.erase_targets = erase;
        return M;
    }
};

struct Result {
    std::vector<int32_t> ck, cw, cn, ok, ow, on, status, need, parent, t_obs, t_mk, t_mw, t_add, t_par, loop, n_loop;
    std::vector<uint8_t> flags, touched;
    void size(const CovMap& M) {
        ck.assign((size_t)M.n_kf * M.ccap, 77); cw = ok = ow = ck; cn.assign(M.n_kf, 77); on = parent = cn; flags.assign(M.n_kf, 77); touched = flags;
        status.assign(M.batch, 77); need = status; t_obs.assign(M.n_target, 77); t_mk = t_mw = t_add = t_par = n_loop = t_obs; loop.assign((size_t)M.n_target * M.ccap, 77);
    }
    CovOut out() {
        CovOut R;
        R.conn_kf_out = ck.data(); R.conn_w_out = cw.data(); R.conn_n_out = cn.data(); R.ord_kf_out = ok.data(); R.ord_w_out = ow.data(); R.ord_n_out = on.data();
        R.status = status.data(); R.need = need.data(); R.kf_parent_out = parent.data(); R.kf_flags_out = flags.data(); R.kf_touched = touched.data();
        R.t_observers = t_obs.data(); R.t_max_kf = t_mk.data(); R.t_max_w = t_mw.data(); R.t_added = t_add.data(); R.t_parent = t_par.data();
        R.loop_conn = loop.data(); R.n_loop_conn = n_loop.data();
        return R;
    }
};

struct Workspace {
    std::vector<int32_t> rank, flags, mark, votes, ckf, cw, cinfo, info;
    CovWork work(const CovMap& M) {
        rank.assign(M.n_kf, -5); flags = mark = votes = rank; ckf.assign((size_t)M.n_target * M.ccap, -5); cw = ckf; cinfo.assign((size_t)M.n_target * COV_C, -5); info.assign(M.batch, -5);
        CovWork W;
        W.rank = rank.data(); W.flags = flags.data(); W.mark = mark.data(); W.votes = votes.data(); W.ckf = ckf.data(); W.cw = cw.data(); W.cinfo = cinfo.data(); W.info = info.data();
        return W;
    }
};

// ---- the literal loop: objects, std::map in key order, sort and push_front, in-place mutation (KeyFrame.cc:414-448, 580-676) --------------
// A key frame's address is its position in kf_by_key: std::map<int, ...> keyed by it iterates as std::map<KeyFrame*, ...> does, and
// pair<int, int> (weight, key) sorts as pair<int, KeyFrame*> does.
struct Seen { long long fallback = 0, tie = 0, equal_weights = 0, early_return = 0, pulls = 0, first_parent = 0, stale = 0, loop_nonempty = 0, loop_empty = 0; };
static Seen g_seen;
static double g_loop_ms = 0;
struct Overflow { int need; };

struct LPoint { bool bad; std::map<int, int> obs; };                                     // key -> slot
struct LKeyFrame {
    int slot, key, mnId, parent; bool first; int touched;
    std::vector<int> pts;
    std::map<int, int> weights;                                                          // key -> weight
    std::vector<int> ordered, ordered_w;                                                 // keys
};
struct LMap {
    std::vector<LKeyFrame> kf; std::vector<LPoint> pt; std::vector<int> slot_of_key; int ccap;
    void UpdateBestCovisibles(LKeyFrame& K, int adding) {
        std::vector<std::pair<int, int> > vPairs;
        for (std::map<int, int>::iterator mit = K.weights.begin(); mit != K.weights.end(); ++mit) vPairs.push_back(std::make_pair(mit->second, mit->first));
        std::sort(vPairs.begin(), vPairs.end());
        std::list<int> lKFs, lWs;
        for (size_t i = 0; i < vPairs.size(); i++) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
        const std::set<int> before(K.ordered.begin(), K.ordered.end());
        for (size_t i = 0; i < vPairs.size(); i++) if (vPairs[i].first < 15 && vPairs[i].second != adding && !before.count(vPairs[i].second)) { g_seen.pulls++; break; }
        K.ordered.assign(lKFs.begin(), lKFs.end()); K.ordered_w.assign(lWs.begin(), lWs.end());
        for (size_t i = 1; i < K.ordered_w.size(); i++) if (K.ordered_w[i] == K.ordered_w[i - 1]) { g_seen.equal_weights++; break; }
        K.touched |= COV_ORD_REBUILT;
    }
    void AddConnection(LKeyFrame& K, int pKF, int weight) {
        if (!K.weights.count(pKF)) {
            if ((int)K.weights.size() + 1 > ccap) throw Overflow{(int)K.weights.size() + 1};
            K.weights[pKF] = weight;
        } else if (K.weights[pKF] != weight) K.weights[pKF] = weight;
        else { g_seen.early_return++; return; }
        K.touched |= COV_MAP_CHANGED;
        UpdateBestCovisibles(K, pKF);
    }
    // returns the parent it set or -1; info = observers, pKFmax (slot), nmax, vPairs.size()
    int UpdateConnections(LKeyFrame& T, int info[4]) {
        std::map<int, int> KFcounter;
        for (size_t i = 0; i < T.pts.size(); i++) {
            if (T.pts[i] < 0) continue;
            const LPoint& P = pt[T.pts[i]];
            if (P.bad) continue;
            for (std::map<int, int>::const_iterator mit = P.obs.begin(); mit != P.obs.end(); ++mit) {
                if (kf[mit->second].mnId == T.mnId) continue;
                KFcounter[mit->first]++;
            }
        }
        info[0] = (int)KFcounter.size(); info[1] = -1; info[2] = 0; info[3] = 0;
        if (KFcounter.empty()) return -1;
        if ((int)KFcounter.size() > ccap) throw Overflow{(int)KFcounter.size()};
        int nmax = 0, pKFmax = -1, ties = 0;
        const int th = 15;
        std::vector<std::pair<int, int> > vPairs;
        for (std::map<int, int>::iterator mit = KFcounter.begin(); mit != KFcounter.end(); ++mit) {
            if (mit->second > nmax) { nmax = mit->second; pKFmax = mit->first; ties = 0; } else if (mit->second == nmax) ties++;
            if (mit->second >= th) { vPairs.push_back(std::make_pair(mit->second, mit->first)); AddConnection(kf[slot_of_key[mit->first]], T.key, mit->second); }
        }
        if (ties) g_seen.tie++;
        if (vPairs.empty()) { g_seen.fallback++; vPairs.push_back(std::make_pair(nmax, pKFmax)); AddConnection(kf[slot_of_key[pKFmax]], T.key, nmax); }
        std::sort(vPairs.begin(), vPairs.end());
        std::list<int> lKFs, lWs;
        for (size_t i = 0; i < vPairs.size(); i++) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
        for (std::map<int, int>::iterator mit = T.weights.begin(); mit != T.weights.end(); ++mit)
            if (!KFcounter.count(mit->first) && kf[slot_of_key[mit->first]].weights.count(T.key)) g_seen.stale++;
        T.weights = KFcounter;
        T.ordered.assign(lKFs.begin(), lKFs.end()); T.ordered_w.assign(lWs.begin(), lWs.end());
        for (size_t i = 1; i < T.ordered_w.size(); i++) if (T.ordered_w[i] == T.ordered_w[i - 1]) { g_seen.equal_weights++; break; }
        T.touched |= COV_MAP_CHANGED | COV_ORD_REBUILT;
        int parent = -1;
        if (T.first && T.mnId != 0) { T.parent = parent = slot_of_key[T.ordered.front()]; T.first = false; g_seen.first_parent++; }
        info[1] = slot_of_key[pKFmax]; info[2] = nmax; info[3] = (int)vPairs.size();
        return parent;
    }
};

static void literal_stream(const CovMap& M, int b, Result& E) {
    const int k0 = M.kf_start[b], nk = M.kf_start[b + 1] - k0, p0 = M.pt_start[b], np = M.pt_start[b + 1] - p0, t0 = M.target_start[b], nt = M.target_start[b + 1] - t0;
    LMap L; L.ccap = M.ccap; L.kf.resize(nk); L.pt.resize(np); L.slot_of_key.resize(nk);
    for (int j = 0; j < nk; j++) { L.kf[M.kf_by_key[k0 + j]].key = j; L.slot_of_key[j] = M.kf_by_key[k0 + j]; }
    for (int k = 0; k < nk; k++) {
        LKeyFrame& K = L.kf[k];
        K.slot = k; K.mnId = (M.kf_flags[k0 + k] & COV_KF_ID0) ? 0 : k + 1; K.first = (M.kf_flags[k0 + k] & COV_KF_FIRST) != 0; K.parent = M.kf_parent[k0 + k]; K.touched = 0;
        for (int i = M.kp_start[k0 + k]; i < M.kp_start[k0 + k + 1]; i++) K.pts.push_back(M.kp_point[i]);
        for (int i = M.conn_start[k0 + k]; i < M.conn_start[k0 + k + 1]; i++) K.weights[L.kf[M.conn_kf[i]].key] = M.conn_w[i];
        for (int i = M.ord_start[k0 + k]; i < M.ord_start[k0 + k + 1]; i++) { K.ordered.push_back(L.kf[M.ord_kf[i]].key); K.ordered_w.push_back(M.ord_w[i]); }
    }
    for (int p = 0; p < np; p++) {
        L.pt[p].bad = M.pt_bad[p0 + p] != 0;
        for (int o = M.obs_start[p0 + p]; o < M.obs_start[p0 + p + 1]; o++) { const int s = (int)(M.obs[o] & 0xffffu); L.pt[p].obs[L.kf[s].key] = s; }
    }
    const auto loop_t0 = std::chrono::steady_clock::now();
    E.status[b] = COV_OK; E.need[b] = 0;
    try {
        std::map<int, std::set<int> > LoopConnections;                                  // LoopClosing.cc:572-590, keys
        for (int t = 0; t < nt; t++) {
            LKeyFrame& pKFi = L.kf[M.target_kf[t0 + t]];
            const std::vector<int> vpPreviousNeighbors = pKFi.ordered;
            int info[4];
            E.t_par[t0 + t] = L.UpdateConnections(pKFi, info);
            E.t_obs[t0 + t] = info[0]; E.t_mk[t0 + t] = info[1]; E.t_mw[t0 + t] = info[2]; E.t_add[t0 + t] = info[3];
            std::set<int>& C = LoopConnections[pKFi.key];
            C.clear();
            for (std::map<int, int>::iterator mit = pKFi.weights.begin(); mit != pKFi.weights.end(); ++mit) C.insert(mit->first);
            for (size_t i = 0; i < vpPreviousNeighbors.size(); i++) C.erase(vpPreviousNeighbors[i]);
            if (M.erase_targets) for (int t2 = 0; t2 < nt; t2++) C.erase(L.kf[M.target_kf[t0 + t2]].key);
            int m = 0;
            for (std::set<int>::iterator it = C.begin(); it != C.end(); ++it) E.loop[(size_t)(t0 + t) * M.ccap + m++] = L.slot_of_key[*it];
            for (int i = m; i < M.ccap; i++) E.loop[(size_t)(t0 + t) * M.ccap + i] = -1;
            E.n_loop[t0 + t] = m;
            if (m) g_seen.loop_nonempty++; else g_seen.loop_empty++;
        }
    } catch (const Overflow& o) { E.status[b] = COV_OVERFLOW; E.need[b] = o.need; }
    g_loop_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - loop_t0).count();
    if (E.status[b] != COV_OK) return;
    for (int k = 0; k < nk; k++) {
        const LKeyFrame& K = L.kf[k];
        const size_t row = (size_t)(k0 + k) * M.ccap;
        int n = 0;
        for (std::map<int, int>::const_iterator mit = K.weights.begin(); mit != K.weights.end(); ++mit, n++) { E.ck[row + n] = L.slot_of_key[mit->first]; E.cw[row + n] = mit->second; }
        for (int i = n; i < M.ccap; i++) E.ck[row + i] = E.cw[row + i] = -1;
        E.cn[k0 + k] = n;
        n = (int)K.ordered.size();
        for (int i = 0; i < M.ccap; i++) { E.ok[row + i] = i < n ? L.slot_of_key[K.ordered[i]] : -1; E.ow[row + i] = i < n ? K.ordered_w[i] : -1; }
        E.on[k0 + k] = n;
        E.parent[k0 + k] = K.parent; E.flags[k0 + k] = (uint8_t)((K.mnId == 0 ? COV_KF_ID0 : 0) | (K.first ? COV_KF_FIRST : 0)); E.touched[k0 + k] = (uint8_t)K.touched;
    }
}

// ---- random streams ----------------------------------------------------------------------------------------------------------------------
static std::vector<int> distinct(int n, int range) {
    std::vector<int> all(range), out;
    for (int i = 0; i < range; i++) all[i] = i;
    for (int i = 0; i < n && i < range; i++) { std::swap(all[i], all[i + (int)(rnd() % (unsigned)(range - i))]); out.push_back(all[i]); }
    return out;
}

static void add_stream(Packed& P) {
    const int nk = rnd() % 25 == 0 ? 0 : rint_(1, 12), np = nk ? rint_(0, 10) : 0;
    const std::vector<int> order = distinct(nk, nk);
    std::vector<int> rank(nk);
    for (int j = 0; j < nk; j++) { P.kf_by_key.push_back(order[j]); rank[order[j]] = j; }
    const int p0 = (int)P.pt_bad.size();
    for (int p = 0; p < np; p++) {
        const std::vector<int> ob = distinct(rint_(0, 4), nk);
        for (size_t i = 0; i < ob.size(); i++) P.obs.push_back((uint32_t)ob[i] | ((rnd() & 0xffu) << 16));       // the higher bits are ignored
        P.obs_start.push_back((int)P.obs.size());
        P.pt_bad.push_back(rnd() % 10 == 0);
    }
    std::vector<std::vector<int> > tabs(nk);
    std::vector<std::map<int, int> > votes(nk);                                          // what k as a target hands to slot o
    for (int k = 0; k < nk; k++) {
        for (int i = (np ? rint_(0, 70) : 0); i > 0; i--) tabs[k].push_back(rnd() % 8 ? rint_(0, np - 1) : -1);
        for (size_t i = 0; i < tabs[k].size(); i++) {
            const int p = tabs[k][i];
            if (p < 0 || P.pt_bad[p0 + p]) continue;
            for (int o = P.obs_start[p0 + p]; o < P.obs_start[p0 + p + 1]; o++) { const int s = (int)(P.obs[o] & 0xffffu); if (s != k) votes[k][s]++; }
        }
    }
    for (int k = 0; k < nk; k++) {
        const bool first = rnd() % 2 == 0;
        P.kf_flags.push_back((uint8_t)((k == 0 && rnd() % 2 ? COV_KF_ID0 : 0) | (first ? COV_KF_FIRST : 0)));
        P.kf_parent.push_back(first ? -1 : rint_(-1, nk - 1));
        for (size_t i = 0; i < tabs[k].size(); i++) P.kp_point.push_back(tabs[k][i]);
        P.kp_start.push_back((int)P.kp_point.size());
        std::vector<std::pair<int, int> > full;                                          // (weight, rank) of the map, which is laid out by rank
        std::vector<int> by_rank(nk, 0);
        for (int o = 0; o < nk; o++) {
            if (o == k || rnd() % 5 < 3) continue;
            const int now = votes[o].count(k) ? votes[o][k] : 0;
            by_rank[rank[o]] = now && rnd() % 2 ? now : rint_(1, 40);
        }
        for (int j = 0; j < nk; j++) if (by_rank[j]) { P.conn_kf.push_back(order[j]); P.conn_w.push_back(by_rank[j]); full.push_back(std::make_pair(by_rank[j], j)); }
        P.conn_start.push_back((int)P.conn_kf.size());
        std::sort(full.begin(), full.end());
        const int mode = (int)(rnd() % 5);                                               // the whole map in order, thresholded, or empty
        for (int i = (int)full.size() - 1; i >= 0; i--) if (mode < 2 || (mode < 4 && full[i].first >= 15)) { P.ord_kf.push_back(order[full[i].second]); P.ord_w.push_back(full[i].first); }
        P.ord_start.push_back((int)P.ord_kf.size());
    }
    if (nk) {
        const std::vector<int> tg = distinct(rint_(0, 5), nk);
        for (size_t i = 0; i < tg.size(); i++) P.target_kf.push_back(tg[i]);
        if (!tg.empty() && rnd() % 6 == 0) P.target_kf.push_back(tg[0]);
    }
    P.batch++;
    P.kf_start.push_back((int)P.kf_flags.size()); P.pt_start.push_back((int)P.pt_bad.size()); P.target_start.push_back((int)P.target_kf.size());
}

static Packed make_batch(int n) {
    Packed P;
    P.kf_start.push_back(0); P.pt_start.push_back(0); P.target_start.push_back(0); P.kp_start.push_back(0); P.obs_start.push_back(0); P.conn_start.push_back(0); P.ord_start.push_back(0);
    for (int b = 0; b < n; b++) add_stream(P);
    P.ccap = 11; P.erase = (int)(rnd() % 2);
    return P;
}

template <class T> static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a == b; }
static bool same_range(const std::vector<int32_t>& a, const std::vector<int32_t>& b, size_t i0, size_t i1) { return std::equal(a.begin() + i0, a.begin() + i1, b.begin() + i0); }

// every output of stream b against the literal loop's
static void compare_stream(const CovMap& M, const Result& G, const Result& E, int b, const char* what) {
    if (G.status[b] != E.status[b] || G.need[b] != E.need[b]) fail(what);
    if (E.status[b] != COV_OK) return;
    const size_t k0 = M.kf_start[b], k1 = M.kf_start[b + 1], t0 = M.target_start[b], t1 = M.target_start[b + 1], cc = M.ccap;
    bool ok = same_range(G.ck, E.ck, k0 * cc, k1 * cc) && same_range(G.cw, E.cw, k0 * cc, k1 * cc) && same_range(G.ok, E.ok, k0 * cc, k1 * cc) && same_range(G.ow, E.ow, k0 * cc, k1 * cc);
    ok = ok && same_range(G.cn, E.cn, k0, k1) && same_range(G.on, E.on, k0, k1) && same_range(G.parent, E.parent, k0, k1);
    ok = ok && std::equal(G.flags.begin() + k0, G.flags.begin() + k1, E.flags.begin() + k0) && std::equal(G.touched.begin() + k0, G.touched.begin() + k1, E.touched.begin() + k0);
    ok = ok && same_range(G.t_obs, E.t_obs, t0, t1) && same_range(G.t_mk, E.t_mk, t0, t1) && same_range(G.t_mw, E.t_mw, t0, t1) && same_range(G.t_add, E.t_add, t0, t1);
    ok = ok && same_range(G.t_par, E.t_par, t0, t1) && same_range(G.n_loop, E.n_loop, t0, t1) && same_range(G.loop, E.loop, t0 * cc, t1 * cc);
    if (!ok) fail(what);
}

static void compare(const Packed& P) {
    const CovMap M = P.map();
    Result G, E;
    G.size(M); E.size(M);
    Workspace S;
    cov_run_host(M, S.work(M), G.out());
    for (int b = 0; b < M.batch; b++) { literal_stream(M, b, E); compare_stream(M, G, E, b, "a stream differs from the literal loop"); sum += G.status[b] + G.need[b]; }
    for (size_t i = 0; i < G.cn.size(); i++) sum += G.cn[i] * 3 + G.on[i];
}

// one stream broken in one way between two good ones: it alone is refused and writes nothing, nothing is read through the broken index
static void expect_refused(const Packed& P, const char* what) {
    const CovMap M = P.map();
    Result G, E;
    G.size(M); E.size(M);
    Workspace S;
    cov_run_host(M, S.work(M), G.out());
    if (G.status[1] != COV_INVALID) fail(what);
    if (G.status[0] < 0 || G.status[2] < 0) fail("a stream beside a broken one was refused");
    // the ranges of the two accepted streams; everything else still holds the fill
    std::vector<char> kf_mine(M.n_kf, 0), t_mine(M.n_target, 0);
    for (int b = 0; b < 3; b += 2) {
        for (int k = M.kf_start[b]; k < M.kf_start[b + 1]; k++) kf_mine[k] = 1;
        for (int t = M.target_start[b]; t < M.target_start[b + 1]; t++) t_mine[t] = 1;
    }
    for (int k = 0; k < M.n_kf; k++) {
        if (kf_mine[k]) continue;
        if (G.cn[k] != 77 || G.on[k] != 77 || G.parent[k] != 77 || G.flags[k] != 77 || G.touched[k] != 77) fail("a refused stream wrote more than its status");
        for (int i = 0; i < M.ccap; i++) if (G.ck[(size_t)k * M.ccap + i] != 77 || G.ow[(size_t)k * M.ccap + i] != 77) fail("a refused stream wrote more than its status");
    }
    for (int t = 0; t < M.n_target; t++) if (!t_mine[t] && (G.t_obs[t] != 77 || G.n_loop[t] != 77 || G.loop[(size_t)t * M.ccap] != 77)) fail("a refused stream wrote more than its status");
    if (G.need[1] != 77) fail("a refused stream wrote more than its status");
    literal_stream(M, 0, E); literal_stream(M, 2, E);
    compare_stream(M, G, E, 0, "a stream beside a broken one changed"); compare_stream(M, G, E, 2, "a stream beside a broken one changed");
    sum += G.status[2];
}

static void broken_snapshots() {
    for (int round = 0; round < 40; round++) {
        Packed P;
        for (;;) {
            P = make_batch(3);
            const int k0 = P.kf_start[1], nk = P.kf_start[2] - k0, p0 = P.pt_start[1], t0 = P.target_start[1];
            if (nk < 3 || P.pt_start[2] - p0 < 2 || P.target_start[2] - t0 < 1 || P.obs_start[p0 + 1] - P.obs_start[p0] < 1) continue;
            const int g = k0 + P.target_kf[t0];
            if (P.kp_start[g + 1] - P.kp_start[g] < 1 || P.conn_start[k0 + 1] - P.conn_start[k0] < 2 || P.ord_start[k0 + 1] - P.ord_start[k0] < 2) continue;
            break;
        }
        const int k0 = P.kf_start[1], nk = P.kf_start[2] - k0, p0 = P.pt_start[1], np = P.pt_start[2] - p0, t0 = P.target_start[1], o0 = P.obs_start[p0];
        const int i0 = P.kp_start[k0 + P.target_kf[t0]], c0 = P.conn_start[k0], r0 = P.ord_start[k0];
        const int big = 1 << 28;
        { Packed Q = P; Q.kp_point[i0] = np; expect_refused(Q, "a point index at the end of the stream was accepted"); }
        { Packed Q = P; Q.kp_point[i0] = big; expect_refused(Q, "a point index far past the end was accepted"); }
        { Packed Q = P; Q.kp_point[i0] = -2; expect_refused(Q, "a point index below -1 was accepted"); }
        { Packed Q = P; Q.obs[o0] = (uint32_t)nk; expect_refused(Q, "an observation slot at the end was accepted"); }
        { Packed Q = P; Q.obs[o0] |= 0xffffu; expect_refused(Q, "an observation slot past the end was accepted"); }
        { Packed Q = P; Q.kp_start[k0 + 1] = Q.kp_start[k0 + 2] + 1; expect_refused(Q, "descending keypoint offsets were accepted"); }
        { Packed Q = P; Q.kp_start[k0 + 1] = big; expect_refused(Q, "a keypoint offset past the total was accepted"); }
        { Packed Q = P; Q.obs_start[p0 + 1] = Q.obs_start[p0 + 2] + 1; expect_refused(Q, "descending observation offsets were accepted"); }
        { Packed Q = P; Q.obs_start[p0 + 1] = -big; expect_refused(Q, "a negative observation offset was accepted"); }
        { Packed Q = P; Q.conn_start[k0 + 1] = Q.conn_start[k0 + 2] + 1; expect_refused(Q, "descending conn offsets were accepted"); }
        { Packed Q = P; Q.conn_start[k0 + 1] = big; expect_refused(Q, "a conn offset past the total was accepted"); }
        { Packed Q = P; Q.ord_start[k0 + 1] = Q.ord_start[k0 + 2] + 1; expect_refused(Q, "descending ord offsets were accepted"); }
        { Packed Q = P; Q.ord_start[k0 + 1] = -big; expect_refused(Q, "a negative ord offset was accepted"); }
        { Packed Q = P; Q.kf_parent[k0] = nk; expect_refused(Q, "a parent outside the snapshot was accepted"); }
        { Packed Q = P; Q.kf_parent[k0 + 1] = -2; expect_refused(Q, "a parent below -1 was accepted"); }
        { Packed Q = P; Q.kf_by_key[k0] = Q.kf_by_key[k0 + 1]; expect_refused(Q, "kf_by_key with a slot twice was accepted"); }
        { Packed Q = P; Q.kf_by_key[k0 + 2] = nk; expect_refused(Q, "kf_by_key with a slot out of range was accepted"); }
        { Packed Q = P; Q.kf_by_key[k0 + 2] = -big; expect_refused(Q, "kf_by_key with a negative slot was accepted"); }
        { Packed Q = P; Q.conn_kf[c0] = nk; expect_refused(Q, "a conn slot at the end was accepted"); }
        { Packed Q = P; Q.conn_kf[c0 + 1] = -1; expect_refused(Q, "a negative conn slot was accepted"); }
        { Packed Q = P; std::swap(Q.conn_kf[c0], Q.conn_kf[c0 + 1]); expect_refused(Q, "a conn row out of key order was accepted"); }
        { Packed Q = P; Q.conn_kf[c0] = Q.conn_kf[c0 + 1]; expect_refused(Q, "a conn row with a slot twice was accepted"); }
        { Packed Q = P; Q.conn_kf[c0] = 0; expect_refused(Q, "a conn row that names its own key frame was accepted"); }
        { Packed Q = P; Q.ord_kf[r0] = nk; expect_refused(Q, "an ord slot at the end was accepted"); }
        { Packed Q = P; Q.ord_kf[r0 + 1] = -big; expect_refused(Q, "a negative ord slot was accepted"); }
        { Packed Q = P; Q.ord_kf[r0] = Q.ord_kf[r0 + 1]; expect_refused(Q, "an ord row with a slot twice was accepted"); }
        { Packed Q = P; Q.target_kf[t0] = nk; expect_refused(Q, "a target outside the snapshot was accepted"); }
        { Packed Q = P; Q.target_kf[t0] = -1; expect_refused(Q, "a negative target was accepted"); }
    }
    // an input row longer than ccap
    for (int round = 0, seen = 0; seen < 5; round++) {
        if (round > 400) fail("no long input rows were made");
        Packed P = make_batch(3);
        int longest[3] = {0, 0, 0};
        for (int b = 0; b < 3; b++) for (int k = P.kf_start[b]; k < P.kf_start[b + 1]; k++) longest[b] = std::max(longest[b], std::max(P.conn_start[k + 1] - P.conn_start[k], P.ord_start[k + 1] - P.ord_start[k]));
        if (longest[1] < 2 || longest[0] >= longest[1] || longest[2] >= longest[1]) continue;
        P.ccap = longest[1] - 1;
        const CovMap M = P.map();
        Result G; G.size(M);
        Workspace S;
        cov_run_host(M, S.work(M), G.out());
        if (G.status[0] < 0 || G.status[1] != COV_INVALID || G.status[2] < 0) fail("an input row longer than ccap was accepted");
        seen++;
    }
    // offsets of the batch level: a stream is refused together with every later one
    for (int which = 0; which < 3; which++) {
        Packed P;
        do { P = make_batch(3); } while (P.kf_start[1] < 1 || P.pt_start[1] < 1 || P.target_start[1] < 1);
        std::vector<int32_t>& v = which == 0 ? P.kf_start : which == 1 ? P.pt_start : P.target_start;
        v[2] = v[1] - 1;
        const CovMap M = P.map();
        Result G; G.size(M);
        Workspace S;
        cov_run_host(M, S.work(M), G.out());
        if (G.status[0] < 0 || G.status[1] != COV_INVALID || G.status[2] != COV_INVALID) fail("descending offsets of the batch were accepted");
    }
    // a nested offset at a stream boundary that falls back into an earlier stream's range: the streams on both sides of it are refused
    Packed Q;
    do { Q = make_batch(3); } while (Q.conn_start[Q.kf_start[1]] < 1 || Q.kf_start[2] == Q.kf_start[1]);
    Q.conn_start[Q.kf_start[2]] = Q.conn_start[Q.kf_start[1]] - 1;
    const CovMap N = Q.map();
    Result H; H.size(N);
    Workspace S3;
    cov_run_host(N, S3.work(N), H.out());
    if (H.status[0] < 0 || H.status[1] != COV_INVALID || H.status[2] != COV_INVALID) fail("a conn offset at a stream boundary that overlaps an earlier stream was accepted");
}

// overflow by one: the row that needs the most entries gets one less; the needed length comes back, and with exactly that length nothing overflows
static void overflows() {
    int seen = 0, seen_added = 0;
    for (int round = 0; round < 400 && (seen < 10 || seen_added < 3); round++) {
        Packed P = make_batch(1);
        const CovMap M0 = P.map();
        Result E; E.size(M0);
        literal_stream(M0, 0, E);
        if (E.status[0] != COV_OK) fail("a random stream overflows 11 entries");
        int longest_in = 1, longest_out = 0;                                             // longest_out: the shortest rows with which nothing overflows (a row may be longer on the way than at the end)
        for (int k = 0; k < M0.n_kf; k++) longest_in = std::max(longest_in, std::max(P.conn_start[k + 1] - P.conn_start[k], P.ord_start[k + 1] - P.ord_start[k]));
        for (int c = longest_in; c <= 11 && !longest_out; c++) {
            Packed Q = P; Q.ccap = c;
            const CovMap M = Q.map();
            Result F; F.size(M);
            literal_stream(M, 0, F);
            if (F.status[0] == COV_OK) longest_out = c;
        }
        if (longest_out <= longest_in) continue;                                         // one entry less would refuse the input itself
        for (int d = 0; d < 2; d++) {
            Packed Q = P; Q.ccap = longest_out - 1 + d;
            const CovMap M = Q.map();
            Result G, F; G.size(M); F.size(M);
            Workspace S;
            cov_run_host(M, S.work(M), G.out());
            literal_stream(M, 0, F);
            compare_stream(M, G, F, 0, "an overflow by one differs from the literal loop");
            if (d == 0 && (G.status[0] != COV_OVERFLOW || G.need[0] != longest_out)) fail("an overflow by one does not report the needed length");
            if (d == 1 && G.status[0] != COV_OK) fail("a row that reaches exactly ccap overflowed");
            if (d == 0) { seen++; bool own = false; for (int t = 0; t < M.n_target; t++) own = own || E.t_obs[t] == longest_out; if (!own) seen_added++; }
        }
    }
    if (seen < 10 || seen_added < 3) fail("no overflow cases were made");
}

template <class T> static void read_into(std::vector<T>& v, size_t n, FILE* f) { v.resize(n); if (n && std::fread(v.data(), sizeof(T), n, f) != n) fail("short snapshot file"); }

static int time_literal(const char* path, int reps) {
    FILE* f = std::fopen(path, "rb");
    if (!f) fail("cannot open the snapshot file");
    int32_t h[10];
    if (std::fread(h, 4, 10, f) != 10) fail("short snapshot file");
    Packed P;
    const size_t nb = h[0], nk = h[1], ni = h[2], np = h[3], no = h[4], nc = h[5], nr = h[6], nt = h[7];
    P.batch = h[0]; P.ccap = h[8]; P.erase = h[9];
    read_into(P.kf_start, nb + 1, f); read_into(P.kf_by_key, nk, f); read_into(P.kf_flags, nk, f); read_into(P.kf_parent, nk, f); read_into(P.kp_start, nk + 1, f); read_into(P.kp_point, ni, f);
    read_into(P.pt_start, nb + 1, f); read_into(P.pt_bad, np, f); read_into(P.obs_start, np + 1, f); read_into(P.obs, no, f);
    read_into(P.conn_start, nk + 1, f); read_into(P.conn_kf, nc, f); read_into(P.conn_w, nc, f); read_into(P.ord_start, nk + 1, f); read_into(P.ord_kf, nr, f); read_into(P.ord_w, nr, f);
    read_into(P.target_start, nb + 1, f); read_into(P.target_kf, nt, f);
    std::fclose(f);
    const CovMap M = P.map();
    Result E, G; E.size(M); G.size(M);
    double best = 1e300, best_core = 1e300;
    for (int r = 0; r < reps; r++) {
        g_loop_ms = 0;
        for (int b = 0; b < M.batch; b++) literal_stream(M, b, E);
        best = std::min(best, g_loop_ms);
        Workspace S; const CovWork W = S.work(M);
        const auto t1 = std::chrono::steady_clock::now();
        cov_run_host(M, W, G.out());
        best_core = std::min(best_core, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    }
    for (int b = 0; b < M.batch; b++) compare_stream(M, G, E, b, "the flat form differs from the literal loop on the snapshot");
    long long added = 0, observers = 0;
    for (size_t t = 0; t < nt; t++) { added += E.t_add[t]; observers += E.t_obs[t]; }
    std::printf("{\"streams\": %d, \"targets\": %d, \"literal_loop_ms\": %.3f, \"flat_core_one_thread_ms\": %.3f, \"observers_per_target\": %.1f, \"added_per_target\": %.1f}\n",
                M.batch, (int)nt, best, best_core, nt ? (double)observers / nt : 0.0, nt ? (double)added / nt : 0.0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "time")) return time_literal(argv[2], argc >= 4 ? std::atoi(argv[3]) : 3);
    long long streams = 0;
    for (int round = 0; round < 110; round++) {
        const Packed P = make_batch(rint_(1, 60));
        streams += P.batch;
        compare(P);
    }
    if (streams < 3000) fail("fewer than 3000 random streams");
    const Seen s = g_seen;
    broken_snapshots();
    overflows();
    std::printf("checksum %lld streams %lld fallback %lld tie %lld equal-weights %lld early-return %lld rebuild-pulls-sub-threshold %lld first-parent %lld stale %lld loop-nonempty %lld loop-empty %lld\n",
                sum, streams, s.fallback, s.tie, s.equal_weights, s.early_return, s.pulls, s.first_parent, s.stale, s.loop_nonempty, s.loop_empty);
    return 0;
}
