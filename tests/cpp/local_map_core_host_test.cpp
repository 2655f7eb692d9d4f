// tests/cpp/local_map_core_host_test.cpp — the host build of viorb_amd/csrc/local_map_core.h as a stand-alone program. No GPU, no library:
// only the header.
//   local_map_core_host_test                    the self-test that tests/test_local_map_host_sanitized.py compiles with
//                                               -fsanitize=address,undefined and runs as a child process: ulm_run_host (validate, votes,
//                                               voted list, neighbour loop, points) against the literal loop below on a few thousand random
//                                               small streams, and every kind of broken snapshot, which the validator must refuse without
//                                               reading through it. The program requires its random set to hold at least one case of:
//                                               no votes, a tie for the most votes, the break at more than 80 entries, a bad neighbour
//                                               skipped, a point dropped because an earlier key frame holds it. Prints one checksum line.
//   local_map_core_host_test time FILE [reps]   the literal loop (one thread) timed on a packed snapshot that tools/local_map_time.py writes:
//                                               6 totals and cap, lcap, pcap as int32, then the arrays of viorb_local_map_snapshot in their
//                                               order (the two byte arrays as bytes).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "local_map_core.h"

using namespace viorb;

static long long sum = 0;
static unsigned rng_state = 24680u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rint_(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }
static void fail(const char* what) { std::printf("FAILED: %s\n", what); std::exit(2); }

// a packed batch with exactly sized arrays, so that the address sanitizer sees any read past an end
struct Packed {
    int batch = 0, cap = 1, lcap = 1, pcap = 1;
    std::vector<int32_t> kf_start, kf_parent, kf_prev, kf_next, covis10, child_start, child_kf, kf_by_key, kp_start, kp_point, pt_start, obs_start;
    std::vector<int32_t> frame_point, frame_count, prev_lkf, prev_n_lkf, prev_ref_kf;
    std::vector<uint8_t> kf_bad, pt_bad;
    std::vector<uint32_t> obs;
    std::vector<std::vector<int32_t>> frames, prevs;                 // per stream, laid out as rows by finish()
    void finish() {
        cap = lcap = 1;
        for (int b = 0; b < batch; b++) { cap = std::max<int>(cap, (int)frames[b].size()); lcap = std::max<int>(lcap, (int)prevs[b].size()); lcap = std::max(lcap, kf_start[b + 1] - kf_start[b]); }
        pcap = 1;
        for (int b = 0; b < batch; b++) pcap = std::max(pcap, pt_start[b + 1] - pt_start[b]);
        frame_point.assign((size_t)batch * cap, -1); prev_lkf.assign((size_t)batch * lcap, -1); frame_count.clear(); prev_n_lkf.clear();
        for (int b = 0; b < batch; b++) {
            std::copy(frames[b].begin(), frames[b].end(), frame_point.begin() + (size_t)b * cap); frame_count.push_back((int)frames[b].size());
            std::copy(prevs[b].begin(), prevs[b].end(), prev_lkf.begin() + (size_t)b * lcap); prev_n_lkf.push_back((int)prevs[b].size());
        }
    }
    UlmMap map() const {
        UlmMap M;
        M.batch = batch; M.n_kf = (int)kf_bad.size(); M.n_child = (int)child_kf.size(); M.n_kp = (int)kp_point.size(); M.n_pt = (int)pt_bad.size(); M.n_obs = (int)obs.size();
        M.kf_start = kf_start.data(); M.kf_bad = kf_bad.data(); M.kf_parent = kf_parent.data(); M.kf_prev = kf_prev.data(); M.kf_next = kf_next.data();
        M.covis10 = covis10.data(); M.child_start = child_start.data(); M.child_kf = child_kf.data(); M.kf_by_key = kf_by_key.data();
        M.kp_start = kp_start.data(); M.kp_point = kp_point.data(); M.pt_start = pt_start.data(); M.pt_bad = pt_bad.data(); M.obs_start = obs_start.data(); M.obs = obs.data();
        M.frame_point = frame_point.data(); M.frame_count = frame_count.data(); M.prev_lkf = prev_lkf.data(); M.prev_n_lkf = prev_n_lkf.data(); M.prev_ref_kf = prev_ref_kf.data();
        M.cap = cap; M.lcap = lcap; M.pcap = pcap;
        return M;
    }
};

struct Result {
    std::vector<int32_t> lkf, n_lkf, n_voted, ref, lpt, n_lpt, status, fpo, votes;
    void size(const UlmMap& M) {
        lkf.assign((size_t)M.batch * M.lcap, 77); lpt.assign((size_t)M.batch * M.pcap, 77); fpo.assign((size_t)M.batch * M.cap, 77);
        n_lkf.assign(M.batch, 77); n_voted = ref = n_lpt = status = n_lkf; votes.assign(M.n_kf, 77);
    }
    UlmOut out() {
        UlmOut R;
        R.lkf = lkf.data(); R.n_lkf = n_lkf.data(); R.n_voted = n_voted.data(); R.ref_kf = ref.data(); R.lpt = lpt.data(); R.n_lpt = n_lpt.data(); R.status = status.data();
        R.frame_point_out = fpo.data(); R.kf_votes = votes.data();
        return R;
    }
};

struct Workspace {
    std::vector<int32_t> votes, mark, list, estart, first, info;
    UlmWork work(const UlmMap& M) {
        votes.assign(M.n_kf, 0); mark = votes; list.assign((size_t)M.n_kf + M.batch, 0); estart = list; first.assign(M.n_pt, 0); info.assign((size_t)M.batch * ULM_INFO, 0);
        UlmWork W;
        W.votes = votes.data(); W.mark = mark.data(); W.list = list.data(); W.estart = estart.data(); W.first = first.data(); W.info = info.data();
        return W;
    }
};

// ---- the literal loop: objects, std::map counters in key order, marks, in-place mutation (src/Tracking.cc:1970-2125) ------------------------
// A key frame's address is its position in kf_by_key: std::map<int, ...> keyed by it iterates as std::map<KeyFrame*, ...> does.
struct LPoint { bool bad; long mark; std::map<int, int> obs; };                          // key -> slot
struct LKeyFrame { bool bad; int key, parent, prev, next; long mark; std::vector<int> neigh, children, pts; };
struct Seen { long long no_votes = 0, tie = 0, limit_break = 0, bad_neighbour = 0, first_occurrence = 0, all_bad = 0; };
static Seen g_seen;
static double g_loop_ms = 0;          // the time inside the two routines alone (the objects exist already in the reference)

static void literal_stream(const UlmMap& M, int b, Result& E) {
    const int k0 = M.kf_start[b], nk = M.kf_start[b + 1] - k0, p0 = M.pt_start[b], np = M.pt_start[b + 1] - p0;
    std::vector<LKeyFrame> kf(nk);
    std::vector<LPoint> pt(np);
    std::vector<int> slot_of_key(nk);
    for (int j = 0; j < nk; j++) { kf[M.kf_by_key[k0 + j]].key = j; slot_of_key[j] = M.kf_by_key[k0 + j]; }
    for (int k = 0; k < nk; k++) {
        LKeyFrame& K = kf[k];
        K.bad = M.kf_bad[k0 + k] != 0; K.parent = M.kf_parent[k0 + k]; K.prev = M.kf_prev[k0 + k]; K.next = M.kf_next[k0 + k]; K.mark = 0;
        for (int i = 0; i < 10; i++) if (M.covis10[(size_t)(k0 + k) * 10 + i] >= 0) K.neigh.push_back(M.covis10[(size_t)(k0 + k) * 10 + i]);
        for (int c = M.child_start[k0 + k]; c < M.child_start[k0 + k + 1]; c++) K.children.push_back(M.child_kf[c]);
        for (int i = M.kp_start[k0 + k]; i < M.kp_start[k0 + k + 1]; i++) K.pts.push_back(M.kp_point[i]);
    }
    for (int p = 0; p < np; p++) {
        pt[p].bad = M.pt_bad[p0 + p] != 0; pt[p].mark = 0;
        for (int o = M.obs_start[p0 + p]; o < M.obs_start[p0 + p + 1]; o++) { const int s = (int)(M.obs[o] & 0xffffu); pt[p].obs[kf[s].key] = s; }
    }
    std::vector<int> frame(M.frame_point + (size_t)b * M.cap, M.frame_point + (size_t)b * M.cap + M.frame_count[b]);
    std::vector<int> local(M.prev_lkf + (size_t)b * M.lcap, M.prev_lkf + (size_t)b * M.lcap + M.prev_n_lkf[b]);
    int ref = M.prev_ref_kf[b], status = ULM_OK, n_voted = 0;
    const long id = 1234;
    const auto loop_t0 = std::chrono::steady_clock::now();
    // UpdateLocalKeyFrames
    std::map<int, int> keyframeCounter;                                                 // key -> votes
    for (size_t i = 0; i < frame.size(); i++) {
        if (frame[i] >= 0) {
            LPoint& P = pt[frame[i]];
            if (!P.bad) { for (std::map<int, int>::const_iterator it = P.obs.begin(); it != P.obs.end(); ++it) keyframeCounter[it->first]++; }
            else frame[i] = -1;
        }
    }
    if (keyframeCounter.empty()) { status = ULM_NO_VOTES; g_seen.no_votes++; }
    else {
        int max = 0, pKFmax = -1, ties = 0;
        local.clear();
        for (std::map<int, int>::const_iterator it = keyframeCounter.begin(); it != keyframeCounter.end(); ++it) {
            const int k = slot_of_key[it->first];
            if (kf[k].bad) continue;
            if (it->second > max) { max = it->second; pKFmax = k; ties = 0; } else if (it->second == max) ties++;
            local.push_back(k);
            kf[k].mark = id;
        }
        g_seen.tie += ties > 0; g_seen.all_bad += local.empty();
        n_voted = (int)local.size();
        for (int j = 0; j < n_voted; j++) {                                              // itEndKF is the end before the loop
            if (local.size() > 80) { g_seen.limit_break++; break; }
            const LKeyFrame& K = kf[local[j]];
            for (size_t q = 0; q < K.neigh.size(); q++) {
                LKeyFrame& N = kf[K.neigh[q]];
                if (!N.bad) { if (N.mark != id) { local.push_back(K.neigh[q]); N.mark = id; break; } }
                else if (N.mark != id) g_seen.bad_neighbour++;
            }
            for (size_t q = 0; q < K.children.size(); q++) {
                LKeyFrame& N = kf[K.children[q]];
                if (!N.bad) { if (N.mark != id) { local.push_back(K.children[q]); N.mark = id; break; } }
            }
            const int links[3] = {K.parent, K.prev, K.next};
            for (int q = 0; q < 3; q++) if (links[q] >= 0) { if (kf[links[q]].mark != id) { local.push_back(links[q]); kf[links[q]].mark = id; } }
        }
        if (pKFmax >= 0) ref = pKFmax;
    }
    // UpdateLocalPoints
    std::vector<int> points;
    for (size_t j = 0; j < local.size(); j++) {
        const std::vector<int>& vpMPs = kf[local[j]].pts;
        for (size_t i = 0; i < vpMPs.size(); i++) {
            if (vpMPs[i] < 0) continue;
            LPoint& P = pt[vpMPs[i]];
            if (P.mark == id) { g_seen.first_occurrence++; continue; }
            if (!P.bad) { points.push_back(vpMPs[i]); P.mark = id; }
        }
    }
    g_loop_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - loop_t0).count();
    if ((int)local.size() > M.lcap || (int)points.size() > M.pcap) status = ULM_OVERFLOW;
    for (int j = 0; j < M.lcap; j++) E.lkf[(size_t)b * M.lcap + j] = j < (int)local.size() ? local[j] : -1;
    for (int j = 0; j < M.pcap; j++) E.lpt[(size_t)b * M.pcap + j] = j < (int)points.size() ? points[j] : -1;
    for (int i = 0; i < M.cap; i++) E.fpo[(size_t)b * M.cap + i] = i < (int)frame.size() ? frame[i] : -1;
    for (int k = 0; k < nk; k++) E.votes[k0 + k] = 0;
    for (std::map<int, int>::const_iterator it = keyframeCounter.begin(); it != keyframeCounter.end(); ++it) E.votes[k0 + slot_of_key[it->first]] = it->second;
    E.n_lkf[b] = (int)local.size(); E.n_voted[b] = n_voted; E.ref[b] = ref; E.n_lpt[b] = (int)points.size(); E.status[b] = status;
}

// ---- random small streams ----------------------------------------------------------------------------------------------------------------
static std::vector<int> distinct(int n, int nk) {
    std::vector<int> s(nk);
    for (int k = 0; k < nk; k++) s[k] = k;
    n = std::min(n, nk);
    for (int k = 0; k < n; k++) std::swap(s[k], s[rint_(k, nk - 1)]);
    s.resize(n);
    return s;
}
static void add_stream(Packed& P, bool large) {
    const int nk = large ? rint_(78, 96) : (rnd() % 25 == 0 ? 0 : rint_(1, 9)), np = nk ? (large ? rint_(80, 120) : rint_(0, 24)) : 0;
    for (int k = 0; k < nk; k++) {
        P.kf_bad.push_back(rnd() % (large ? 40 : 6) == 0);
        P.kf_parent.push_back(rnd() % 3 ? rint_(0, nk - 1) : -1); P.kf_prev.push_back(rnd() % 3 ? rint_(0, nk - 1) : -1); P.kf_next.push_back(rnd() % 3 ? rint_(0, nk - 1) : -1);
        const std::vector<int> nb = distinct(rint_(0, 10), nk), ch = distinct(rint_(0, 4), nk);
        for (int i = 0; i < 10; i++) P.covis10.push_back(i < (int)nb.size() ? nb[i] : -1);
        P.child_kf.insert(P.child_kf.end(), ch.begin(), ch.end());
        P.child_start.push_back((int)P.child_kf.size());
        for (int i = rint_(0, np ? 12 : 0); i > 0; i--) P.kp_point.push_back(rnd() % 5 ? rint_(0, np - 1) : -1);
        P.kp_start.push_back((int)P.kp_point.size());
    }
    const std::vector<int> perm = distinct(nk, nk);
    P.kf_by_key.insert(P.kf_by_key.end(), perm.begin(), perm.end());
    for (int p = 0; p < np; p++) {
        const std::vector<int> ob = distinct(large ? rint_(1, 3) : rint_(0, 5), nk);
        for (size_t o = 0; o < ob.size(); o++) P.obs.push_back((uint32_t)ob[o] | ((rnd() & 0x1ffu) << 16));     // the higher bits are ignored
        P.obs_start.push_back((int)P.obs.size());
        P.pt_bad.push_back(rnd() % 8 == 0);
    }
    std::vector<int32_t> frame;
    const int mode = (int)(rnd() % 12);
    for (int i = (np && mode ? rint_(1, large ? 110 : 16) : 0); i > 0; i--) frame.push_back(rnd() % 4 ? rint_(0, np - 1) : -1);
    if (mode == 1) for (size_t i = 0; i < frame.size(); i++) if (frame[i] >= 0 && !P.pt_bad[P.pt_start.back() + frame[i]]) frame[i] = -1;     // bad points only
    P.frames.push_back(frame);
    const std::vector<int> pv = distinct(rint_(0, nk), nk);
    P.prevs.push_back(std::vector<int32_t>(pv.begin(), pv.end()));
    P.prev_ref_kf.push_back(nk ? rint_(-1, nk - 1) : -1);
    P.batch++;
    P.kf_start.push_back((int)P.kf_bad.size()); P.pt_start.push_back((int)P.pt_bad.size());
}

static Packed make_batch(int n, int large_every = 0) {
    Packed P;
    P.kf_start.push_back(0); P.pt_start.push_back(0); P.kp_start.push_back(0); P.child_start.push_back(0); P.obs_start.push_back(0);
    for (int b = 0; b < n; b++) add_stream(P, large_every && b % large_every == large_every - 1);
    P.finish();
    return P;
}

template <class T> static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a == b; }

static void compare(const Packed& P) {
    const UlmMap M = P.map();
    Result G, E;
    G.size(M); E.size(M);
    Workspace S;
    ulm_run_host(M, S.work(M), G.out());
    for (int b = 0; b < M.batch; b++) literal_stream(M, b, E);
    if (!same(G.status, E.status)) fail("status differs from the literal loop (a valid stream refused?)");
    if (!same(G.votes, E.votes)) fail("kf_votes differ from the literal loop");
    if (!same(G.fpo, E.fpo)) fail("frame_point_out differs from the literal loop");
    if (!same(G.lkf, E.lkf) || !same(G.n_lkf, E.n_lkf) || !same(G.n_voted, E.n_voted)) fail("the local key frames differ from the literal loop");
    if (!same(G.ref, E.ref)) fail("ref_kf differs from the literal loop");
    if (!same(G.lpt, E.lpt) || !same(G.n_lpt, E.n_lpt)) fail("the local points differ from the literal loop");
    for (int b = 0; b < M.batch; b++) sum += G.n_lkf[b] * 7 + G.n_lpt[b] + G.ref[b];
}

// one stream broken in one way between two good ones: it alone is refused and writes nothing, nothing is read through the broken index
static void expect_refused(Packed P, const char* what) {
    const UlmMap M = P.map();
    Result G, E;
    G.size(M); E.size(M);
    Workspace S;
    ulm_run_host(M, S.work(M), G.out());
    if (G.status[1] != ULM_INVALID) fail(what);
    if (G.n_lkf[1] != 77 || G.n_lpt[1] != 77 || G.ref[1] != 77 || G.lkf[(size_t)M.lcap] != 77 || G.lpt[(size_t)M.pcap] != 77 || G.fpo[(size_t)M.cap] != 77) fail("a refused stream wrote more than its status");
    if (G.status[0] < 0 || G.status[2] < 0) fail("a stream beside a broken one was refused");
    literal_stream(M, 0, E); literal_stream(M, 2, E);
    for (int b = 0; b < 3; b += 2) {
        if (G.n_lkf[b] != E.n_lkf[b] || G.n_lpt[b] != E.n_lpt[b] || G.ref[b] != E.ref[b]) fail("a stream beside a broken one changed");
        for (int j = 0; j < M.lcap; j++) if (G.lkf[(size_t)b * M.lcap + j] != E.lkf[(size_t)b * M.lcap + j]) fail("a stream beside a broken one changed");
        for (int j = 0; j < M.pcap; j++) if (G.lpt[(size_t)b * M.pcap + j] != E.lpt[(size_t)b * M.pcap + j]) fail("a stream beside a broken one changed");
    }
    sum += G.status[2];
}

static void broken_snapshots() {
    for (int round = 0; round < 40; round++) {
        Packed P;
        for (;;) {
            P = make_batch(3);
            const int k0 = P.kf_start[1], nk = P.kf_start[2] - k0, p0 = P.pt_start[1];
            if (nk >= 3 && P.pt_start[2] - p0 >= 2 && P.kp_start[k0 + 1] - P.kp_start[k0] >= 1 && P.obs_start[p0 + 1] - P.obs_start[p0] >= 1 && P.child_start[k0 + 1] - P.child_start[k0] >= 1 &&
                P.frames[1].size() >= 1 && P.prevs[1].size() >= 2) break;
        }
        const int k0 = P.kf_start[1], nk = P.kf_start[2] - k0, p0 = P.pt_start[1], np = P.pt_start[2] - p0, i0 = P.kp_start[k0], o0 = P.obs_start[p0], c0 = P.child_start[k0];
        const int big = 1 << 28;
        { Packed Q = P; Q.kp_point[i0] = np; expect_refused(Q, "a point index at the end of the stream was accepted"); }
        { Packed Q = P; Q.kp_point[i0] = big; expect_refused(Q, "a point index far past the end was accepted"); }
        { Packed Q = P; Q.kp_point[i0] = -2; expect_refused(Q, "a point index below -1 was accepted"); }
        { Packed Q = P; Q.frame_point[(size_t)Q.cap] = np; expect_refused(Q, "a frame point at the end of the stream was accepted"); }
        { Packed Q = P; Q.frame_point[(size_t)Q.cap] = -big; expect_refused(Q, "a frame point far below -1 was accepted"); }
        { Packed Q = P; Q.obs[o0] = (uint32_t)nk; expect_refused(Q, "an observation slot at the end was accepted"); }
        { Packed Q = P; Q.obs[o0] |= 0xffffu; expect_refused(Q, "an observation slot past the end was accepted"); }
        { Packed Q = P; Q.kp_start[k0 + 1] = Q.kp_start[k0 + 2] + 1; expect_refused(Q, "descending keypoint offsets were accepted"); }
        { Packed Q = P; Q.kp_start[k0 + 1] = big; expect_refused(Q, "a keypoint offset past the total was accepted"); }
        { Packed Q = P; Q.obs_start[p0 + 1] = Q.obs_start[p0 + 2] + 1; expect_refused(Q, "descending observation offsets were accepted"); }
        { Packed Q = P; Q.obs_start[p0 + 1] = -big; expect_refused(Q, "a negative observation offset was accepted"); }
        { Packed Q = P; Q.child_start[k0 + 1] = Q.child_start[k0 + 2] + 1; expect_refused(Q, "descending child offsets were accepted"); }
        { Packed Q = P; Q.child_start[k0 + 1] = big; expect_refused(Q, "a child offset past the total was accepted"); }
        { Packed Q = P; Q.child_kf[c0] = nk; expect_refused(Q, "a child slot at the end was accepted"); }
        { Packed Q = P; Q.child_kf[c0] = -1; expect_refused(Q, "a negative child slot was accepted"); }
        { Packed Q = P; Q.kf_parent[k0] = nk; expect_refused(Q, "a parent outside the snapshot was accepted"); }
        { Packed Q = P; Q.kf_prev[k0 + 1] = -2; expect_refused(Q, "a prev below -1 was accepted"); }
        { Packed Q = P; Q.kf_next[k0 + 2] = big; expect_refused(Q, "a next outside the snapshot was accepted"); }
        { Packed Q = P; Q.covis10[(size_t)(k0 + 1) * 10 + 9] = nk; expect_refused(Q, "a neighbour outside the snapshot was accepted"); }
        { Packed Q = P; Q.kf_by_key[k0] = Q.kf_by_key[k0 + 1]; expect_refused(Q, "kf_by_key with a slot twice was accepted"); }
        { Packed Q = P; Q.kf_by_key[k0 + 2] = nk; expect_refused(Q, "kf_by_key with a slot out of range was accepted"); }
        { Packed Q = P; Q.kf_by_key[k0 + 2] = -big; expect_refused(Q, "kf_by_key with a negative slot was accepted"); }
        { Packed Q = P; Q.prev_lkf[(size_t)Q.lcap] = nk; expect_refused(Q, "prev_lkf with a slot out of range was accepted"); }
        { Packed Q = P; Q.prev_lkf[(size_t)Q.lcap] = Q.prev_lkf[(size_t)Q.lcap + 1]; expect_refused(Q, "prev_lkf with a slot twice was accepted"); }
        { Packed Q = P; Q.prev_ref_kf[1] = nk; expect_refused(Q, "prev_ref_kf out of range was accepted"); }
        { Packed Q = P; Q.prev_ref_kf[1] = -2; expect_refused(Q, "prev_ref_kf below -1 was accepted"); }
        { Packed Q = P; Q.frame_count[1] = Q.cap + 1; expect_refused(Q, "frame_count above cap was accepted"); }
        { Packed Q = P; Q.frame_count[1] = -1; expect_refused(Q, "a negative frame_count was accepted"); }
        { Packed Q = P; Q.prev_n_lkf[1] = nk + 1; expect_refused(Q, "more previous key frames than the stream has were accepted"); }
        { Packed Q = P; Q.prev_n_lkf[1] = -1; expect_refused(Q, "a negative prev_n_lkf was accepted"); }
    }
    // offsets of the batch level: a stream is refused together with every later one
    Packed P = make_batch(3);
    P.kf_start[2] = P.kf_start[1] - 1;
    const UlmMap M = P.map();
    Result G; G.size(M);
    Workspace S;
    ulm_run_host(M, S.work(M), G.out());
    if (G.status[0] < 0 || G.status[1] != ULM_INVALID || G.status[2] != ULM_INVALID) fail("descending key-frame offsets of the batch were accepted");
    // a nested offset at a stream boundary that falls back into an earlier stream's range: the streams on both sides of it are refused
    Packed Q;
    do { Q = make_batch(3); } while (Q.obs_start[Q.pt_start[1]] < 1 || Q.pt_start[2] == Q.pt_start[1]);
    Q.obs_start[Q.pt_start[2]] = Q.obs_start[Q.pt_start[1]] - 1;
    const UlmMap N = Q.map();
    Result H; H.size(N);
    Workspace S3;
    ulm_run_host(N, S3.work(N), H.out());
    if (H.status[0] < 0 || H.status[1] != ULM_INVALID || H.status[2] != ULM_INVALID) fail("an observation offset at a stream boundary that overlaps an earlier stream was accepted");
}

// overflow by one of each list: the needed sizes come back
static void overflows() {
    int seen_l = 0, seen_p = 0;
    for (int round = 0; round < 200 && (seen_l < 5 || seen_p < 5); round++) {
        Packed P = make_batch(1);
        const UlmMap M0 = P.map();
        Result E; E.size(M0);
        literal_stream(M0, 0, E);
        for (int which = 0; which < 2; which++) {
            const int n = which ? E.n_lpt[0] : E.n_lkf[0];
            if (n < 2 || (!which && n - 1 < P.prev_n_lkf[0])) continue;
            Packed Q = P;
            if (which) Q.pcap = n - 1; else { Q.lcap = n - 1; Q.prev_lkf.assign(P.prev_lkf.begin(), P.prev_lkf.begin() + Q.lcap); }
            const UlmMap M = Q.map();
            Result G; G.size(M);
            Workspace S;
            ulm_run_host(M, S.work(M), G.out());
            if (G.status[0] != ULM_OVERFLOW || G.n_lkf[0] != E.n_lkf[0] || G.n_lpt[0] != E.n_lpt[0]) fail("an overflow by one does not report the needed sizes");
            (which ? seen_p : seen_l)++;
        }
    }
    if (seen_l < 5 || seen_p < 5) fail("no overflow cases were made");
}

template <class T> static void read_into(std::vector<T>& v, size_t n, FILE* f) { v.resize(n); if (n && std::fread(v.data(), sizeof(T), n, f) != n) fail("short snapshot file"); }

static int time_literal(const char* path, int reps) {
    FILE* f = std::fopen(path, "rb");
    if (!f) fail("cannot open the snapshot file");
    int32_t h[9];
    if (std::fread(h, 4, 9, f) != 9) fail("short snapshot file");
    Packed P;
    const size_t nb = h[0], nk = h[1], nc = h[2], ni = h[3], np = h[4], no = h[5];
    P.batch = h[0]; P.cap = h[6]; P.lcap = h[7]; P.pcap = h[8];
    read_into(P.kf_start, nb + 1, f); read_into(P.kf_bad, nk, f); read_into(P.kf_parent, nk, f); read_into(P.kf_prev, nk, f); read_into(P.kf_next, nk, f);
    read_into(P.covis10, nk * 10, f); read_into(P.child_start, nk + 1, f); read_into(P.child_kf, nc, f); read_into(P.kf_by_key, nk, f);
    read_into(P.kp_start, nk + 1, f); read_into(P.kp_point, ni, f); read_into(P.pt_start, nb + 1, f); read_into(P.pt_bad, np, f); read_into(P.obs_start, np + 1, f);
    read_into(P.obs, no, f); read_into(P.frame_point, nb * P.cap, f); read_into(P.frame_count, nb, f); read_into(P.prev_lkf, nb * P.lcap, f);
    read_into(P.prev_n_lkf, nb, f); read_into(P.prev_ref_kf, nb, f);
    std::fclose(f);
    const UlmMap M = P.map();
    Result E, G; E.size(M); G.size(M);
    double best = 1e300, best_core = 1e300;
    for (int r = 0; r < reps; r++) {
        g_loop_ms = 0;
        for (int b = 0; b < M.batch; b++) literal_stream(M, b, E);
        best = std::min(best, g_loop_ms);
        Workspace S; const UlmWork W = S.work(M);
        const auto t1 = std::chrono::steady_clock::now();
        ulm_run_host(M, W, G.out());
        best_core = std::min(best_core, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    }
    if (!same(G.lkf, E.lkf) || !same(G.lpt, E.lpt) || !same(G.status, E.status)) fail("the flat form differs from the literal loop on the snapshot");
    long long lk = 0, lp = 0, nv = 0;
    for (int b = 0; b < M.batch; b++) { lk += E.n_lkf[b]; lp += E.n_lpt[b]; nv += E.n_voted[b]; }
    std::printf("{\"streams\": %d, \"literal_loop_ms\": %.3f, \"flat_core_one_thread_ms\": %.3f, \"voted_per_stream\": %.1f, \"local_key_frames_per_stream\": %.1f, \"local_points_per_stream\": %.1f}\n",
                M.batch, best, best_core, (double)nv / M.batch, (double)lk / M.batch, (double)lp / M.batch);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "time")) return time_literal(argv[2], argc >= 4 ? std::atoi(argv[3]) : 3);
    long long streams = 0;
    for (int round = 0; round < 110; round++) {
        const Packed P = make_batch(rint_(1, 60), 15);
        streams += P.batch;
        compare(P);
    }
    const Seen& s = g_seen;
    if (streams < 3000) fail("fewer than 3000 random streams");
    if (s.no_votes < 1) fail("the random streams hold no case without votes");
    if (s.tie < 1) fail("the random streams hold no tie for the most votes");
    if (s.limit_break < 1) fail("the random streams never break at more than 80 entries");
    if (s.bad_neighbour < 1) fail("the random streams never skip a bad neighbour");
    if (s.first_occurrence < 1) fail("the random streams never drop a point that an earlier key frame holds");
    const Seen before = g_seen;
    broken_snapshots();
    overflows();
    std::printf("checksum %lld streams %lld no-votes %lld tie %lld limit-break %lld skipped-bad-neighbour %lld first-occurrence %lld all-voted-bad %lld\n", sum, streams, before.no_votes,
                before.tie, before.limit_break, before.bad_neighbour, before.first_occurrence, before.all_bad);
    return 0;
}
