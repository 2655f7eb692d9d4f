// tests/cpp/culling_core_host_test.cpp — the host build of viorb_amd/csrc/culling_core.h as a stand-alone program. No GPU, no library:
// only the header.
//   culling_core_host_test                    the self-test that tests/test_culling_host_sanitized.py compiles with
//                                             -fsanitize=address,undefined and runs as a child process: cull_run_host (validate, prepare,
//                                             ordered phase) against the literal loop below on a few thousand random small streams,
//                                             and every kind of broken snapshot, which the validator must refuse without reading through it.
//                                             Prints one checksum line.
//   culling_core_host_test time FILE [reps]   the literal loop (one thread) timed on a packed snapshot that tools/culling_time.py writes:
//                                             6 totals and the monocular flag as int32, then the arrays of viorb_cull_map in their order.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "culling_core.h"

using namespace viorb;

static long long sum = 0;
static unsigned rng_state = 97531u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rint_(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }
static void fail(const char* what) { std::printf("FAILED: %s\n", what); std::exit(2); }

// a packed batch with exactly sized arrays, so that the address sanitizer sees any read past an end
struct Packed {
    int batch = 0;
    std::vector<int32_t> kf_start, kf_prev, kf_next, cur_kf, cand_start, cand_kf, kp_start, kp_point, pt_start, pt_nobs, obs_start;
    std::vector<uint8_t> kf_flags, vins, kp_octave, pt_bad;
    std::vector<double> kf_time;
    std::vector<float> th, kp_depth;
    std::vector<uint32_t> obs;
    CullMap map() const {
        CullMap M;
        M.batch = batch; M.n_kf = (int)kf_flags.size(); M.n_cand = (int)cand_kf.size(); M.n_kp = (int)kp_point.size(); M.n_pt = (int)pt_nobs.size(); M.n_obs = (int)obs.size();
        M.kf_start = kf_start.data(); M.kf_flags = kf_flags.data(); M.kf_time = kf_time.data(); M.kf_prev = kf_prev.data(); M.kf_next = kf_next.data();
        M.cur_kf = cur_kf.data(); M.vins_inited = vins.data(); M.th_depth = th.data();
        M.cand_start = cand_start.data(); M.cand_kf = cand_kf.data(); M.kp_start = kp_start.data(); M.kp_point = kp_point.data(); M.kp_octave = kp_octave.data();
        M.kp_depth = kp_depth.data(); M.pt_start = pt_start.data(); M.pt_nobs = pt_nobs.data(); M.pt_bad = pt_bad.data(); M.obs_start = obs_start.data(); M.obs = obs.data();
        return M;
    }
};

struct Result {
    std::vector<int32_t> reason, red, mps, recounted, order, n_culled, status, prev, next, nobs;
    std::vector<uint8_t> bad, tbe, repreint, pt_bad, alive;
    void size(const CullMap& M) {
        reason.assign(M.n_cand, 77); red = mps = recounted = order = reason; n_culled.assign(M.batch, 77); status = n_culled;
        prev.assign(M.n_kf, 77); next = prev; bad.assign(M.n_kf, 77); tbe = repreint = bad; nobs.assign(M.n_pt, 77); pt_bad.assign(M.n_pt, 77); alive.assign(M.n_obs, 77);
    }
    CullOut out() {
        CullOut R;
        R.cand_reason = reason.data(); R.cand_redundant = red.data(); R.cand_mps = mps.data(); R.cand_recounted = recounted.data(); R.culled_order = order.data();
        R.n_culled = n_culled.data(); R.status = status.data(); R.kf_bad = bad.data(); R.kf_to_be_erased = tbe.data(); R.kf_prev_out = prev.data();
        R.kf_next_out = next.data(); R.kf_repreint = repreint.data(); R.pt_nobs_out = nobs.data(); R.pt_bad_out = pt_bad.data(); R.obs_alive = alive.data();
        return R;
    }
};

struct Workspace {
    std::vector<int32_t> pt, cok, prev, next, ok; std::vector<uint32_t> obs; std::vector<uint8_t> kst;
    CullWork work(const CullMap& M) {
        pt.assign(M.n_pt, 0); obs.assign(M.n_obs, 0); cok.assign(M.n_kf, 0); prev = next = cok; kst.assign(M.n_kf, 0); ok.assign(M.batch, 0);
        CullWork W;
        W.pt = pt.data(); W.obs = obs.data(); W.cand_of_kf = cok.data(); W.prev = prev.data(); W.next = next.data(); W.kf_state = kst.data();
        W.ok = ok.data();
        return W;
    }
};

// ---- the literal loop: objects, std::map observations, in-place mutation (src/LocalMapping.cc:1694-1821, KeyFrame.cc:744-882, MapPoint.cc:118-175)
struct LObs { int octave; bool stereo; int index; };
struct LPoint { int nObs; bool bad; std::map<int, LObs> obs; };
struct LKeyFrame { int flags; double t; int prev, next; bool bad, tbe, repreint; std::vector<int> pts, octave; std::vector<float> depth; };

static double g_loop_ms = 0;          // the time inside the candidate loop alone (the objects exist already in the reference)

static void literal_stream(const CullMap& M, int b, bool mono, Result& E) {
    const int k0 = M.kf_start[b], nk = M.kf_start[b + 1] - k0, c0 = M.cand_start[b], nc = M.cand_start[b + 1] - c0, p0 = M.pt_start[b], np = M.pt_start[b + 1] - p0;
    std::vector<LKeyFrame> kf(nk);
    std::vector<LPoint> pt(np);
    for (int k = 0; k < nk; k++) kf[k] = LKeyFrame{M.kf_flags[k0 + k], M.kf_time[k0 + k], M.kf_prev[k0 + k], M.kf_next[k0 + k], false, false, false, {}, {}, {}};
    for (int p = 0; p < np; p++) {
        pt[p].nObs = M.pt_nobs[p0 + p]; pt[p].bad = M.pt_bad[p0 + p] != 0;
        for (int o = M.obs_start[p0 + p]; o < M.obs_start[p0 + p + 1]; o++) pt[p].obs[(int)(M.obs[o] & 0xffffu)] = LObs{(int)((M.obs[o] >> 16) & 0xffu), (M.obs[o] & (1u << 24)) != 0, o};
    }
    for (int j = 0; j < nc; j++) {
        LKeyFrame& K = kf[M.cand_kf[c0 + j]];
        for (int i = M.kp_start[c0 + j]; i < M.kp_start[c0 + j + 1]; i++) { K.pts.push_back(M.kp_point[i]); K.octave.push_back(M.kp_octave[i]); K.depth.push_back(mono ? 0.f : M.kp_depth[i]); }
    }
    const int cur = M.cur_kf[b];
    int n_culled = 0;
    const auto loop_t0 = std::chrono::steady_clock::now();
    for (int j = 0; j < nc; j++) {
        const int c = M.cand_kf[c0 + j];
        LKeyFrame& K = kf[c];
        E.red[c0 + j] = 0; E.mps[c0 + j] = 0;
        if (K.flags & 1) { E.reason[c0 + j] = KFC_FIRST_KF; continue; }
        if (K.prev >= 0 && K.next >= 0 && !M.vins_inited[b]) { if (std::fabs(kf[K.next].t - kf[K.prev].t) > 0.5) { E.reason[c0 + j] = KFC_TIME_GAP; continue; } }
        if (K.next == cur) { E.reason[c0 + j] = KFC_BEFORE_CURRENT; continue; }
        if (K.t >= kf[cur].t - 0.2) { E.reason[c0 + j] = KFC_RECENT; continue; }
        const int thObs = 3;
        int nRedundantObservations = 0, nMPs = 0;
        for (size_t i = 0; i < K.pts.size(); i++) {
            if (K.pts[i] < 0) continue;
            LPoint& P = pt[K.pts[i]];
            if (P.bad) continue;
            if (!mono) { if (K.depth[i] > M.th_depth[b] || K.depth[i] < 0) continue; }
            nMPs++;
            if (P.nObs > thObs) {
                int nObs = 0;
                for (std::map<int, LObs>::const_iterator mit = P.obs.begin(); mit != P.obs.end(); ++mit) {
                    if (mit->first == c) continue;
                    if (mit->second.octave <= K.octave[i] + 1) { nObs++; if (nObs >= thObs) break; }
                }
                if (nObs >= thObs) nRedundantObservations++;
            }
        }
        E.red[c0 + j] = nRedundantObservations; E.mps[c0 + j] = nMPs;
        E.reason[c0 + j] = KFC_KEPT;
        if (nRedundantObservations > 0.9 * nMPs) {                   // SetBadFlag()
            if (K.flags & 2) { K.tbe = true; E.reason[c0 + j] = KFC_DEFERRED; continue; }
            for (size_t i = 0; i < K.pts.size(); i++) {
                if (K.pts[i] < 0) continue;
                LPoint& P = pt[K.pts[i]];                            // EraseObservation(this)
                std::map<int, LObs>::iterator it = P.obs.find(c);
                if (it == P.obs.end()) continue;
                P.nObs -= it->second.stereo ? 2 : 1;
                P.obs.erase(it);
                if (P.nObs <= 2) { P.bad = true; P.obs.clear(); }
            }
            K.bad = true;
            const int pv = K.prev, nx = K.next;
            if (pv >= 0) kf[pv].next = nx;
            if (nx >= 0) kf[nx].prev = pv;
            K.prev = K.next = -1;
            if (pv >= 0 && nx >= 0) kf[nx].repreint = true;
            E.reason[c0 + j] = KFC_CULLED; E.order[c0 + n_culled++] = j;
        }
    }
    g_loop_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - loop_t0).count();
    for (int j = n_culled; j < nc; j++) E.order[c0 + j] = -1;
    E.n_culled[b] = n_culled; E.status[b] = 0;
    for (int k = 0; k < nk; k++) { E.bad[k0 + k] = kf[k].bad; E.tbe[k0 + k] = kf[k].tbe; E.repreint[k0 + k] = kf[k].repreint; E.prev[k0 + k] = kf[k].prev; E.next[k0 + k] = kf[k].next; }
    for (int p = 0; p < np; p++) {
        E.nobs[p0 + p] = pt[p].nObs; E.pt_bad[p0 + p] = pt[p].bad;
        for (int o = M.obs_start[p0 + p]; o < M.obs_start[p0 + p + 1]; o++) E.alive[o] = 0;
        for (std::map<int, LObs>::const_iterator mit = pt[p].obs.begin(); mit != pt[p].obs.end(); ++mit) E.alive[mit->second.index] = 1;
    }
}

// ---- random small streams ----------------------------------------------------------------------------------------------------------------
static void add_stream(Packed& P) {
    const int nk = rint_(2, 9), np = rint_(0, 24), k0 = (int)P.kf_flags.size();
    double t = 10.0;
    for (int k = 0; k < nk; k++) {
        t += (rnd() % 5 == 0) ? 0.35 : 0.04 * rint_(1, 4);
        P.kf_flags.push_back((uint8_t)((k == 0 && rnd() % 2 ? 1 : 0) | (rnd() % 6 == 0 ? 2 : 0)));
        P.kf_time.push_back(t); P.kf_prev.push_back(k - 1); P.kf_next.push_back(k + 1 < nk ? k + 1 : -1);
    }
    P.kf_time[k0 + nk - 1] += 0.3 * rint_(0, 3);
    P.cur_kf.push_back(nk - 1); P.vins.push_back(rnd() % 2); P.th.push_back(40.f);
    std::vector<std::vector<int>> seen(nk);
    for (int p = 0; p < np; p++) {
        int n = 0;
        const int base = rint_(0, 7), want = rint_(0, nk < 6 ? nk : 6);
        std::vector<int> slots(nk);
        for (int k = 0; k < nk; k++) slots[k] = k;
        for (int k = 0; k < want; k++) {
            const int pick = rint_(k, nk - 1);
            std::swap(slots[k], slots[pick]);
            const bool stereo = rnd() % 3 == 0;
            int oc = base + (rnd() % 3 == 0 ? rint_(-2, 2) : 0);
            oc = oc < 0 ? 0 : oc > 7 ? 7 : oc;
            P.obs.push_back(snap_obs_pack(slots[k], oc, stereo));
            seen[slots[k]].push_back(p);
            n += stereo ? 2 : 1;
        }
        P.obs_start.push_back((int)P.obs.size());
        P.pt_nobs.push_back(rnd() % 10 == 0 ? n + rint_(-1, 1) : n);
        P.pt_bad.push_back(rnd() % 20 == 0);
    }
    std::vector<int> order(nk - 1);
    for (int k = 0; k < nk - 1; k++) order[k] = k;
    for (int k = nk - 2; k > 0; k--) std::swap(order[k], order[rint_(0, k)]);
    const int nc = rint_(0, nk - 1);
    for (int j = 0; j < nc; j++) {
        const int c = order[j];
        P.cand_kf.push_back(c);
        for (size_t q = 0; q < seen[c].size(); q++) {
            if (rnd() % 5 == 0) continue;
            P.kp_point.push_back(seen[c][q]); P.kp_octave.push_back((uint8_t)rint_(0, 7)); P.kp_depth.push_back(rnd() % 8 == 0 ? 41.f : rnd() % 9 == 0 ? -1.f : 5.f);
            if (rnd() % 6 == 0) { P.kp_point.push_back(rnd() % 2 && np ? rint_(0, np - 1) : -1); P.kp_octave.push_back((uint8_t)rint_(0, 7)); P.kp_depth.push_back(5.f); }
        }
        P.kp_start.push_back((int)P.kp_point.size());
    }
    P.batch++;
    P.kf_start.push_back((int)P.kf_flags.size()); P.cand_start.push_back((int)P.cand_kf.size()); P.pt_start.push_back((int)P.pt_nobs.size());
}

static Packed make_batch(int n) {
    Packed P;
    P.kf_start.push_back(0); P.cand_start.push_back(0); P.pt_start.push_back(0); P.kp_start.push_back(0); P.obs_start.push_back(0);
    for (int b = 0; b < n; b++) add_stream(P);
    return P;
}

template <class T> static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a == b; }

static void compare(const Packed& P, bool mono, long long& culls, long long& changed) {
    const CullMap M = P.map();
    Result G, E;
    G.size(M); E.size(M);
    Workspace S;
    cull_run_host(M, S.work(M), G.out(), mono);
    for (int b = 0; b < M.batch; b++) literal_stream(M, b, mono, E);
    if (!same(G.status, E.status)) fail("a valid stream was refused");
    if (!same(G.reason, E.reason)) fail("cand_reason differs from the literal loop");
    if (!same(G.red, E.red) || !same(G.mps, E.mps)) fail("cand_redundant / cand_mps differ from the literal loop");
    if (!same(G.order, E.order) || !same(G.n_culled, E.n_culled)) fail("culled_order / n_culled differ from the literal loop");
    if (!same(G.bad, E.bad) || !same(G.tbe, E.tbe) || !same(G.repreint, E.repreint)) fail("key-frame flags differ from the literal loop");
    if (!same(G.prev, E.prev) || !same(G.next, E.next)) fail("links differ from the literal loop");
    if (!same(G.nobs, E.nobs) || !same(G.pt_bad, E.pt_bad) || !same(G.alive, E.alive)) fail("point state differs from the literal loop");
    // how many candidates the order matters for: their counts differ from those of a stream in which nothing was culled before them
    for (int b = 0; b < M.batch; b++)
        for (int j = M.cand_start[b]; j < M.cand_start[b + 1]; j++) {
            if (G.reason[j] < KFC_KEPT) continue;
            CullStream St = cull_stream(M, b);
            Workspace S2; const CullWork W2 = S2.work(M);
            cull_prepare(M, St, W2, 0, 1);
            int mps = 0, red = 0;
            for (int i = M.kp_start[j]; i < M.kp_start[j + 1]; i++) { const int r = cull_count_keypoint(M, St, W2, M.cand_kf[j], i, mono, M.th_depth[b]); mps += r & 1; red += (r >> 1) & 1; }
            changed += mps != G.mps[j] || red != G.red[j];
        }
    for (size_t j = 0; j < G.reason.size(); j++) {
        const bool counted = G.reason[j] >= KFC_KEPT;
        if (counted != (G.recounted[j] != 0)) fail("cand_recounted is not 1 exactly for the counted candidates");
        culls += G.reason[j] == KFC_CULLED;
        sum += G.reason[j] * 7 + G.red[j] + G.mps[j];
    }
}

// one stream broken in one way between two good ones: it alone is refused, nothing is read through the broken index
static void expect_refused(Packed P, const char* what) {
    const CullMap M = P.map();
    Result G, E;
    G.size(M); E.size(M);
    Workspace S;
    cull_run_host(M, S.work(M), G.out(), true);
    if (G.status[1] != -1 || G.n_culled[1] != 0) fail(what);
    if (G.status[0] != 0) fail("the stream before a broken one was refused");
    literal_stream(M, 0, true, E);
    for (int j = M.cand_start[0]; j < M.cand_start[1]; j++) if (G.reason[j] != E.reason[j]) fail("the stream before a broken one changed");
    sum += G.status[2];
}

static void broken_snapshots() {
    for (int round = 0; round < 40; round++) {
        Packed P;
        do { P = make_batch(3); } while (P.cand_start[2] - P.cand_start[1] < 2 || P.pt_start[2] - P.pt_start[1] < 2 || P.kp_start[P.cand_start[2]] - P.kp_start[P.cand_start[1]] < 1 ||
                                         P.obs_start[P.pt_start[2]] - P.obs_start[P.pt_start[1]] < 1);
        const int c0 = P.cand_start[1], p0 = P.pt_start[1], k0 = P.kf_start[1], i0 = P.kp_start[c0], o0 = P.obs_start[p0];
        const int big = 1 << 28;
        { Packed Q = P; Q.kp_point[i0] = Q.pt_start[2] - p0; expect_refused(Q, "a point index at the end of the stream was accepted"); }
        { Packed Q = P; Q.kp_point[i0] = big; expect_refused(Q, "a point index far past the end was accepted"); }
        { Packed Q = P; Q.kp_point[i0] = -2; expect_refused(Q, "a point index below -1 was accepted"); }
        { Packed Q = P; Q.obs[o0] = (Q.obs[o0] & ~0xffffu) | (uint32_t)(Q.kf_start[2] - k0); expect_refused(Q, "an observation slot at the end was accepted"); }
        { Packed Q = P; Q.obs[o0] |= 0xffffu; expect_refused(Q, "an observation slot past the end was accepted"); }
        { Packed Q = P; Q.kp_start[c0 + 1] = Q.kp_start[c0 + 2] + 1; expect_refused(Q, "descending keypoint offsets were accepted"); }
        { Packed Q = P; Q.kp_start[c0 + 1] = big; expect_refused(Q, "a keypoint offset past the total was accepted"); }
        { Packed Q = P; Q.obs_start[p0 + 1] = Q.obs_start[p0 + 2] + 1; expect_refused(Q, "descending observation offsets were accepted"); }
        { Packed Q = P; Q.obs_start[p0 + 1] = -big; expect_refused(Q, "a negative observation offset was accepted"); }
        { Packed Q = P; Q.kf_prev[k0 + Q.cand_kf[c0]] = Q.kf_start[2] - k0; expect_refused(Q, "a candidate whose prev lies outside the snapshot was accepted"); }
        { Packed Q = P; Q.kf_next[k0 + Q.cand_kf[c0]] = -2; expect_refused(Q, "a candidate whose next is below -1 was accepted"); }
        { Packed Q = P; Q.cur_kf[1] = Q.kf_start[2] - k0; expect_refused(Q, "cur_kf out of range was accepted"); }
        { Packed Q = P; Q.cur_kf[1] = -1; expect_refused(Q, "a negative cur_kf was accepted"); }
        { Packed Q = P; Q.cand_kf[c0] = big; expect_refused(Q, "a candidate slot past the end was accepted"); }
        { Packed Q = P; Q.pt_nobs[p0] = 1 << 30; expect_refused(Q, "an observation count of 2^30 was accepted"); }
        { Packed Q = P; Q.cand_kf[c0 + 1] = Q.cand_kf[c0]; expect_refused(Q, "a candidate listed twice was accepted"); }
    }
    // offsets of the batch level: a stream is refused together with every later one
    Packed P = make_batch(3);
    P.kf_start[2] = P.kf_start[1] - 1;
    const CullMap M = P.map();
    Result G; G.size(M);
    Workspace S;
    cull_run_host(M, S.work(M), G.out(), true);
    if (G.status[0] != 0 || G.status[1] != -1 || G.status[2] != -1) fail("descending key-frame offsets of the batch were accepted");
    // a nested offset at a stream boundary that falls back into an earlier stream's range: the streams on both sides of it are refused,
    // so no two accepted streams share observation words
    Packed Q;
    do { Q = make_batch(3); } while (Q.obs_start[Q.pt_start[1]] < 1 || Q.pt_start[2] == Q.pt_start[1]);
    Q.obs_start[Q.pt_start[2]] = Q.obs_start[Q.pt_start[1]] - 1;
    const CullMap N = Q.map();
    Result H; H.size(N);
    Workspace S3;
    cull_run_host(N, S3.work(N), H.out(), true);
    if (H.status[0] != 0 || H.status[1] != -1 || H.status[2] != -1) fail("an observation offset at a stream boundary that overlaps an earlier stream was accepted");
}

template <class T> static void read_into(std::vector<T>& v, size_t n, FILE* f) { v.resize(n); if (n && std::fread(v.data(), sizeof(T), n, f) != n) fail("short snapshot file"); }

static int time_literal(const char* path, int reps) {
    FILE* f = std::fopen(path, "rb");
    if (!f) fail("cannot open the snapshot file");
    int32_t h[8];
    if (std::fread(h, 4, 8, f) != 8) fail("short snapshot file");
    Packed P;
    const size_t nb = h[0], nk = h[1], nc = h[2], ni = h[3], np = h[4], no = h[5];
    const bool mono = h[6] != 0;
    P.batch = h[0];
    read_into(P.kf_start, nb + 1, f); read_into(P.kf_flags, nk, f); read_into(P.kf_time, nk, f); read_into(P.kf_prev, nk, f); read_into(P.kf_next, nk, f);
    read_into(P.cur_kf, nb, f); read_into(P.vins, nb, f); read_into(P.th, nb, f); read_into(P.cand_start, nb + 1, f); read_into(P.cand_kf, nc, f);
    read_into(P.kp_start, nc + 1, f); read_into(P.kp_point, ni, f); read_into(P.kp_octave, ni, f); read_into(P.kp_depth, ni, f); read_into(P.pt_start, nb + 1, f);
    read_into(P.pt_nobs, np, f); read_into(P.pt_bad, np, f); read_into(P.obs_start, np + 1, f); read_into(P.obs, no, f);
    std::fclose(f);
    const CullMap M = P.map();
    Result E, G; E.size(M); G.size(M);
    double best = 1e300, best_core = 1e300;
    for (int r = 0; r < reps; r++) {
        g_loop_ms = 0;
        for (int b = 0; b < M.batch; b++) literal_stream(M, b, mono, E);
        best = std::min(best, g_loop_ms);
        Workspace S; const CullWork W = S.work(M);
        const auto t1 = std::chrono::steady_clock::now();
        cull_run_host(M, W, G.out(), mono);
        best_core = std::min(best_core, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    }
    long long culled = 0;
    for (int b = 0; b < M.batch; b++) culled += E.n_culled[b];
    if (!same(G.reason, E.reason) || !same(G.nobs, E.nobs)) fail("the flat form differs from the literal loop on the snapshot");
    std::printf("{\"streams\": %d, \"literal_loop_ms\": %.3f, \"flat_core_one_thread_ms\": %.3f, \"culled\": %lld}\n", M.batch, best, best_core, culled);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "time")) return time_literal(argv[2], argc >= 4 ? std::atoi(argv[3]) : 3);
    long long culls = 0, changed = 0, streams = 0;
    for (int round = 0; round < 130; round++) {
        const Packed P = make_batch(rint_(1, 60));
        streams += P.batch;
        for (int mono = 0; mono < 2; mono++) compare(P, mono != 0, culls, changed);
    }
    if (streams < 3000 || culls < 800 || changed < 50) { std::printf("streams %lld culls %lld changed %lld\n", streams, culls, changed); fail("the random streams do not exercise the loop"); }
    broken_snapshots();
    if (cull_map_point(0, 1, 4, 0, 9, 0, true) != MPC_KEEP || cull_map_point(0, 4194303, 16777213, 0, 9, 0, true) != MPC_CULL_FOUND_RATIO) fail("map-point code");
    std::printf("checksum %lld streams %lld culls %lld candidates that an earlier cull changed %lld\n", sum, streams, culls, changed);
    return 0;
}
