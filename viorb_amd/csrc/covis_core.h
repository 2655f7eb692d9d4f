// viorb_amd/csrc/covis_core.h — KeyFrame::UpdateConnections for an ordered list of targets, shared by the HIP kernels of covisibility.hip
// and by the host (tests/cpp/covis_core_host_test.cpp drives this header alone, under the address and undefined-behaviour sanitizers,
// against the literal loop).
//
// What is restated (reference file:line):
//   KeyFrame::UpdateConnections      src/KeyFrame.cc:580-670  (votes :593-611, the early return :614, nmax / pKFmax and the threshold
//                                                              :619-643, the sort :645-652, the target's members :658-667)
//   KeyFrame::AddConnection          src/KeyFrame.cc:414-427, UpdateBestCovisibles :429-448, AddChild :672-676
//   LoopClosing::CorrectLoop         src/LoopClosing.cc:574-590 (LoopConnections)
// Everything is integer arithmetic. The working state is the result's rows: [n_kf][ccap] of (slot, weight) for mConnectedKeyFrameWeights
// in ascending key order and for the ordered list, with their counts. sort(pair<int, KeyFrame*>) followed by push_front is a descending
// order of (weight, key); the keys of a row are distinct, so the order is total and a rank sort reproduces it whatever the schedule.
#pragma once
#include <stdint.h>
#include "map_snapshot_core.h"      // the snapshot's layout, its observation word, the validator's checks, the memory shim

namespace viorb {

enum { COV_OK = 0, COV_OVERFLOW = 1, COV_INVALID = -1 };              // status (VIORB_COVIS_OVERFLOW of include/viorb_covisibility.h)
enum { COV_TH = 15, COV_KF_ID0 = 1, COV_KF_FIRST = 2, COV_MAP_CHANGED = 1, COV_ORD_REBUILT = 2 };
enum { COV_C_N = 0, COV_C_MAX_KF = 1, COV_C_MAX_W = 2, COV_C_ADDED = 3, COV_C = 4 };      // cinfo[target][4]: the counter's size, pKFmax, nmax, vPairs.size()

// The snapshot (viorb_covis_map with the row length and erase_targets), the working state (the workspace; host: plain arrays) and the result
struct CovMap {
    int batch, n_kf, n_kp, n_pt, n_obs, n_conn, n_ord, n_target;
    const int32_t* kf_start; const int32_t* kf_by_key; const uint8_t* kf_flags; const int32_t* kf_parent;
    const int32_t* kp_start; const int32_t* kp_point;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* obs_start; const uint32_t* obs;
    const int32_t* conn_start; const int32_t* conn_kf; const int32_t* conn_w;
    const int32_t* ord_start; const int32_t* ord_kf; const int32_t* ord_w;
    const int32_t* target_start; const int32_t* target_kf;
    int ccap, erase_targets;
};
struct CovWork {
    int32_t* rank;                       // [n_kf]: a slot's key position, the inverse of kf_by_key (the permutation check's marks)
    int32_t* flags;                      // [n_kf]: kf_flags as the ordered loop changes them
    int32_t* mark;                       // [n_kf]: bit 0 = a target of the stream, higher bits = the ordinal + 1 of the target whose previous ordered list holds the slot (device: LDS while a stream's key frames fit)
    int32_t* votes;                      // [vote groups][n_kf]: KFcounter by slot, one array per concurrent target of a stream (device: LDS while they fit)
    int32_t* ckf; int32_t* cw;           // [n_target][ccap]: KFcounter of every target in key order, the first ccap entries
    int32_t* cinfo;                      // [n_target][COV_C]
    int32_t* info;                       // [batch]: accepted
};
struct CovOut {
    int32_t* conn_kf_out; int32_t* conn_w_out; int32_t* conn_n_out; int32_t* ord_kf_out; int32_t* ord_w_out; int32_t* ord_n_out; int32_t* status;
    int32_t* need; int32_t* kf_parent_out; uint8_t* kf_flags_out; uint8_t* kf_touched;
    int32_t* t_observers; int32_t* t_max_kf; int32_t* t_max_w; int32_t* t_added; int32_t* t_parent; int32_t* loop_conn; int32_t* n_loop_conn;
};

// ---- the stream validator: the steps of map_snapshot_core.h on this snapshot's arrays ----------------------------------------------------
// Step 1: kp_start, conn_start and ord_start are nested under kf_start, obs_start under pt_start; target_start is a batch-level array.
VIORB_HD bool cov_validate_ranges(const CovMap& M, int b, int tid, int nt) {
    bool ok = true;
    for (int i = tid; i <= b; i += nt) {
        if (!(snap_span(M.kf_start, i, i + 1, M.n_kf) && snap_span(M.pt_start, i, i + 1, M.n_pt) && snap_span(M.target_start, i, i + 1, M.n_target))) { ok = false; continue; }
        const int k0 = M.kf_start[i], k1 = M.kf_start[i + 1];
        ok = ok && snap_span(M.kp_start, k0, k1, M.n_kp) && snap_span(M.conn_start, k0, k1, M.n_conn) && snap_span(M.ord_start, k0, k1, M.n_ord);
        ok = ok && snap_span(M.obs_start, M.pt_start[i], M.pt_start[i + 1], M.n_obs);
    }
    return ok;
}
// Step 2: the nested offsets, the length of every input row, every key frame's parent and its entry of kf_by_key, the targets.
VIORB_HD bool cov_validate_offsets(const CovMap& M, const SnapStream& S, int b, int tid, int nt) {
    bool ok = S.nk <= SNAP_MAX_KF;
    ok &= snap_offsets_run(M.kp_start, S.k0, S.nk, M.n_kp, tid, nt);
    ok &= snap_offsets_run(M.conn_start, S.k0, S.nk, M.n_conn, tid, nt);
    ok &= snap_offsets_run(M.ord_start, S.k0, S.nk, M.n_ord, tid, nt);
    ok &= snap_offsets_run(M.obs_start, S.p0, S.np, M.n_obs, tid, nt);
    for (int k = tid; k < S.nk; k += nt) {
        const int g = S.k0 + k, key = M.kf_by_key[g];
        ok &= snap_slot_or_none(M.kf_parent[g], S.nk) && key >= 0 && key < S.nk;
        ok &= (long long)M.conn_start[g + 1] - M.conn_start[g] <= M.ccap && (long long)M.ord_start[g + 1] - M.ord_start[g] <= M.ccap;
    }
    ok &= snap_entries_within(M.target_kf, M.target_start[b], M.target_start[b + 1], 0, S.nk, tid, nt);
    return ok;
}
// Step 3: every slot of the rows and of the observations, and every point index of the targets' keypoint ranges (the only ones read).
VIORB_HD bool cov_validate_entries(const CovMap& M, const SnapStream& S, int b, int tid, int nt) {
    bool ok = snap_entries_within(M.conn_kf, M.conn_start[S.k0], M.conn_start[S.k0 + S.nk], 0, S.nk, tid, nt);
    ok &= snap_entries_within(M.ord_kf, M.ord_start[S.k0], M.ord_start[S.k0 + S.nk], 0, S.nk, tid, nt);
    ok &= snap_obs_slots_below(M.obs, M.obs_start[S.p0], M.obs_start[S.p0 + S.np], S.nk, tid, nt);
    for (int t = M.target_start[b], e = M.target_start[b + 1]; t < e; t++) {
        const int g = S.k0 + M.target_kf[t];
        ok &= snap_entries_within(M.kp_point, M.kp_start[g], M.kp_start[g + 1], -1, S.np, tid, nt);
    }
    return ok;
}
// Step 4 is snap_distinct_fill / snap_distinct_check of kf_by_key on rank[], which leaves rank = the inverse permutation. Step 5, the rows:
// the key frame whose row holds flat entry e of a CSR array (start[k0 .. k0 + nk] ascending, start[k0] <= e < start[k0 + nk])
VIORB_HD int cov_row_of(const int32_t* start, int k0, int nk, int e) {
    int lo = 0, hi = nk;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (start[k0 + mid] <= e) lo = mid; else hi = mid; }
    return lo;
}
// every conn row ascends strictly in key rank (so its slots are distinct) and does not name its own key frame; no ord row names a slot twice
VIORB_HD bool cov_validate_rows(const CovMap& M, const SnapStream& S, const int32_t* rank, int tid, int nt) {
    bool ok = true;
    for (int e = M.conn_start[S.k0] + tid, e1 = M.conn_start[S.k0 + S.nk]; e < e1; e += nt) {
        const int k = cov_row_of(M.conn_start, S.k0, S.nk, e), s = M.conn_kf[e];
        ok &= s != k;
        if (e > M.conn_start[S.k0 + k]) ok &= rank[M.conn_kf[e - 1]] < rank[s];
    }
    for (int e = M.ord_start[S.k0] + tid, e1 = M.ord_start[S.k0 + S.nk]; e < e1; e += nt) {
        const int k = cov_row_of(M.ord_start, S.k0, S.nk, e), s = M.ord_kf[e];
        for (int j = M.ord_start[S.k0 + k]; j < e; j++) ok &= M.ord_kf[j] != s;
    }
    return ok;
}
// The working state of an accepted stream: the output rows hold the input rows, -1 behind them
VIORB_HD void cov_copy_rows(const CovMap& M, const SnapStream& S, const CovWork& W, const CovOut& R, int tid, int nt) {
    for (long long x = tid, n = (long long)S.nk * M.ccap; x < n; x += nt) {
        const int k = (int)(x / M.ccap), i = (int)(x % M.ccap), g = S.k0 + k;
        const int c0 = M.conn_start[g], cn = M.conn_start[g + 1] - c0, o0 = M.ord_start[g], on = M.ord_start[g + 1] - o0;
        const size_t at = (size_t)g * M.ccap + i;
        R.conn_kf_out[at] = i < cn ? M.conn_kf[c0 + i] : -1; R.conn_w_out[at] = i < cn ? M.conn_w[c0 + i] : -1;
        R.ord_kf_out[at] = i < on ? M.ord_kf[o0 + i] : -1; R.ord_w_out[at] = i < on ? M.ord_w[o0 + i] : -1;
    }
    for (int k = tid; k < S.nk; k += nt) {
        const int g = S.k0 + k;
        R.conn_n_out[g] = M.conn_start[g + 1] - M.conn_start[g]; R.ord_n_out[g] = M.ord_start[g + 1] - M.ord_start[g];
        W.flags[g] = M.kf_flags[g];
        if (R.kf_parent_out) R.kf_parent_out[g] = M.kf_parent[g];
        if (R.kf_flags_out) R.kf_flags_out[g] = M.kf_flags[g];
        if (R.kf_touched) R.kf_touched[g] = 0;
    }
}

// ---- votes (:593-611): keypoint i of target kt. votes is the counter by slot, the stream's own [nk] -------------------------------------
VIORB_HD void cov_vote_keypoint(const CovMap& M, const SnapStream& S, int32_t* votes, int kt, int i) {
    const int p = M.kp_point[M.kp_start[S.k0 + kt] + i];
    if (p < 0 || M.pt_bad[S.p0 + p]) return;                                                    // :597-601
    for (int o = M.obs_start[S.p0 + p], e = M.obs_start[S.p0 + p + 1]; o < e; o++) {
        const int s = snap_obs_slot(M.obs[o]);
        if (s != kt) snap_fetch_add(&votes[s], 1);                                              // :607: bad observers are counted
    }
}
// The walk of KFcounter (:625-637) at key position j: the slot when it is in the counter, else -1. key = (votes, first key position wins)
// for the search of pKFmax with its strict >, larger is better.
VIORB_HD int cov_counter_slot(const CovMap& M, const SnapStream& S, const int32_t* votes, int j, int* v, long long* key) {
    const int k = M.kf_by_key[S.k0 + j];
    *v = snap_ld_agent(&votes[k]);
    if (*v <= 0) return -1;
    *key = (long long)*v * 65536 + (SNAP_MAX_KF - j);
    return k;
}
VIORB_HD void cov_write_counter_info(const CovMap& M, const SnapStream& S, const CovWork& W, int gt, int n, int n_th, long long best) {
    int32_t* c = W.cinfo + (size_t)gt * COV_C;
    c[COV_C_N] = n;
    c[COV_C_MAX_KF] = n ? M.kf_by_key[S.k0 + (SNAP_MAX_KF - (int)(best & 0xffff))] : -1;
    c[COV_C_MAX_W] = n ? (int)(best >> 16) : 0;
    c[COV_C_ADDED] = n ? (n_th ? n_th : 1) : 0;                                                 // :639-643: none reached th, pKFmax alone
}
// Entry (slot k, weight w) of a target's counter is in vPairs
VIORB_HD bool cov_is_added(const int32_t* cinfo, int k, int w) { return w >= COV_TH || (cinfo[COV_C_MAX_W] < COV_TH && k == cinfo[COV_C_MAX_KF]); }

// ---- the order of an ordered list: entry (weight wj, row position j) comes before (wi, i) ---------------------------------------------
// Rows are in ascending key, so a higher position is a higher key: descending weight, then descending key.
VIORB_HD bool cov_before(int wj, int j, int wi, int i) { return wj > wi || (wj == wi && j > i); }

// ---- UpdateBestCovisibles (:429-448): the ordered list (ok_, ow) of a key frame from its whole map (ck, cw) of n entries -----------------
// The rank sort of the share of `lane` of `nl`; old_n: the list's length before, -1 goes behind the new end. Also kf_removal_core.h's.
VIORB_HD void cov_rebuild_ordered(const int32_t* ck, const int32_t* cw, int32_t* ok_, int32_t* ow, int n, int old_n, int lane, int nl) {
    for (int i0 = 0; i0 < n; i0 += nl) {
        const int i = i0 + lane;
        if (i >= n) continue;
        const int wi = snap_ld_wg(&cw[i]);
        int before = 0;
        for (int j = 0; j < n; j++) before += cov_before(snap_ld_wg(&cw[j]), j, wi, i) ? 1 : 0;
        snap_st_wg(&ok_[before], snap_ld_wg(&ck[i])); snap_st_wg(&ow[before], wi);
    }
    for (int i = n + lane; i < old_n; i += nl) { snap_st_wg(&ok_[i], -1); snap_st_wg(&ow[i], -1); }
}

// ---- AddConnection (:414-427) with UpdateBestCovisibles (:429-448): key frame x learns weight w for target kt ---------------------------
// Run by `nl` lanes in step (the device: one wavefront; the host: lane 0 of 1); Wave::sum and Wave::any combine a value over them. The
// row's words go through snap_ld_wg / snap_st_wg, with a fence between a lane's write and another lane's read. Returns 0 for the early
// return on an unchanged weight, 1 when the row changed and the ordered list was rebuilt, -(length needed) when the insert does not fit.
template <class Wave>
VIORB_HD int cov_add_connection(const CovMap& M, const SnapStream& S, const CovOut& R, const int32_t* rank, int x, int kt, int w, int lane, int nl, Wave wave) {
    const int g = S.k0 + x, rt = rank[kt];
    int32_t* ck = R.conn_kf_out + (size_t)g * M.ccap; int32_t* cw = R.conn_w_out + (size_t)g * M.ccap;
    int32_t* ok_ = R.ord_kf_out + (size_t)g * M.ccap; int32_t* ow = R.ord_w_out + (size_t)g * M.ccap;
    const int cn = snap_ld_wg(&R.conn_n_out[g]);
    int pos = 0; bool found = false;
    for (int i0 = 0; i0 < cn; i0 += nl) {
        const int i = i0 + lane, s = i < cn ? snap_ld_wg(&ck[i]) : -1;
        pos += wave.sum(s >= 0 && rank[s] < rt ? 1 : 0);
        found = wave.any(s == kt) || found;
    }
    int n = cn;
    if (found) {
        if (snap_ld_wg(&cw[pos]) == w) return 0;                                                // :422-423
        if (lane == 0) snap_st_wg(&cw[pos], w);
    } else {
        if (cn + 1 > M.ccap) return -(cn + 1);
        for (int hi = cn; hi > pos; hi -= nl) {                                                  // the tail moves up by one, from its end, nl entries at a time
            const int i = hi - 1 - lane;
            int s = 0, v = 0;
            if (i >= pos) { s = snap_ld_wg(&ck[i]); v = snap_ld_wg(&cw[i]); }
            snap_fence_wg();
            if (i >= pos) { snap_st_wg(&ck[i + 1], s); snap_st_wg(&cw[i + 1], v); }
            snap_fence_wg();
        }
        if (lane == 0) { snap_st_wg(&ck[pos], kt); snap_st_wg(&cw[pos], w); snap_st_wg(&R.conn_n_out[g], cn + 1); }
        n = cn + 1;
    }
    snap_fence_wg();
    const int old_n = snap_ld_wg(&R.ord_n_out[g]);
    cov_rebuild_ordered(ck, cw, ok_, ow, n, old_n, lane, nl);                                    // the rank sort of the whole map
    if (lane == 0) {
        snap_st_wg(&R.ord_n_out[g], n);
        if (R.kf_touched) R.kf_touched[g] |= COV_MAP_CHANGED | COV_ORD_REBUILT;
    }
    return 1;
}

// ---- the target's own members (:645-660): its map becomes the counter, its ordered list vPairs in order --------------------------------
// The share of `tid`. ckf / cw: the target's counter row of n <= ccap entries; *front receives the head of the new list (one thread writes it).
VIORB_HD void cov_replace_target(const CovMap& M, const SnapStream& S, const CovOut& R, const int32_t* ckf, const int32_t* cw, const int32_t* cinfo,
                                 int kt, int32_t* front, int tid, int nt) {
    const int g = S.k0 + kt, n = cinfo[COV_C_N], n_add = cinfo[COV_C_ADDED], old_cn = R.conn_n_out[g], old_on = R.ord_n_out[g];
    const size_t row = (size_t)g * M.ccap;
    for (int i = tid; i < n || i < old_cn; i += nt) { R.conn_kf_out[row + i] = i < n ? ckf[i] : -1; R.conn_w_out[row + i] = i < n ? cw[i] : -1; }
    for (int i = tid; i < n; i += nt) {
        const int wi = cw[i];
        if (!cov_is_added(cinfo, ckf[i], wi)) continue;
        int before = 0;
        for (int j = 0; j < n; j++) before += cov_is_added(cinfo, ckf[j], cw[j]) && cov_before(cw[j], j, wi, i) ? 1 : 0;
        R.ord_kf_out[row + before] = ckf[i]; R.ord_w_out[row + before] = wi;
        if (before == 0) *front = ckf[i];
    }
    for (int i = n_add + tid; i < old_on; i += nt) { R.ord_kf_out[row + i] = -1; R.ord_w_out[row + i] = -1; }
}
// What one thread does after that: the counts, the first connection (:662-667), the per-target outputs. Returns nothing; the flags live in W.
VIORB_HD void cov_finish_target(const CovMap& M, const SnapStream& S, const CovWork& W, const CovOut& R, const int32_t* cinfo, int gt, int kt, int front) {
    const int g = S.k0 + kt, n = cinfo[COV_C_N];
    int parent = -1;
    if (n > 0) {
        R.conn_n_out[g] = n; R.ord_n_out[g] = cinfo[COV_C_ADDED];
        if (R.kf_touched) R.kf_touched[g] |= COV_MAP_CHANGED | COV_ORD_REBUILT;
        const int f = W.flags[g];
        if ((f & COV_KF_FIRST) && !(f & COV_KF_ID0)) {
            parent = front;
            W.flags[g] = f & ~COV_KF_FIRST;
            if (R.kf_parent_out) R.kf_parent_out[g] = parent;
            if (R.kf_flags_out) R.kf_flags_out[g] = (uint8_t)(f & ~COV_KF_FIRST);
        }
    }
    if (R.t_observers) R.t_observers[gt] = n;
    if (R.t_max_kf) R.t_max_kf[gt] = cinfo[COV_C_MAX_KF];
    if (R.t_max_w) R.t_max_w[gt] = cinfo[COV_C_MAX_W];
    if (R.t_added) R.t_added[gt] = cinfo[COV_C_ADDED];
    if (R.t_parent) R.t_parent[gt] = parent;
}

// ---- LoopConnections (LoopClosing.cc:577-589) ----------------------------------------------------------------------------------------------
// mark[s]: bit 0 = s is a target of the stream (set only with erase_targets), the rest = gen of the target whose ordered list held s just
// before its call. Entry i of the target's map after the call stays in the set, or -1.
VIORB_HD void cov_mark_previous(const CovMap& M, const SnapStream& S, const CovOut& R, int32_t* mark, int kt, int gen, int tid, int nt) {
    const int g = S.k0 + kt, n = R.ord_n_out[g];
    for (int i = tid; i < n; i += nt) { const int s = R.ord_kf_out[(size_t)g * M.ccap + i]; mark[s] = (mark[s] & 1) | (gen << 1); }
}
VIORB_HD int cov_loop_kept(const CovMap& M, const SnapStream& S, const CovOut& R, const int32_t* mark, int kt, int gen, int i) {
    const int s = R.conn_kf_out[(size_t)(S.k0 + kt) * M.ccap + i], m = mark[s];
    return ((m >> 1) == gen || (m & 1)) ? -1 : s;
}

VIORB_HD void cov_write_refused(const CovOut& R, int b) { R.status[b] = COV_INVALID; }

// The phases of the device form on one host thread, stream by stream. W holds arrays of the sizes CovWork names (votes: [n_kf]).
inline void cov_run_host(const CovMap& M, const CovWork& W, const CovOut& R) {
    struct One { int sum(int v) const { return v; } bool any(bool v) const { return v; } };
    for (int b = 0; b < M.batch; b++) {
        bool ok = cov_validate_ranges(M, b, 0, 1);
        SnapStream S = {0, 0, 0, 0};
        if (ok) { S = snap_stream(M.kf_start, M.pt_start, b); ok = cov_validate_offsets(M, S, b, 0, 1); }
        ok = ok && cov_validate_entries(M, S, b, 0, 1);
        if (ok) { snap_distinct_fill(M.kf_by_key + S.k0, S.nk, W.rank + S.k0, 0, 1); ok = snap_distinct_check(M.kf_by_key + S.k0, S.nk, W.rank + S.k0, 0, 1); }
        ok = ok && cov_validate_rows(M, S, W.rank + S.k0, 0, 1);
        W.info[b] = ok;
        if (!ok) { cov_write_refused(R, b); continue; }
        cov_copy_rows(M, S, W, R, 0, 1);
        const int t0 = M.target_start[b], nt = M.target_start[b + 1] - t0;
        int32_t* votes = W.votes + S.k0; int32_t* mark = W.mark + S.k0; const int32_t* rank = W.rank + S.k0;
        for (int t = 0; t < nt; t++) {                                                           // the counters: no target changes what they read
            const int gt = t0 + t, kt = M.target_kf[gt], g = S.k0 + kt;
            for (int k = 0; k < S.nk; k++) votes[k] = 0;
            for (int i = 0, e = M.kp_start[g + 1] - M.kp_start[g]; i < e; i++) cov_vote_keypoint(M, S, votes, kt, i);
            int n = 0, n_th = 0; long long best = -1, key = 0;
            for (int j = 0; j < S.nk; j++) {
                int v; const int k = cov_counter_slot(M, S, votes, j, &v, &key);
                if (k < 0) continue;
                if (n < M.ccap) { W.ckf[(size_t)gt * M.ccap + n] = k; W.cw[(size_t)gt * M.ccap + n] = v; }
                n++; n_th += v >= COV_TH; if (key > best) best = key;
            }
            cov_write_counter_info(M, S, W, gt, n, n_th, best);
        }
        const bool loop = R.loop_conn || R.n_loop_conn;
        for (int k = 0; k < S.nk; k++) mark[k] = 0;
        if (M.erase_targets) for (int t = 0; t < nt; t++) mark[M.target_kf[t0 + t]] = 1;
        int status = COV_OK, need = 0;
        for (int t = 0; t < nt && status == COV_OK; t++) {                                       // the ordered phase
            const int gt = t0 + t, kt = M.target_kf[gt], gen = t + 1;
            const int32_t* cinfo = W.cinfo + (size_t)gt * COV_C; const int32_t* ckf = W.ckf + (size_t)gt * M.ccap; const int32_t* cw = W.cw + (size_t)gt * M.ccap;
            const int n = cinfo[COV_C_N];
            if (loop) cov_mark_previous(M, S, R, mark, kt, gen, 0, 1);
            int32_t front = -1;
            if (n > M.ccap) { status = COV_OVERFLOW; need = n; break; }
            for (int i = 0; i < n; i++) {
                if (!cov_is_added(cinfo, ckf[i], cw[i])) continue;
                const int rc = cov_add_connection(M, S, R, rank, ckf[i], kt, cw[i], 0, 1, One());
                if (rc < 0) { status = COV_OVERFLOW; need = -rc; break; }
            }
            if (status != COV_OK) break;
            if (n > 0) cov_replace_target(M, S, R, ckf, cw, cinfo, kt, &front, 0, 1);
            cov_finish_target(M, S, W, R, cinfo, gt, kt, front);
            if (loop) {
                const int cn = R.conn_n_out[S.k0 + kt];
                int m = 0;
                for (int i = 0; i < cn; i++) { const int s = cov_loop_kept(M, S, R, mark, kt, gen, i); if (s >= 0) { if (R.loop_conn) R.loop_conn[(size_t)gt * M.ccap + m] = s; m++; } }
                if (R.loop_conn) for (int i = m; i < M.ccap; i++) R.loop_conn[(size_t)gt * M.ccap + i] = -1;
                if (R.n_loop_conn) R.n_loop_conn[gt] = m;
            }
        }
        R.status[b] = status;
        if (R.need) R.need[b] = need;
    }
}

} // namespace viorb
