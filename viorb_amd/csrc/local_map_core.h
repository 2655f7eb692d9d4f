// viorb_amd/csrc/local_map_core.h — Tracking::UpdateLocalMap, shared by the HIP kernels of local_map.hip and by the host
// (tests/cpp/local_map_core_host_test.cpp drives this header alone, under the address and undefined-behaviour sanitizers, against the
// literal loop).
//
// What is restated (reference file:line):
//   Tracking::UpdateLocalKeyFrames   src/Tracking.cc:1996-2125  (votes :1999-2016, the early return :2018, the voted list :2028-2043,
//                                                                the neighbour loop :2047-2118, the reference key frame :2120-2124)
//   Tracking::UpdateLocalPoints      src/Tracking.cc:1970-1993
// Everything is integer arithmetic. The two mnTrackReferenceForFrame members are only ever compared with mCurrentFrame.mnId,
// so a fresh mark per call stands for them: `mark` for key frames, the first position of a point for map points.
#pragma once
#include <stdint.h>
#include "map_snapshot_core.h"      // the snapshot's layout, its observation word, the validator's checks, the memory shim

namespace viorb {

enum { ULM_OK = 0, ULM_NO_VOTES = 1, ULM_OVERFLOW = 2, ULM_INVALID = -1 };     // status (VIORB_ULM_* of include/viorb_local_map.h)
enum { ULM_LIMIT = 80, ULM_COVIS = 10, ULM_NO_POS = 0x7fffffff };
enum { ULM_INFO_OK = 0, ULM_INFO_LIST = 1, ULM_INFO_STATUS = 2, ULM_INFO_ENTRIES = 3, ULM_INFO = 4 };       // info[b][4]

// The snapshot (viorb_local_map_snapshot with the three row lengths) and the working state (the workspace; host: plain arrays)
struct UlmMap {
    int batch, n_kf, n_child, n_kp, n_pt, n_obs;
    const int32_t* kf_start; const uint8_t* kf_bad; const int32_t* kf_parent; const int32_t* kf_prev; const int32_t* kf_next;
    const int32_t* covis10; const int32_t* child_start; const int32_t* child_kf; const int32_t* kf_by_key;
    const int32_t* kp_start; const int32_t* kp_point;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* obs_start; const uint32_t* obs;
    const int32_t* frame_point; const int32_t* frame_count;
    const int32_t* prev_lkf; const int32_t* prev_n_lkf; const int32_t* prev_ref_kf;
    int cap, lcap, pcap;
};
struct UlmWork {
    int32_t* votes; int32_t* mark;       // [n_kf]: keyframeCounter; "in the list" (the validator's scratch before that). The device keeps both in LDS while a stream's key frames fit
    int32_t* list; int32_t* estart;      // [n_kf + batch], a stream's part at kf_start[b] + b: the local key frames (at most nk: they are distinct); estart[j] = keypoints of list[0..j)
    int32_t* first;                      // [n_pt]: the lowest flat (list ordinal, keypoint) position that holds the point, ULM_NO_POS before
    int32_t* info;                       // [batch][ULM_INFO]: accepted, list length, status so far, keypoint entries of the list
};
struct UlmOut {
    int32_t* lkf; int32_t* n_lkf; int32_t* n_voted; int32_t* ref_kf; int32_t* lpt; int32_t* n_lpt; int32_t* status;
    int32_t* frame_point_out; int32_t* kf_votes;
};

// ---- the stream validator: the steps of map_snapshot_core.h on this snapshot's arrays ----------------------------------------------------
// In the neighbour loop one wavefront's lanes read marks and list entries that another lane has just written (snap_ld_wg, snap_st_wg,
// snap_fence_wg after a push); the votes are integer atomic adds and are read with snap_ld_agent.
// Step 1: kp_start and child_start are nested under kf_start, obs_start under pt_start.
VIORB_HD bool ulm_validate_ranges(const UlmMap& M, int b, int tid, int nt) {
    bool ok = true;
    for (int i = tid; i <= b; i += nt) {
        if (!(snap_span(M.kf_start, i, i + 1, M.n_kf) && snap_span(M.pt_start, i, i + 1, M.n_pt))) { ok = false; continue; }
        const int k0 = M.kf_start[i], k1 = M.kf_start[i + 1];
        ok = ok && snap_span(M.kp_start, k0, k1, M.n_kp) && snap_span(M.child_start, k0, k1, M.n_child);
        ok = ok && snap_span(M.obs_start, M.pt_start[i], M.pt_start[i + 1], M.n_obs);
    }
    return ok;
}
// Step 2: the per-stream scalars, the nested offsets, every key frame's links, the neighbour table and the range of kf_by_key.
VIORB_HD bool ulm_validate_offsets(const UlmMap& M, const SnapStream& S, int b, int tid, int nt) {
    const int fc = M.frame_count[b], pn = M.prev_n_lkf[b];
    bool ok = S.nk <= SNAP_MAX_KF && fc >= 0 && fc <= M.cap && pn >= 0 && pn <= M.lcap && pn <= S.nk && snap_slot_or_none(M.prev_ref_kf[b], S.nk);
    ok &= snap_offsets_run(M.kp_start, S.k0, S.nk, M.n_kp, tid, nt);
    ok &= snap_offsets_run(M.child_start, S.k0, S.nk, M.n_child, tid, nt);
    ok &= snap_offsets_run(M.obs_start, S.p0, S.np, M.n_obs, tid, nt);
    for (int k = tid; k < S.nk; k += nt) {
        const int g = S.k0 + k, parent = M.kf_parent[g], prev = M.kf_prev[g], next = M.kf_next[g], key = M.kf_by_key[g];
        ok &= snap_slot_or_none(parent, S.nk) && snap_slot_or_none(prev, S.nk) && snap_slot_or_none(next, S.nk) && key >= 0 && key < S.nk;
        for (int i = 0; i < ULM_COVIS; i++) ok &= snap_slot_or_none(M.covis10[(size_t)g * ULM_COVIS + i], S.nk);
    }
    return ok;
}
// Step 3: every point index of the keypoint tables and of the frame, every slot of the children, the observations and the previous list.
VIORB_HD bool ulm_validate_entries(const UlmMap& M, const SnapStream& S, int b, int tid, int nt) {
    bool ok = snap_entries_within(M.kp_point, M.kp_start[S.k0], M.kp_start[S.k0 + S.nk], -1, S.np, tid, nt);
    ok &= snap_entries_within(M.child_kf, M.child_start[S.k0], M.child_start[S.k0 + S.nk], 0, S.nk, tid, nt);
    ok &= snap_obs_slots_below(M.obs, M.obs_start[S.p0], M.obs_start[S.p0 + S.np], S.nk, tid, nt);
    ok &= snap_entries_within(M.frame_point + (size_t)b * M.cap, 0, M.frame_count[b], -1, S.np, tid, nt);
    ok &= snap_entries_within(M.prev_lkf + (size_t)b * M.lcap, 0, M.prev_n_lkf[b], 0, S.nk, tid, nt);
    return ok;
}
// Step 4, twice (snap_distinct_fill / snap_distinct_check on mark[]): kf_by_key, which n = nk distinct slots make a permutation, and the
// previous list. Then the working state the later phases expect:
VIORB_HD void ulm_prepare(const SnapStream& S, const UlmWork& W, int tid, int nt) { for (int p = tid; p < S.np; p += nt) W.first[S.p0 + p] = ULM_NO_POS; }

// ---- votes (:2000-2016): keypoint i of the frame; the number of votes it cast ------------------------------------------------------------
// votes is the stream's own [nk].
VIORB_HD int ulm_vote_keypoint(const UlmMap& M, const SnapStream& S, int32_t* votes, const UlmOut& R, int b, int i) {
    const size_t g = (size_t)b * M.cap + i;
    int p = M.frame_point[g], n = 0;
    if (p >= 0) {
        if (M.pt_bad[S.p0 + p]) p = -1;                                                         // :2013
        else for (int o = M.obs_start[S.p0 + p], e = M.obs_start[S.p0 + p + 1]; o < e; o++, n++) snap_fetch_add(&votes[snap_obs_slot(M.obs[o])], 1);
    }
    if (R.frame_point_out) R.frame_point_out[g] = p;
    return n;
}
// The walk of keyframeCounter (:2028-2043) at key position j: the slot when it enters the list, else -1. key = (votes, first key position
// wins) for the search of pKFmax, larger is better.
VIORB_HD int ulm_voted_slot(const UlmMap& M, const SnapStream& S, const int32_t* votes, int j, long long* key) {
    const int k = M.kf_by_key[S.k0 + j], v = snap_ld_agent(&votes[k]);
    if (v <= 0 || M.kf_bad[S.k0 + k]) return -1;
    *key = (long long)v * 65536 + (SNAP_MAX_KF - j);
    return k;
}
VIORB_HD int ulm_key_slot(const UlmMap& M, const SnapStream& S, long long key) { return M.kf_by_key[S.k0 + (SNAP_MAX_KF - (int)(key & 0xffff))]; }

// ---- the neighbour loop (:2047-2118) ----------------------------------------------------------------------------------------------------
// Run by `nl` lanes in step (the device: one wavefront; the host: lane 0 of 1). first_of(c) returns the c of the lowest lane whose c >= 0,
// or -1, the same value to every lane. mark and list are the stream's own; list holds the n voted key frames.
VIORB_HD int ulm_push(int32_t* mark, int32_t* list, int size, int c, int lane) {
    if (lane == 0) { snap_st_wg(&list[size], c); snap_st_wg(&mark[c], 1); }
    snap_fence_wg();
    return size + 1;
}
template <class First>
VIORB_HD int ulm_first_eligible(const UlmMap& M, const SnapStream& S, const int32_t* mark, const int32_t* cand, int n, int lane, int nl, First first_of) {
    for (int i0 = 0; i0 < n; i0 += nl) {
        int c = -1;
        if (i0 + lane < n) { c = cand[i0 + lane]; if (c >= 0 && (M.kf_bad[S.k0 + c] || snap_ld_wg(&mark[c]))) c = -1; }
        c = first_of(c);
        if (c >= 0) return c;
    }
    return -1;
}
template <class First>
VIORB_HD int ulm_neighbour_loop(const UlmMap& M, const SnapStream& S, int32_t* mark, int32_t* list, int n, int lane, int nl, First first_of) {
    int size = n;
    for (int j = 0; j < n; j++) {                                                              // itEndKF is taken before the loop
        if (size > ULM_LIMIT) break;                                                            // :2050
        const int kf = snap_ld_wg(&list[j]), g = S.k0 + kf;
        int c = ulm_first_eligible(M, S, mark, M.covis10 + (size_t)g * ULM_COVIS, ULM_COVIS, lane, nl, first_of);      // :2055-2069
        if (c >= 0) size = ulm_push(mark, list, size, c, lane);
        c = ulm_first_eligible(M, S, mark, M.child_kf + M.child_start[g], M.child_start[g + 1] - M.child_start[g], lane, nl, first_of);   // :2071-2084
        if (c >= 0) size = ulm_push(mark, list, size, c, lane);
        const int link[3] = {M.kf_parent[g], M.kf_prev[g], M.kf_next[g]};                       // :2086-2117: no isBad() test
        for (int q = 0; q < 3; q++) if (link[q] >= 0 && !snap_ld_wg(&mark[link[q]])) size = ulm_push(mark, list, size, link[q], lane);
    }
    return size;
}

// ---- local points (:1970-1993) -------------------------------------------------------------------------------------------------------------
// The point at flat position pos of the stream's (list ordinal, keypoint) entries, or -1. estart[j] <= pos < estart[j + 1] picks j; a key
// frame without keypoints owns no position.
VIORB_HD int ulm_entry_point(const UlmMap& M, const SnapStream& S, const int32_t* list, const int32_t* estart, int n_list, int pos) {
    int lo = 0, hi = n_list;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (estart[mid] <= pos) lo = mid; else hi = mid; }
    return M.kp_point[M.kp_start[S.k0 + list[lo]] + (pos - estart[lo])];
}
VIORB_HD void ulm_claim(const UlmMap& M, const SnapStream& S, const UlmWork& W, const int32_t* list, const int32_t* estart, int n_list, int pos) {
    const int p = ulm_entry_point(M, S, list, estart, n_list, pos);
    if (p >= 0 && !M.pt_bad[S.p0 + p]) snap_min(&W.first[S.p0 + p], pos);
}
// The point that position pos appends to mvpLocalMapPoints, or -1: not null, not bad, and not taken by a lower position.
VIORB_HD int ulm_kept_point(const UlmMap& M, const SnapStream& S, const UlmWork& W, const int32_t* list, const int32_t* estart, int n_list, int pos) {
    const int p = ulm_entry_point(M, S, list, estart, n_list, pos);
    return (p >= 0 && !M.pt_bad[S.p0 + p] && W.first[S.p0 + p] == pos) ? p : -1;
}

// ---- outputs --------------------------------------------------------------------------------------------------------------------------------
VIORB_HD void ulm_write_refused(const UlmOut& R, int b) { if (R.status) R.status[b] = ULM_INVALID; }
// lkf[b], the share of `tid`: the first min(n, lcap) entries of the list, then -1
VIORB_HD void ulm_write_list(const UlmMap& M, const UlmOut& R, const int32_t* list, int n, int b, int tid, int nt) {
    if (!R.lkf) return;
    for (int j = tid; j < M.lcap; j += nt) R.lkf[(size_t)b * M.lcap + j] = j < n ? list[j] : -1;
}

// The phases of the device form on one host thread, stream by stream. W holds arrays of the sizes UlmWork names.
inline void ulm_run_host(const UlmMap& M, const UlmWork& W, const UlmOut& R) {
    struct Self { VIORB_HD int operator()(int c) const { return c; } };
    for (int b = 0; b < M.batch; b++) {
        bool ok = ulm_validate_ranges(M, b, 0, 1);
        SnapStream S = {0, 0, 0, 0};
        if (ok) { S = snap_stream(M.kf_start, M.pt_start, b); ok = ulm_validate_offsets(M, S, b, 0, 1); }
        ok = ok && ulm_validate_entries(M, S, b, 0, 1);
        if (ok) { snap_distinct_fill(M.kf_by_key + S.k0, S.nk, W.mark + S.k0, 0, 1); ok = snap_distinct_check(M.kf_by_key + S.k0, S.nk, W.mark + S.k0, 0, 1); }
        if (ok) {
            const int32_t* prev = M.prev_lkf + (size_t)b * M.lcap;
            snap_distinct_fill(prev, M.prev_n_lkf[b], W.mark + S.k0, 0, 1); ok = snap_distinct_check(prev, M.prev_n_lkf[b], W.mark + S.k0, 0, 1);
        }
        W.info[b * ULM_INFO + ULM_INFO_OK] = ok;
        if (!ok) { ulm_write_refused(R, b); continue; }
        ulm_prepare(S, W, 0, 1);
        int32_t* votes = W.votes + S.k0; int32_t* mark = W.mark + S.k0; int32_t* list = W.list + S.k0 + b; int32_t* estart = W.estart + S.k0 + b;
        for (int k = 0; k < S.nk; k++) { votes[k] = 0; mark[k] = 0; }
        long long cast = 0;
        const int fc = M.frame_count[b];
        for (int i = 0; i < fc; i++) cast += ulm_vote_keypoint(M, S, votes, R, b, i);
        if (R.frame_point_out) for (int i = fc; i < M.cap; i++) R.frame_point_out[(size_t)b * M.cap + i] = -1;
        if (R.kf_votes) for (int k = 0; k < S.nk; k++) R.kf_votes[S.k0 + k] = votes[k];
        int n = 0, n_voted = 0, ref = M.prev_ref_kf[b], status = ULM_OK;
        if (cast == 0) {                                                                        // :2018
            status = ULM_NO_VOTES; n = M.prev_n_lkf[b];
            for (int j = 0; j < n; j++) list[j] = M.prev_lkf[(size_t)b * M.lcap + j];
        } else {
            long long best = -1, key = 0;
            for (int j = 0; j < S.nk; j++) {
                const int k = ulm_voted_slot(M, S, votes, j, &key);
                if (k < 0) continue;
                list[n++] = k; mark[k] = 1;
                if (key > best) best = key;
            }
            if (best >= 0) ref = ulm_key_slot(M, S, best);
            n_voted = n;
            n = ulm_neighbour_loop(M, S, mark, list, n, 0, 1, Self());
        }
        if (n > M.lcap) status = ULM_OVERFLOW;
        ulm_write_list(M, R, list, n, b, 0, 1);
        if (R.n_lkf) R.n_lkf[b] = n;
        if (R.n_voted) R.n_voted[b] = n_voted;
        if (R.ref_kf) R.ref_kf[b] = ref;
        estart[0] = 0;
        for (int j = 0; j < n; j++) estart[j + 1] = estart[j] + (M.kp_start[S.k0 + list[j] + 1] - M.kp_start[S.k0 + list[j]]);
        const int entries = estart[n];
        for (int pos = 0; pos < entries; pos++) ulm_claim(M, S, W, list, estart, n, pos);
        int n_lpt = 0;
        for (int pos = 0; pos < entries; pos++) {
            const int p = ulm_kept_point(M, S, W, list, estart, n, pos);
            if (p < 0) continue;
            if (R.lpt && n_lpt < M.pcap) R.lpt[(size_t)b * M.pcap + n_lpt] = p;
            n_lpt++;
        }
        if (R.lpt) for (int j = n_lpt; j < M.pcap; j++) R.lpt[(size_t)b * M.pcap + j] = -1;
        if (n_lpt > M.pcap) status = ULM_OVERFLOW;
        if (R.n_lpt) R.n_lpt[b] = n_lpt;
        if (R.status) R.status[b] = status;
        W.info[b * ULM_INFO + ULM_INFO_LIST] = n; W.info[b * ULM_INFO + ULM_INFO_STATUS] = status; W.info[b * ULM_INFO + ULM_INFO_ENTRIES] = entries;
    }
}

} // namespace viorb
