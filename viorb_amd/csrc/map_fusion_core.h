// viorb_amd/csrc/map_fusion_core.h — the results of the fuse searches applied to a map snapshot, for an ordered list of calls per stream,
// shared by the HIP kernels of map_fusion.hip and by the host (tests/cpp/map_fusion_core_host_test.cpp drives this header alone, under
// the address and undefined-behaviour sanitizers).
//
// What is restated (reference file:line):
//   ORBmatcher::Fuse(pKF, vpMapPoints)        src/ORBmatcher.cc:842-972 without the search (guards :846-850, replace / add :951-971)
//   ORBmatcher::Fuse(pKF, Scw, ...)           src/ORBmatcher.cc:993 (spAlreadyFound), :1000-1097 (guard :1005, record / add :1081-1096)
//   LoopClosing::SearchAndFuse                src/LoopClosing.cc:632-640 (the Replace loop)
//   MapPoint::Replace                         src/MapPoint.cc:184-222, AddObservation :105-116, ComputeDistinctiveDescriptors :258, :272-274
// Everything is integer arithmetic.
//
// The working state. kp_point_out and pt_nobs_out are the working copies of mvpMapPoints and nObs. mObservations of a point is a chain
// of segments of a pool of observation entries in the workspace: the stream's input observations in their CSR order, then one slot per
// list entry of the stream's calls for the observation that entry may add. A point's CSR range is segment `point`, the slot of list
// entry j is segment `points + j`; head / tail / next link them. Replace appends the replaced point's chain to the survivor's and clears
// the alive bit of the entries whose key frame the survivor already lists, so no entry is ever copied. An entry's word is the slot
// with SNAP_OBS_ALIVE; a point's alive entries name distinct key frames (the validator for the input, the operations afterwards).
//
// The ordered phase is run by `nl` lanes in step (the device: one wavefront; the host: lane 0 of 1), as cov_add_connection: the state's
// words go through snap_ld_wg / snap_st_wg, with snap_fence_wg between a lane's write and another lane's read.
#pragma once
#include <stdint.h>
#include "covis_core.h"             // map_snapshot_core.h, cov_row_of, COV_OK / COV_OVERFLOW / COV_INVALID

namespace viorb {

enum { FUSE_POSE = 0, FUSE_SIM3 = 1 };                                                                                   // call_kind
enum { FUSE_ADDED = 0, FUSE_REPLACED_KF_POINT = 1, FUSE_REPLACED_CANDIDATE = 2, FUSE_COUNTED_ONLY = 3, FUSE_SKIP_BAD = 4, FUSE_SKIP_IN_KF = 5,
       FUSE_NONE = 6, FUSE_NULL_POINT = 7 };                                                                             // op_reason

struct FuseMap {
    int batch, n_kf, n_kp, n_pt, n_obs, n_call, n_list, n_feat, n_op, n_obs_out;
    const int32_t* kf_start; const int32_t* kf_by_key; const uint8_t* kf_bad;
    const int32_t* kp_start; const int32_t* kp_point; const uint8_t* kp_octave; const uint8_t* kp_stereo;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* pt_nobs; const int32_t* pt_found; const int32_t* pt_visible;
    const int32_t* obs_start; const uint32_t* obs; const int32_t* obs_feat;
    const int32_t* call_start; const int32_t* call_kf; const uint8_t* call_kind; const int32_t* call_list; const int32_t* call_n; const int32_t* call_feat;
    const int32_t* call_op;
    const int32_t* list_point; const int32_t* op_feat; const int32_t* obs_out_start;
};
struct FuseWork {
    int32_t* rank;                       // [n_kf]: a slot's key position
    int32_t* bad; int32_t* replaced; int32_t* dirty; int32_t* stamp;       // [n_pt]: isBad, mpReplaced, CDD ran, the call (ordinal + 1) whose spAlreadyFound holds the point
    uint32_t* found; uint32_t* visible;  // [n_pt]
    int32_t* head; int32_t* tail;        // [n_pt]: the first and the last segment of the point's chain, -1 for none
    int32_t* cnt; int32_t* dcnt;         // [n_pt]: the alive entries, the entries of the dirty list
    int32_t* next;                       // [n_pt + n_op]: the segment behind a segment, -1 for none
    int32_t* rep;                        // [n_op]: vpReplacePoint
    uint32_t* pool; int32_t* pfeat;      // [n_obs + n_op]: the entries
    int32_t* info; int32_t* tot; int32_t* dtot;                           // [batch]: accepted, the sums of cnt and dcnt
};
struct FuseOut {
    int32_t* status; int32_t* kp_point_out; uint8_t* pt_bad_out; int32_t* pt_nobs_out; int32_t* obs_start_out; uint32_t* obs_out; int32_t* obs_feat_out;
    int32_t* need; int32_t* pt_found_out; int32_t* pt_visible_out; int32_t* pt_replaced_out; uint8_t* pt_dirty; uint8_t* obs_touched;
    int32_t* dirty_obs_start; int32_t* dirty_obs_kf; int32_t* dirty_obs_feat;
    int32_t* op_reason; int32_t* op_other; int32_t* call_nfused;
};
// A stream's ranges: key frames and points (S), calls, list entries, the input observations, the pool and the segments
struct FuseStream { SnapStream S; int c0, nc, j0, nj, o0, no, e0, s0; };
VIORB_HD FuseStream fuse_stream(const FuseMap& M, int b) {
    FuseStream F;
    F.S = snap_stream(M.kf_start, M.pt_start, b);
    F.c0 = M.call_start[b]; F.nc = M.call_start[b + 1] - F.c0;
    F.j0 = M.call_op[F.c0]; F.nj = M.call_op[F.c0 + F.nc] - F.j0;
    F.o0 = M.obs_start[F.S.p0]; F.no = M.obs_start[F.S.p0 + F.S.np] - F.o0;
    F.e0 = F.o0 + F.j0; F.s0 = F.S.p0 + F.j0;
    return F;
}
VIORB_HD int fuse_nkp(const FuseMap& M, const SnapStream& S, int k) { return M.kp_start[S.k0 + k + 1] - M.kp_start[S.k0 + k]; }

// ---- the stream validator: the steps of map_snapshot_core.h on this snapshot's arrays ------------------------------------------------------
// Step 1: the batch-level offsets of streams 0..b and the nested offsets at their boundaries.
VIORB_HD bool fuse_validate_ranges(const FuseMap& M, int b, int tid, int nt) {
    bool ok = true;
    for (int i = tid; i <= b; i += nt) {
        if (!(snap_span(M.kf_start, i, i + 1, M.n_kf) && snap_span(M.pt_start, i, i + 1, M.n_pt) && snap_span(M.call_start, i, i + 1, M.n_call)
              && snap_span(M.obs_out_start, i, i + 1, M.n_obs_out))) { ok = false; continue; }
        ok = ok && snap_span(M.kp_start, M.kf_start[i], M.kf_start[i + 1], M.n_kp) && snap_span(M.obs_start, M.pt_start[i], M.pt_start[i + 1], M.n_obs)
                && snap_span(M.call_op, M.call_start[i], M.call_start[i + 1], M.n_op);
    }
    return ok;
}
// Step 2: the nested offsets, kf_by_key, the scalars of every call (F.nj is not used).
VIORB_HD bool fuse_validate_offsets(const FuseMap& M, const FuseStream& F, int tid, int nt) {
    const SnapStream& S = F.S;
    bool ok = S.nk <= SNAP_MAX_KF;
    ok &= snap_offsets_run(M.kp_start, S.k0, S.nk, M.n_kp, tid, nt);
    ok &= snap_offsets_run(M.obs_start, S.p0, S.np, M.n_obs, tid, nt);
    ok &= snap_offsets_run(M.call_op, F.c0, F.nc, M.n_op, tid, nt);
    for (int k = tid; k < S.nk; k += nt) { const int key = M.kf_by_key[S.k0 + k]; ok &= key >= 0 && key < S.nk; }
    for (int c = F.c0 + tid; c < F.c0 + F.nc; c += nt) {
        const long long n = M.call_n[c], l = M.call_list[c], f = M.call_feat[c];
        ok &= M.call_kf[c] >= 0 && M.call_kf[c] < S.nk && M.call_kind[c] <= FUSE_SIM3;
        ok &= n >= 0 && n == (long long)M.call_op[c + 1] - M.call_op[c] && l >= 0 && l + n <= M.n_list && f >= 0 && f + n <= M.n_feat;
    }
    return ok;
}
// Step 3: what step 2's offsets delimit.
VIORB_HD bool fuse_validate_entries(const FuseMap& M, const FuseStream& F, int tid, int nt) {
    const SnapStream& S = F.S;
    bool ok = snap_entries_within(M.kp_point, M.kp_start[S.k0], M.kp_start[S.k0 + S.nk], -1, S.np, tid, nt);
    ok &= snap_obs_slots_below(M.obs, F.o0, F.o0 + F.no, S.nk, tid, nt);
    for (int c = F.c0; c < F.c0 + F.nc; c++) {
        ok &= snap_entries_within(M.list_point, M.call_list[c], M.call_list[c] + M.call_n[c], -1, S.np, tid, nt);
        ok &= snap_entries_within(M.op_feat, M.call_feat[c], M.call_feat[c] + M.call_n[c], -1, fuse_nkp(M, S, M.call_kf[c]), tid, nt);
    }
    return ok;
}
// Step 4, after the slots have been accepted: obs_feat inside its key frame's keypoints; no observation list names a key frame twice.
VIORB_HD bool fuse_validate_observations(const FuseMap& M, const FuseStream& F, int tid, int nt) {
    const SnapStream& S = F.S;
    bool ok = true;
    for (int o = F.o0 + tid; o < F.o0 + F.no; o += nt) {
        const int k = snap_obs_slot(M.obs[o]), f = M.obs_feat[o], p = cov_row_of(M.obs_start, S.p0, S.np, o);
        ok &= f >= 0 && f < fuse_nkp(M, S, k);
        for (int j = M.obs_start[S.p0 + p]; j < o; j++) ok &= snap_obs_slot(M.obs[j]) != k;
    }
    return ok;
}
// The working state of an accepted stream, the share of `tid`
VIORB_HD void fuse_prepare(const FuseMap& M, const FuseStream& F, const FuseWork& W, const FuseOut& R, int tid, int nt) {
    const SnapStream& S = F.S;
    for (int i = M.kp_start[S.k0] + tid, e = M.kp_start[S.k0 + S.nk]; i < e; i += nt) R.kp_point_out[i] = M.kp_point[i];
    for (int p = tid; p < S.np; p += nt) {
        const int g = S.p0 + p, n = M.obs_start[g + 1] - M.obs_start[g];
        W.bad[g] = M.pt_bad[g] != 0; W.replaced[g] = -1; W.dirty[g] = 0; W.stamp[g] = 0;
        W.found[g] = (uint32_t)M.pt_found[g]; W.visible[g] = (uint32_t)M.pt_visible[g];
        R.pt_nobs_out[g] = M.pt_nobs[g];
        W.head[g] = n ? p : -1; W.tail[g] = n ? p : -1;
    }
    for (int s = tid; s < S.np + F.nj; s += nt) W.next[F.s0 + s] = -1;
    for (int o = tid; o < F.no; o += nt) {
        W.pool[F.e0 + o] = (uint32_t)snap_obs_slot(M.obs[F.o0 + o]) | SNAP_OBS_ALIVE; W.pfeat[F.e0 + o] = M.obs_feat[F.o0 + o];
        if (R.obs_touched) R.obs_touched[F.o0 + o] = 0;
    }
    for (int j = tid; j < F.nj; j += nt) { W.pool[F.e0 + F.no + j] = 0u; W.pfeat[F.e0 + F.no + j] = -1; W.rep[F.j0 + j] = -1; }
}

// ---- mObservations as a chain of segments ----------------------------------------------------------------------------------------------------
// Segment s of the stream: its first entry (a pool index) and its length
VIORB_HD int fuse_seg(const FuseMap& M, const FuseStream& F, int s, int* len) {
    if (s < F.S.np) { *len = M.obs_start[F.S.p0 + s + 1] - M.obs_start[F.S.p0 + s]; return F.e0 + (M.obs_start[F.S.p0 + s] - F.o0); }
    *len = 1;
    return F.e0 + F.no + (s - F.S.np);
}
VIORB_HD int32_t fuse_ld(const void* p) { return snap_ld_wg(static_cast<const int32_t*>(p)); }
VIORB_HD void fuse_st(void* p, int32_t v) { snap_st_wg(static_cast<int32_t*>(p), v); }
// mObservations.count(k) of point p, asked by one lane for itself: the chain is walked entry by entry
VIORB_HD bool fuse_lists_lane(const FuseMap& M, const FuseStream& F, const FuseWork& W, int p, int k) {
    const uint32_t want = (uint32_t)k | SNAP_OBS_ALIVE;
    bool hit = false;
    for (int s = fuse_ld(&W.head[F.S.p0 + p]); s >= 0; s = fuse_ld(&W.next[F.s0 + s])) {
        int len; const int e = fuse_seg(M, F, s, &len);
        for (int i = 0; i < len; i++) hit |= (uint32_t)fuse_ld(&W.pool[e + i]) == want;
    }
    return hit;
}
// The same asked by all lanes together: the lanes cover a segment. The same answer in every lane.
template <class Wave>
VIORB_HD bool fuse_lists(const FuseMap& M, const FuseStream& F, const FuseWork& W, int p, int k, int lane, int nl, Wave wave) {
    const uint32_t want = (uint32_t)k | SNAP_OBS_ALIVE;
    bool hit = false;
    for (int s = fuse_ld(&W.head[F.S.p0 + p]); s >= 0; s = fuse_ld(&W.next[F.s0 + s])) {
        int len; const int e = fuse_seg(M, F, s, &len);
        for (int i = lane; i < len; i += nl) hit |= (uint32_t)fuse_ld(&W.pool[e + i]) == want;
    }
    return wave.any(hit);
}
VIORB_HD int fuse_kp_weight(const FuseMap& M, const SnapStream& S, int k, int f) { return M.kp_stereo[M.kp_start[S.k0 + k] + f] ? 2 : 1; }
// One lane: segment s goes behind point p's chain
VIORB_HD void fuse_append(const FuseStream& F, const FuseWork& W, int p, int s, int s_last) {
    const int g = F.S.p0 + p, t = fuse_ld(&W.tail[g]);
    if (t < 0) fuse_st(&W.head[g], s); else fuse_st(&W.next[F.s0 + t], s);
    fuse_st(&W.tail[g], s_last);
}

// ---- MapPoint::AddObservation(k, f) of point p by list entry j of the stream (:105-116) --------------------------------------------------------
template <class Wave>
VIORB_HD void fuse_add_observation(const FuseMap& M, const FuseStream& F, const FuseWork& W, const FuseOut& R, int p, int k, int f, int j, int lane, int nl, Wave wave) {
    if (fuse_lists(M, F, W, p, k, lane, nl, wave)) return;                                      // :108-109
    if (lane == 0) {
        const int e = F.e0 + F.no + j;
        fuse_st(&W.pool[e], (int32_t)((uint32_t)k | SNAP_OBS_ALIVE)); fuse_st(&W.pfeat[e], f);
        fuse_append(F, W, p, F.S.np + j, F.S.np + j);
        fuse_st(&R.pt_nobs_out[F.S.p0 + p], fuse_ld(&R.pt_nobs_out[F.S.p0 + p]) + fuse_kp_weight(M, F.S, k, f));
    }
    snap_fence_wg();
}

// ---- MapPoint::Replace (:184-222): a->Replace(s) ------------------------------------------------------------------------------------------------
// The former observers are spread over the lanes; each asks for itself whether the survivor lists its key frame. The survivor's chain
// does not change while they ask: a's entries join it afterwards. Wave::sum adds a 0 / 1 value over the lanes.
template <class Wave>
VIORB_HD void fuse_replace(const FuseMap& M, const FuseStream& F, const FuseWork& W, const FuseOut& R, int a, int s, int lane, int nl, Wave wave) {
    if (a == s) return;                                                                         // :186-187
    const SnapStream& S = F.S;
    const int ga = S.p0 + a, gs = S.p0 + s;
    int gained = 0;
    for (int sg = fuse_ld(&W.head[ga]); sg >= 0; sg = fuse_ld(&W.next[F.s0 + sg])) {
        int len; const int e0 = fuse_seg(M, F, sg, &len);
        for (int i0 = 0; i0 < len; i0 += nl) {
            const int i = i0 + lane;
            int w1 = 0, w2 = 0;
            if (i < len) {
                const uint32_t w = (uint32_t)fuse_ld(&W.pool[e0 + i]);
                if (w & SNAP_OBS_ALIVE) {
                    const int k = snap_obs_slot(w), f = fuse_ld(&W.pfeat[e0 + i]);
                    int32_t* cell = R.kp_point_out + M.kp_start[S.k0 + k] + f;
                    if (!fuse_lists_lane(M, F, W, s, k)) {                                      // :207-211
                        fuse_st(cell, s);
                        w1 = 1; w2 = fuse_kp_weight(M, S, k, f) == 2;
                    } else {                                                                    // :214
                        fuse_st(cell, -1);
                        fuse_st(&W.pool[e0 + i], (int32_t)(w & ~SNAP_OBS_ALIVE));
                    }
                    if (R.obs_touched && e0 + i < F.e0 + F.no) R.obs_touched[F.o0 + (e0 + i - F.e0)] = 1;
                }
            }
            gained += wave.sum(w1) + wave.sum(w2);
        }
    }
    snap_fence_wg();
    if (lane == 0) {
        const int h = fuse_ld(&W.head[ga]);
        if (h >= 0) { fuse_append(F, W, s, h, fuse_ld(&W.tail[ga])); fuse_st(&W.head[ga], -1); fuse_st(&W.tail[ga], -1); }
        fuse_st(&R.pt_nobs_out[gs], fuse_ld(&R.pt_nobs_out[gs]) + gained);
        fuse_st(&W.bad[ga], 1); fuse_st(&W.replaced[ga], s);
        fuse_st(&W.found[gs], (int32_t)((uint32_t)fuse_ld(&W.found[gs]) + (uint32_t)fuse_ld(&W.found[ga])));         // :217-218, wrapping
        fuse_st(&W.visible[gs], (int32_t)((uint32_t)fuse_ld(&W.visible[gs]) + (uint32_t)fuse_ld(&W.visible[ga])));
        fuse_st(&W.dirty[gs], 1);                                                               // :219
    }
    snap_fence_wg();
}

// ---- one call --------------------------------------------------------------------------------------------------------------------------------
// Call c of the stream, gen = its ordinal + 1. Returns nFused (the same in every lane).
template <class Wave>
VIORB_HD int fuse_call(const FuseMap& M, const FuseStream& F, const FuseWork& W, const FuseOut& R, int c, int gen, int lane, int nl, Wave wave) {
    const SnapStream& S = F.S;
    const int kf = M.call_kf[c], kind = M.call_kind[c], n = M.call_n[c], l0 = M.call_list[c], f0 = M.call_feat[c], j0 = M.call_op[c] - F.j0;
    const int kp0 = M.kp_start[S.k0 + kf], nkp = fuse_nkp(M, S, kf);
    if (kind == FUSE_SIM3) {                                                                    // :993: GetMapPoints, the non-null and non-bad ones
        for (int i = lane; i < nkp; i += nl) {
            const int q = fuse_ld(&R.kp_point_out[kp0 + i]);
            if (q >= 0 && !fuse_ld(&W.bad[S.p0 + q])) fuse_st(&W.stamp[S.p0 + q], gen);
        }
        snap_fence_wg();
    }
    int nfused = 0;
    for (int i = 0; i < n; i++) {
        const int p = M.list_point[l0 + i], f = M.op_feat[f0 + i], j = j0 + i;
        int reason, q = -1;
        if (p < 0) reason = FUSE_NULL_POINT;
        else if (fuse_ld(&W.bad[S.p0 + p])) reason = FUSE_SKIP_BAD;
        else if (kind == FUSE_SIM3 ? fuse_ld(&W.stamp[S.p0 + p]) == gen : fuse_lists(M, F, W, p, kf, lane, nl, wave)) reason = FUSE_SKIP_IN_KF;
        else if (f < 0) reason = FUSE_NONE;
        else {
            q = fuse_ld(&R.kp_point_out[kp0 + f]);
            nfused++;
            if (q >= 0) {
                if (fuse_ld(&W.bad[S.p0 + q])) reason = FUSE_COUNTED_ONLY;
                else if (kind == FUSE_SIM3) { reason = FUSE_REPLACED_KF_POINT; if (lane == 0) W.rep[F.j0 + j] = q; }       // :1088
                else if (fuse_ld(&R.pt_nobs_out[S.p0 + q]) > fuse_ld(&R.pt_nobs_out[S.p0 + p])) { reason = FUSE_REPLACED_CANDIDATE; fuse_replace(M, F, W, R, p, q, lane, nl, wave); }
                else { reason = FUSE_REPLACED_KF_POINT; fuse_replace(M, F, W, R, q, p, lane, nl, wave); }
            } else {
                reason = FUSE_ADDED;
                fuse_add_observation(M, F, W, R, p, kf, f, j, lane, nl, wave);
                if (lane == 0) fuse_st(&R.kp_point_out[kp0 + f], p);
                snap_fence_wg();
            }
        }
        if (lane == 0) {
            if (R.op_reason) R.op_reason[F.j0 + j] = reason;
            if (R.op_other) R.op_other[F.j0 + j] = q;
        }
    }
    if (kind == FUSE_SIM3)                                                                      // LoopClosing.cc:633-640; rep is read by the lane that wrote it
        for (int i = 0; i < n; i++) {
            const int p = M.list_point[l0 + i], f = M.op_feat[f0 + i];
            if (p < 0 || f < 0) continue;                                                       // never recorded
            int a = lane == 0 ? W.rep[F.j0 + j0 + i] : 0;
            a = wave.first(a);
            if (a >= 0) fuse_replace(M, F, W, R, a, p, lane, nl, wave);
        }
    if (lane == 0 && R.call_nfused) R.call_nfused[c] = nfused;
    return nfused;
}

// ---- after the calls: the counts of the stream's points and the per-point outputs, point p -----------------------------------------------------
VIORB_HD void fuse_count_point(const FuseMap& M, const FuseStream& F, const FuseWork& W, const FuseOut& R, int p) {
    const SnapStream& S = F.S;
    const int g = S.p0 + p;
    const int bad = W.bad[g], dirty = W.dirty[g];
    int n = 0, nd = 0;
    for (int s = W.head[g]; s >= 0; s = W.next[F.s0 + s]) {
        int len; const int e = fuse_seg(M, F, s, &len);
        for (int i = 0; i < len; i++) {
            const uint32_t w = W.pool[e + i];
            if (!(w & SNAP_OBS_ALIVE)) continue;
            n++; nd += M.kf_bad[S.k0 + snap_obs_slot(w)] ? 0 : 1;                               // :272-274
        }
    }
    W.cnt[g] = n; W.dcnt[g] = (dirty && !bad) ? nd : 0;                                         // :258
    R.pt_bad_out[g] = (uint8_t)bad;
    if (R.pt_found_out) R.pt_found_out[g] = (int32_t)W.found[g];
    if (R.pt_visible_out) R.pt_visible_out[g] = (int32_t)W.visible[g];
    if (R.pt_replaced_out) R.pt_replaced_out[g] = W.replaced[g];
    if (R.pt_dirty) R.pt_dirty[g] = (uint8_t)dirty;
}

// ---- emit --------------------------------------------------------------------------------------------------------------------------------------
// Where the dirty lists of stream b begin: the streams before it, those that fit their regions (a refused stream counts 0)
VIORB_HD bool fuse_fits(const FuseMap& M, const FuseWork& W, int b) { return W.tot[b] <= M.obs_out_start[b + 1] - M.obs_out_start[b]; }
// Point p's observations at `at` and its dirty list at `dat`, in ascending key: gathered in chain order, then sorted where they lie
// (one thread; the keys are distinct)
VIORB_HD void fuse_emit_point(const FuseMap& M, const FuseStream& F, const FuseWork& W, const FuseOut& R, int p, int at, int dat) {
    const SnapStream& S = F.S;
    const int g = S.p0 + p;
    int n = 0;
    for (int s = W.head[g]; s >= 0; s = W.next[F.s0 + s]) {
        int len; const int e = fuse_seg(M, F, s, &len);
        for (int i = 0; i < len; i++) {
            const uint32_t w = W.pool[e + i];
            if (!(w & SNAP_OBS_ALIVE)) continue;
            const int k = snap_obs_slot(w), f = W.pfeat[e + i], r = W.rank[S.k0 + k];
            int at_i = n++;
            for (; at_i > 0 && W.rank[S.k0 + snap_obs_slot(R.obs_out[at + at_i - 1])] > r; at_i--) { R.obs_out[at + at_i] = R.obs_out[at + at_i - 1]; R.obs_feat_out[at + at_i] = R.obs_feat_out[at + at_i - 1]; }
            R.obs_out[at + at_i] = snap_obs_pack(k, M.kp_octave[M.kp_start[S.k0 + k] + f], M.kp_stereo[M.kp_start[S.k0 + k] + f]);
            R.obs_feat_out[at + at_i] = f;
        }
    }
    if (!R.dirty_obs_start || !W.dcnt[g]) return;
    for (int i = 0; i < n; i++) {
        const int k = snap_obs_slot(R.obs_out[at + i]);
        if (M.kf_bad[S.k0 + k]) continue;
        R.dirty_obs_kf[dat] = S.k0 + k; R.dirty_obs_feat[dat] = R.obs_feat_out[at + i]; dat++;
    }
}

// The phases of the device form on one host thread, stream by stream. W holds arrays of the sizes FuseWork names.
inline void fuse_run_host(const FuseMap& M, const FuseWork& W, const FuseOut& R) {
    struct One { int sum(int v) const { return v; } bool any(bool v) const { return v; } int first(int v) const { return v; } };
    for (int b = 0; b < M.batch; b++) {
        bool ok = fuse_validate_ranges(M, b, 0, 1);
        FuseStream F = {};
        if (ok) { F = fuse_stream(M, b); ok = fuse_validate_offsets(M, F, 0, 1); }
        ok = ok && fuse_validate_entries(M, F, 0, 1);
        if (ok) { snap_distinct_fill(M.kf_by_key + F.S.k0, F.S.nk, W.rank + F.S.k0, 0, 1); ok = snap_distinct_check(M.kf_by_key + F.S.k0, F.S.nk, W.rank + F.S.k0, 0, 1); }
        ok = ok && fuse_validate_observations(M, F, 0, 1);
        W.info[b] = ok; W.tot[b] = 0; W.dtot[b] = 0;
        if (!ok) continue;
        fuse_prepare(M, F, W, R, 0, 1);
        for (int c = 0; c < F.nc; c++) fuse_call(M, F, W, R, F.c0 + c, c + 1, 0, 1, One());
        for (int p = 0; p < F.S.np; p++) { fuse_count_point(M, F, W, R, p); W.tot[b] += W.cnt[F.S.p0 + p]; W.dtot[b] += W.dcnt[F.S.p0 + p]; }
    }
    int dbase = 0;
    for (int b = 0; b < M.batch; b++) {
        if (!W.info[b]) { R.status[b] = COV_INVALID; continue; }
        const FuseStream F = fuse_stream(M, b);
        const bool fits = fuse_fits(M, W, b), last = b + 1 == M.batch || !W.info[b + 1];
        int at = M.obs_out_start[b], dat = dbase;
        for (int p = 0; p < F.S.np; p++) {
            const int g = F.S.p0 + p;
            if (fits) { R.obs_start_out[g] = at; fuse_emit_point(M, F, W, R, p, at, dat); at += W.cnt[g]; }
            if (R.dirty_obs_start) { R.dirty_obs_start[g] = dat; if (fits) dat += W.dcnt[g]; }
        }
        if (last && fits) R.obs_start_out[F.S.p0 + F.S.np] = at;
        if (R.dirty_obs_start) R.dirty_obs_start[F.S.p0 + F.S.np] = dat;
        dbase = dat;
        if (R.need) R.need[b] = W.tot[b];
        R.status[b] = fits ? COV_OK : COV_OVERFLOW;
    }
}

} // namespace viorb
