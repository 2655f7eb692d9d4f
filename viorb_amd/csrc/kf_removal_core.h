// viorb_amd/csrc/kf_removal_core.h — KeyFrame::SetBadFlag and KeyFrame::SetErase for an ordered list of operations per stream, shared by
// the HIP kernels of kf_removal.hip and by the host (tests/cpp/kf_removal_core_host_test.cpp drives this header alone, under the address
// and undefined-behaviour sanitizers).
//
// What is restated (reference file:line):
//   KeyFrame::SetErase               src/KeyFrame.cc:728-742
//   KeyFrame::SetBadFlag             src/KeyFrame.cc:744-882  (guards :747-769, EraseConnection loop :772-773, EraseObservation loop :775-777,
//                                                              own state :782-783, spanning tree :786-843, mTcp :844, links :849-875)
//   KeyFrame::EraseConnection        src/KeyFrame.cc:890-904, UpdateBestCovisibles :429-448, GetWeight :492-500, ChangeParent :684-689
//   MapPoint::EraseObservation       src/MapPoint.cc:118-144, MapPoint::SetBadFlag :158-175
// Everything is integer arithmetic except mTcp, whose float products are those of map_correct_core.h (mc_camera_centre, mc_Tic).
//
// The working state. The rows of mConnectedKeyFrameWeights and of the ordered lists are the result's rows, as in covis_core.h, whose
// validator, row copy and rank sort are used as they are. Flags, parents, links, point words and mpRefKF live in the workspace. There is
// no copy of the observations: observation (p, k) of the snapshot is still in mObservations when p has not been cleared in this call
// and k has not been removed in this call while its keypoint table held p (kfr_obs_alive); a key frame is removed at most once per call.
#pragma once
#include <stdint.h>
#include "covis_core.h"             // the snapshot's layout and validator, the rows, cov_rebuild_ordered
#include "map_correct_core.h"       // mc_camera_centre, mc_Tic

namespace viorb {

enum { KFR_KF_ID0 = 1, KFR_KF_BAD = 2, KFR_KF_NOT_ERASE = 4, KFR_KF_TO_BE_ERASED = 8, KFR_KF_LOOP_EDGES = 16, KFR_KF_INPUT = 31,
       KFR_KF_REMOVED_NOW = 256 };                                    // kf_flags (VIORB_KFR_KF_*); the last one only in the working state
enum { KFR_PARENT_CHANGED = 4 };                                      // kf_touched beside COV_MAP_CHANGED and COV_ORD_REBUILT
enum { KFR_REMOVED = 0, KFR_ALREADY_BAD = 1, KFR_FIRST_KF = 2, KFR_DEFERRED = 3, KFR_RELEASED = 4 };      // op_reason
enum { KFR_SET_BAD_FLAG = 0, KFR_SET_ERASE = 1 };                     // op_kind
enum { KFR_NOBS_LIMIT = 1 << 29 };
enum { KFR_N_REBUILT = 0, KFR_N_POINTS_BAD = 1, KFR_N_CHILDREN = 2, KFR_N_FALLBACK = 3, KFR_N = 4 };      // the counters of one operation

// A point word: nObs in bits 2-31 (two's complement, |nObs| < 2^29: the validator), bit 1 = mObservations was cleared in this call, bit 0 = isBad()
VIORB_HD int32_t kfr_pt_pack(int32_t nobs, int bad, int cleared) { return (int32_t)(((uint32_t)nobs << 2) | (cleared ? 2u : 0u) | (bad ? 1u : 0u)); }
VIORB_HD int32_t kfr_pt_nobs(int32_t w) { return w >> 2; }
VIORB_HD int kfr_pt_bad(int32_t w) { return w & 1; }
VIORB_HD int kfr_pt_cleared(int32_t w) { return (w >> 1) & 1; }

// The snapshot (viorb_kfr_map: C holds what it shares with viorb_covis_map, the operations as its targets), the working state (the
// workspace; host: plain arrays) and the result (C: the rows and status; its other members are null except kf_touched)
struct KfrMap {
    CovMap C;
    const int32_t* kf_prev; const int32_t* kf_next; const float* kf_pose12; const int32_t* pt_nobs; const int32_t* pt_ref; const uint8_t* op_kind;
};
struct KfrWork {
    CovWork C;                           // rank, flags (int32 [n_kf]: KFR_KF_*) and info are used
    int32_t* parent; int32_t* prev; int32_t* next;       // [n_kf]
    int32_t* mark;                       // [n_kf]: the ordinal + 1 of the operation whose parent candidates hold the slot (device: LDS while a stream's key frames fit)
    int32_t* child;                      // [n_kf]: the children of the operation's key frame, in no order
    int32_t* pt; int32_t* ref;           // [n_pt]: point words, mpRefKF
};
struct KfrOut {
    CovOut C;
    int32_t* kf_parent_out; uint8_t* kf_flags_out; int32_t* kf_prev_out; int32_t* kf_next_out; uint8_t* kf_repreint; float* kf_Tcp_out;
    int32_t* pt_nobs_out; uint8_t* pt_bad_out; uint8_t* obs_alive; int32_t* pt_ref_out; int32_t* kp_point_out;
    int32_t* op_reason; int32_t* op_children; int32_t* op_fallback; int32_t* op_rebuilt; int32_t* op_points_bad;
};

// ---- the stream validator: covis_core.h's steps on C, and what this snapshot adds -------------------------------------------------------------
// After cov_validate_offsets: the links, mpRefKF, the observation counts, the kinds.
VIORB_HD bool kfr_validate_scalars(const KfrMap& M, const SnapStream& S, int b, int tid, int nt) {
    bool ok = true;
    for (int k = tid; k < S.nk; k += nt) ok &= snap_slot_or_none(M.kf_prev[S.k0 + k], S.nk) && snap_slot_or_none(M.kf_next[S.k0 + k], S.nk);
    for (int p = tid; p < S.np; p += nt) {
        const int32_t n = M.pt_nobs[S.p0 + p];
        ok &= snap_slot_or_none(M.pt_ref[S.p0 + p], S.nk) && n > -KFR_NOBS_LIMIT && n < KFR_NOBS_LIMIT;
    }
    for (int j = M.C.target_start[b] + tid, e = M.C.target_start[b + 1]; j < e; j += nt) ok &= M.op_kind[j] <= KFR_SET_ERASE;
    return ok;
}
VIORB_HD bool kfr_finite12(const float* T) { bool ok = true; for (int i = 0; i < 12; i++) ok &= (T[i] - T[i] == 0.0f); return ok; }
// After the slots have been accepted: every operation's key frame. One that is neither the first nor bad has a parent (:843 dereferences
// it); its chain of parents does not come back to it; its pose and its parent's are finite.
VIORB_HD bool kfr_validate_ops(const KfrMap& M, const SnapStream& S, int b, int tid, int nt) {
    bool ok = true;
    for (int j = M.C.target_start[b] + tid, e = M.C.target_start[b + 1]; j < e; j += nt) {
        const int x = M.C.target_kf[j], f = M.C.kf_flags[S.k0 + x], P = M.C.kf_parent[S.k0 + x];
        ok &= kfr_finite12(M.kf_pose12 + 12 * (size_t)(S.k0 + x));
        if (P < 0) { ok &= (f & (KFR_KF_ID0 | KFR_KF_BAD)) != 0; continue; }
        ok &= kfr_finite12(M.kf_pose12 + 12 * (size_t)(S.k0 + P));
        int k = P;
        for (int step = 0; step < S.nk && k >= 0; step++) { if (k == x) { ok = false; break; } k = M.C.kf_parent[S.k0 + k]; }
    }
    return ok;
}
// The working state of an accepted stream beside the rows (cov_copy_rows), the share of `tid`
VIORB_HD void kfr_prepare(const KfrMap& M, const SnapStream& S, const KfrWork& W, const KfrOut& R, int tid, int nt) {
    for (int k = tid; k < S.nk; k += nt) {
        const int g = S.k0 + k;
        W.parent[g] = M.C.kf_parent[g]; W.prev[g] = M.kf_prev[g]; W.next[g] = M.kf_next[g];
        if (R.kf_repreint) R.kf_repreint[g] = 0;
    }
    for (int p = tid; p < S.np; p += nt) { W.pt[S.p0 + p] = kfr_pt_pack(M.pt_nobs[S.p0 + p], M.C.pt_bad[S.p0 + p] != 0, 0); W.ref[S.p0 + p] = M.pt_ref[S.p0 + p]; }
    if (R.kp_point_out) for (int i = M.C.kp_start[S.k0] + tid, e = M.C.kp_start[S.k0 + S.nk]; i < e; i += nt) R.kp_point_out[i] = M.C.kp_point[i];
}

// ---- SetErase (:728-742) and the guards of SetBadFlag (:747-769) on the flags f: the reason, *nf = the flags they leave -------------------------
VIORB_HD int kfr_decide(int f, int kind, int* nf) {
    if (kind == KFR_SET_ERASE) {
        if (!(f & KFR_KF_LOOP_EDGES)) f &= ~KFR_KF_NOT_ERASE;
        *nf = f;
        if (!(f & KFR_KF_TO_BE_ERASED)) return KFR_RELEASED;
    }
    *nf = f;
    if (f & KFR_KF_BAD) return KFR_ALREADY_BAD;
    if (f & KFR_KF_ID0) return KFR_FIRST_KF;
    if (f & KFR_KF_NOT_ERASE) { *nf = f | KFR_KF_TO_BE_ERASED; return KFR_DEFERRED; }
    return KFR_REMOVED;
}

// ---- EraseConnection (:890-904): neighbour n forgets x and rebuilds its list -----------------------------------------------------------------
// Run by `nl` lanes in step (the device: one wavefront; the host: lane 0 of 1), as cov_add_connection. Returns 1 when n's map held x.
template <class Wave>
VIORB_HD int kfr_erase_connection(const CovMap& M, const SnapStream& S, const CovOut& R, const int32_t* rank, int n, int x, int lane, int nl, Wave wave) {
    const int g = S.k0 + n, rx = rank[x];
    int32_t* ck = R.conn_kf_out + (size_t)g * M.ccap; int32_t* cw = R.conn_w_out + (size_t)g * M.ccap;
    int32_t* ok_ = R.ord_kf_out + (size_t)g * M.ccap; int32_t* ow = R.ord_w_out + (size_t)g * M.ccap;
    const int cn = snap_ld_wg(&R.conn_n_out[g]);
    int pos = 0; bool found = false;
    for (int i0 = 0; i0 < cn; i0 += nl) {
        const int i = i0 + lane, s = i < cn ? snap_ld_wg(&ck[i]) : -1;
        pos += wave.sum(s >= 0 && rank[s] < rx ? 1 : 0);
        found = wave.any(s == x) || found;
    }
    if (!found) return 0;
    for (int lo = pos; lo < cn - 1; lo += nl) {                                                  // the tail moves down by one, from its start, nl entries at a time
        const int i = lo + lane;
        int s = 0, v = 0;
        if (i < cn - 1) { s = snap_ld_wg(&ck[i + 1]); v = snap_ld_wg(&cw[i + 1]); }
        snap_fence_wg();
        if (i < cn - 1) { snap_st_wg(&ck[i], s); snap_st_wg(&cw[i], v); }
        snap_fence_wg();
    }
    if (lane == 0) { snap_st_wg(&ck[cn - 1], -1); snap_st_wg(&cw[cn - 1], -1); snap_st_wg(&R.conn_n_out[g], cn - 1); }
    snap_fence_wg();
    cov_rebuild_ordered(ck, cw, ok_, ow, cn - 1, snap_ld_wg(&R.ord_n_out[g]), lane, nl);
    if (lane == 0) {
        snap_st_wg(&R.ord_n_out[g], cn - 1);
        if (R.kf_touched) R.kf_touched[g] |= COV_MAP_CHANGED | COV_ORD_REBUILT;
    }
    return 1;
}

// ---- the observations ------------------------------------------------------------------------------------------------------------------------
VIORB_HD bool kfr_table_holds(const CovMap& M, const SnapStream& S, int k, int p) {
    for (int i = M.kp_start[S.k0 + k], e = M.kp_start[S.k0 + k + 1]; i < e; i++) if (M.kp_point[i] == p) return true;
    return false;
}
// Observation word ow of point p, which has not been cleared: still in mObservations
VIORB_HD bool kfr_obs_alive(const CovMap& M, const SnapStream& S, const KfrWork& W, uint32_t ow, int p) {
    const int k = snap_obs_slot(ow);
    return !((W.C.flags[S.k0 + k] & KFR_KF_REMOVED_NOW) && kfr_table_holds(M, S, k, p));
}
// MapPoint::EraseObservation(x) of keypoint i (a flat index) of x, with MapPoint::SetBadFlag when nObs <= 2. One lane; the points of x's
// table are distinct (the precondition), so no two lanes work on one point. cnt: the operation's counters.
VIORB_HD void kfr_erase_observation(const CovMap& M, const SnapStream& S, const KfrWork& W, const KfrOut& R, const int32_t* rank, int x, int i, int32_t* cnt) {
    const int p = M.kp_point[i];
    if (p < 0) return;
    const int gp = S.p0 + p;
    const int32_t w = W.pt[gp];
    if (kfr_pt_cleared(w)) return;                                                              // mObservations is empty
    const int o0 = M.obs_start[gp], o1 = M.obs_start[gp + 1];
    int delta = 0;
    for (int o = o0; o < o1 && !delta; o++) if (snap_obs_slot(M.obs[o]) == x) delta = snap_obs_weight(M.obs[o]);
    if (!delta) return;                                                                         // MapPoint.cc:123
    const int nobs = kfr_pt_nobs(w) - delta;
    if (W.ref[gp] == x) {                                                                       // :133-134: begin() of what remains, the lowest key
        int best = -1, best_rank = SNAP_MAX_KF + 1;
        for (int o = o0; o < o1; o++) {
            const int k = snap_obs_slot(M.obs[o]);
            if (k != x && rank[k] < best_rank && kfr_obs_alive(M, S, W, M.obs[o], p)) { best = k; best_rank = rank[k]; }
        }
        W.ref[gp] = best;
    }
    const bool bad = nobs <= 2;                                                                 // :137
    if (bad) {
        if (R.kp_point_out)                                                                     // MapPoint.cc:168-172: EraseMapPointMatch at the remaining observers
            for (int o = o0; o < o1; o++) {
                const int k = snap_obs_slot(M.obs[o]);
                if (k == x || !kfr_obs_alive(M, S, W, M.obs[o], p)) continue;
                for (int j = M.kp_start[S.k0 + k], e = M.kp_start[S.k0 + k + 1]; j < e; j++) if (M.kp_point[j] == p) R.kp_point_out[j] = -1;
            }
        snap_fetch_add(&cnt[KFR_N_POINTS_BAD], 1);
    }
    W.pt[gp] = kfr_pt_pack(nobs, bad || kfr_pt_bad(w), bad);
}

// ---- the spanning tree (:786-841) ---------------------------------------------------------------------------------------------------------------
// mspChildrens of x: the good key frames whose parent is x. The share of `tid`; the list is in no order (the search orders by key).
VIORB_HD void kfr_collect_children(const SnapStream& S, const KfrWork& W, int x, int32_t* cnt, int tid, int nt) {
    for (int k = tid; k < S.nk; k += nt)
        if (W.parent[S.k0 + k] == x && !(W.C.flags[S.k0 + k] & KFR_KF_BAD)) W.child[S.k0 + snap_fetch_add(&cnt[KFR_N_CHILDREN], 1)] = k;
}
// One round of the search (:799-824), the share of wavefront `wave` of `nw` (a child each) and of `lane` of `nl` (the positions of its
// list): the best packed key, 0 for none. The key is (weight + 1) above the inverted (key of the child, list position): its maximum is
// the first strict maximum of the reference's loops. A child that has been adopted has another parent and is no longer looked at.
VIORB_HD unsigned long long kfr_search_round(const CovMap& M, const SnapStream& S, const KfrWork& W, const CovOut& R, const int32_t* rank, const int32_t* mark,
                                             int x, int gen, int n_child, int wave, int nw, int lane, int nl) {
    unsigned long long best = 0ull;
    for (int ci = wave; ci < n_child; ci += nw) {
        const int c = W.child[S.k0 + ci];
        if (W.parent[S.k0 + c] != x) continue;
        const size_t row = (size_t)(S.k0 + c) * M.ccap;
        const int on = R.ord_n_out[S.k0 + c], cn = R.conn_n_out[S.k0 + c];
        for (int i = lane; i < on; i += nl) {
            const int s = R.ord_kf_out[row + i];
            if (mark[s] != gen) continue;                                                       // :811
            const int rs = rank[s];
            int lo = 0, hi = cn;                                                                // GetWeight (:492-500): the child's map, 0 where it does not hold s
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (rank[R.conn_kf_out[row + mid]] < rs) lo = mid + 1; else hi = mid; }
            const int w = (lo < cn && R.conn_kf_out[row + lo] == s) ? R.conn_w_out[row + lo] : 0;
            if (w < 0) continue;                                                                // never above max = -1
            const unsigned long long key = ((unsigned long long)((long long)w + 1) << 32) | ((unsigned long long)(0xffff - rank[c]) << 16) | (unsigned long long)(0xffff - i);
            if (key > best) best = key;
        }
    }
    return best;
}
// The winner of a round (:826-831), one thread: ChangeParent, the child joins the candidates
VIORB_HD void kfr_adopt(const CovMap& M, const SnapStream& S, const KfrWork& W, const CovOut& R, int32_t* mark, unsigned long long key, int gen) {
    const int c = M.kf_by_key[S.k0 + (0xffff - (int)((key >> 16) & 0xffff))], i = 0xffff - (int)(key & 0xffff);
    W.parent[S.k0 + c] = R.ord_kf_out[(size_t)(S.k0 + c) * M.ccap + i];
    mark[c] = gen;
    if (R.kf_touched) R.kf_touched[S.k0 + c] |= KFR_PARENT_CHANGED;
}
// The children no round took go to x's parent P (:837-841), the share of `tid`
VIORB_HD void kfr_fallback(const SnapStream& S, const KfrWork& W, const CovOut& R, int x, int P, int n_child, int32_t* cnt, int tid, int nt) {
    for (int ci = tid; ci < n_child; ci += nt) {
        const int c = W.child[S.k0 + ci];
        if (W.parent[S.k0 + c] != x) continue;
        W.parent[S.k0 + c] = P;
        if (R.kf_touched) R.kf_touched[S.k0 + c] |= KFR_PARENT_CHANGED;
        snap_fetch_add(&cnt[KFR_N_FALLBACK], 1);
    }
}
// x's own map and list (:782-783), the share of `tid`
VIORB_HD void kfr_clear_own(const CovMap& M, const SnapStream& S, const CovOut& R, int x, int tid, int nt) {
    const size_t row = (size_t)(S.k0 + x) * M.ccap;
    const int cn = R.conn_n_out[S.k0 + x], on = R.ord_n_out[S.k0 + x];
    for (int i = tid; i < cn; i += nt) { R.conn_kf_out[row + i] = -1; R.conn_w_out[row + i] = -1; }
    for (int i = tid; i < on; i += nt) { R.ord_kf_out[row + i] = -1; R.ord_w_out[row + i] = -1; }
}
// mTcp (:844), mbBad (:845) and the links (:849-875), one thread, after every other step of the operation
VIORB_HD void kfr_finish_removal(const KfrMap& M, const SnapStream& S, const KfrWork& W, const KfrOut& R, int x, int P) {
    const int g = S.k0 + x;
    R.C.conn_n_out[g] = 0; R.C.ord_n_out[g] = 0;
    if (R.C.kf_touched) R.C.kf_touched[g] |= COV_MAP_CHANGED | COV_ORD_REBUILT;
    if (R.kf_Tcp_out && P >= 0) {                                                               // Tcw * Twc of the parent, Twc as KeyFrame::SetPose builds it
        const float* T = M.kf_pose12 + 12 * (size_t)g; const float* Tp = M.kf_pose12 + 12 * (size_t)(S.k0 + P);
        float Owp[3], Rcp[9], tcp[3];
        mc_camera_centre(Tp, Owp);
        mc_Tic(T, Tp, Owp, Rcp, tcp);
        float* o = R.kf_Tcp_out + 12 * (size_t)g;
        for (int i = 0; i < 9; i++) o[i] = Rcp[i];
        o[9] = tcp[0]; o[10] = tcp[1]; o[11] = tcp[2];
    }
    W.C.flags[g] |= KFR_KF_BAD | KFR_KF_REMOVED_NOW;
    const int prev = W.prev[g], next = W.next[g];
    if (prev >= 0) W.next[S.k0 + prev] = next;
    if (next >= 0) W.prev[S.k0 + next] = prev;
    W.prev[g] = -1; W.next[g] = -1;
    if (prev >= 0 && next >= 0 && R.kf_repreint) R.kf_repreint[S.k0 + next] = 1;
}
VIORB_HD void kfr_write_op(const KfrOut& R, int go, int reason, const int32_t* cnt) {
    const bool rm = reason == KFR_REMOVED;
    if (R.op_reason) R.op_reason[go] = reason;
    if (R.op_children) R.op_children[go] = rm ? cnt[KFR_N_CHILDREN] : 0;
    if (R.op_fallback) R.op_fallback[go] = rm ? cnt[KFR_N_FALLBACK] : 0;
    if (R.op_rebuilt) R.op_rebuilt[go] = rm ? cnt[KFR_N_REBUILT] : 0;
    if (R.op_points_bad) R.op_points_bad[go] = rm ? cnt[KFR_N_POINTS_BAD] : 0;
}
// The state the operations leave, the share of `tid`
VIORB_HD void kfr_write_state(const KfrMap& M, const SnapStream& S, const KfrWork& W, const KfrOut& R, int tid, int nt) {
    for (int k = tid; k < S.nk; k += nt) {
        const int g = S.k0 + k;
        if (R.kf_parent_out) R.kf_parent_out[g] = W.parent[g];
        if (R.kf_flags_out) R.kf_flags_out[g] = (uint8_t)(W.C.flags[g] & KFR_KF_INPUT);
        if (R.kf_prev_out) R.kf_prev_out[g] = W.prev[g];
        if (R.kf_next_out) R.kf_next_out[g] = W.next[g];
    }
    for (int p = tid; p < S.np; p += nt) {
        const int gp = S.p0 + p;
        const int32_t w = W.pt[gp];
        if (R.pt_nobs_out) R.pt_nobs_out[gp] = kfr_pt_nobs(w);
        if (R.pt_bad_out) R.pt_bad_out[gp] = (uint8_t)kfr_pt_bad(w);
        if (R.pt_ref_out) R.pt_ref_out[gp] = W.ref[gp];
        if (R.obs_alive)
            for (int o = M.C.obs_start[gp], e = M.C.obs_start[gp + 1]; o < e; o++) R.obs_alive[o] = (!kfr_pt_cleared(w) && kfr_obs_alive(M.C, S, W, M.C.obs[o], p)) ? 1 : 0;
    }
}

// The phases of the device form on one host thread, stream by stream. W holds arrays of the snapshot's totals.
inline void kfr_run_host(const KfrMap& M, const KfrWork& W, const KfrOut& R) {
    struct One { int sum(int v) const { return v; } bool any(bool v) const { return v; } };
    const CovMap& C = M.C;
    for (int b = 0; b < C.batch; b++) {
        bool ok = cov_validate_ranges(C, b, 0, 1);
        SnapStream S = {0, 0, 0, 0};
        if (ok) { S = snap_stream(C.kf_start, C.pt_start, b); ok = cov_validate_offsets(C, S, b, 0, 1); }
        ok = ok && kfr_validate_scalars(M, S, b, 0, 1);
        ok = ok && cov_validate_entries(C, S, b, 0, 1);
        if (ok) { snap_distinct_fill(C.kf_by_key + S.k0, S.nk, W.C.rank + S.k0, 0, 1); ok = snap_distinct_check(C.kf_by_key + S.k0, S.nk, W.C.rank + S.k0, 0, 1); }
        ok = ok && cov_validate_rows(C, S, W.C.rank + S.k0, 0, 1);
        ok = ok && kfr_validate_ops(M, S, b, 0, 1);
        W.C.info[b] = ok;
        if (!ok) { cov_write_refused(R.C, b); continue; }
        cov_copy_rows(C, S, W.C, R.C, 0, 1);
        kfr_prepare(M, S, W, R, 0, 1);
        int32_t* mark = W.mark + S.k0; const int32_t* rank = W.C.rank + S.k0;
        for (int k = 0; k < S.nk; k++) mark[k] = 0;
        for (int j = C.target_start[b]; j < C.target_start[b + 1]; j++) {
            const int x = C.target_kf[j], gen = j - C.target_start[b] + 1, g = S.k0 + x;
            int32_t cnt[KFR_N] = {0, 0, 0, 0};
            int nf;
            const int reason = kfr_decide(W.C.flags[g], M.op_kind[j], &nf);
            W.C.flags[g] = nf;
            if (reason == KFR_REMOVED) {
                const int P = W.parent[g];
                for (int i = 0, cn = R.C.conn_n_out[g]; i < cn; i++)
                    cnt[KFR_N_REBUILT] += kfr_erase_connection(C, S, R.C, rank, R.C.conn_kf_out[(size_t)g * C.ccap + i], x, 0, 1, One());
                for (int i = C.kp_start[g]; i < C.kp_start[g + 1]; i++) kfr_erase_observation(C, S, W, R, rank, x, i, cnt);
                kfr_clear_own(C, S, R.C, x, 0, 1);
                kfr_collect_children(S, W, x, cnt, 0, 1);
                if (P >= 0) mark[P] = gen;
                for (;;) {
                    const unsigned long long key = kfr_search_round(C, S, W, R.C, rank, mark, x, gen, cnt[KFR_N_CHILDREN], 0, 1, 0, 1);
                    if (!key) break;
                    kfr_adopt(C, S, W, R.C, mark, key, gen);
                }
                kfr_fallback(S, W, R.C, x, P, cnt[KFR_N_CHILDREN], cnt, 0, 1);
                kfr_finish_removal(M, S, W, R, x, P);
            }
            kfr_write_op(R, j, reason, cnt);
        }
        kfr_write_state(M, S, W, R, 0, 1);
        R.C.status[b] = COV_OK;
    }
}

} // namespace viorb
