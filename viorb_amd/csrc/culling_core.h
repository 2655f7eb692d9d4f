// viorb_amd/csrc/culling_core.h — the arithmetic of LocalMapping::KeyFrameCulling and LocalMapping::MapPointCulling, shared by the HIP
// kernels of culling.hip and by the host (tests/cpp/culling_core_host_test.cpp drives this header alone, under the address and
// undefined-behaviour sanitizers, against the literal loop).
//
// What is restated (reference file:line):
//   LocalMapping::KeyFrameCulling     src/LocalMapping.cc:1694-1821  (skip tests :1697-1750, count :1772-1817, decision :1819)
//   KeyFrame::SetBadFlag              src/KeyFrame.cc:744-882        (mbNotErase :765-769, EraseObservation loop :775-777, links :849-875)
//   MapPoint::EraseObservation        src/MapPoint.cc:118-144, MapPoint::SetBadFlag :158-175
//   LocalMapping::MapPointCulling     src/LocalMapping.cc:1198-1233
// Everything is integer arithmetic except three double compares (two time tests, 0.9 * nMPs) and the float depth compare.
#pragma once
#include <stdint.h>
#include <math.h>
#include "map_snapshot_core.h"      // the snapshot's layout, its observation word, the validator's checks, the memory shim

namespace viorb {

// cand_reason (VIORB_KFC_* of include/viorb_culling.h) and the codes of map-point culling (VIORB_MPC_*)
enum { KFC_FIRST_KF = 0, KFC_TIME_GAP = 1, KFC_BEFORE_CURRENT = 2, KFC_RECENT = 3, KFC_KEPT = 4, KFC_CULLED = 5, KFC_DEFERRED = 6 };
enum { MPC_KEEP = 0, MPC_DROP_BAD = 1, MPC_CULL_FOUND_RATIO = 2, MPC_CULL_FEW_OBS = 3, MPC_RETIRE = 4 };
enum { CULL_KF_FIRST = 1, CULL_KF_NOT_ERASE = 2 };                              // kf_flags
enum { CULL_ST_BAD = 1, CULL_ST_TO_BE_ERASED = 2, CULL_ST_REPREINT = 4 };       // the working state of a key frame
enum { CULL_NOBS_LIMIT = 1 << 30 };

// A point word: nObs in bits 1-31 (two's complement), isBad() in bit 0; |nObs| < 2^30 (the validator), so nothing overflows.
VIORB_HD int32_t cull_pt_pack(int32_t nobs, int bad) { return (int32_t)(((uint32_t)nobs << 1) | (bad ? 1u : 0u)); }
VIORB_HD int32_t cull_pt_nobs(int32_t w) { return w >> 1; }
VIORB_HD int cull_pt_bad(int32_t w) { return w & 1; }

// The snapshot (viorb_cull_map) and the working state (the workspace; host: plain arrays)
struct CullMap {
    int batch, n_kf, n_cand, n_kp, n_pt, n_obs;
    const int32_t* kf_start; const uint8_t* kf_flags; const double* kf_time; const int32_t* kf_prev; const int32_t* kf_next;
    const int32_t* cur_kf; const uint8_t* vins_inited; const float* th_depth;
    const int32_t* cand_start; const int32_t* cand_kf; const int32_t* kp_start; const int32_t* kp_point; const uint8_t* kp_octave; const float* kp_depth;
    const int32_t* pt_start; const int32_t* pt_nobs; const uint8_t* pt_bad; const int32_t* obs_start; const uint32_t* obs;
};
struct CullWork {
    int32_t* pt; uint32_t* obs;                          // [n_pt] point words, [n_obs] observation words with the alive bit
    int32_t* cand_of_kf; int32_t* prev; int32_t* next;   // [n_kf]: the candidate ordinal of a slot or -1 (the validator's mark: none twice); the current links
    uint8_t* kf_state;                                   // [n_kf] CULL_ST_*
    int32_t* ok;                                         // [batch]
};
struct CullStream : SnapStream { int c0, nc; };          // the stream's ranges of key frames and points, and of candidates

// ---- the stream validator: the steps of map_snapshot_core.h on this snapshot's arrays ----------------------------------------------------
// The erase step updates point and observation words with integer atomics, so the ordered kernel reads them with snap_ld_agent.
// Step 1: kp_start is nested under cand_start, obs_start under pt_start.
VIORB_HD bool cull_validate_ranges(const CullMap& M, int b, int tid, int nt) {
    bool ok = true;
    for (int i = tid; i <= b; i += nt) {
        ok = ok && snap_span(M.kf_start, i, i + 1, M.n_kf);
        if (!(snap_span(M.cand_start, i, i + 1, M.n_cand) && snap_span(M.pt_start, i, i + 1, M.n_pt))) { ok = false; continue; }
        ok = ok && snap_span(M.kp_start, M.cand_start[i], M.cand_start[i + 1], M.n_kp);
        ok = ok && snap_span(M.obs_start, M.pt_start[i], M.pt_start[i + 1], M.n_obs);
    }
    return ok;
}
VIORB_HD CullStream cull_stream(const CullMap& M, int b) {
    CullStream S;
    static_cast<SnapStream&>(S) = snap_stream(M.kf_start, M.pt_start, b);
    S.c0 = M.cand_start[b]; S.nc = M.cand_start[b + 1] - S.c0;
    return S;
}
// Step 2: at least one key frame and the current one among them, the nested offsets, the candidates' slots and their links (only
// candidates' links are followed), the observation counts.
VIORB_HD bool cull_validate_offsets(const CullMap& M, const CullStream& S, int b, int tid, int nt) {
    bool ok = S.nk >= 1 && S.nk <= SNAP_MAX_KF && M.cur_kf[b] >= 0 && M.cur_kf[b] < S.nk;
    ok &= snap_offsets_run(M.kp_start, S.c0, S.nc, M.n_kp, tid, nt);
    ok &= snap_offsets_run(M.obs_start, S.p0, S.np, M.n_obs, tid, nt);
    for (int j = tid; j < S.nc; j += nt) {
        const int c = M.cand_kf[S.c0 + j];
        if (c < 0 || c >= S.nk) { ok = false; continue; }
        const int p = M.kf_prev[S.k0 + c], n = M.kf_next[S.k0 + c];
        ok &= snap_slot_or_none(p, S.nk) && snap_slot_or_none(n, S.nk);
    }
    for (int p = tid; p < S.np; p += nt) { const int32_t n = M.pt_nobs[S.p0 + p]; ok &= n > -CULL_NOBS_LIMIT && n < CULL_NOBS_LIMIT; }
    return ok;
}
// Step 3: every point index of the keypoint tables and every slot of the observation words.
VIORB_HD bool cull_validate_entries(const CullMap& M, const CullStream& S, int tid, int nt) {
    bool ok = snap_entries_within(M.kp_point, M.kp_start[S.c0], M.kp_start[S.c0 + S.nc], -1, S.np, tid, nt);
    ok &= snap_obs_slots_below(M.obs, M.obs_start[S.p0], M.obs_start[S.p0 + S.np], S.nk, tid, nt);
    return ok;
}
// The working state of the share of `tid`. cand_of_kf holds -1 in every slot before step 4 (snap_distinct_fill of cand_kf, after a
// barrier) gives the candidates' slots their ordinals; a key frame listed twice is refused by snap_distinct_check.
VIORB_HD void cull_prepare(const CullMap& M, const CullStream& S, const CullWork& W, int tid, int nt) {
    for (int p = tid; p < S.np; p += nt) W.pt[S.p0 + p] = cull_pt_pack(M.pt_nobs[S.p0 + p], M.pt_bad[S.p0 + p] != 0);
    for (int o = M.obs_start[S.p0] + tid, e = M.obs_start[S.p0 + S.np]; o < e; o += nt) W.obs[o] = (M.obs[o] & 0x01ffffffu) | SNAP_OBS_ALIVE;
    for (int k = tid; k < S.nk; k += nt) { W.cand_of_kf[S.k0 + k] = -1; W.prev[S.k0 + k] = M.kf_prev[S.k0 + k]; W.next[S.k0 + k] = M.kf_next[S.k0 + k]; W.kf_state[S.k0 + k] = 0; }
}

// ---- the skip tests (:1697-1750) on the current links: a reason, or -1 when the candidate is counted -----------------------------------
VIORB_HD int cull_skip(const CullMap& M, const CullStream& S, const CullWork& W, int c, int cur, bool vins_inited) {
    if (M.kf_flags[S.k0 + c] & CULL_KF_FIRST) return KFC_FIRST_KF;
    const int prev = W.prev[S.k0 + c], next = W.next[S.k0 + c];
    if (prev >= 0 && next >= 0 && !vins_inited && fabs(M.kf_time[S.k0 + next] - M.kf_time[S.k0 + prev]) > 0.5) return KFC_TIME_GAP;
    if (next == cur) return KFC_BEFORE_CURRENT;
    if (M.kf_time[S.k0 + c] >= M.kf_time[S.k0 + cur] - 0.2) return KFC_RECENT;
    return -1;
}

// ---- the count of one keypoint (:1774-1814): bit 0 nMPs++, bit 1 nRedundantObservations++ ----------------------------------------------
VIORB_HD int cull_count_keypoint(const CullMap& M, const CullStream& S, const CullWork& W, int c, int i, bool monocular, float th_depth) {
    const int p = M.kp_point[i];
    if (p < 0) return 0;
    const int32_t w = snap_ld_agent(&W.pt[S.p0 + p]);
    if (cull_pt_bad(w)) return 0;
    if (!monocular) { const float d = M.kp_depth[i]; if (d > th_depth || d < 0) return 0; }
    const int level = M.kp_octave[i];
    int n = 0;
    for (int o = M.obs_start[S.p0 + p], e = M.obs_start[S.p0 + p + 1]; o < e; o++) {
        const uint32_t ow = snap_ld_agent(&W.obs[o]);
        if (!(ow & SNAP_OBS_ALIVE)) continue;
        if (snap_obs_slot(ow) == c) continue;
        if (snap_obs_octave(ow) <= level + 1) n++;           // the break at thObs does not change nObs >= thObs
    }
    return 1 | ((cull_pt_nobs(w) > 3 && n >= 3) ? 2 : 0);
}

// :1819, in double as the reference compares an int with 0.9 * int
VIORB_HD bool cull_decide(int redundant, int mps) { return (double)redundant > 0.9 * (double)mps; }

// ---- the erase step of one keypoint (KeyFrame.cc:775-777, MapPoint.cc:118-175) ---------------------------------------------------------
// The lane that flips the alive bit of the point's observation of c does the erase; an entry that names the same point again finds the
// bit already clear. When the point goes bad its remaining observations are cleared.
VIORB_HD void cull_erase_keypoint(const CullMap& M, const CullStream& S, const CullWork& W, int c, int i) {
    const int p = M.kp_point[i];
    if (p < 0) return;
    const int o0 = M.obs_start[S.p0 + p], o1 = M.obs_start[S.p0 + p + 1];
    int delta = 0;
    for (int o = o0; o < o1; o++) {
        const uint32_t ow = snap_ld_agent(&W.obs[o]);
        if ((ow & SNAP_OBS_ALIVE) && snap_obs_slot(ow) == c && (snap_fetch_and(&W.obs[o], ~SNAP_OBS_ALIVE) & SNAP_OBS_ALIVE)) delta += snap_obs_weight(ow);
    }
    if (delta == 0) return;
    const int32_t w = snap_fetch_add(&W.pt[S.p0 + p], -2 * delta) - 2 * delta;
    const bool goes_bad = cull_pt_nobs(w) <= 2;                                  // MapPoint.cc:137
    if (!goes_bad) return;
    snap_or(&W.pt[S.p0 + p], 1);
    for (int o = o0; o < o1; o++) snap_fetch_and(&W.obs[o], ~SNAP_OBS_ALIVE);    // mObservations.clear()
}

// ---- the links (KeyFrame.cc:849-875), one thread ---------------------------------------------------------------------------------------
VIORB_HD void cull_unlink(const CullStream& S, const CullWork& W, int c) {
    const int prev = W.prev[S.k0 + c], next = W.next[S.k0 + c];
    if (prev >= 0) W.next[S.k0 + prev] = next;
    if (next >= 0) W.prev[S.k0 + next] = prev;
    W.prev[S.k0 + c] = -1; W.next[S.k0 + c] = -1;
    if (prev >= 0 && next >= 0) W.kf_state[S.k0 + next] |= CULL_ST_REPREINT;
    W.kf_state[S.k0 + c] |= CULL_ST_BAD;
}

// ---- LocalMapping::MapPointCulling :1214-1231, one point ---------------------------------------------------------------------------------
// GetFoundRatio() < 0.25f is float(mnFound) / mnVisible < 0.25f. For 0 <= found, visible < 2^24 both conversions are exact and the
// correctly rounded quotient is below 0.25f exactly when 4 * found < visible: found / visible <= 0.25 - 1 / (4 visible), and 1 / (4 visible)
// > 2^-26 is more than half an ulp (2^-27) below 0.25, while a quotient >= 0.25 rounds to >= 0.25. visible == 0 gives inf or NaN, neither
// below 0.25f, as 4 * found < 0 is false.
VIORB_HD int cull_map_point(int bad, int32_t found, int32_t visible, int32_t first_kf_id, int32_t nobs, int32_t cur_kf_id, bool monocular) {
    if (bad) return MPC_DROP_BAD;
    if (4 * (int64_t)found < (int64_t)visible) return MPC_CULL_FOUND_RATIO;
    const int64_t age = (int64_t)cur_kf_id - (int64_t)first_kf_id;
    if (age >= 2 && nobs <= (monocular ? 2 : 3)) return MPC_CULL_FEW_OBS;
    if (age >= 3) return MPC_RETIRE;
    return MPC_KEEP;
}

// ---- the result arrays (viorb_cull_result; every pointer may be null) and what a stream writes into them --------------------------------
struct CullOut {
    int32_t* cand_reason; int32_t* cand_redundant; int32_t* cand_mps; int32_t* cand_recounted; int32_t* culled_order;
    int32_t* n_culled; int32_t* status;
    uint8_t* kf_bad; uint8_t* kf_to_be_erased; int32_t* kf_prev_out; int32_t* kf_next_out; uint8_t* kf_repreint;
    int32_t* pt_nobs_out; uint8_t* pt_bad_out; uint8_t* obs_alive;
};
VIORB_HD void cull_write_candidate(const CullOut& R, int g, int reason, int redundant, int mps, int recounted) {
    if (R.cand_reason) R.cand_reason[g] = reason;
    if (R.cand_redundant) R.cand_redundant[g] = redundant;
    if (R.cand_mps) R.cand_mps[g] = mps;
    if (R.cand_recounted) R.cand_recounted[g] = recounted;
}
// The state the loop leaves, the share of `tid`
VIORB_HD void cull_write_state(const CullMap& M, const CullStream& S, const CullWork& W, const CullOut& R, int n_culled, int tid, int nt) {
    for (int k = tid; k < S.nk; k += nt) {
        const int st = snap_ld_agent(&W.kf_state[S.k0 + k]);
        if (R.kf_bad) R.kf_bad[S.k0 + k] = (st & CULL_ST_BAD) ? 1 : 0;
        if (R.kf_to_be_erased) R.kf_to_be_erased[S.k0 + k] = (st & CULL_ST_TO_BE_ERASED) ? 1 : 0;
        if (R.kf_repreint) R.kf_repreint[S.k0 + k] = (st & CULL_ST_REPREINT) ? 1 : 0;
        if (R.kf_prev_out) R.kf_prev_out[S.k0 + k] = snap_ld_agent(&W.prev[S.k0 + k]);
        if (R.kf_next_out) R.kf_next_out[S.k0 + k] = snap_ld_agent(&W.next[S.k0 + k]);
    }
    if (R.culled_order) for (int j = n_culled + tid; j < S.nc; j += nt) R.culled_order[S.c0 + j] = -1;
    if (R.pt_nobs_out || R.pt_bad_out)
        for (int p = tid; p < S.np; p += nt) {
            const int32_t w = snap_ld_agent(&W.pt[S.p0 + p]);
            if (R.pt_nobs_out) R.pt_nobs_out[S.p0 + p] = cull_pt_nobs(w);
            if (R.pt_bad_out) R.pt_bad_out[S.p0 + p] = (uint8_t)cull_pt_bad(w);
        }
    if (R.obs_alive) for (int o = M.obs_start[S.p0] + tid, e = M.obs_start[S.p0 + S.np]; o < e; o += nt) R.obs_alive[o] = (snap_ld_agent(&W.obs[o]) & SNAP_OBS_ALIVE) ? 1 : 0;
}

// The phases of the device form on one host thread, stream by stream: validate and prepare, then the ordered loop. W holds arrays of
// the snapshot's totals.
inline void cull_run_host(const CullMap& M, const CullWork& W, const CullOut& R, bool monocular) {
    for (int b = 0; b < M.batch; b++) {
        bool ok = cull_validate_ranges(M, b, 0, 1);
        CullStream S = CullStream();
        if (ok) { S = cull_stream(M, b); ok = cull_validate_offsets(M, S, b, 0, 1); }
        ok = ok && cull_validate_entries(M, S, 0, 1);
        if (ok) {
            cull_prepare(M, S, W, 0, 1);
            snap_distinct_fill(M.cand_kf + S.c0, S.nc, W.cand_of_kf + S.k0, 0, 1);
            ok = snap_distinct_check(M.cand_kf + S.c0, S.nc, W.cand_of_kf + S.k0, 0, 1);
        }
        W.ok[b] = ok;
        if (R.status) R.status[b] = ok ? 0 : -1;
        if (R.n_culled) R.n_culled[b] = 0;
        if (!ok) continue;
        const float th = M.th_depth[b];
        int n_culled = 0;
        for (int j = 0; j < S.nc; j++) {
            const int c = M.cand_kf[S.c0 + j], i0 = M.kp_start[S.c0 + j], i1 = M.kp_start[S.c0 + j + 1];
            int reason = cull_skip(M, S, W, c, M.cur_kf[b], M.vins_inited[b] != 0), mps = 0, red = 0, counted = 0;
            if (reason < 0) {
                counted = 1;
                for (int i = i0; i < i1; i++) { const int r = cull_count_keypoint(M, S, W, c, i, monocular, th); mps += r & 1; red += (r >> 1) & 1; }
                reason = KFC_KEPT;
                if (cull_decide(red, mps)) {
                    if (M.kf_flags[S.k0 + c] & CULL_KF_NOT_ERASE) { reason = KFC_DEFERRED; W.kf_state[S.k0 + c] |= CULL_ST_TO_BE_ERASED; }
                    else {
                        reason = KFC_CULLED;
                        for (int i = i0; i < i1; i++) cull_erase_keypoint(M, S, W, c, i);
                        cull_unlink(S, W, c);
                        if (R.culled_order) R.culled_order[S.c0 + n_culled] = j;
                        n_culled++;
                    }
                }
            }
            cull_write_candidate(R, S.c0 + j, reason, red, mps, counted);
        }
        if (R.n_culled) R.n_culled[b] = n_culled;
        cull_write_state(M, S, W, R, n_culled, 0, 1);
    }
}

} // namespace viorb
