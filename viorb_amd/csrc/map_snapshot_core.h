// viorb_amd/csrc/map_snapshot_core.h — what the device stages that read the map (culling_core.h, local_map_core.h) share: the snapshot's
// layout and its observation word, the bound checks their validators are composed of, and the loads, stores and read-modify-writes of
// a working state that several lanes touch. Compiled for the host and for the device like the other *_core.h.
//
// A batch of per-stream snapshots is a set of flat arrays: kf_start and pt_start [batch + 1] cut the key-frame and point arrays into
// streams; nested CSR offsets under them (kp_start, obs_start, child_start) are indices into flat arrays of the whole batch; slots and
// point indices are stream-local.
#pragma once
#include <stdint.h>
#include "orb_math.h"               // VIORB_HD

namespace viorb {

// ---- the observation word ----------------------------------------------------------------------------------------------------------------
// Bits 0-15 the key-frame slot (so a stream holds at most SNAP_MAX_KF key frames), 16-23 the octave of that key frame's keypoint, bit 24
// mvuRight >= 0. A working copy may add bit 31: the observation is still in mObservations.
enum { SNAP_MAX_KF = 65535 };
static const uint32_t SNAP_OBS_STEREO = 1u << 24, SNAP_OBS_ALIVE = 1u << 31;
VIORB_HD uint32_t snap_obs_pack(int slot, int octave, int stereo) { return (uint32_t)slot | ((uint32_t)octave << 16) | (stereo ? SNAP_OBS_STEREO : 0u); }
VIORB_HD int snap_obs_slot(uint32_t w) { return (int)(w & 0xffffu); }
VIORB_HD int snap_obs_octave(uint32_t w) { return (int)((w >> 16) & 0xffu); }
VIORB_HD int snap_obs_weight(uint32_t w) { return (w & SNAP_OBS_STEREO) ? 2 : 1; }      // AddObservation / EraseObservation: nObs += 2 when stereo

// ---- the working state in memory ---------------------------------------------------------------------------------------------------------
// The host forms are the plain operation. On the device two situations need more than a plain load or store:
//  - A word that integer atomics change (snap_fetch_add, snap_fetch_and, snap_or, snap_min) is changed in L2, where they execute. Whoever
//    reads it afterwards uses snap_ld_agent, a relaxed agent-scope load, which is served by L2, past an L1 line from before the atomic.
//  - Words that the lanes of one workgroup write and read among themselves inside a phase, with no barrier in between (one wavefront's
//    lanes in step), go through snap_ld_wg / snap_st_wg, relaxed workgroup-scope atomics, with snap_fence_wg after a write that a later
//    read depends on, so the compiler keeps them in memory and in order. Workgroup scope suffices: a workgroup runs on one CU, whose L1
//    and LDS its wavefronts share. For the same reason plain stores of one phase are visible to the workgroup's next phase after a
//    __syncthreads(), which carries the workgroup-scope release and acquire and waits for the outstanding stores.
#if defined(__HIP_DEVICE_COMPILE__)
template <class T> VIORB_HD T snap_ld_agent(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
VIORB_HD int32_t snap_ld_wg(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
VIORB_HD void snap_st_wg(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
VIORB_HD void snap_fence_wg() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }
VIORB_HD int32_t snap_fetch_add(int32_t* p, int32_t v) { return atomicAdd(p, v); }
VIORB_HD uint32_t snap_fetch_and(uint32_t* p, uint32_t v) { return atomicAnd(p, v); }
VIORB_HD void snap_or(int32_t* p, int32_t v) { atomicOr(p, v); }
VIORB_HD void snap_min(int32_t* p, int32_t v) { atomicMin(p, v); }
#else
template <class T> VIORB_HD T snap_ld_agent(const T* p) { return *p; }
VIORB_HD int32_t snap_ld_wg(const int32_t* p) { return *p; }
VIORB_HD void snap_st_wg(int32_t* p, int32_t v) { *p = v; }
VIORB_HD void snap_fence_wg() {}
VIORB_HD int32_t snap_fetch_add(int32_t* p, int32_t v) { const int32_t o = *p; *p = o + v; return o; }
VIORB_HD uint32_t snap_fetch_and(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o & v; return o; }
VIORB_HD void snap_or(int32_t* p, int32_t v) { *p |= v; }
VIORB_HD void snap_min(int32_t* p, int32_t v) { if (v < *p) *p = v; }
#endif

// ---- a stream's ranges of key frames and points --------------------------------------------------------------------------------------------
struct SnapStream { int k0, nk, p0, np; };
VIORB_HD SnapStream snap_stream(const int32_t* kf_start, const int32_t* pt_start, int b) {
    SnapStream S;
    S.k0 = kf_start[b]; S.nk = kf_start[b + 1] - S.k0; S.p0 = pt_start[b]; S.np = pt_start[b + 1] - S.p0;
    return S;
}

// ---- the bound checks a stream validator is composed of -----------------------------------------------------------------------------------
// A validator runs in steps. Thread `tid` of `nt` checks its share of a step and the caller ANDs the shares over the workgroup before
// the next step (the host calls with 0 of 1); a step whose predecessor failed is not run. No step reads through an index that an
// earlier step has not accepted:
//   1. the batch-level offsets of streams 0..b, and the nested offsets at those streams' boundaries (snap_span);
//   2. the stream's scalars, its nested offsets (snap_offsets_run) and whatever is indexed by a key frame or a point alone;
//   3. the entries that step 2's offsets delimit (snap_entries_within, snap_obs_slots_below);
//   4. where a list must hold distinct slots, snap_distinct_fill, a barrier, snap_distinct_check.
// Steps 1 and 2 together keep the ranges of two accepted streams apart in every array, whatever a refused stream between them holds:
// a refused stream is neither read through nor written, and its neighbours' results do not depend on it.
// Inside a step every index read at was accepted by an earlier step, so the loops below load unconditionally and AND the compares
// (`ok &=`): a failed compare need not stop the loads after it, and no load waits for the compare before it.

// start[i0] .. start[i1] is a span of [0, total]: non-negative, ascending, inside the total. i0 <= i1 index start[].
VIORB_HD bool snap_span(const int32_t* start, int i0, int i1, int total) { return start[i0] >= 0 && start[i0] <= start[i1] && start[i1] <= total; }
// -1 (none) or a slot below n
VIORB_HD bool snap_slot_or_none(int v, int n) { return v >= -1 && v < n; }
// The run start[r0 .. r0 + n] of nested offsets: each within [0, total], ascending.
VIORB_HD bool snap_offsets_run(const int32_t* start, int r0, int n, int total, int tid, int nt) {
    bool ok = true;
    for (int j = tid; j <= n; j += nt) {
        const int a = start[r0 + j], up = j < n ? start[r0 + j + 1] : a;
        ok &= a >= 0 && a <= total && a <= up;
    }
    return ok;
}
// Every entry of v[i0, i1) within [lo, hi)
VIORB_HD bool snap_entries_within(const int32_t* v, int i0, int i1, int lo, int hi, int tid, int nt) {
    bool ok = true;
    for (int i = i0 + tid; i < i1; i += nt) { const int e = v[i]; ok &= e >= lo && e < hi; }
    return ok;
}
// Every observation word of obs[o0, o1) names a slot below nk
VIORB_HD bool snap_obs_slots_below(const uint32_t* obs, int o0, int o1, int nk, int tid, int nt) {
    bool ok = true;
    for (int o = o0 + tid; o < o1; o += nt) ok &= snap_obs_slot(obs[o]) < nk;
    return ok;
}
// n in-range slots are distinct when every one finds its own ordinal in mark[] after all have written theirs (fill, a barrier, check):
// of two ordinals that name one slot, one lost it.
VIORB_HD void snap_distinct_fill(const int32_t* slots, int n, int32_t* mark, int tid, int nt) { for (int j = tid; j < n; j += nt) mark[slots[j]] = j; }
VIORB_HD bool snap_distinct_check(const int32_t* slots, int n, const int32_t* mark, int tid, int nt) {
    bool ok = true;
    for (int j = tid; j < n; j += nt) ok &= mark[slots[j]] == j;
    return ok;
}

} // namespace viorb
