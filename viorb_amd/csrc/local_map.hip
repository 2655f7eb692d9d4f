// viorb_amd/csrc/local_map.hip — Tracking::UpdateLocalMap for a batch of streams (include/viorb_local_map.h):
//   k_ulm_prepare       validates a stream's part of the snapshot and resets its points' first positions     (one workgroup per stream)
//   k_ulm_key_frames    UpdateLocalKeyFrames: votes, the voted list in key order, pKFmax, the neighbour loop  (one workgroup per stream)
//   k_ulm_claim_points  every (list ordinal, keypoint) entry claims its point with atomicMin of its position  (workgroups over entries)
//   k_ulm_local_points  UpdateLocalPoints: the entries that own their point, compacted in order               (one workgroup per stream)
//   k_ulm_frame_marks, k_ulm_gather   the packing for viorb_frontend_search_local_points_device
// The logic is local_map_core.h. Shape (DESIGN.md "Local map"): votes are integer atomic adds, in LDS while the stream's key frames fit;
// the voted list is an ordered compaction over kf_by_key by prefix scan (no sort); the neighbour loop is sequential, at most 81
// iterations, and one wavefront runs it with ballots; the points are deduplicated by the lowest position, which no schedule changes.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "local_map_core.h"

namespace viorb {

enum { ULM_WAVE = 64, ULM_PREP_THREADS = 256, ULM_KF_THREADS = 256, ULM_PT_THREADS = 1024, ULM_CLAIM_THREADS = 256, ULM_CLAIM_GROUPS = 32,
       ULM_LDS_KF = 2048, ULM_GATHER_THREADS = 256 };

// The exclusive prefix of v over the workgroup's NT threads and the total, to every thread. Every thread calls it.
template <int NT> __device__ __forceinline__ int ulm_block_scan(int v, int& total, int* s_part) {
    const int lane = threadIdx.x & (ULM_WAVE - 1), w = threadIdx.x / ULM_WAVE;
    int x = v;
#pragma unroll
    for (int d = 1; d < ULM_WAVE; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
    if (lane == ULM_WAVE - 1) s_part[w] = x;
    __syncthreads();
    int base = 0; total = 0;
#pragma unroll
    for (int k = 0; k < NT / ULM_WAVE; k++) { const int s = s_part[k]; if (k < w) base += s; total += s; }
    __syncthreads();
    return base + x - v;
}

// The value of the lowest lane whose c >= 0, or -1, to every lane of the wavefront (all 64 active).
struct UlmWaveFirst {
    __device__ int operator()(int c) const {
        const unsigned long long m = __ballot(c >= 0);
        return m ? __shfl(c, __ffsll((long long)m) - 1) : -1;
    }
};

// blockIdx.x = stream. A refused stream gets info[OK] = 0 and nothing else; the later kernels read that first.
__global__ __launch_bounds__(ULM_PREP_THREADS) void k_ulm_prepare(UlmMap M, UlmWork W) {
    const int b = blockIdx.x, t = threadIdx.x, nt = ULM_PREP_THREADS;
    int ok = __syncthreads_and(ulm_validate_ranges(M, b, t, nt));
    SnapStream S = {0, 0, 0, 0};
    if (ok) { S = snap_stream(M.kf_start, M.pt_start, b); ok = __syncthreads_and(ulm_validate_offsets(M, S, b, t, nt)); }
    if (ok) ok = __syncthreads_and(ulm_validate_entries(M, S, b, t, nt));
    if (ok) {                                                        // plain stores of this workgroup, one CU: a barrier between fill and check
        snap_distinct_fill(M.kf_by_key + S.k0, S.nk, W.mark + S.k0, t, nt);
        __syncthreads();
        ok = __syncthreads_and(snap_distinct_check(M.kf_by_key + S.k0, S.nk, W.mark + S.k0, t, nt));
    }
    if (ok) {
        const int32_t* prev = M.prev_lkf + (size_t)b * M.lcap;
        snap_distinct_fill(prev, M.prev_n_lkf[b], W.mark + S.k0, t, nt);
        __syncthreads();
        ok = __syncthreads_and(snap_distinct_check(prev, M.prev_n_lkf[b], W.mark + S.k0, t, nt));
    }
    if (ok) ulm_prepare(S, W, t, nt);
    if (t == 0) W.info[b * ULM_INFO + ULM_INFO_OK] = ok;
}

// blockIdx.x = stream.
__global__ __launch_bounds__(ULM_KF_THREADS) void k_ulm_key_frames(UlmMap M, UlmWork W, UlmOut R) {
    __shared__ int32_t s_votes[ULM_LDS_KF], s_mark[ULM_LDS_KF];
    __shared__ int s_part[ULM_KF_THREADS / ULM_WAVE];
    __shared__ long long s_best[ULM_KF_THREADS / ULM_WAVE];
    __shared__ int s_size;
    const int b = blockIdx.x, t = threadIdx.x, nt = ULM_KF_THREADS;
    if (!W.info[b * ULM_INFO + ULM_INFO_OK]) { if (t == 0) ulm_write_refused(R, b); return; }      // the whole workgroup
    const SnapStream S = snap_stream(M.kf_start, M.pt_start, b);
    const bool lds = S.nk <= ULM_LDS_KF;
    int32_t* votes = lds ? s_votes : W.votes + S.k0;
    int32_t* mark = lds ? s_mark : W.mark + S.k0;
    int32_t* list = W.list + S.k0 + b;
    int32_t* estart = W.estart + S.k0 + b;
    for (int k = t; k < S.nk; k += nt) { votes[k] = 0; mark[k] = 0; }
    __syncthreads();
    // votes (:2000-2016): a lane per keypoint of the frame
    const int fc = M.frame_count[b];
    int cast = 0;
    for (int i = t; i < fc; i += nt) cast += ulm_vote_keypoint(M, S, votes, R, b, i);
    if (R.frame_point_out) for (int i = fc + t; i < M.cap; i += nt) R.frame_point_out[(size_t)b * M.cap + i] = -1;
    const int any = __syncthreads_or(cast != 0);                     // also: every atomic add has been performed (s_waitcnt before the barrier)
    if (R.kf_votes) for (int k = t; k < S.nk; k += nt) R.kf_votes[S.k0 + k] = snap_ld_agent(&votes[k]);
    int n = 0, n_voted = 0, ref = M.prev_ref_kf[b], status = ULM_OK;
    if (!any) {                                                      // :2018
        status = ULM_NO_VOTES; n = M.prev_n_lkf[b];
        for (int j = t; j < n; j += nt) list[j] = M.prev_lkf[(size_t)b * M.lcap + j];
    } else {
        // the walk of keyframeCounter in key order (:2028-2043): an ordered compaction, nt key positions a pass
        long long best = -1;
        for (int j0 = 0; j0 < S.nk; j0 += nt) {
            long long key = -1;
            const int k = j0 + t < S.nk ? ulm_voted_slot(M, S, votes, j0 + t, &key) : -1;
            int total;
            const int at = n + ulm_block_scan<ULM_KF_THREADS>(k >= 0, total, s_part);
            if (k >= 0) { list[at] = k; mark[k] = 1; if (key > best) best = key; }
            n += total;
        }
#pragma unroll
        for (int s = ULM_WAVE / 2; s >= 1; s >>= 1) { const long long o = __shfl_xor(best, s); if (o > best) best = o; }
        if ((t & (ULM_WAVE - 1)) == 0) s_best[t / ULM_WAVE] = best;
        __syncthreads();                                             // also: list[0..n) and the marks are written
        for (int k = 0; k < ULM_KF_THREADS / ULM_WAVE; k++) if (s_best[k] > best) best = s_best[k];
        if (best >= 0) ref = ulm_key_slot(M, S, best);               // :2120-2124; every voted key frame bad: unchanged
        n_voted = n;
        if (t < ULM_WAVE) {                                          // the neighbour loop (:2047-2118): wavefront 0
            const int size = ulm_neighbour_loop(M, S, mark, list, n, t, ULM_WAVE, UlmWaveFirst());
            if (t == 0) s_size = size;
        }
        __syncthreads();
        n = s_size;
    }
    __syncthreads();                                                 // the list is complete for every thread
    if (n > M.lcap) status = ULM_OVERFLOW;
    ulm_write_list(M, R, list, n, b, t, nt);
    // estart: the prefix of the list's keypoint counts
    int entries = 0;
    for (int j0 = 0; j0 < n; j0 += nt) {
        const int j = j0 + t;
        int c = 0;
        if (j < n) { const int g = S.k0 + snap_ld_wg(&list[j]); c = M.kp_start[g + 1] - M.kp_start[g]; }
        int total;
        const int at = entries + ulm_block_scan<ULM_KF_THREADS>(c, total, s_part);
        if (j < n) estart[j] = at;
        entries += total;
    }
    if (t == 0) {
        estart[n] = entries;
        if (R.n_lkf) R.n_lkf[b] = n;
        if (R.n_voted) R.n_voted[b] = n_voted;
        if (R.ref_kf) R.ref_kf[b] = ref;
        W.info[b * ULM_INFO + ULM_INFO_LIST] = n; W.info[b * ULM_INFO + ULM_INFO_STATUS] = status; W.info[b * ULM_INFO + ULM_INFO_ENTRIES] = entries;
    }
}

// blockIdx.y = stream; the workgroups of a stream stride over its entries. atomicMin on integers: the minimum is the same whatever the order.
__global__ __launch_bounds__(ULM_CLAIM_THREADS) void k_ulm_claim_points(UlmMap M, UlmWork W) {
    const int b = blockIdx.y;
    if (!W.info[b * ULM_INFO + ULM_INFO_OK]) return;
    const SnapStream S = snap_stream(M.kf_start, M.pt_start, b);
    const int n = W.info[b * ULM_INFO + ULM_INFO_LIST], entries = W.info[b * ULM_INFO + ULM_INFO_ENTRIES];
    const int32_t* list = W.list + S.k0 + b; const int32_t* estart = W.estart + S.k0 + b;
    for (long long pos = (long long)blockIdx.x * ULM_CLAIM_THREADS + threadIdx.x; pos < entries; pos += (long long)gridDim.x * ULM_CLAIM_THREADS)
        ulm_claim(M, S, W, list, estart, n, (int)pos);
}

// blockIdx.x = stream: the entries in order, ULM_PT_THREADS a pass.
__global__ __launch_bounds__(ULM_PT_THREADS) void k_ulm_local_points(UlmMap M, UlmWork W, UlmOut R) {
    __shared__ int s_part[ULM_PT_THREADS / ULM_WAVE];
    const int b = blockIdx.x, t = threadIdx.x, nt = ULM_PT_THREADS;
    if (!W.info[b * ULM_INFO + ULM_INFO_OK]) return;                 // the whole workgroup; its status is written
    const SnapStream S = snap_stream(M.kf_start, M.pt_start, b);
    const int n = W.info[b * ULM_INFO + ULM_INFO_LIST], entries = W.info[b * ULM_INFO + ULM_INFO_ENTRIES];
    const int32_t* list = W.list + S.k0 + b; const int32_t* estart = W.estart + S.k0 + b;
    int n_lpt = 0;
    for (long long p0 = 0; p0 < entries; p0 += nt) {                // 64-bit: entries + nt may pass 2^31
        const long long pos = p0 + t;
        const int p = pos < entries ? ulm_kept_point(M, S, W, list, estart, n, (int)pos) : -1;
        int total;
        const int at = n_lpt + ulm_block_scan<ULM_PT_THREADS>(p >= 0, total, s_part);
        if (p >= 0 && at < M.pcap && R.lpt) R.lpt[(size_t)b * M.pcap + at] = p;
        n_lpt += total;
    }
    if (R.lpt) for (int j = n_lpt + t; j < M.pcap; j += nt) R.lpt[(size_t)b * M.pcap + j] = -1;
    if (t == 0) {
        int status = W.info[b * ULM_INFO + ULM_INFO_STATUS];
        if (n_lpt > M.pcap) status = ULM_OVERFLOW;
        if (R.n_lpt) R.n_lpt[b] = n_lpt;
        if (R.status) R.status[b] = status;
    }
}

// ---- the packing for SearchLocalPoints ----------------------------------------------------------------------------------------------------
struct UlmGather {
    const int32_t* pt_start; const int32_t* frame_count; const int32_t* lpt; const int32_t* n_lpt; const int32_t* status; const int32_t* frame_point_out;
    const float* map_pts_f; const uint8_t* map_pts_desc; const int32_t* pt_nobs;
    float* pts_f; uint8_t* pts_desc; int32_t* pts_count; uint8_t* pts_flags; uint8_t* held;
    int cap, pcap;
};
__device__ __forceinline__ bool ulm_gather_stream(const UlmGather& G, int b) { return G.status[b] == ULM_OK || G.status[b] == ULM_NO_VOTES; }

// blockIdx.x = stream: held[p] = 1 where a keypoint of frame_point_out holds point p. Only an accepted stream's ranges are read.
__global__ __launch_bounds__(ULM_GATHER_THREADS) void k_ulm_frame_marks(UlmGather G) {
    const int b = blockIdx.x, t = threadIdx.x, nt = ULM_GATHER_THREADS;
    if (!ulm_gather_stream(G, b)) { if (t == 0) G.pts_count[b] = 0; return; }
    const int p0 = G.pt_start[b], np = G.pt_start[b + 1] - p0;
    for (int p = t; p < np; p += nt) G.held[p0 + p] = 0;
    __syncthreads();
    for (int i = t, e = G.frame_count[b]; i < e; i += nt) { const int p = G.frame_point_out[(size_t)b * G.cap + i]; if (p >= 0) G.held[p0 + p] = 1; }
    if (t == 0) G.pts_count[b] = min(G.n_lpt[b], G.pcap);
}

// One thread per entry of [batch][pcap]: 32 bytes of pts_f and 32 of pts_desc as two 16-byte loads and stores each.
__global__ __launch_bounds__(ULM_GATHER_THREADS) void k_ulm_gather(UlmGather G) {
    const int b = blockIdx.y, j = blockIdx.x * ULM_GATHER_THREADS + threadIdx.x;
    if (j >= G.pcap) return;
    const size_t o = (size_t)b * G.pcap + j;
    float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
    uint4 d0 = make_uint4(0u, 0u, 0u, 0u), d1 = d0;
    uint8_t flags = 0;
    if (ulm_gather_stream(G, b) && j < G.n_lpt[b]) {
        const size_t p = (size_t)G.pt_start[b] + G.lpt[o];
        const float4* sf = reinterpret_cast<const float4*>(G.map_pts_f + p * 8);
        const uint4* sd = reinterpret_cast<const uint4*>(G.map_pts_desc + p * 32);
        f0 = sf[0]; f1 = sf[1]; d0 = sd[0]; d1 = sd[1];
        flags = (uint8_t)(1 | (G.held[p] ? 2 : 0) | (G.pt_nobs[p] > 0 ? 4 : 0));
    }
    float4* df = reinterpret_cast<float4*>(G.pts_f + o * 8);
    uint4* dd = reinterpret_cast<uint4*>(G.pts_desc + o * 32);
    df[0] = f0; df[1] = f1; dd[0] = d0; dd[1] = d1;
    G.pts_flags[o] = flags;
}

} // namespace viorb

using namespace viorb;

namespace {

struct UlmLayout { UlmWork W; size_t total; };
UlmLayout ulm_layout(void* base, int batch, int n_kf, int n_pt) {
    UlmLayout L; WorkspaceLayout Y(base);
    Y.take(&L.W.votes, (size_t)n_kf); Y.take(&L.W.mark, (size_t)n_kf);
    Y.take(&L.W.list, (size_t)n_kf + batch); Y.take(&L.W.estart, (size_t)n_kf + batch);
    Y.take(&L.W.first, (size_t)n_pt); Y.take(&L.W.info, (size_t)batch * ULM_INFO);
    L.total = Y.end();
    return L;
}

int ulm_check(const viorb_local_map_snapshot* m, int cap, int lcap, int pcap) {
    VIORB_REQUIRE(m, "null snapshot");
    VIORB_REQUIRE(m->batch >= 1 && m->batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(m->n_kf >= 0 && m->n_child >= 0 && m->n_kp >= 0 && m->n_pt >= 0 && m->n_obs >= 0, "a negative total");
    VIORB_REQUIRE(cap >= 1 && lcap >= 1 && pcap >= 1, "cap, lcap, pcap >= 1");
    VIORB_REQUIRE(m->kf_start && m->kf_bad && m->kf_parent && m->kf_prev && m->kf_next && m->covis10 && m->child_start && m->child_kf && m->kf_by_key, "null array");
    VIORB_REQUIRE(m->kp_start && m->kp_point && m->pt_start && m->pt_bad && m->obs_start && m->obs, "null array");
    VIORB_REQUIRE(m->frame_point && m->frame_count && m->prev_lkf && m->prev_n_lkf && m->prev_ref_kf, "null array");
    return VIORB_OK;
}

UlmMap ulm_map(const viorb_local_map_snapshot& m, int cap, int lcap, int pcap) {
    UlmMap M;
    M.batch = m.batch; M.n_kf = m.n_kf; M.n_child = m.n_child; M.n_kp = m.n_kp; M.n_pt = m.n_pt; M.n_obs = m.n_obs;
    M.kf_start = m.kf_start; M.kf_bad = m.kf_bad; M.kf_parent = m.kf_parent; M.kf_prev = m.kf_prev; M.kf_next = m.kf_next;
    M.covis10 = m.covis10; M.child_start = m.child_start; M.child_kf = m.child_kf; M.kf_by_key = m.kf_by_key;
    M.kp_start = m.kp_start; M.kp_point = m.kp_point; M.pt_start = m.pt_start; M.pt_bad = m.pt_bad; M.obs_start = m.obs_start; M.obs = m.obs;
    M.frame_point = m.frame_point; M.frame_count = m.frame_count; M.prev_lkf = m.prev_lkf; M.prev_n_lkf = m.prev_n_lkf; M.prev_ref_kf = m.prev_ref_kf;
    M.cap = cap; M.lcap = lcap; M.pcap = pcap;
    return M;
}
UlmOut ulm_out(const viorb_local_map_result* r) {
    UlmOut R;
    memset(&R, 0, sizeof(R));
    if (!r) return R;
    R.lkf = r->lkf; R.n_lkf = r->n_lkf; R.n_voted = r->n_voted; R.ref_kf = r->ref_kf; R.lpt = r->lpt; R.n_lpt = r->n_lpt; R.status = r->status;
    R.frame_point_out = r->frame_point_out; R.kf_votes = r->kf_votes;
    return R;
}

} // namespace

extern "C" {

size_t viorb_update_local_map_workspace_bytes(int batch, int n_kf, int n_pt) {
    if (batch < 1 || batch > 65535 || n_kf < 0 || n_pt < 0) return 0;
    return ulm_layout(nullptr, batch, n_kf, n_pt).total;
}

int viorb_update_local_map_shape(int32_t* out4) {
    VIORB_REQUIRE(out4, "null array");
    out4[0] = ULM_KF_THREADS; out4[1] = ULM_PT_THREADS; out4[2] = ULM_WAVE; out4[3] = ULM_LDS_KF;
    return VIORB_OK;
}

int viorb_update_local_map_device(const viorb_local_map_snapshot* map, const viorb_local_map_result* result, int cap, int lcap, int pcap,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(ulm_check(map, cap, lcap, pcap));
    VIORB_REQUIRE_WORKSPACE(workspace, workspace_bytes, ulm_layout(nullptr, map->batch, map->n_kf, map->n_pt).total, "viorb_update_local_map_workspace_bytes");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const UlmMap M = ulm_map(*map, cap, lcap, pcap);
    const UlmWork W = ulm_layout(workspace, map->batch, map->n_kf, map->n_pt).W;
    const UlmOut R = ulm_out(result);
    // the claim grid: enough workgroups for a single stream's entries (which the host does not know: the average, doubled), at most 32
    const long long per = ((long long)M.n_kp / M.batch) * 2 / ULM_CLAIM_THREADS + 1;
    const int groups = (int)std::min<long long>(per, ULM_CLAIM_GROUPS);
    VIORB_LAUNCH(k_ulm_prepare, M.batch, ULM_PREP_THREADS, 0, st, M, W);
    VIORB_LAUNCH(k_ulm_key_frames, M.batch, ULM_KF_THREADS, 0, st, M, W, R);
    VIORB_LAUNCH(k_ulm_claim_points, dim3(groups, M.batch), ULM_CLAIM_THREADS, 0, st, M, W);
    VIORB_LAUNCH(k_ulm_local_points, M.batch, ULM_PT_THREADS, 0, st, M, W, R);
    return VIORB_OK;
}

int viorb_update_local_map(const viorb_local_map_snapshot* map, const viorb_local_map_result* result, int cap, int lcap, int pcap) {
    VIORB_TRY(ulm_check(map, cap, lcap, pcap));
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t nb = (size_t)map->batch, nk = (size_t)map->n_kf, nc = (size_t)map->n_child, ni = (size_t)map->n_kp, np = (size_t)map->n_pt, no = (size_t)map->n_obs;
    viorb_local_map_snapshot D = *map;
    D.kf_start = B.up(map->kf_start, nb + 1); D.kf_bad = B.up(map->kf_bad, nk); D.kf_parent = B.up(map->kf_parent, nk); D.kf_prev = B.up(map->kf_prev, nk);
    D.kf_next = B.up(map->kf_next, nk); D.covis10 = B.up(map->covis10, nk * ULM_COVIS); D.child_start = B.up(map->child_start, nk + 1);
    D.child_kf = B.up(map->child_kf, nc); D.kf_by_key = B.up(map->kf_by_key, nk); D.kp_start = B.up(map->kp_start, nk + 1); D.kp_point = B.up(map->kp_point, ni);
    D.pt_start = B.up(map->pt_start, nb + 1); D.pt_bad = B.up(map->pt_bad, np); D.obs_start = B.up(map->obs_start, np + 1); D.obs = B.up(map->obs, no);
    D.frame_point = B.up(map->frame_point, nb * cap); D.frame_count = B.up(map->frame_count, nb);
    D.prev_lkf = B.up(map->prev_lkf, nb * lcap); D.prev_n_lkf = B.up(map->prev_n_lkf, nb); D.prev_ref_kf = B.up(map->prev_ref_kf, nb);
    viorb_local_map_result O;
    O.lkf = B.zeros<int32_t>(nb * lcap); O.n_lkf = B.zeros<int32_t>(nb); O.n_voted = B.zeros<int32_t>(nb); O.ref_kf = B.zeros<int32_t>(nb);
    O.lpt = B.zeros<int32_t>(nb * pcap); O.n_lpt = B.zeros<int32_t>(nb); O.status = B.zeros<int32_t>(nb);
    O.frame_point_out = B.zeros<int32_t>(nb * cap); O.kf_votes = B.zeros<int32_t>(nk);
    const size_t wb = viorb_update_local_map_workspace_bytes(map->batch, map->n_kf, map->n_pt);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_update_local_map_device(&D, &O, cap, lcap, pcap, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    if (result) {
        // a refused stream writes nothing but its status: its rows of the caller's arrays stay as they are. The key frames of an accepted
        // stream lie at kf_start[b] .. kf_start[b + 1], which the validator keeps apart from every other accepted stream's.
        std::vector<int32_t> status(nb), tmp;
        VIORB_TRY(download(status.data(), O.status, nb));
        if (result->status) std::copy(status.begin(), status.end(), result->status);
        struct Rows { int32_t* host; const int32_t* dev; size_t row; };
        const Rows rows[] = {{result->lkf, O.lkf, (size_t)lcap}, {result->lpt, O.lpt, (size_t)pcap}, {result->frame_point_out, O.frame_point_out, (size_t)cap},
                             {result->n_lkf, O.n_lkf, 1}, {result->n_voted, O.n_voted, 1}, {result->ref_kf, O.ref_kf, 1}, {result->n_lpt, O.n_lpt, 1}};
        for (const Rows& r : rows) {
            if (!r.host) continue;
            tmp.resize(nb * r.row);
            VIORB_TRY(download(tmp.data(), r.dev, tmp.size()));
            for (size_t b = 0; b < nb; b++)
                if (status[b] != VIORB_ERR_INVALID_ARG) std::copy(tmp.begin() + b * r.row, tmp.begin() + (b + 1) * r.row, r.host + b * r.row);
        }
        if (result->kf_votes) {
            tmp.resize(nk);
            VIORB_TRY(download(tmp.data(), O.kf_votes, nk));
            for (size_t b = 0; b < nb; b++)
                if (status[b] != VIORB_ERR_INVALID_ARG) std::copy(tmp.begin() + map->kf_start[b], tmp.begin() + map->kf_start[b + 1], result->kf_votes + map->kf_start[b]);
        }
    }
    return VIORB_OK;
}

size_t viorb_local_points_gather_workspace_bytes(int n_pt) {
    if (n_pt < 0) return 0;
    WorkspaceLayout Y(nullptr);
    Y.take((uint8_t**)nullptr, (size_t)n_pt);
    return Y.end();
}

int viorb_local_points_gather_device(const viorb_local_map_snapshot* map, const viorb_local_map_result* result, int cap, int pcap,
                                     const float* map_pts_f, const uint8_t* map_pts_desc, const int32_t* pt_nobs, float* pts_f, uint8_t* pts_desc,
                                     int32_t* pts_count, uint8_t* pts_flags, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_REQUIRE(map && result, "null struct");
    VIORB_REQUIRE(map->batch >= 1 && map->batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(map->n_pt >= 0, "a negative total");
    VIORB_REQUIRE(cap >= 1 && pcap >= 1, "cap, pcap >= 1");
    VIORB_REQUIRE(map->pt_start && map->frame_count && result->lpt && result->n_lpt && result->status && result->frame_point_out, "null array");
    VIORB_REQUIRE(map_pts_f && map_pts_desc && pt_nobs && pts_f && pts_desc && pts_count && pts_flags, "null array");
    VIORB_REQUIRE((((uintptr_t)map_pts_f | (uintptr_t)map_pts_desc | (uintptr_t)pts_f | (uintptr_t)pts_desc) & 15) == 0, "point arrays not 16-byte aligned");
    VIORB_REQUIRE_WORKSPACE(workspace, workspace_bytes, viorb_local_points_gather_workspace_bytes(map->n_pt), "viorb_local_points_gather_workspace_bytes");
    VIORB_TRY(require_device());
    UlmGather G;
    G.pt_start = map->pt_start; G.frame_count = map->frame_count; G.lpt = result->lpt; G.n_lpt = result->n_lpt; G.status = result->status;
    G.frame_point_out = result->frame_point_out; G.map_pts_f = map_pts_f; G.map_pts_desc = map_pts_desc; G.pt_nobs = pt_nobs;
    G.pts_f = pts_f; G.pts_desc = pts_desc; G.pts_count = pts_count; G.pts_flags = pts_flags; G.held = static_cast<uint8_t*>(workspace);
    G.cap = cap; G.pcap = pcap;
    hipStream_t st = (hipStream_t)stream;
    VIORB_LAUNCH(k_ulm_frame_marks, map->batch, ULM_GATHER_THREADS, 0, st, G);
    VIORB_LAUNCH(k_ulm_gather, dim3((pcap + ULM_GATHER_THREADS - 1) / ULM_GATHER_THREADS, map->batch), ULM_GATHER_THREADS, 0, st, G);
    return VIORB_OK;
}

// ---- host-only test hook: local_map_core.h compiled for the host --------------------------------------------------------------------------
int viorb_debug_update_local_map_host(const viorb_local_map_snapshot* map, const viorb_local_map_result* result, int cap, int lcap, int pcap) {
    VIORB_TRY(ulm_check(map, cap, lcap, pcap));
    const size_t nk = (size_t)map->n_kf + 1, nb = (size_t)map->batch;
    std::vector<int32_t> votes(nk), mark(nk), list(nk + nb), estart(nk + nb), first((size_t)map->n_pt + 1), info(nb * ULM_INFO);
    UlmWork W;
    W.votes = votes.data(); W.mark = mark.data(); W.list = list.data(); W.estart = estart.data(); W.first = first.data(); W.info = info.data();
    ulm_run_host(ulm_map(*map, cap, lcap, pcap), W, ulm_out(result));
    return VIORB_OK;
}

} // extern "C"
