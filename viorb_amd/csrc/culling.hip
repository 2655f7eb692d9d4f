// viorb_amd/csrc/culling.hip — the two culling routines of LocalMapping::Run (include/viorb_culling.h):
//   k_cull_prepare     validates a stream's part of the snapshot and makes its working state             (one workgroup per stream)
//   k_cull_ordered     the candidate loop (src/LocalMapping.cc:1694-1821) with KeyFrame::SetBadFlag's effects in between (one workgroup per stream)
//   k_cull_map_points  LocalMapping::MapPointCulling (:1214-1231), elementwise
// The arithmetic is culling_core.h. Shape (DESIGN.md "Map culling"): the loop is ordered, so a stream is one workgroup that takes the
// candidates in turn and spreads each count and each erase over its lanes, a lane per keypoint walking its point's short observation
// run. A separate count of every candidate on the snapshot state, reused until a cull touched the candidate, was built and measured:
// it did not pay, so every candidate is counted where it is decided.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "culling_core.h"

namespace viorb {

enum { CULL_WAVE = 64, CULL_PREP_THREADS = 256, CULL_ORDERED_THREADS = 1024, CULL_MP_THREADS = 256 };

// blockIdx.x = stream. A refused stream gets ok = 0 and nothing else; the later kernels read ok first.
__global__ __launch_bounds__(CULL_PREP_THREADS) void k_cull_prepare(CullMap M, CullWork W) {
    const int b = blockIdx.x, t = threadIdx.x, nt = CULL_PREP_THREADS;
    int ok = __syncthreads_and(cull_validate_ranges(M, b, t, nt));
    CullStream S = CullStream();
    if (ok) { S = cull_stream(M, b); ok = __syncthreads_and(cull_validate_offsets(M, S, b, t, nt)); }
    if (ok) ok = __syncthreads_and(cull_validate_entries(M, S, t, nt));
    if (ok) {
        cull_prepare(M, S, W, t, nt);
        __syncthreads();                                             // every slot of cand_of_kf holds -1 (plain stores of this workgroup, one CU)
        snap_distinct_fill(M.cand_kf + S.c0, S.nc, W.cand_of_kf + S.k0, t, nt);
        __syncthreads();
        ok = __syncthreads_and(snap_distinct_check(M.cand_kf + S.c0, S.nc, W.cand_of_kf + S.k0, t, nt));
    }
    if (t == 0) W.ok[b] = ok;
}

// The workgroup's sums of a and b, returned to every thread. Every thread calls it.
__device__ __forceinline__ void cull_block_sum2(int& a, int& b, int (*s_part)[2]) {
    const int lane = threadIdx.x & (CULL_WAVE - 1), w = threadIdx.x / CULL_WAVE;
#pragma unroll
    for (int s = CULL_WAVE / 2; s >= 1; s >>= 1) { a += __shfl_xor(a, s); b += __shfl_xor(b, s); }
    if (lane == 0) { s_part[w][0] = a; s_part[w][1] = b; }
    __syncthreads();
    a = 0; b = 0;
    for (int k = 0; k < CULL_ORDERED_THREADS / CULL_WAVE; k++) { a += s_part[k][0]; b += s_part[k][1]; }
    __syncthreads();
}

// blockIdx.x = stream; the candidates in order. Thread 0 holds the links and evaluates the skip tests; a count or an erase spreads the
// candidate's keypoints over the workgroup. What one phase writes to global memory with plain stores the next one reads after a
// __syncthreads(); the words the erase step changes with atomics (point and observation words) are read with snap_ld_agent
// (map_snapshot_core.h has the reasoning for both).
__global__ __launch_bounds__(CULL_ORDERED_THREADS) void k_cull_ordered(CullMap M, CullWork W, CullOut R, int monocular) {
    __shared__ int s_part[CULL_ORDERED_THREADS / CULL_WAVE][2];
    __shared__ int s_reason;
    const int b = blockIdx.x, t = threadIdx.x, nt = CULL_ORDERED_THREADS;
    if (!W.ok[b]) {                                                  // the whole workgroup
        if (t == 0) { if (R.status) R.status[b] = VIORB_ERR_INVALID_ARG; if (R.n_culled) R.n_culled[b] = 0; }
        return;
    }
    const CullStream S = cull_stream(M, b);
    const int cur = M.cur_kf[b];
    const bool vins = M.vins_inited[b] != 0, mono = monocular != 0;
    const float th = M.th_depth[b];
    int n_culled = 0;
    for (int j = 0; j < S.nc; j++) {
        const int g = S.c0 + j, c = M.cand_kf[g], i0 = M.kp_start[g], i1 = M.kp_start[g + 1];
        if (t == 0) s_reason = cull_skip(M, S, W, c, cur, vins);
        __syncthreads();                                             // also: the previous candidate's erase is complete
        int reason = s_reason, mps = 0, red = 0, counted = 0;
        if (reason < 0) {
            counted = 1;
            for (int i = i0 + t; i < i1; i += nt) { const int r = cull_count_keypoint(M, S, W, c, i, mono, th); mps += r & 1; red += (r >> 1) & 1; }
            cull_block_sum2(mps, red, s_part);
            reason = KFC_KEPT;
            if (cull_decide(red, mps)) {
                if (M.kf_flags[S.k0 + c] & CULL_KF_NOT_ERASE) {
                    reason = KFC_DEFERRED;
                    if (t == 0) W.kf_state[S.k0 + c] |= CULL_ST_TO_BE_ERASED;
                } else {
                    reason = KFC_CULLED;
                    for (int i = i0 + t; i < i1; i += nt) cull_erase_keypoint(M, S, W, c, i);
                    if (t == 0) { cull_unlink(S, W, c); if (R.culled_order) R.culled_order[S.c0 + n_culled] = j; }
                    n_culled++;
                }
            }
        }
        if (t == 0) cull_write_candidate(R, g, reason, red, mps, counted);
        __syncthreads();                                             // s_reason is read before thread 0 writes the next one
    }
    if (t == 0) { if (R.status) R.status[b] = VIORB_OK; if (R.n_culled) R.n_culled[b] = n_culled; }
    cull_write_state(M, S, W, R, n_culled, t, nt);
}

// One thread per entry of [batch][cap].
__global__ __launch_bounds__(CULL_MP_THREADS) void k_cull_map_points(const uint8_t* __restrict__ bad, const int* __restrict__ found, const int* __restrict__ visible,
                                                                     const int* __restrict__ first_kf_id, const int* __restrict__ nobs, const int* __restrict__ count,
                                                                     const int* __restrict__ cur_kf_id, int cap, int monocular, int* __restrict__ code) {
    const int b = blockIdx.y, i = blockIdx.x * CULL_MP_THREADS + threadIdx.x;
    if (i >= cap) return;
    const size_t o = (size_t)b * cap + i;
    const int n = min(max(count[b], 0), cap);
    code[o] = i < n ? cull_map_point(bad[o], found[o], visible[o], first_kf_id[o], nobs[o], cur_kf_id[b], monocular != 0) : -1;
}

} // namespace viorb

using namespace viorb;

namespace {

struct CullLayout { CullWork W; size_t total; };
CullLayout cull_layout(void* base, int batch, int n_kf, int n_cand, int n_pt, int n_obs) {
    CullLayout L; WorkspaceLayout Y(base);
    Y.take(&L.W.pt, (size_t)n_pt); Y.take(&L.W.obs, (size_t)n_obs);
    Y.take(&L.W.cand_of_kf, (size_t)n_kf); Y.take(&L.W.prev, (size_t)n_kf); Y.take(&L.W.next, (size_t)n_kf); Y.take(&L.W.kf_state, (size_t)n_kf);
    Y.take(&L.W.ok, (size_t)batch);
    L.total = Y.end();
    return L;
}

int cull_check_map(const viorb_cull_map* m, int monocular) {
    VIORB_REQUIRE(m, "null snapshot");
    VIORB_REQUIRE(m->batch >= 1 && m->batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(m->n_kf >= 0 && m->n_cand >= 0 && m->n_kp >= 0 && m->n_pt >= 0 && m->n_obs >= 0, "a negative total");
    VIORB_REQUIRE(m->kf_start && m->kf_flags && m->kf_time && m->kf_prev && m->kf_next && m->cur_kf && m->vins_inited && m->th_depth, "null array");
    VIORB_REQUIRE(m->cand_start && m->cand_kf && m->kp_start && m->kp_point && m->kp_octave && (monocular || m->kp_depth), "null array");
    VIORB_REQUIRE(m->pt_start && m->pt_nobs && m->pt_bad && m->obs_start && m->obs, "null array");
    return VIORB_OK;
}

CullMap cull_map(const viorb_cull_map& m) {
    CullMap M;
    M.batch = m.batch; M.n_kf = m.n_kf; M.n_cand = m.n_cand; M.n_kp = m.n_kp; M.n_pt = m.n_pt; M.n_obs = m.n_obs;
    M.kf_start = m.kf_start; M.kf_flags = m.kf_flags; M.kf_time = m.kf_time; M.kf_prev = m.kf_prev; M.kf_next = m.kf_next;
    M.cur_kf = m.cur_kf; M.vins_inited = m.vins_inited; M.th_depth = m.th_depth;
    M.cand_start = m.cand_start; M.cand_kf = m.cand_kf; M.kp_start = m.kp_start; M.kp_point = m.kp_point; M.kp_octave = m.kp_octave; M.kp_depth = m.kp_depth;
    M.pt_start = m.pt_start; M.pt_nobs = m.pt_nobs; M.pt_bad = m.pt_bad; M.obs_start = m.obs_start; M.obs = m.obs;
    return M;
}
CullOut cull_out(const viorb_cull_result* r) {
    CullOut R;
    memset(&R, 0, sizeof(R));
    if (!r) return R;
    R.cand_reason = r->cand_reason; R.cand_redundant = r->cand_redundant; R.cand_mps = r->cand_mps; R.cand_recounted = r->cand_recounted;
    R.culled_order = r->culled_order; R.n_culled = r->n_culled; R.status = r->status;
    R.kf_bad = r->kf_bad; R.kf_to_be_erased = r->kf_to_be_erased; R.kf_prev_out = r->kf_prev_out; R.kf_next_out = r->kf_next_out; R.kf_repreint = r->kf_repreint;
    R.pt_nobs_out = r->pt_nobs_out; R.pt_bad_out = r->pt_bad_out; R.obs_alive = r->obs_alive;
    return R;
}

int mpc_check(const void* bad, const void* found, const void* visible, const void* first, const void* nobs, const void* code) {
    VIORB_REQUIRE(bad && found && visible && first && nobs && code, "null array");
    return VIORB_OK;
}

} // namespace

extern "C" {

size_t viorb_key_frame_culling_workspace_bytes(int batch, int n_kf, int n_cand, int n_pt, int n_obs) {
    if (batch < 1 || batch > 65535 || n_kf < 0 || n_cand < 0 || n_pt < 0 || n_obs < 0) return 0;
    return cull_layout(nullptr, batch, n_kf, n_cand, n_pt, n_obs).total;
}

int viorb_key_frame_culling_shape(int32_t* out4) {
    VIORB_REQUIRE(out4, "null array");
    out4[0] = CULL_ORDERED_THREADS; out4[1] = CULL_ORDERED_THREADS; out4[2] = CULL_WAVE; out4[3] = 0;
    return VIORB_OK;
}

int viorb_key_frame_culling_device(const viorb_cull_map* map, int monocular, const viorb_cull_result* result, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    VIORB_TRY(cull_check_map(map, monocular));
    VIORB_REQUIRE_WORKSPACE(workspace, workspace_bytes, cull_layout(nullptr, map->batch, map->n_kf, map->n_cand, map->n_pt, map->n_obs).total,
                            "viorb_key_frame_culling_workspace_bytes");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const CullMap M = cull_map(*map);
    const CullWork W = cull_layout(workspace, map->batch, map->n_kf, map->n_cand, map->n_pt, map->n_obs).W;
    const CullOut R = cull_out(result);
    VIORB_LAUNCH(k_cull_prepare, M.batch, CULL_PREP_THREADS, 0, st, M, W);
    VIORB_LAUNCH(k_cull_ordered, M.batch, CULL_ORDERED_THREADS, 0, st, M, W, R, monocular);
    return VIORB_OK;
}

int viorb_key_frame_culling(const viorb_cull_map* map, int monocular, const viorb_cull_result* result) {
    VIORB_TRY(cull_check_map(map, monocular));
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t nb = (size_t)map->batch, nk = (size_t)map->n_kf, nc = (size_t)map->n_cand, ni = (size_t)map->n_kp, np = (size_t)map->n_pt, no = (size_t)map->n_obs;
    viorb_cull_map D = *map;
    D.kf_start = B.up(map->kf_start, nb + 1); D.kf_flags = B.up(map->kf_flags, nk); D.kf_time = B.up(map->kf_time, nk);
    D.kf_prev = B.up(map->kf_prev, nk); D.kf_next = B.up(map->kf_next, nk);
    D.cur_kf = B.up(map->cur_kf, nb); D.vins_inited = B.up(map->vins_inited, nb); D.th_depth = B.up(map->th_depth, nb);
    D.cand_start = B.up(map->cand_start, nb + 1); D.cand_kf = B.up(map->cand_kf, nc); D.kp_start = B.up(map->kp_start, nc + 1);
    D.kp_point = B.up(map->kp_point, ni); D.kp_octave = B.up(map->kp_octave, ni); D.kp_depth = map->kp_depth ? B.up(map->kp_depth, ni) : nullptr;
    D.pt_start = B.up(map->pt_start, nb + 1); D.pt_nobs = B.up(map->pt_nobs, np); D.pt_bad = B.up(map->pt_bad, np);
    D.obs_start = B.up(map->obs_start, np + 1); D.obs = B.up(map->obs, no);
    viorb_cull_result O;
    O.cand_reason = B.zeros<int32_t>(nc); O.cand_redundant = B.zeros<int32_t>(nc); O.cand_mps = B.zeros<int32_t>(nc); O.cand_recounted = B.zeros<int32_t>(nc);
    O.culled_order = B.zeros<int32_t>(nc); O.n_culled = B.zeros<int32_t>(nb); O.status = B.zeros<int32_t>(nb);
    O.kf_bad = B.zeros<uint8_t>(nk); O.kf_to_be_erased = B.zeros<uint8_t>(nk); O.kf_prev_out = B.zeros<int32_t>(nk); O.kf_next_out = B.zeros<int32_t>(nk);
    O.kf_repreint = B.zeros<uint8_t>(nk); O.pt_nobs_out = B.zeros<int32_t>(np); O.pt_bad_out = B.zeros<uint8_t>(np); O.obs_alive = B.zeros<uint8_t>(no);
    const size_t wb = viorb_key_frame_culling_workspace_bytes(map->batch, map->n_kf, map->n_cand, map->n_pt, map->n_obs);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_key_frame_culling_device(&D, monocular, &O, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    if (result) {
        VIORB_TRY(download(result->cand_reason, O.cand_reason, nc)); VIORB_TRY(download(result->cand_redundant, O.cand_redundant, nc));
        VIORB_TRY(download(result->cand_mps, O.cand_mps, nc)); VIORB_TRY(download(result->cand_recounted, O.cand_recounted, nc));
        VIORB_TRY(download(result->culled_order, O.culled_order, nc)); VIORB_TRY(download(result->n_culled, O.n_culled, nb));
        VIORB_TRY(download(result->status, O.status, nb)); VIORB_TRY(download(result->kf_bad, O.kf_bad, nk));
        VIORB_TRY(download(result->kf_to_be_erased, O.kf_to_be_erased, nk)); VIORB_TRY(download(result->kf_prev_out, O.kf_prev_out, nk));
        VIORB_TRY(download(result->kf_next_out, O.kf_next_out, nk)); VIORB_TRY(download(result->kf_repreint, O.kf_repreint, nk));
        VIORB_TRY(download(result->pt_nobs_out, O.pt_nobs_out, np)); VIORB_TRY(download(result->pt_bad_out, O.pt_bad_out, np));
        VIORB_TRY(download(result->obs_alive, O.obs_alive, no));
    }
    return VIORB_OK;
}

int viorb_map_point_culling_device(const uint8_t* bad, const int32_t* found, const int32_t* visible, const int32_t* first_kf_id, const int32_t* nobs,
                                   const int32_t* count, const int32_t* cur_kf_id, int cap, int batch, int monocular, int32_t* code, void* stream) {
    VIORB_TRY(mpc_check(bad, found, visible, first_kf_id, nobs, code));
    VIORB_REQUIRE(count && cur_kf_id, "null array");
    VIORB_REQUIRE(cap >= 1, "cap >= 1");
    VIORB_REQUIRE(batch >= 1 && batch <= 65535, "1 <= batch <= 65535");
    VIORB_TRY(require_device());
    VIORB_LAUNCH(k_cull_map_points, dim3((cap + CULL_MP_THREADS - 1) / CULL_MP_THREADS, batch), CULL_MP_THREADS, 0, (hipStream_t)stream, bad, found, visible,
                 first_kf_id, nobs, count, cur_kf_id, cap, monocular, code);
    return VIORB_OK;
}

int viorb_map_point_culling(const uint8_t* bad, const int32_t* found, const int32_t* visible, const int32_t* first_kf_id, const int32_t* nobs, int n,
                            int cur_kf_id, int monocular, int32_t* code) {
    VIORB_REQUIRE(n >= 0, "a negative count");
    if (n > 0) VIORB_TRY(mpc_check(bad, found, visible, first_kf_id, nobs, code));
    VIORB_TRY(require_device());
    if (n == 0) return VIORB_OK;
    DeviceBufs B;
    const size_t m = (size_t)n;
    uint8_t* db = B.up(bad, m); int32_t* df = B.up(found, m); int32_t* dv = B.up(visible, m); int32_t* d1 = B.up(first_kf_id, m); int32_t* dn = B.up(nobs, m);
    int32_t* dc = B.up(&n, 1); int32_t* dk = B.up(&cur_kf_id, 1); int32_t* dcode = B.zeros<int32_t>(m);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_map_point_culling_device(db, df, dv, d1, dn, dc, dk, n, 1, monocular, dcode, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    return download(code, dcode, m);
}

// ---- host-only test hooks: culling_core.h compiled for the host ------------------------------------------------------------------------
int viorb_debug_key_frame_culling_host(const viorb_cull_map* map, int monocular, const viorb_cull_result* result) {
    VIORB_TRY(cull_check_map(map, monocular));
    const size_t one = 1;
    std::vector<int32_t> pt(std::max<size_t>(map->n_pt, one)), cok(std::max<size_t>(map->n_kf, one)), prev(cok.size()), next(cok.size());
    std::vector<uint32_t> obs(std::max<size_t>(map->n_obs, one));
    std::vector<uint8_t> kst(cok.size());
    std::vector<int32_t> ok((size_t)map->batch);
    CullWork W;
    W.pt = pt.data(); W.obs = obs.data(); W.cand_of_kf = cok.data(); W.prev = prev.data(); W.next = next.data(); W.kf_state = kst.data();
    W.ok = ok.data();
    cull_run_host(cull_map(*map), W, cull_out(result), monocular != 0);
    return VIORB_OK;
}

int viorb_debug_map_point_code(int bad, int found, int visible, int first_kf_id, int nobs, int cur_kf_id, int monocular) {
    return cull_map_point(bad, found, visible, first_kf_id, nobs, cur_kf_id, monocular != 0);
}

} // extern "C"
