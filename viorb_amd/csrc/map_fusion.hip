// viorb_amd/csrc/map_fusion.hip — the fuse searches' results applied to a batch of map snapshots (include/viorb_map_fusion.h):
//   k_fuse_prepare   validates a stream's part of the snapshot, builds the rank, the working copies and the observation pool
//   k_fuse_ordered   the calls of a stream in order, one wavefront per stream: the lanes cover a point's segments for a membership
//                    question, a key frame's keypoints for spAlreadyFound and the former observers inside a Replace; then a lane per
//                    point counts what is left
//   k_fuse_emit      scans the counts of a stream's points and writes the observations and the dirty lists in key order
//                                                                                                       (all: one workgroup per stream)
// The logic is map_fusion_core.h. Shape (DESIGN.md "Map fusion"): an entry reads what the earlier ones left (bad flags, observer sets,
// nObs, the key frame's table), so the entries of a stream are serial and the batch is the parallelism; inside an entry the observers
// of the replaced point name distinct key frames, so the lanes touch disjoint words.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "map_fusion_core.h"

namespace viorb {

enum { FUSE_WAVE = 64, FUSE_THREADS = 256 };

struct FuseWave {
    __device__ int sum(int v) const { return __popcll(__ballot(v != 0)); }          // v is 0 or 1
    __device__ bool any(bool v) const { return __ballot(v) != 0; }
    __device__ int first(int v) const { return __builtin_amdgcn_readfirstlane(v); }
};

// blockIdx.x = stream. A refused stream gets info = 0 and nothing else; the other kernels read that first.
__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_prepare(FuseMap M, FuseWork W, FuseOut R) {
    const int b = blockIdx.x, t = threadIdx.x, nt = FUSE_THREADS;
    int ok = __syncthreads_and(fuse_validate_ranges(M, b, t, nt));
    FuseStream F = {};
    if (ok) { F = fuse_stream(M, b); ok = __syncthreads_and(fuse_validate_offsets(M, F, t, nt)); }
    if (ok) ok = __syncthreads_and(fuse_validate_entries(M, F, t, nt));
    if (ok) {
        snap_distinct_fill(M.kf_by_key + F.S.k0, F.S.nk, W.rank + F.S.k0, t, nt);
        __syncthreads();
        ok = __syncthreads_and(snap_distinct_check(M.kf_by_key + F.S.k0, F.S.nk, W.rank + F.S.k0, t, nt));
    }
    if (ok) ok = __syncthreads_and(fuse_validate_observations(M, F, t, nt));
    if (ok) fuse_prepare(M, F, W, R, t, nt);
    if (t == 0) { W.info[b] = ok; W.tot[b] = 0; W.dtot[b] = 0; }
}

// blockIdx.x = stream; one wavefront.
__global__ __launch_bounds__(FUSE_WAVE) void k_fuse_ordered(FuseMap M, FuseWork W, FuseOut R) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!W.info[b]) return;                                              // the whole wavefront
    const FuseStream F = fuse_stream(M, b);
    for (int c = 0; c < F.nc; c++) fuse_call(M, F, W, R, F.c0 + c, c + 1, lane, FUSE_WAVE, FuseWave());
    snap_fence_wg();
    __syncthreads();
    int n = 0, nd = 0;
    for (int p = lane; p < F.S.np; p += FUSE_WAVE) { fuse_count_point(M, F, W, R, p); n += W.cnt[F.S.p0 + p]; nd += W.dcnt[F.S.p0 + p]; }
    for (int d = FUSE_WAVE / 2; d > 0; d >>= 1) { n += __shfl_xor(n, d); nd += __shfl_xor(nd, d); }
    if (lane == 0) { W.tot[b] = n; W.dtot[b] = nd; }
}

// Exclusive scan of one value per thread over the workgroup; *total = the sum
__device__ int fuse_block_scan(int v, int32_t* s_wave, int* total) {
    const int t = threadIdx.x, lane = t & (FUSE_WAVE - 1), wave = t / FUSE_WAVE;
    int incl = v;
    for (int d = 1; d < FUSE_WAVE; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl += o; }
    __syncthreads();                                                     // s_wave is free again
    if (lane == FUSE_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < FUSE_THREADS / FUSE_WAVE; w++) { if (w < wave) base += s_wave[w]; sum += s_wave[w]; }
    *total = sum;
    return base + incl - v;
}

// blockIdx.x = stream.
__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_emit(FuseMap M, FuseWork W, FuseOut R) {
    __shared__ int32_t s_wave[FUSE_THREADS / FUSE_WAVE];
    __shared__ int32_t s_red[FUSE_THREADS];
    const int b = blockIdx.x, t = threadIdx.x, nt = FUSE_THREADS;
    if (!W.info[b]) { if (t == 0) R.status[b] = COV_INVALID; return; }   // the whole workgroup
    const FuseStream F = fuse_stream(M, b);
    // the dirty lists are packed over the batch: the streams before this one (their offsets passed this stream's step 1)
    int mine = 0;
    for (int i = t; i < b; i += nt) mine += (W.info[i] && fuse_fits(M, W, i)) ? W.dtot[i] : 0;
    s_red[t] = mine;
    __syncthreads();
    for (int d = nt / 2; d > 0; d >>= 1) { if (t < d) s_red[t] += s_red[t + d]; __syncthreads(); }
    const bool fits = fuse_fits(M, W, b), last = b + 1 == M.batch || !W.info[b + 1];
    int at = M.obs_out_start[b], dat = s_red[0];
    for (int p0 = 0; p0 < F.S.np; p0 += nt) {                            // the same trip count for every thread
        const int p = p0 + t, g = F.S.p0 + p;
        const int n = p < F.S.np ? W.cnt[g] : 0, nd = (p < F.S.np && fits) ? W.dcnt[g] : 0;
        int sum, dsum;
        const int off = fuse_block_scan(n, s_wave, &sum), doff = fuse_block_scan(nd, s_wave, &dsum);
        if (p < F.S.np) {
            if (fits) { R.obs_start_out[g] = at + off; fuse_emit_point(M, F, W, R, p, at + off, dat + doff); }
            if (R.dirty_obs_start) R.dirty_obs_start[g] = dat + doff;
        }
        at += sum; dat += dsum;
    }
    if (t == 0) {
        if (last && fits) R.obs_start_out[F.S.p0 + F.S.np] = at;
        if (R.dirty_obs_start) R.dirty_obs_start[F.S.p0 + F.S.np] = dat;         // the packed lists: an accepted stream behind this one writes the same value
        if (R.need) R.need[b] = W.tot[b];
        R.status[b] = fits ? COV_OK : COV_OVERFLOW;
    }
}

// a thread per 4 bytes of a row
__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_merge_desc(const uint8_t* pt_dirty, const int32_t* dirty_obs_start, const uint32_t* new_desc, uint32_t* pts_desc, int n_pt) {
    const long long i = (long long)blockIdx.x * FUSE_THREADS + threadIdx.x;
    const int p = (int)(i >> 3);
    if (p >= n_pt || !pt_dirty[p]) return;
    if (dirty_obs_start && dirty_obs_start[p + 1] <= dirty_obs_start[p]) return;
    pts_desc[i] = new_desc[i];
}

} // namespace viorb

using namespace viorb;

namespace {

struct FuseLayout { FuseWork W; size_t total; };
FuseLayout fuse_layout(void* base, int batch, int n_kf, int n_pt, int n_obs, int n_op) {
    FuseLayout L; WorkspaceLayout Y(base);
    const size_t np = (size_t)n_pt, ne = (size_t)n_obs + (size_t)n_op;
    Y.take(&L.W.rank, (size_t)n_kf);
    Y.take(&L.W.bad, np); Y.take(&L.W.replaced, np); Y.take(&L.W.dirty, np); Y.take(&L.W.stamp, np); Y.take(&L.W.found, np); Y.take(&L.W.visible, np);
    Y.take(&L.W.head, np); Y.take(&L.W.tail, np); Y.take(&L.W.cnt, np); Y.take(&L.W.dcnt, np);
    Y.take(&L.W.next, np + (size_t)n_op); Y.take(&L.W.rep, (size_t)n_op); Y.take(&L.W.pool, ne); Y.take(&L.W.pfeat, ne);
    Y.take(&L.W.info, (size_t)batch); Y.take(&L.W.tot, (size_t)batch); Y.take(&L.W.dtot, (size_t)batch);
    L.total = Y.end();
    return L;
}

int fuse_check(const viorb_fuse_map* m, const viorb_fuse_result* r) {
    VIORB_REQUIRE(m && r, "null struct");
    VIORB_REQUIRE(m->batch >= 1 && m->batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(m->n_kf >= 0 && m->n_kp >= 0 && m->n_pt >= 0 && m->n_obs >= 0 && m->n_call >= 0 && m->n_list >= 0 && m->n_feat >= 0 && m->n_op >= 0 && m->n_obs_out >= 0,
                  "a negative total");
    VIORB_REQUIRE((long long)m->n_obs + m->n_op <= 0x7fffffffLL && (long long)m->n_pt + m->n_op <= 0x7fffffffLL, "n_obs + n_op and n_pt + n_op below 2^31");
    VIORB_REQUIRE(m->kf_start && m->kf_by_key && m->kf_bad && m->kp_start && m->kp_point && m->kp_octave && m->kp_stereo, "null array");
    VIORB_REQUIRE(m->pt_start && m->pt_bad && m->pt_nobs && m->pt_found && m->pt_visible && m->obs_start && m->obs && m->obs_feat, "null array");
    VIORB_REQUIRE(m->call_start && m->call_kf && m->call_kind && m->call_list && m->call_n && m->call_feat && m->call_op && m->list_point && m->op_feat && m->obs_out_start, "null array");
    VIORB_REQUIRE(r->status && r->kp_point_out && r->pt_bad_out && r->pt_nobs_out && r->obs_start_out && r->obs_out && r->obs_feat_out, "null required result array");
    VIORB_REQUIRE((!r->dirty_obs_start) == (!r->dirty_obs_kf) && (!r->dirty_obs_start) == (!r->dirty_obs_feat), "dirty_obs_start, dirty_obs_kf, dirty_obs_feat: all or none");
    return VIORB_OK;
}

FuseMap fuse_map(const viorb_fuse_map& m) {
    FuseMap M;
    M.batch = m.batch; M.n_kf = m.n_kf; M.n_kp = m.n_kp; M.n_pt = m.n_pt; M.n_obs = m.n_obs; M.n_call = m.n_call; M.n_list = m.n_list; M.n_feat = m.n_feat;
    M.n_op = m.n_op; M.n_obs_out = m.n_obs_out;
    M.kf_start = m.kf_start; M.kf_by_key = m.kf_by_key; M.kf_bad = m.kf_bad; M.kp_start = m.kp_start; M.kp_point = m.kp_point; M.kp_octave = m.kp_octave;
    M.kp_stereo = m.kp_stereo; M.pt_start = m.pt_start; M.pt_bad = m.pt_bad; M.pt_nobs = m.pt_nobs; M.pt_found = m.pt_found; M.pt_visible = m.pt_visible;
    M.obs_start = m.obs_start; M.obs = m.obs; M.obs_feat = m.obs_feat; M.call_start = m.call_start; M.call_kf = m.call_kf; M.call_kind = m.call_kind;
    M.call_list = m.call_list; M.call_n = m.call_n; M.call_feat = m.call_feat; M.call_op = m.call_op; M.list_point = m.list_point; M.op_feat = m.op_feat;
    M.obs_out_start = m.obs_out_start;
    return M;
}
FuseOut fuse_out(const viorb_fuse_result& r) {
    FuseOut R;
    R.status = r.status; R.kp_point_out = r.kp_point_out; R.pt_bad_out = r.pt_bad_out; R.pt_nobs_out = r.pt_nobs_out; R.obs_start_out = r.obs_start_out;
    R.obs_out = r.obs_out; R.obs_feat_out = r.obs_feat_out; R.need = r.need; R.pt_found_out = r.pt_found_out; R.pt_visible_out = r.pt_visible_out;
    R.pt_replaced_out = r.pt_replaced_out; R.pt_dirty = r.pt_dirty; R.obs_touched = r.obs_touched; R.dirty_obs_start = r.dirty_obs_start;
    R.dirty_obs_kf = r.dirty_obs_kf; R.dirty_obs_feat = r.dirty_obs_feat; R.op_reason = r.op_reason; R.op_other = r.op_other; R.call_nfused = r.call_nfused;
    return R;
}

// One result array of the host form: the caller's contents go up, so that what the kernels do not write comes back as it was
template <class T> struct FuseArr { T* host; T* dev; size_t n; };
template <class T> FuseArr<T> fuse_arr(DeviceBufs& B, T* host, size_t n, T** dev) {
    *dev = host ? B.up(host, n) : nullptr;
    return FuseArr<T>{host, *dev, n};
}

} // namespace

extern "C" {

size_t viorb_apply_fuse_workspace_bytes(int batch, int n_kf, int n_pt, int n_obs, int n_op) {
    if (batch < 1 || batch > 65535 || n_kf < 0 || n_pt < 0 || n_obs < 0 || n_op < 0) return 0;
    return fuse_layout(nullptr, batch, n_kf, n_pt, n_obs, n_op).total;
}

int viorb_apply_fuse_shape(int32_t* out4) {
    VIORB_REQUIRE(out4, "null array");
    out4[0] = FUSE_THREADS; out4[1] = FUSE_WAVE; out4[2] = 0; out4[3] = 0;
    return VIORB_OK;
}

int viorb_apply_fuse_device(const viorb_fuse_map* map, const viorb_fuse_result* result, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(fuse_check(map, result));
    VIORB_REQUIRE_WORKSPACE(workspace, workspace_bytes, fuse_layout(nullptr, map->batch, map->n_kf, map->n_pt, map->n_obs, map->n_op).total, "viorb_apply_fuse_workspace_bytes");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const FuseMap M = fuse_map(*map);
    const FuseWork W = fuse_layout(workspace, map->batch, map->n_kf, map->n_pt, map->n_obs, map->n_op).W;
    const FuseOut R = fuse_out(*result);
    VIORB_LAUNCH(k_fuse_prepare, M.batch, FUSE_THREADS, 0, st, M, W, R);
    VIORB_LAUNCH(k_fuse_ordered, M.batch, FUSE_WAVE, 0, st, M, W, R);
    VIORB_LAUNCH(k_fuse_emit, M.batch, FUSE_THREADS, 0, st, M, W, R);
    return VIORB_OK;
}

int viorb_apply_fuse(const viorb_fuse_map* map, const viorb_fuse_result* result) {
    VIORB_TRY(fuse_check(map, result));
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t nb = (size_t)map->batch, nk = (size_t)map->n_kf, ni = (size_t)map->n_kp, np = (size_t)map->n_pt, no = (size_t)map->n_obs, nc = (size_t)map->n_call,
                 nl = (size_t)map->n_list, nf = (size_t)map->n_feat, nj = (size_t)map->n_op, nq = (size_t)map->n_obs_out;
    viorb_fuse_map D = *map;
    D.kf_start = B.up(map->kf_start, nb + 1); D.kf_by_key = B.up(map->kf_by_key, nk); D.kf_bad = B.up(map->kf_bad, nk);
    D.kp_start = B.up(map->kp_start, nk + 1); D.kp_point = B.up(map->kp_point, ni); D.kp_octave = B.up(map->kp_octave, ni); D.kp_stereo = B.up(map->kp_stereo, ni);
    D.pt_start = B.up(map->pt_start, nb + 1); D.pt_bad = B.up(map->pt_bad, np); D.pt_nobs = B.up(map->pt_nobs, np); D.pt_found = B.up(map->pt_found, np);
    D.pt_visible = B.up(map->pt_visible, np); D.obs_start = B.up(map->obs_start, np + 1); D.obs = B.up(map->obs, no); D.obs_feat = B.up(map->obs_feat, no);
    D.call_start = B.up(map->call_start, nb + 1); D.call_kf = B.up(map->call_kf, nc); D.call_kind = B.up(map->call_kind, nc); D.call_list = B.up(map->call_list, nc);
    D.call_n = B.up(map->call_n, nc); D.call_feat = B.up(map->call_feat, nc); D.call_op = B.up(map->call_op, nc + 1);
    D.list_point = B.up(map->list_point, nl); D.op_feat = B.up(map->op_feat, nf); D.obs_out_start = B.up(map->obs_out_start, nb + 1);
    viorb_fuse_result O;
    const FuseArr<int32_t> i32[] = {
        fuse_arr(B, result->status, nb, &O.status), fuse_arr(B, result->kp_point_out, ni, &O.kp_point_out), fuse_arr(B, result->pt_nobs_out, np, &O.pt_nobs_out),
        fuse_arr(B, result->obs_start_out, np + 1, &O.obs_start_out), fuse_arr(B, result->obs_feat_out, nq, &O.obs_feat_out), fuse_arr(B, result->need, nb, &O.need),
        fuse_arr(B, result->pt_found_out, np, &O.pt_found_out), fuse_arr(B, result->pt_visible_out, np, &O.pt_visible_out),
        fuse_arr(B, result->pt_replaced_out, np, &O.pt_replaced_out), fuse_arr(B, result->dirty_obs_start, np + 1, &O.dirty_obs_start),
        fuse_arr(B, result->dirty_obs_kf, nq, &O.dirty_obs_kf), fuse_arr(B, result->dirty_obs_feat, nq, &O.dirty_obs_feat),
        fuse_arr(B, result->op_reason, nj, &O.op_reason), fuse_arr(B, result->op_other, nj, &O.op_other), fuse_arr(B, result->call_nfused, nc, &O.call_nfused)};
    const FuseArr<uint8_t> u8[] = {fuse_arr(B, result->pt_bad_out, np, &O.pt_bad_out), fuse_arr(B, result->pt_dirty, np, &O.pt_dirty),
                                   fuse_arr(B, result->obs_touched, no, &O.obs_touched)};
    const FuseArr<uint32_t> u32[] = {fuse_arr(B, result->obs_out, nq, &O.obs_out)};
    const size_t wb = viorb_apply_fuse_workspace_bytes(map->batch, map->n_kf, map->n_pt, map->n_obs, map->n_op);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_apply_fuse_device(&D, &O, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    for (const FuseArr<int32_t>& a : i32) VIORB_TRY(download(a.host, a.dev, a.n));
    for (const FuseArr<uint8_t>& a : u8) VIORB_TRY(download(a.host, a.dev, a.n));
    for (const FuseArr<uint32_t>& a : u32) VIORB_TRY(download(a.host, a.dev, a.n));
    return VIORB_OK;
}

int viorb_fuse_merge_descriptors_device(const uint8_t* pt_dirty, const int32_t* dirty_obs_start, const uint8_t* new_desc, uint8_t* pts_desc, int n_pt, void* stream) {
    VIORB_REQUIRE(pt_dirty && new_desc && pts_desc, "null array");
    VIORB_REQUIRE(n_pt >= 0, "n_pt >= 0");
    VIORB_REQUIRE((((uintptr_t)new_desc | (uintptr_t)pts_desc) & 3) == 0, "descriptor rows 4-byte aligned");
    VIORB_TRY(require_device());
    if (n_pt == 0) return VIORB_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)(((long long)n_pt * 8 + FUSE_THREADS - 1) / FUSE_THREADS);
    VIORB_LAUNCH(k_fuse_merge_desc, blocks, FUSE_THREADS, 0, st, pt_dirty, dirty_obs_start, (const uint32_t*)new_desc, (uint32_t*)pts_desc, n_pt);
    return VIORB_OK;
}

// ---- host-only test hook: map_fusion_core.h compiled for the host ---------------------------------------------------------------------------
int viorb_debug_apply_fuse_host(const viorb_fuse_map* map, const viorb_fuse_result* result) {
    VIORB_TRY(fuse_check(map, result));
    const size_t nk = (size_t)map->n_kf + 1, nb = (size_t)map->batch, np = (size_t)map->n_pt + 1, nj = (size_t)map->n_op + 1, ne = (size_t)map->n_obs + nj;
    std::vector<int32_t> rank(nk), bad(np), replaced(np), dirty(np), stamp(np), head(np), tail(np), cnt(np), dcnt(np), next(np + nj), rep(nj), pfeat(ne), info(nb), tot(nb), dtot(nb);
    std::vector<uint32_t> found(np), visible(np), pool(ne);
    FuseWork W;
    W.rank = rank.data(); W.bad = bad.data(); W.replaced = replaced.data(); W.dirty = dirty.data(); W.stamp = stamp.data(); W.found = found.data(); W.visible = visible.data();
    W.head = head.data(); W.tail = tail.data(); W.cnt = cnt.data(); W.dcnt = dcnt.data(); W.next = next.data(); W.rep = rep.data(); W.pool = pool.data(); W.pfeat = pfeat.data();
    W.info = info.data(); W.tot = tot.data(); W.dtot = dtot.data();
    fuse_run_host(fuse_map(*map), W, fuse_out(*result));
    return VIORB_OK;
}

} // extern "C"
