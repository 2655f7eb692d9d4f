// viorb_amd/csrc/covisibility.hip — KeyFrame::UpdateConnections for the targets of a batch of streams (include/viorb_covisibility.h):
//   k_covis_prepare   validates a stream's part of the snapshot and copies its rows into the result, the working state  (one workgroup per stream)
//   k_covis_votes     KFcounter of every target: votes, then the counter in key order with nmax, pKFmax, vPairs.size()  (workgroups over stream x target)
//   k_covis_ordered   the targets of a stream in call order: AddConnection on the added key frames, one wavefront each;
//                     the target's own members; the first connection; LoopConnections                                    (one workgroup per stream)
// The logic is covis_core.h. Shape (DESIGN.md "Covisibility graph"): during a call the votes depend only on kp_point, pt_bad and obs, which
// no target changes, so all counters are computed first and in parallel, by integer atomic adds, in LDS while the stream's key frames
// fit; a counter becomes a row in key order by prefix scan (no sort); only AddConnection and the target's own members are ordered, and
// every rebuild of an ordered list is a rank sort over a total order, which no schedule changes.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "covis_core.h"

namespace viorb {

enum { COV_WAVE = 64, COV_THREADS = 256, COV_WAVES = COV_THREADS / COV_WAVE, COV_LDS_KF = 2048, COV_VOTE_GROUPS = 32 };

// The exclusive prefix of a flag over the workgroup's threads and the total, to every thread. Every thread calls it.
__device__ __forceinline__ int cov_block_scan_flag(bool f, int& total, int* s_part) {
    const int lane = threadIdx.x & (COV_WAVE - 1), w = threadIdx.x / COV_WAVE;
    const unsigned long long m = __ballot(f);
    if (lane == 0) s_part[w] = __popcll(m);
    __syncthreads();
    int base = 0; total = 0;
#pragma unroll
    for (int k = 0; k < COV_WAVES; k++) { const int s = s_part[k]; if (k < w) base += s; total += s; }
    __syncthreads();
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

// A value combined over the wavefront's 64 lanes (all active)
struct CovWave {
    __device__ int sum(int v) const { return __popcll(__ballot(v != 0)); }          // v is 0 or 1
    __device__ bool any(bool v) const { return __ballot(v) != 0; }
};

// blockIdx.x = stream. A refused stream gets info = 0 and nothing else; the later kernels read that first.
__global__ __launch_bounds__(COV_THREADS) void k_covis_prepare(CovMap M, CovWork W, CovOut R) {
    const int b = blockIdx.x, t = threadIdx.x, nt = COV_THREADS;
    int ok = __syncthreads_and(cov_validate_ranges(M, b, t, nt));
    SnapStream S = {0, 0, 0, 0};
    if (ok) { S = snap_stream(M.kf_start, M.pt_start, b); ok = __syncthreads_and(cov_validate_offsets(M, S, b, t, nt)); }
    if (ok) ok = __syncthreads_and(cov_validate_entries(M, S, b, t, nt));
    if (ok) {                                                        // plain stores of this workgroup, one CU: a barrier between fill and check
        snap_distinct_fill(M.kf_by_key + S.k0, S.nk, W.rank + S.k0, t, nt);
        __syncthreads();
        ok = __syncthreads_and(snap_distinct_check(M.kf_by_key + S.k0, S.nk, W.rank + S.k0, t, nt));
    }
    if (ok) ok = __syncthreads_and(cov_validate_rows(M, S, W.rank + S.k0, t, nt));
    if (ok) cov_copy_rows(M, S, W, R, t, nt);
    if (t == 0) W.info[b] = ok;
}

// blockIdx.y = stream; the workgroups of a stream stride over its targets. One counter per workgroup.
__global__ __launch_bounds__(COV_THREADS) void k_covis_votes(CovMap M, CovWork W) {
    __shared__ int32_t s_votes[COV_LDS_KF];
    __shared__ int s_part[COV_WAVES];
    __shared__ unsigned long long s_best;
    __shared__ int s_nth;
    const int b = blockIdx.y, t = threadIdx.x, nt = COV_THREADS;
    if (!W.info[b]) return;                                          // the whole workgroup
    const SnapStream S = snap_stream(M.kf_start, M.pt_start, b);
    const int t0 = M.target_start[b], n_t = M.target_start[b + 1] - t0;
    int32_t* votes = S.nk <= COV_LDS_KF ? s_votes : W.votes + (size_t)blockIdx.x * M.n_kf + S.k0;
    for (int ti = blockIdx.x; ti < n_t; ti += gridDim.x) {
        const int gt = t0 + ti, kt = M.target_kf[gt], g = S.k0 + kt;
        for (int k = t; k < S.nk; k += nt) votes[k] = 0;
        if (t == 0) { s_best = 0ull; s_nth = 0; }
        __syncthreads();
        for (int i = t, e = M.kp_start[g + 1] - M.kp_start[g]; i < e; i += nt) cov_vote_keypoint(M, S, votes, kt, i);    // :593-611: a lane per keypoint
        __syncthreads();                                             // every atomic add has been performed (s_waitcnt before the barrier)
        // the walk of KFcounter in key order (:625-637): an ordered compaction, nt key positions a pass
        int n = 0, n_th = 0; long long best = 0;
        for (int j0 = 0; j0 < S.nk; j0 += nt) {
            int v = 0; long long key = 0;
            const int k = j0 + t < S.nk ? cov_counter_slot(M, S, votes, j0 + t, &v, &key) : -1;
            int total;
            const int at = n + cov_block_scan_flag(k >= 0, total, s_part);
            if (k >= 0) {
                if (at < M.ccap) { W.ckf[(size_t)gt * M.ccap + at] = k; W.cw[(size_t)gt * M.ccap + at] = v; }
                if (key > best) best = key;
                n_th += v >= COV_TH;
            }
            n += total;
        }
        if (best > 0) atomicMax(&s_best, (unsigned long long)best);
        if (n_th) atomicAdd(&s_nth, n_th);
        __syncthreads();
        if (t == 0) cov_write_counter_info(M, S, W, gt, n, s_nth, (long long)s_best);
        __syncthreads();                                             // s_best, s_nth and the counter are free for the next target
    }
}

// blockIdx.x = stream.
__global__ __launch_bounds__(COV_THREADS) void k_covis_ordered(CovMap M, CovWork W, CovOut R) {
    __shared__ int32_t s_mark[COV_LDS_KF];
    __shared__ int s_part[COV_WAVES];
    __shared__ unsigned int s_ovf;
    __shared__ int32_t s_front;
    const int b = blockIdx.x, t = threadIdx.x, nt = COV_THREADS, lane = t & (COV_WAVE - 1), wave = t / COV_WAVE;
    if (!W.info[b]) { if (t == 0) cov_write_refused(R, b); return; }       // the whole workgroup
    const SnapStream S = snap_stream(M.kf_start, M.pt_start, b);
    const int t0 = M.target_start[b], n_t = M.target_start[b + 1] - t0;
    const bool loop = R.loop_conn || R.n_loop_conn;
    int32_t* mark = S.nk <= COV_LDS_KF ? s_mark : W.mark + S.k0;
    const int32_t* rank = W.rank + S.k0;
    if (loop) {
        for (int k = t; k < S.nk; k += nt) mark[k] = 0;
        __syncthreads();
        if (M.erase_targets) for (int i = t; i < n_t; i += nt) mark[M.target_kf[t0 + i]] = 1;      // a repeated target: the same value twice
    }
    int status = COV_OK, need = 0;
    for (int ti = 0; ti < n_t; ti++) {
        const int gt = t0 + ti, kt = M.target_kf[gt], gen = ti + 1;
        const int32_t* cinfo = W.cinfo + (size_t)gt * COV_C; const int32_t* ckf = W.ckf + (size_t)gt * M.ccap; const int32_t* cw = W.cw + (size_t)gt * M.ccap;
        const int n = cinfo[COV_C_N];
        __syncthreads();                                             // the rows and marks as the earlier targets left them
        if (loop) cov_mark_previous(M, S, R, mark, kt, gen, t, nt);
        if (t == 0) { s_ovf = 0xffffffffu; s_front = -1; }
        if (n > M.ccap) { status = COV_OVERFLOW; need = n; break; }   // the same n for every thread
        __syncthreads();
        // AddConnection (:635, :642) on every key frame of vPairs: they are distinct and none is the target, so their rows are disjoint.
        // Every wavefront walks the counter and takes the added entries whose ordinal is its own modulo the number of wavefronts.
        int ordinal = 0;
        for (int i0 = 0; i0 < n; i0 += COV_WAVE) {
            const int i = i0 + lane, k = i < n ? ckf[i] : -1, v = i < n ? cw[i] : 0;
            unsigned long long m = __ballot(k >= 0 && cov_is_added(cinfo, k, v));
            while (m) {
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                if (ordinal++ % COV_WAVES != wave) continue;
                const int x = __shfl(k, src), w = __shfl(v, src);
                const int rc = cov_add_connection(M, S, R, rank, x, kt, w, lane, COV_WAVE, CovWave());
                if (rc < 0 && lane == 0) atomicMin(&s_ovf, ((unsigned int)rank[x] << 16) | (unsigned int)(-rc));      // the first in key order
            }
        }
        __syncthreads();
        if (s_ovf != 0xffffffffu) { status = COV_OVERFLOW; need = (int)(s_ovf & 0xffffu); break; }
        if (n > 0) cov_replace_target(M, S, R, ckf, cw, cinfo, kt, &s_front, t, nt);
        __syncthreads();
        if (t == 0) cov_finish_target(M, S, W, R, cinfo, gt, kt, s_front);
        if (loop) {                                                  // LoopConnections: the map after the call in key order, compacted
            __syncthreads();
            const int cn = R.conn_n_out[S.k0 + kt];
            int m = 0;
            for (int i0 = 0; i0 < cn; i0 += nt) {
                const int s = i0 + t < cn ? cov_loop_kept(M, S, R, mark, kt, gen, i0 + t) : -1;
                int total;
                const int at = m + cov_block_scan_flag(s >= 0, total, s_part);
                if (s >= 0 && R.loop_conn) R.loop_conn[(size_t)gt * M.ccap + at] = s;
                m += total;
            }
            if (R.loop_conn) for (int i = m + t; i < M.ccap; i += nt) R.loop_conn[(size_t)gt * M.ccap + i] = -1;
            if (t == 0 && R.n_loop_conn) R.n_loop_conn[gt] = m;
        }
    }
    if (t == 0) { R.status[b] = status; if (R.need) R.need[b] = need; }
}

} // namespace viorb

using namespace viorb;

namespace {

int cov_vote_groups(int batch, int n_target) { return (int)std::min<long long>(((long long)n_target / batch) * 2 + 1, COV_VOTE_GROUPS); }

struct CovLayout { CovWork W; size_t total; };
CovLayout cov_layout(void* base, int batch, int n_kf, int n_target, int ccap) {
    CovLayout L; WorkspaceLayout Y(base);
    Y.take(&L.W.rank, (size_t)n_kf); Y.take(&L.W.flags, (size_t)n_kf); Y.take(&L.W.mark, (size_t)n_kf);
    Y.take(&L.W.votes, n_kf > COV_LDS_KF ? (size_t)cov_vote_groups(batch, n_target) * n_kf : 0);      // no stream can be above the LDS limit otherwise
    Y.take(&L.W.ckf, (size_t)n_target * ccap); Y.take(&L.W.cw, (size_t)n_target * ccap);
    Y.take(&L.W.cinfo, (size_t)n_target * COV_C); Y.take(&L.W.info, (size_t)batch);
    L.total = Y.end();
    return L;
}

int cov_check(const viorb_covis_map* m, const viorb_covis_result* r, int ccap) {
    VIORB_REQUIRE(m && r, "null struct");
    VIORB_REQUIRE(m->batch >= 1 && m->batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(m->n_kf >= 0 && m->n_kp >= 0 && m->n_pt >= 0 && m->n_obs >= 0 && m->n_conn >= 0 && m->n_ord >= 0 && m->n_target >= 0, "a negative total");
    VIORB_REQUIRE(ccap >= 1, "ccap >= 1");
    VIORB_REQUIRE(m->kf_start && m->kf_by_key && m->kf_flags && m->kf_parent && m->kp_start && m->kp_point && m->pt_start && m->pt_bad && m->obs_start && m->obs, "null array");
    VIORB_REQUIRE(m->conn_start && m->conn_kf && m->conn_w && m->ord_start && m->ord_kf && m->ord_w && m->target_start && m->target_kf, "null array");
    VIORB_REQUIRE(r->conn_kf_out && r->conn_w_out && r->conn_n_out && r->ord_kf_out && r->ord_w_out && r->ord_n_out && r->status, "null required result array");
    return VIORB_OK;
}

CovMap cov_map(const viorb_covis_map& m, int ccap, int erase_targets) {
    CovMap M;
    M.batch = m.batch; M.n_kf = m.n_kf; M.n_kp = m.n_kp; M.n_pt = m.n_pt; M.n_obs = m.n_obs; M.n_conn = m.n_conn; M.n_ord = m.n_ord; M.n_target = m.n_target;
    M.kf_start = m.kf_start; M.kf_by_key = m.kf_by_key; M.kf_flags = m.kf_flags; M.kf_parent = m.kf_parent; M.kp_start = m.kp_start; M.kp_point = m.kp_point;
    M.pt_start = m.pt_start; M.pt_bad = m.pt_bad; M.obs_start = m.obs_start; M.obs = m.obs;
    M.conn_start = m.conn_start; M.conn_kf = m.conn_kf; M.conn_w = m.conn_w; M.ord_start = m.ord_start; M.ord_kf = m.ord_kf; M.ord_w = m.ord_w;
    M.target_start = m.target_start; M.target_kf = m.target_kf;
    M.ccap = ccap; M.erase_targets = erase_targets ? 1 : 0;
    return M;
}
CovOut cov_out(const viorb_covis_result& r) {
    CovOut R;
    R.conn_kf_out = r.conn_kf_out; R.conn_w_out = r.conn_w_out; R.conn_n_out = r.conn_n_out; R.ord_kf_out = r.ord_kf_out; R.ord_w_out = r.ord_w_out;
    R.ord_n_out = r.ord_n_out; R.status = r.status; R.need = r.need; R.kf_parent_out = r.kf_parent_out; R.kf_flags_out = r.kf_flags_out; R.kf_touched = r.kf_touched;
    R.t_observers = r.t_observers; R.t_max_kf = r.t_max_kf; R.t_max_w = r.t_max_w; R.t_added = r.t_added; R.t_parent = r.t_parent;
    R.loop_conn = r.loop_conn; R.n_loop_conn = r.n_loop_conn;
    return R;
}

} // namespace

extern "C" {

size_t viorb_update_connections_workspace_bytes(int batch, int n_kf, int n_target, int ccap) {
    if (batch < 1 || batch > 65535 || n_kf < 0 || n_target < 0 || ccap < 1) return 0;
    return cov_layout(nullptr, batch, n_kf, n_target, ccap).total;
}

int viorb_update_connections_shape(int32_t* out4) {
    VIORB_REQUIRE(out4, "null array");
    out4[0] = COV_THREADS; out4[1] = COV_WAVE; out4[2] = COV_LDS_KF; out4[3] = COV_TH;
    return VIORB_OK;
}

int viorb_update_connections_device(const viorb_covis_map* map, const viorb_covis_result* result, int ccap, int erase_targets,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(cov_check(map, result, ccap));
    VIORB_REQUIRE_WORKSPACE(workspace, workspace_bytes, cov_layout(nullptr, map->batch, map->n_kf, map->n_target, ccap).total, "viorb_update_connections_workspace_bytes");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const CovMap M = cov_map(*map, ccap, erase_targets);
    const CovWork W = cov_layout(workspace, map->batch, map->n_kf, map->n_target, ccap).W;
    const CovOut R = cov_out(*result);
    VIORB_LAUNCH(k_covis_prepare, M.batch, COV_THREADS, 0, st, M, W, R);
    VIORB_LAUNCH(k_covis_votes, dim3(cov_vote_groups(M.batch, M.n_target), M.batch), COV_THREADS, 0, st, M, W);
    VIORB_LAUNCH(k_covis_ordered, M.batch, COV_THREADS, 0, st, M, W, R);
    return VIORB_OK;
}

int viorb_update_connections(const viorb_covis_map* map, const viorb_covis_result* result, int ccap, int erase_targets) {
    VIORB_TRY(cov_check(map, result, ccap));
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t nb = (size_t)map->batch, nk = (size_t)map->n_kf, ni = (size_t)map->n_kp, np = (size_t)map->n_pt, no = (size_t)map->n_obs, nc = (size_t)map->n_conn,
                 nr = (size_t)map->n_ord, ntg = (size_t)map->n_target, cc = (size_t)ccap;
    viorb_covis_map D = *map;
    D.kf_start = B.up(map->kf_start, nb + 1); D.kf_by_key = B.up(map->kf_by_key, nk); D.kf_flags = B.up(map->kf_flags, nk); D.kf_parent = B.up(map->kf_parent, nk);
    D.kp_start = B.up(map->kp_start, nk + 1); D.kp_point = B.up(map->kp_point, ni); D.pt_start = B.up(map->pt_start, nb + 1); D.pt_bad = B.up(map->pt_bad, np);
    D.obs_start = B.up(map->obs_start, np + 1); D.obs = B.up(map->obs, no);
    D.conn_start = B.up(map->conn_start, nk + 1); D.conn_kf = B.up(map->conn_kf, nc); D.conn_w = B.up(map->conn_w, nc);
    D.ord_start = B.up(map->ord_start, nk + 1); D.ord_kf = B.up(map->ord_kf, nr); D.ord_w = B.up(map->ord_w, nr);
    D.target_start = B.up(map->target_start, nb + 1); D.target_kf = B.up(map->target_kf, ntg);
    viorb_covis_result O;
    O.conn_kf_out = B.zeros<int32_t>(nk * cc); O.conn_w_out = B.zeros<int32_t>(nk * cc); O.conn_n_out = B.zeros<int32_t>(nk);
    O.ord_kf_out = B.zeros<int32_t>(nk * cc); O.ord_w_out = B.zeros<int32_t>(nk * cc); O.ord_n_out = B.zeros<int32_t>(nk);
    O.status = B.zeros<int32_t>(nb); O.need = B.zeros<int32_t>(nb);
    O.kf_parent_out = B.zeros<int32_t>(nk); O.kf_flags_out = B.zeros<uint8_t>(nk); O.kf_touched = B.zeros<uint8_t>(nk);
    O.t_observers = B.zeros<int32_t>(ntg); O.t_max_kf = B.zeros<int32_t>(ntg); O.t_max_w = B.zeros<int32_t>(ntg); O.t_added = B.zeros<int32_t>(ntg);
    O.t_parent = B.zeros<int32_t>(ntg); O.loop_conn = B.zeros<int32_t>(ntg * cc); O.n_loop_conn = B.zeros<int32_t>(ntg);
    const size_t wb = viorb_update_connections_workspace_bytes(map->batch, map->n_kf, map->n_target, ccap);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_update_connections_device(&D, &O, ccap, erase_targets, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    // a refused stream writes nothing but its status: its ranges of the caller's arrays stay as they are. The key frames and targets of an
    // accepted stream lie at kf_start / target_start [b] .. [b + 1], which the validator keeps apart from every other accepted stream's.
    std::vector<int32_t> status(nb), tmp;
    std::vector<uint8_t> tmp8;
    VIORB_TRY(download(status.data(), O.status, nb));
    std::copy(status.begin(), status.end(), result->status);
    if (result->need) { tmp.resize(nb); VIORB_TRY(download(tmp.data(), O.need, nb)); for (size_t b = 0; b < nb; b++) if (status[b] != VIORB_ERR_INVALID_ARG) result->need[b] = tmp[b]; }
    struct Rows { int32_t* host; const int32_t* dev; const int32_t* start; size_t n, row; };
    const Rows rows[] = {{result->conn_kf_out, O.conn_kf_out, map->kf_start, nk, cc}, {result->conn_w_out, O.conn_w_out, map->kf_start, nk, cc}, {result->conn_n_out, O.conn_n_out, map->kf_start, nk, 1},
                         {result->ord_kf_out, O.ord_kf_out, map->kf_start, nk, cc}, {result->ord_w_out, O.ord_w_out, map->kf_start, nk, cc}, {result->ord_n_out, O.ord_n_out, map->kf_start, nk, 1},
                         {result->kf_parent_out, O.kf_parent_out, map->kf_start, nk, 1},
                         {result->t_observers, O.t_observers, map->target_start, ntg, 1}, {result->t_max_kf, O.t_max_kf, map->target_start, ntg, 1}, {result->t_max_w, O.t_max_w, map->target_start, ntg, 1},
                         {result->t_added, O.t_added, map->target_start, ntg, 1}, {result->t_parent, O.t_parent, map->target_start, ntg, 1},
                         {result->loop_conn, O.loop_conn, map->target_start, ntg, cc}, {result->n_loop_conn, O.n_loop_conn, map->target_start, ntg, 1}};
    for (const Rows& r : rows) {
        if (!r.host) continue;
        tmp.resize(r.n * r.row);
        VIORB_TRY(download(tmp.data(), r.dev, tmp.size()));
        for (size_t b = 0; b < nb; b++)
            if (status[b] != VIORB_ERR_INVALID_ARG) std::copy(tmp.begin() + (size_t)r.start[b] * r.row, tmp.begin() + (size_t)r.start[b + 1] * r.row, r.host + (size_t)r.start[b] * r.row);
    }
    struct Bytes { uint8_t* host; const uint8_t* dev; };
    const Bytes bytes[] = {{result->kf_flags_out, O.kf_flags_out}, {result->kf_touched, O.kf_touched}};
    for (const Bytes& r : bytes) {
        if (!r.host) continue;
        tmp8.resize(nk);
        VIORB_TRY(download(tmp8.data(), r.dev, nk));
        for (size_t b = 0; b < nb; b++)
            if (status[b] != VIORB_ERR_INVALID_ARG) std::copy(tmp8.begin() + map->kf_start[b], tmp8.begin() + map->kf_start[b + 1], r.host + map->kf_start[b]);
    }
    return VIORB_OK;
}

// ---- host-only test hook: covis_core.h compiled for the host ----------------------------------------------------------------------------
int viorb_debug_update_connections_host(const viorb_covis_map* map, const viorb_covis_result* result, int ccap, int erase_targets) {
    VIORB_TRY(cov_check(map, result, ccap));
    const size_t nk = (size_t)map->n_kf + 1, nb = (size_t)map->batch, ntg = (size_t)map->n_target + 1;
    std::vector<int32_t> rank(nk), flags(nk), mark(nk), votes(nk), ckf(ntg * ccap), cw(ntg * ccap), cinfo(ntg * COV_C), info(nb);
    CovWork W;
    W.rank = rank.data(); W.flags = flags.data(); W.mark = mark.data(); W.votes = votes.data(); W.ckf = ckf.data(); W.cw = cw.data(); W.cinfo = cinfo.data(); W.info = info.data();
    cov_run_host(cov_map(*map, ccap, erase_targets), W, cov_out(*result));
    return VIORB_OK;
}

} // extern "C"
