// viorb_amd/csrc/kf_removal.hip — KeyFrame::SetBadFlag / KeyFrame::SetErase for the ordered operations of a batch of streams
// (include/viorb_kf_removal.h):
//   k_kfr_prepare   validates a stream's part of the snapshot, builds the rank and copies rows and state into the result and the workspace
//   k_kfr_ordered   the operations of a stream in call order: the neighbours' EraseConnection, one wavefront per neighbour row; the
//                   points' EraseObservation, a lane per keypoint; the parent search, a lane per (child, list position) and one 64-bit
//                   maximum per round; mTcp and the links                                                (both: one workgroup per stream)
// The logic is kf_removal_core.h. Shape (DESIGN.md "Key-frame removal"): an operation reads what the earlier ones left, so the operations
// of a stream are serial and the batch is the parallelism; inside an operation the neighbours' rows are disjoint, the points of the key
// frame are distinct, and the search's winner is the maximum of a total order, so no schedule changes a result.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "kf_removal_core.h"

namespace viorb {

enum { KFR_WAVE = 64, KFR_THREADS = 256, KFR_WAVES = KFR_THREADS / KFR_WAVE, KFR_LDS_KF = 2048 };

struct KfrWave {
    __device__ int sum(int v) const { return __popcll(__ballot(v != 0)); }          // v is 0 or 1
    __device__ bool any(bool v) const { return __ballot(v) != 0; }
};

// blockIdx.x = stream. A refused stream gets info = 0 and nothing else; the ordered kernel reads that first.
__global__ __launch_bounds__(KFR_THREADS) void k_kfr_prepare(KfrMap M, KfrWork W, KfrOut R) {
    const int b = blockIdx.x, t = threadIdx.x, nt = KFR_THREADS;
    const CovMap& C = M.C;
    int ok = __syncthreads_and(cov_validate_ranges(C, b, t, nt));
    SnapStream S = {0, 0, 0, 0};
    if (ok) { S = snap_stream(C.kf_start, C.pt_start, b); ok = __syncthreads_and(cov_validate_offsets(C, S, b, t, nt)); }
    if (ok) ok = __syncthreads_and(kfr_validate_scalars(M, S, b, t, nt));
    if (ok) ok = __syncthreads_and(cov_validate_entries(C, S, b, t, nt));
    if (ok) {
        snap_distinct_fill(C.kf_by_key + S.k0, S.nk, W.C.rank + S.k0, t, nt);
        __syncthreads();
        ok = __syncthreads_and(snap_distinct_check(C.kf_by_key + S.k0, S.nk, W.C.rank + S.k0, t, nt));
    }
    if (ok) ok = __syncthreads_and(cov_validate_rows(C, S, W.C.rank + S.k0, t, nt));
    if (ok) ok = __syncthreads_and(kfr_validate_ops(M, S, b, t, nt));
    if (ok) { cov_copy_rows(C, S, W.C, R.C, t, nt); kfr_prepare(M, S, W, R, t, nt); }
    if (t == 0) W.C.info[b] = ok;
}

// blockIdx.x = stream.
__global__ __launch_bounds__(KFR_THREADS) void k_kfr_ordered(KfrMap M, KfrWork W, KfrOut R) {
    __shared__ int32_t s_mark[KFR_LDS_KF];
    __shared__ int32_t s_cnt[KFR_N];
    __shared__ unsigned long long s_best;
    const int b = blockIdx.x, t = threadIdx.x, nt = KFR_THREADS, lane = t & (KFR_WAVE - 1), wave = t / KFR_WAVE;
    const CovMap& C = M.C;
    if (!W.C.info[b]) { if (t == 0) cov_write_refused(R.C, b); return; }       // the whole workgroup
    const SnapStream S = snap_stream(C.kf_start, C.pt_start, b);
    const int j0 = C.target_start[b], n_op = C.target_start[b + 1] - j0;
    int32_t* mark = S.nk <= KFR_LDS_KF ? s_mark : W.mark + S.k0;
    const int32_t* rank = W.C.rank + S.k0;
    for (int k = t; k < S.nk; k += nt) mark[k] = 0;
    for (int oi = 0; oi < n_op; oi++) {
        const int x = C.target_kf[j0 + oi], g = S.k0 + x, gen = oi + 1;
        __syncthreads();                                             // the state as the earlier operations left it
        int nf;
        const int reason = kfr_decide(W.C.flags[g], M.op_kind[j0 + oi], &nf);        // the same for every thread
        const int P = W.parent[g];
        if (t < KFR_N) s_cnt[t] = 0;
        if (t == 0) s_best = 0ull;
        __syncthreads();                                             // every thread has read the flags
        if (reason != KFR_REMOVED) {
            if (t == 0) { W.C.flags[g] = nf; kfr_write_op(R, j0 + oi, reason, s_cnt); }
            continue;
        }
        // EraseConnection on the key frames of x's map (:772-773): they are distinct and none is x, so their rows are disjoint; entry i goes to
        // wavefront i modulo the number of wavefronts. x's own row is only read here.
        const int cn = R.C.conn_n_out[g];
        for (int i = wave; i < cn; i += KFR_WAVES) {
            const int n = R.C.conn_kf_out[(size_t)g * C.ccap + i];
            if (kfr_erase_connection(C, S, R.C, rank, n, x, lane, KFR_WAVE, KfrWave()) && lane == 0) atomicAdd(&s_cnt[KFR_N_REBUILT], 1);
        }
        // EraseObservation (:775-777): a lane per keypoint
        for (int i = C.kp_start[g] + t, e = C.kp_start[g + 1]; i < e; i += nt) kfr_erase_observation(C, S, W, R, rank, x, i, s_cnt);
        kfr_collect_children(S, W, x, s_cnt, t, nt);
        if (t == 0 && P >= 0) mark[P] = gen;
        __syncthreads();
        kfr_clear_own(C, S, R.C, x, t, nt);
        const int n_child = s_cnt[KFR_N_CHILDREN];
        for (int round = 0; round < n_child; round++) {              // each round takes one child or ends the loop
            const unsigned long long mine = kfr_search_round(C, S, W, R.C, rank, mark, x, gen, n_child, wave, KFR_WAVES, lane, KFR_WAVE);
            if (mine) atomicMax(&s_best, mine);
            __syncthreads();
            const unsigned long long key = s_best;
            if (!key) break;                                         // the same for every thread
            __syncthreads();                                         // every thread has read the winner
            if (t == 0) { kfr_adopt(C, S, W, R.C, mark, key, gen); s_best = 0ull; }
            __syncthreads();
        }
        kfr_fallback(S, W, R.C, x, P, n_child, s_cnt, t, nt);
        __syncthreads();
        if (t == 0) { W.C.flags[g] = nf; kfr_finish_removal(M, S, W, R, x, P); kfr_write_op(R, j0 + oi, reason, s_cnt); }
    }
    __syncthreads();
    kfr_write_state(M, S, W, R, t, nt);
    if (t == 0) R.C.status[b] = COV_OK;
}

} // namespace viorb

using namespace viorb;

namespace {

struct KfrLayout { KfrWork W; size_t total; };
KfrLayout kfr_layout(void* base, int batch, int n_kf, int n_pt) {
    KfrLayout L; WorkspaceLayout Y(base);
    L.W.C = CovWork();
    Y.take(&L.W.C.rank, (size_t)n_kf); Y.take(&L.W.C.flags, (size_t)n_kf); Y.take(&L.W.parent, (size_t)n_kf); Y.take(&L.W.prev, (size_t)n_kf);
    Y.take(&L.W.next, (size_t)n_kf); Y.take(&L.W.mark, (size_t)n_kf); Y.take(&L.W.child, (size_t)n_kf);
    Y.take(&L.W.pt, (size_t)n_pt); Y.take(&L.W.ref, (size_t)n_pt); Y.take(&L.W.C.info, (size_t)batch);
    L.total = Y.end();
    return L;
}

int kfr_check(const viorb_kfr_map* m, const viorb_kfr_result* r, int ccap) {
    VIORB_REQUIRE(m && r, "null struct");
    VIORB_REQUIRE(m->batch >= 1 && m->batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(m->n_kf >= 0 && m->n_kp >= 0 && m->n_pt >= 0 && m->n_obs >= 0 && m->n_conn >= 0 && m->n_ord >= 0 && m->n_op >= 0, "a negative total");
    VIORB_REQUIRE(ccap >= 1, "ccap >= 1");
    VIORB_REQUIRE(m->kf_start && m->kf_by_key && m->kf_flags && m->kf_parent && m->kf_prev && m->kf_next && m->kf_pose12 && m->kp_start && m->kp_point, "null array");
    VIORB_REQUIRE(m->pt_start && m->pt_bad && m->pt_nobs && m->pt_ref && m->obs_start && m->obs, "null array");
    VIORB_REQUIRE(m->conn_start && m->conn_kf && m->conn_w && m->ord_start && m->ord_kf && m->ord_w && m->op_start && m->op_kf && m->op_kind, "null array");
    VIORB_REQUIRE(r->conn_kf_out && r->conn_w_out && r->conn_n_out && r->ord_kf_out && r->ord_w_out && r->ord_n_out && r->status, "null required result array");
    return VIORB_OK;
}

KfrMap kfr_map(const viorb_kfr_map& m, int ccap) {
    KfrMap M;
    CovMap& C = M.C;
    C.batch = m.batch; C.n_kf = m.n_kf; C.n_kp = m.n_kp; C.n_pt = m.n_pt; C.n_obs = m.n_obs; C.n_conn = m.n_conn; C.n_ord = m.n_ord; C.n_target = m.n_op;
    C.kf_start = m.kf_start; C.kf_by_key = m.kf_by_key; C.kf_flags = m.kf_flags; C.kf_parent = m.kf_parent; C.kp_start = m.kp_start; C.kp_point = m.kp_point;
    C.pt_start = m.pt_start; C.pt_bad = m.pt_bad; C.obs_start = m.obs_start; C.obs = m.obs;
    C.conn_start = m.conn_start; C.conn_kf = m.conn_kf; C.conn_w = m.conn_w; C.ord_start = m.ord_start; C.ord_kf = m.ord_kf; C.ord_w = m.ord_w;
    C.target_start = m.op_start; C.target_kf = m.op_kf; C.ccap = ccap; C.erase_targets = 0;
    M.kf_prev = m.kf_prev; M.kf_next = m.kf_next; M.kf_pose12 = m.kf_pose12; M.pt_nobs = m.pt_nobs; M.pt_ref = m.pt_ref; M.op_kind = m.op_kind;
    return M;
}
KfrOut kfr_out(const viorb_kfr_result& r) {
    KfrOut R;
    R.C = CovOut();
    R.C.conn_kf_out = r.conn_kf_out; R.C.conn_w_out = r.conn_w_out; R.C.conn_n_out = r.conn_n_out; R.C.ord_kf_out = r.ord_kf_out; R.C.ord_w_out = r.ord_w_out;
    R.C.ord_n_out = r.ord_n_out; R.C.status = r.status; R.C.kf_touched = r.kf_touched;
    R.kf_parent_out = r.kf_parent_out; R.kf_flags_out = r.kf_flags_out; R.kf_prev_out = r.kf_prev_out; R.kf_next_out = r.kf_next_out; R.kf_repreint = r.kf_repreint;
    R.kf_Tcp_out = r.kf_Tcp_out; R.pt_nobs_out = r.pt_nobs_out; R.pt_bad_out = r.pt_bad_out; R.obs_alive = r.obs_alive; R.pt_ref_out = r.pt_ref_out; R.kp_point_out = r.kp_point_out;
    R.op_reason = r.op_reason; R.op_children = r.op_children; R.op_fallback = r.op_fallback; R.op_rebuilt = r.op_rebuilt; R.op_points_bad = r.op_points_bad;
    return R;
}

// One array of the host form: uploaded (the caller's contents, so that what the kernels do not write comes back as it was) and, for an
// accepted stream, its range [start[b], start[b + 1]) * row copied back.
template <class T> struct KfrArr { T* host; T* dev; const int32_t* start; size_t n, row; };
template <class T> int kfr_down(const KfrArr<T>& a, const std::vector<int32_t>& status) {
    if (!a.host) return VIORB_OK;
    std::vector<T> tmp(a.n * a.row);
    VIORB_TRY(download(tmp.data(), a.dev, tmp.size()));
    for (size_t b = 0; b < status.size(); b++)
        if (status[b] != VIORB_ERR_INVALID_ARG) std::copy(tmp.begin() + (size_t)a.start[b] * a.row, tmp.begin() + (size_t)a.start[b + 1] * a.row, a.host + (size_t)a.start[b] * a.row);
    return VIORB_OK;
}

} // namespace

extern "C" {

size_t viorb_remove_key_frames_workspace_bytes(int batch, int n_kf, int n_pt, int n_op) {
    if (batch < 1 || batch > 65535 || n_kf < 0 || n_pt < 0 || n_op < 0) return 0;
    return kfr_layout(nullptr, batch, n_kf, n_pt).total;
}

int viorb_remove_key_frames_shape(int32_t* out4) {
    VIORB_REQUIRE(out4, "null array");
    out4[0] = KFR_THREADS; out4[1] = KFR_WAVE; out4[2] = KFR_LDS_KF; out4[3] = KFR_WAVES;
    return VIORB_OK;
}

int viorb_remove_key_frames_device(const viorb_kfr_map* map, const viorb_kfr_result* result, int ccap, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(kfr_check(map, result, ccap));
    VIORB_REQUIRE_WORKSPACE(workspace, workspace_bytes, kfr_layout(nullptr, map->batch, map->n_kf, map->n_pt).total, "viorb_remove_key_frames_workspace_bytes");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const KfrMap M = kfr_map(*map, ccap);
    const KfrWork W = kfr_layout(workspace, map->batch, map->n_kf, map->n_pt).W;
    const KfrOut R = kfr_out(*result);
    VIORB_LAUNCH(k_kfr_prepare, M.C.batch, KFR_THREADS, 0, st, M, W, R);
    VIORB_LAUNCH(k_kfr_ordered, M.C.batch, KFR_THREADS, 0, st, M, W, R);
    return VIORB_OK;
}

int viorb_remove_key_frames(const viorb_kfr_map* map, const viorb_kfr_result* result, int ccap) {
    VIORB_TRY(kfr_check(map, result, ccap));
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t nb = (size_t)map->batch, nk = (size_t)map->n_kf, ni = (size_t)map->n_kp, np = (size_t)map->n_pt, no = (size_t)map->n_obs, nc = (size_t)map->n_conn,
                 nr = (size_t)map->n_ord, nop = (size_t)map->n_op, cc = (size_t)ccap;
    viorb_kfr_map D = *map;
    D.kf_start = B.up(map->kf_start, nb + 1); D.kf_by_key = B.up(map->kf_by_key, nk); D.kf_flags = B.up(map->kf_flags, nk); D.kf_parent = B.up(map->kf_parent, nk);
    D.kf_prev = B.up(map->kf_prev, nk); D.kf_next = B.up(map->kf_next, nk); D.kf_pose12 = B.up(map->kf_pose12, 12 * nk);
    D.kp_start = B.up(map->kp_start, nk + 1); D.kp_point = B.up(map->kp_point, ni); D.pt_start = B.up(map->pt_start, nb + 1); D.pt_bad = B.up(map->pt_bad, np);
    D.pt_nobs = B.up(map->pt_nobs, np); D.pt_ref = B.up(map->pt_ref, np); D.obs_start = B.up(map->obs_start, np + 1); D.obs = B.up(map->obs, no);
    D.conn_start = B.up(map->conn_start, nk + 1); D.conn_kf = B.up(map->conn_kf, nc); D.conn_w = B.up(map->conn_w, nc);
    D.ord_start = B.up(map->ord_start, nk + 1); D.ord_kf = B.up(map->ord_kf, nr); D.ord_w = B.up(map->ord_w, nr);
    D.op_start = B.up(map->op_start, nb + 1); D.op_kf = B.up(map->op_kf, nop); D.op_kind = B.up(map->op_kind, nop);
    std::vector<int32_t> status(nb);
    viorb_kfr_result O;
    const KfrArr<int32_t> i32[] = {
        {result->conn_kf_out, O.conn_kf_out = B.zeros<int32_t>(nk * cc), map->kf_start, nk, cc}, {result->conn_w_out, O.conn_w_out = B.zeros<int32_t>(nk * cc), map->kf_start, nk, cc},
        {result->conn_n_out, O.conn_n_out = B.zeros<int32_t>(nk), map->kf_start, nk, 1},
        {result->ord_kf_out, O.ord_kf_out = B.zeros<int32_t>(nk * cc), map->kf_start, nk, cc}, {result->ord_w_out, O.ord_w_out = B.zeros<int32_t>(nk * cc), map->kf_start, nk, cc},
        {result->ord_n_out, O.ord_n_out = B.zeros<int32_t>(nk), map->kf_start, nk, 1},
        {result->kf_parent_out, O.kf_parent_out = B.zeros<int32_t>(nk), map->kf_start, nk, 1},
        {result->kf_prev_out, O.kf_prev_out = B.zeros<int32_t>(nk), map->kf_start, nk, 1}, {result->kf_next_out, O.kf_next_out = B.zeros<int32_t>(nk), map->kf_start, nk, 1},
        {result->pt_nobs_out, O.pt_nobs_out = B.zeros<int32_t>(np), map->pt_start, np, 1}, {result->pt_ref_out, O.pt_ref_out = B.zeros<int32_t>(np), map->pt_start, np, 1},
        {result->op_reason, O.op_reason = B.zeros<int32_t>(nop), map->op_start, nop, 1}, {result->op_children, O.op_children = B.zeros<int32_t>(nop), map->op_start, nop, 1},
        {result->op_fallback, O.op_fallback = B.zeros<int32_t>(nop), map->op_start, nop, 1}, {result->op_rebuilt, O.op_rebuilt = B.zeros<int32_t>(nop), map->op_start, nop, 1},
        {result->op_points_bad, O.op_points_bad = B.zeros<int32_t>(nop), map->op_start, nop, 1}};
    const KfrArr<uint8_t> u8[] = {
        {result->kf_flags_out, O.kf_flags_out = B.zeros<uint8_t>(nk), map->kf_start, nk, 1}, {result->kf_repreint, O.kf_repreint = B.zeros<uint8_t>(nk), map->kf_start, nk, 1},
        {result->kf_touched, O.kf_touched = B.zeros<uint8_t>(nk), map->kf_start, nk, 1}, {result->pt_bad_out, O.pt_bad_out = B.zeros<uint8_t>(np), map->pt_start, np, 1}};
    // mTcp is written for the removed key frames only: the others keep what the caller's array holds
    O.kf_Tcp_out = B.up(result->kf_Tcp_out, result->kf_Tcp_out ? 12 * nk : 0, 12 * nk);
    const KfrArr<float> f32[] = {{result->kf_Tcp_out, O.kf_Tcp_out, map->kf_start, nk, 12}};
    O.kp_point_out = B.zeros<int32_t>(ni); O.obs_alive = B.zeros<uint8_t>(no);
    O.status = B.zeros<int32_t>(nb);
    const size_t wb = viorb_remove_key_frames_workspace_bytes(map->batch, map->n_kf, map->n_pt, map->n_op);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_remove_key_frames_device(&D, &O, ccap, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    // a refused stream writes nothing but its status: its ranges of the caller's arrays stay as they are
    VIORB_TRY(download(status.data(), O.status, nb));
    std::copy(status.begin(), status.end(), result->status);
    for (const KfrArr<int32_t>& a : i32) VIORB_TRY(kfr_down(a, status));
    for (const KfrArr<uint8_t>& a : u8) VIORB_TRY(kfr_down(a, status));
    for (const KfrArr<float>& a : f32) VIORB_TRY(kfr_down(a, status));
    // per keypoint and per observation: an accepted stream's nested offsets have passed the validator
    std::vector<int32_t> kp(result->kp_point_out ? ni : 0);
    std::vector<uint8_t> alive(result->obs_alive ? no : 0);
    VIORB_TRY(download(kp.data(), O.kp_point_out, kp.size()));
    VIORB_TRY(download(alive.data(), O.obs_alive, alive.size()));
    for (size_t b = 0; b < nb; b++) {
        if (status[b] == VIORB_ERR_INVALID_ARG) continue;
        const int32_t i0 = map->kp_start[map->kf_start[b]], i1 = map->kp_start[map->kf_start[b + 1]], o0 = map->obs_start[map->pt_start[b]], o1 = map->obs_start[map->pt_start[b + 1]];
        if (result->kp_point_out) std::copy(kp.begin() + i0, kp.begin() + i1, result->kp_point_out + i0);
        if (result->obs_alive) std::copy(alive.begin() + o0, alive.begin() + o1, result->obs_alive + o0);
    }
    return VIORB_OK;
}

// ---- host-only test hook: kf_removal_core.h compiled for the host -------------------------------------------------------------------------
int viorb_debug_remove_key_frames_host(const viorb_kfr_map* map, const viorb_kfr_result* result, int ccap) {
    VIORB_TRY(kfr_check(map, result, ccap));
    const size_t nk = (size_t)map->n_kf + 1, nb = (size_t)map->batch, np = (size_t)map->n_pt + 1;
    std::vector<int32_t> rank(nk), flags(nk), parent(nk), prev(nk), next(nk), mark(nk), child(nk), pt(np), ref(np), info(nb);
    KfrWork W;
    W.C = CovWork();
    W.C.rank = rank.data(); W.C.flags = flags.data(); W.C.info = info.data();
    W.parent = parent.data(); W.prev = prev.data(); W.next = next.data(); W.mark = mark.data(); W.child = child.data(); W.pt = pt.data(); W.ref = ref.data();
    kfr_run_host(kfr_map(*map, ccap), W, kfr_out(*result));
    return VIORB_OK;
}

} // extern "C"
