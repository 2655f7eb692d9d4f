// viorb_amd/csrc/map_correction.hip — the propagation of LoopClosing::CorrectLoop for a batch of streams (include/viorb_map_correction.h):
//   k_correct_loop_prepare   validates a stream's part of the snapshot, claims every point for the member with the lowest key that holds
//                            it, and computes the stream's key frames: both Sim3 tables, the corrected poses and centres, the members in
//                            key order                                                                           (one workgroup per stream)
//   k_correct_loop_points    moves the claimed points, a lane each, and recomputes their normals and ranges, a wavefront each; copies the
//                            others                                                                              (workgroups over stream x points)
// The logic is map_correct_core.h. Shape (DESIGN.md "Map correction"): who corrects a point is the only thing the reference's loop
// order decides, and it is an integer minimum over the members' keypoints, taken with atomics in the first kernel; the second kernel's
// launch is the barrier behind it. Which camera centre an observer contributes to a normal follows from two integers, its key
// position and the claimer's, and is a select. The normal's float sum runs in ascending key of the observers: the lanes of a wavefront
// store their terms at their key positions and three lanes add them up in that order, a coordinate each.
// Below them: the map update after a global bundle adjustment (k_apply_gba_key_frames, k_apply_gba_points).
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "map_correct_core.h"

namespace viorb {

enum { MC_WAVE = 64, MC_THREADS = 256, MC_WAVES = MC_THREADS / MC_WAVE, MC_LDS_KF = 4096, MC_POINT_GROUPS = 64 };

// blockIdx.x = stream. A refused stream gets info = 0 and its status; the point kernel reads info first.
__global__ __launch_bounds__(MC_THREADS) void k_correct_loop_prepare(ClMap M, ClWork W, ClOut R) {
    const int b = blockIdx.x, t = threadIdx.x, nt = MC_THREADS;
    int ok = __syncthreads_and(cl_validate_ranges(M, b, t, nt));
    SnapStream S = {0, 0, 0, 0};
    if (ok) { S = snap_stream(M.kf_start, M.pt_start, b); ok = __syncthreads_and(cl_validate_offsets(M, S, b, t, nt)); }
    if (ok) ok = __syncthreads_and(cl_validate_entries(M, S, t, nt));
    if (ok) {                                                        // plain stores of this workgroup, one CU: a barrier between fill and check
        snap_distinct_fill(M.kf_by_key + S.k0, S.nk, W.key + S.k0, t, nt);
        cl_members_clear(M, S, W, t, nt);
        __syncthreads();
        cl_members_fill(M, S, W, b, t, nt);
        ok = __syncthreads_and(snap_distinct_check(M.kf_by_key + S.k0, S.nk, W.key + S.k0, t, nt));
    }
    if (ok) ok = __syncthreads_and(cl_members_check(M, S, W, b, t, nt));
    if (ok) ok = __syncthreads_and(cl_validate_and_claim(M, S, W, b, t, nt));
    if (t == 0) { W.info[b] = ok; cl_write_status(R, b, ok, ok ? M.conn_start[b + 1] - M.conn_start[b] + 1 : 0); }
    if (!ok) return;                                                 // the whole workgroup
    for (int k = t; k < S.nk; k += nt) cl_key_frame(M, S, W, R, b, k);
    __syncthreads();                                                 // every share has read key[] without the member bit
    cl_mark_members(M, S, W, b, t, nt);
}

// blockIdx.y = stream; the wavefronts of a stream's workgroups stride over its points, 64 at a time.
__global__ __launch_bounds__(MC_THREADS) void k_correct_loop_points(ClMap M, ClWork W, ClOut R) {
    __shared__ int32_t s_key[MC_LDS_KF];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & (MC_WAVE - 1);
    if (!W.info[b]) return;                                          // the whole workgroup
    const SnapStream S = snap_stream(M.kf_start, M.pt_start, b);
    const int32_t* key = W.key + S.k0;
    if (S.nk <= MC_LDS_KF) {
        for (int k = t; k < S.nk; k += MC_THREADS) s_key[k] = key[k];
        key = s_key;
    }
    __syncthreads();
    const int wave = blockIdx.x * MC_WAVES + t / MC_WAVE, n_waves = gridDim.x * MC_WAVES;
    for (int base = wave * MC_WAVE; base < S.np; base += n_waves * MC_WAVE) {
        const int p = base + lane;
        int c = MC_NO_CLAIM;
        float Pn[3] = {0.0f, 0.0f, 0.0f};
        if (p < S.np) c = cl_point_move(M, S, W, R, b, p, Pn);
        unsigned long long m = __ballot(c != MC_NO_CLAIM);
        while (m) {                                                  // the moved points of these 64, the wavefront on one at a time
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const float P[3] = {__shfl(Pn[0], src), __shfl(Pn[1], src), __shfl(Pn[2], src)};
            cl_point_normal(M, S, W, R, key, base + src, __shfl(c, src), P, lane, MC_WAVE);
        }
    }
}

// ---- the map update after a global bundle adjustment ---------------------------------------------------------------------------------------
//   k_apply_gba_key_frames   validates a stream, builds the parent table from the child lists, and a lane per key frame walks up to its
//                            anchor and multiplies back down: TcwGBA, NavStateGBA, the new NavState and pose     (one workgroup per stream)
//   k_apply_gba_points       a lane per point: mPosGBA, or through the reference key frame's old and new pose    (workgroups over stream x points)
__global__ __launch_bounds__(MC_THREADS) void k_apply_gba_key_frames(AgMap M, AgWork W, AgOut R) {
    const int b = blockIdx.x, t = threadIdx.x, nt = MC_THREADS;
    int ok = __syncthreads_and(ag_validate_ranges(M, b, t, nt));
    SnapStream S = {0, 0, 0, 0};
    if (ok) { S = snap_stream(M.kf_start, M.pt_start, b); ok = __syncthreads_and(ag_validate_entries(M, S, b, t, nt)); }
    if (ok) ok = __syncthreads_and(ag_validate_slots(M, S, b, t, nt));
    if (ok) {
        ag_tree_clear(S, W, t, nt);
        __syncthreads();
        ag_tree_fill(M, S, W, b, t, nt);
        __syncthreads();
        ok = __syncthreads_and(ag_tree_check(M, S, W, b, t, nt));
    }
    if (t == 0) { W.info[b] = ok; R.status[b] = ok ? MC_OK : MC_INVALID; }
    if (!ok) return;                                                 // the whole workgroup
    for (int k = t; k < S.nk; k += nt) ag_key_frame(M, S, W, R, k);
}
__global__ __launch_bounds__(MC_THREADS) void k_apply_gba_points(AgMap M, AgWork W, AgOut R) {
    const int b = blockIdx.y;
    if (!W.info[b]) return;
    const SnapStream S = snap_stream(M.kf_start, M.pt_start, b);
    for (int p = blockIdx.x * MC_THREADS + threadIdx.x; p < S.np; p += gridDim.x * MC_THREADS) ag_point(M, S, R, p);
}

} // namespace viorb

using namespace viorb;

namespace {

int mc_point_groups(int batch, int n_pt) { return (int)std::min<long long>((long long)n_pt / batch / MC_THREADS + 1, MC_POINT_GROUPS); }

struct ClLayout { ClWork W; size_t total; };
ClLayout cl_layout(void* base, int batch, int n_kf, int n_pt, int n_obs) {
    ClLayout L; WorkspaceLayout Y(base);
    Y.take(&L.W.key, (size_t)n_kf); Y.take(&L.W.memb, (size_t)n_kf); Y.take(&L.W.claim, (size_t)n_pt); Y.take(&L.W.Ow_in, (size_t)n_kf * 3);
    Y.take(&L.W.Swi, (size_t)n_kf * 8); Y.take(&L.W.terms, (size_t)n_obs * 3); Y.take(&L.W.info, (size_t)batch);
    L.total = Y.end();
    return L;
}

bool cl_sizes_ok(int batch, long long n_kf, long long n_pt, long long n_obs, long long n_conn) {
    return batch >= 1 && batch <= 65535 && n_kf >= 0 && n_pt >= 0 && n_obs >= 0 && n_conn >= 0 && n_kf <= 0x7fffffff / 12 && n_pt <= 0x7fffffff / 8 && n_obs <= 0x7fffffff / 3 &&
           n_conn <= 0x7fffffff - 65535;
}

int cl_check(const viorb_correct_loop_map* m, const viorb_mapping_camera* cam, const viorb_correct_loop_result* r) {
    VIORB_REQUIRE(m && r, "null struct");
    VIORB_REQUIRE(cam && cam->nlevels >= 1 && cam->nlevels <= 16, "camera: nlevels 1..16");
    VIORB_REQUIRE(m->batch >= 1 && m->batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(m->n_kf >= 0 && m->n_kp >= 0 && m->n_pt >= 0 && m->n_obs >= 0 && m->n_conn >= 0, "a negative total");
    VIORB_REQUIRE(cl_sizes_ok(m->batch, m->n_kf, m->n_pt, m->n_obs, m->n_conn), "a total whose rows no int32 indexes");
    VIORB_REQUIRE(m->kf_start && m->kf_by_key && m->kp_start && m->kp_point && m->pt_start && m->pt_bad && m->obs_start && m->obs, "null array");
    VIORB_REQUIRE(m->pose12 && m->pts_f && m->pt_ref && m->pt_corrected_by && m->cur_kf && m->cur_id && m->Scw8 && m->conn_start && m->conn_kf, "null array");
    VIORB_REQUIRE(r->status && r->n_member && r->member_kf && r->Scw_f12 && r->Scw_out && r->Smeas_out && r->pose12_out && r->Ow_out && r->pts_f_out &&
                  r->pt_corrected_by_out && r->pt_corrected_ref_out && r->pt_touched, "null result array");
    return VIORB_OK;
}

ClMap cl_map(const viorb_correct_loop_map& m, const viorb_mapping_camera& cam) {
    ClMap M;
    M.batch = m.batch; M.n_kf = m.n_kf; M.n_kp = m.n_kp; M.n_pt = m.n_pt; M.n_obs = m.n_obs; M.n_conn = m.n_conn;
    M.kf_start = m.kf_start; M.kf_by_key = m.kf_by_key; M.kp_start = m.kp_start; M.kp_point = m.kp_point;
    M.pt_start = m.pt_start; M.pt_bad = m.pt_bad; M.obs_start = m.obs_start; M.obs = m.obs;
    M.pose12 = m.pose12; M.pts_f = m.pts_f; M.pt_ref = m.pt_ref; M.pt_corrected_by = m.pt_corrected_by;
    M.cur_kf = m.cur_kf; M.cur_id = m.cur_id; M.Scw8 = m.Scw8; M.conn_start = m.conn_start; M.conn_kf = m.conn_kf;
    M.nlevels = cam.nlevels;
    for (int i = 0; i < 16; i++) M.sf[i] = cam.scale_factors[i < cam.nlevels ? i : cam.nlevels - 1];
    return M;
}
ClOut cl_out(const viorb_correct_loop_result& r) {
    ClOut R;
    R.status = r.status; R.n_member = r.n_member; R.member_kf = r.member_kf; R.Scw_f12 = r.Scw_f12; R.Scw_out = r.Scw_out; R.Smeas_out = r.Smeas_out;
    R.pose12_out = r.pose12_out; R.Ow_out = r.Ow_out; R.pts_f_out = r.pts_f_out; R.pt_corrected_by_out = r.pt_corrected_by_out;
    R.pt_corrected_ref_out = r.pt_corrected_ref_out; R.pt_touched = r.pt_touched;
    return R;
}

struct AgLayout { AgWork W; size_t total; };
AgLayout ag_layout(void* base, int batch, int n_kf) {
    AgLayout L; WorkspaceLayout Y(base);
    Y.take(&L.W.parent, (size_t)n_kf); Y.take(&L.W.count, (size_t)n_kf); Y.take(&L.W.mark, (size_t)n_kf); Y.take(&L.W.info, (size_t)batch);
    L.total = Y.end();
    return L;
}
bool ag_sizes_ok(int batch, long long n_kf, long long n_pt) { return batch >= 1 && batch <= 65535 && n_kf >= 0 && n_pt >= 0 && n_kf <= 0x7fffffff / 22 && n_pt <= 0x7fffffff / 3; }
int ag_check(const viorb_apply_gba_map* m, const float* Tbc12, const viorb_apply_gba_result* r) {
    VIORB_REQUIRE(m && r && Tbc12, "null struct or Tbc12");
    VIORB_REQUIRE(m->batch >= 1 && m->batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(m->n_kf >= 0 && m->n_child >= 0 && m->n_origin >= 0 && m->n_pt >= 0, "a negative total");
    VIORB_REQUIRE(ag_sizes_ok(m->batch, m->n_kf, m->n_pt), "a total whose rows no int32 indexes");
    VIORB_REQUIRE(mc_finite12(Tbc12), "Tbc12 is not finite");
    VIORB_REQUIRE(m->kf_start && m->child_start && m->child_kf && m->origin_start && m->origin_kf && m->kf_in_gba && m->pose12 && m->TcwGBA12 && m->ns22 && m->nsGBA22, "null array");
    VIORB_REQUIRE(m->pt_start && m->pt_bad && m->pt_in_gba && m->Pw && m->PosGBA && m->pt_ref, "null array");
    VIORB_REQUIRE(r->status && r->pose12_out && r->ns22_out && r->TcwBef_out && r->nsBef_out && r->TcwGBA_out && r->nsGBA_out && r->kf_in_gba_out && r->kf_reached && r->Pw_out && r->pt_code,
                  "null result array");
    return VIORB_OK;
}
AgMap ag_map(const viorb_apply_gba_map& m, const float* Tbc12) {
    AgMap M;
    M.batch = m.batch; M.n_kf = m.n_kf; M.n_child = m.n_child; M.n_origin = m.n_origin; M.n_pt = m.n_pt;
    M.kf_start = m.kf_start; M.child_start = m.child_start; M.child_kf = m.child_kf; M.origin_start = m.origin_start; M.origin_kf = m.origin_kf;
    M.kf_in_gba = m.kf_in_gba; M.pose12 = m.pose12; M.TcwGBA12 = m.TcwGBA12; M.ns22 = m.ns22; M.nsGBA22 = m.nsGBA22;
    M.pt_start = m.pt_start; M.pt_bad = m.pt_bad; M.pt_in_gba = m.pt_in_gba; M.Pw = m.Pw; M.PosGBA = m.PosGBA; M.pt_ref = m.pt_ref;
    for (int i = 0; i < 12; i++) M.Tbc[i] = Tbc12[i];
    return M;
}
AgOut ag_out(const viorb_apply_gba_result& r) {
    AgOut R;
    R.status = r.status; R.pose12_out = r.pose12_out; R.ns22_out = r.ns22_out; R.TcwBef_out = r.TcwBef_out; R.nsBef_out = r.nsBef_out; R.TcwGBA_out = r.TcwGBA_out;
    R.nsGBA_out = r.nsGBA_out; R.kf_in_gba_out = r.kf_in_gba_out; R.kf_reached = r.kf_reached; R.Pw_out = r.Pw_out; R.pt_code = r.pt_code;
    return R;
}

} // namespace

extern "C" {

size_t viorb_apply_global_ba_workspace_bytes(int batch, int n_kf) {
    if (!ag_sizes_ok(batch, n_kf, 0)) return 0;
    return ag_layout(nullptr, batch, n_kf).total;
}

int viorb_apply_global_ba_shape(int32_t* out4) {
    VIORB_REQUIRE(out4, "null array");
    out4[0] = MC_THREADS; out4[1] = MC_THREADS; out4[2] = MC_WAVE; out4[3] = MC_POINT_GROUPS;
    return VIORB_OK;
}

int viorb_apply_global_ba_device(const viorb_apply_gba_map* map, const float* Tbc12, const viorb_apply_gba_result* result, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(ag_check(map, Tbc12, result));
    VIORB_REQUIRE_WORKSPACE(workspace, workspace_bytes, ag_layout(nullptr, map->batch, map->n_kf).total, "viorb_apply_global_ba_workspace_bytes");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const AgMap M = ag_map(*map, Tbc12);
    const AgWork W = ag_layout(workspace, map->batch, map->n_kf).W;
    const AgOut R = ag_out(*result);
    VIORB_LAUNCH(k_apply_gba_key_frames, M.batch, MC_THREADS, 0, st, M, W, R);
    VIORB_LAUNCH(k_apply_gba_points, dim3(mc_point_groups(M.batch, M.n_pt), M.batch), MC_THREADS, 0, st, M, W, R);
    return VIORB_OK;
}

int viorb_apply_global_ba(const viorb_apply_gba_map* map, const float* Tbc12, const viorb_apply_gba_result* result) {
    VIORB_TRY(ag_check(map, Tbc12, result));
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t nb = (size_t)map->batch, nk = (size_t)map->n_kf, nc = (size_t)map->n_child, no = (size_t)map->n_origin, np = (size_t)map->n_pt;
    viorb_apply_gba_map D = *map;
    D.kf_start = B.up(map->kf_start, nb + 1); D.child_start = B.up(map->child_start, nk + 1); D.child_kf = B.up(map->child_kf, nc); D.origin_start = B.up(map->origin_start, nb + 1);
    D.origin_kf = B.up(map->origin_kf, no); D.kf_in_gba = B.up(map->kf_in_gba, nk); D.pose12 = B.up(map->pose12, nk * 12); D.TcwGBA12 = B.up(map->TcwGBA12, nk * 12);
    D.ns22 = B.up(map->ns22, nk * 22); D.nsGBA22 = B.up(map->nsGBA22, nk * 22); D.pt_start = B.up(map->pt_start, nb + 1); D.pt_bad = B.up(map->pt_bad, np);
    D.pt_in_gba = B.up(map->pt_in_gba, np); D.Pw = B.up(map->Pw, np * 3); D.PosGBA = B.up(map->PosGBA, np * 3); D.pt_ref = B.up(map->pt_ref, np);
    viorb_apply_gba_result O;
    O.status = B.zeros<int32_t>(nb); O.pose12_out = B.zeros<float>(nk * 12); O.ns22_out = B.zeros<double>(nk * 22); O.TcwBef_out = B.zeros<float>(nk * 12);
    O.nsBef_out = B.zeros<double>(nk * 22); O.TcwGBA_out = B.zeros<float>(nk * 12); O.nsGBA_out = B.zeros<double>(nk * 22); O.kf_in_gba_out = B.zeros<uint8_t>(nk);
    O.kf_reached = B.zeros<uint8_t>(nk); O.Pw_out = B.zeros<float>(np * 3); O.pt_code = B.zeros<uint8_t>(np);
    const size_t wb = viorb_apply_global_ba_workspace_bytes(map->batch, map->n_kf);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_apply_global_ba_device(&D, Tbc12, &O, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    std::vector<int32_t> status(nb);
    VIORB_TRY(download(status.data(), O.status, nb));
    std::copy(status.begin(), status.end(), result->status);
    std::vector<unsigned char> tmp;
    struct Rows { void* host; const void* dev; const int32_t* start; size_t n, bytes; };
    const Rows rows[] = {{result->pose12_out, O.pose12_out, map->kf_start, nk, 48}, {result->ns22_out, O.ns22_out, map->kf_start, nk, 176}, {result->TcwBef_out, O.TcwBef_out, map->kf_start, nk, 48},
                         {result->nsBef_out, O.nsBef_out, map->kf_start, nk, 176}, {result->TcwGBA_out, O.TcwGBA_out, map->kf_start, nk, 48}, {result->nsGBA_out, O.nsGBA_out, map->kf_start, nk, 176},
                         {result->kf_in_gba_out, O.kf_in_gba_out, map->kf_start, nk, 1}, {result->kf_reached, O.kf_reached, map->kf_start, nk, 1},
                         {result->Pw_out, O.Pw_out, map->pt_start, np, 12}, {result->pt_code, O.pt_code, map->pt_start, np, 1}};
    for (const Rows& r : rows) {
        tmp.resize(r.n * r.bytes);
        VIORB_TRY(download(tmp.data(), static_cast<const unsigned char*>(r.dev), tmp.size()));
        for (size_t b = 0; b < nb; b++) {
            if (status[b] == VIORB_ERR_INVALID_ARG) continue;
            std::copy(tmp.begin() + (size_t)r.start[b] * r.bytes, tmp.begin() + (size_t)r.start[b + 1] * r.bytes, static_cast<unsigned char*>(r.host) + (size_t)r.start[b] * r.bytes);
        }
    }
    return VIORB_OK;
}

int viorb_debug_apply_global_ba_host(const viorb_apply_gba_map* map, const float* Tbc12, const viorb_apply_gba_result* result) {
    VIORB_TRY(ag_check(map, Tbc12, result));
    const size_t nk = (size_t)map->n_kf + 1;
    std::vector<int32_t> parent(nk), count(nk), mark(nk), info(map->batch);
    AgWork W; W.parent = parent.data(); W.count = count.data(); W.mark = mark.data(); W.info = info.data();
    ag_run_host(ag_map(*map, Tbc12), W, ag_out(*result));
    return VIORB_OK;
}

size_t viorb_correct_loop_workspace_bytes(int batch, int n_kf, int n_pt, int n_obs) {
    if (!cl_sizes_ok(batch, n_kf, n_pt, n_obs, 0)) return 0;
    return cl_layout(nullptr, batch, n_kf, n_pt, n_obs).total;
}

int viorb_correct_loop_shape(int32_t* out4) {
    VIORB_REQUIRE(out4, "null array");
    out4[0] = MC_THREADS; out4[1] = MC_THREADS; out4[2] = MC_WAVE; out4[3] = MC_LDS_KF;
    return VIORB_OK;
}

int viorb_correct_loop_device(const viorb_correct_loop_map* map, const viorb_mapping_camera* cam, const viorb_correct_loop_result* result,
                              void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(cl_check(map, cam, result));
    VIORB_REQUIRE_WORKSPACE(workspace, workspace_bytes, cl_layout(nullptr, map->batch, map->n_kf, map->n_pt, map->n_obs).total, "viorb_correct_loop_workspace_bytes");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const ClMap M = cl_map(*map, *cam);
    const ClWork W = cl_layout(workspace, map->batch, map->n_kf, map->n_pt, map->n_obs).W;
    const ClOut R = cl_out(*result);
    VIORB_LAUNCH(k_correct_loop_prepare, M.batch, MC_THREADS, 0, st, M, W, R);
    VIORB_LAUNCH(k_correct_loop_points, dim3(mc_point_groups(M.batch, M.n_pt), M.batch), MC_THREADS, 0, st, M, W, R);
    return VIORB_OK;
}

int viorb_correct_loop(const viorb_correct_loop_map* map, const viorb_mapping_camera* cam, const viorb_correct_loop_result* result) {
    VIORB_TRY(cl_check(map, cam, result));
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t nb = (size_t)map->batch, nk = (size_t)map->n_kf, ni = (size_t)map->n_kp, np = (size_t)map->n_pt, no = (size_t)map->n_obs, nc = (size_t)map->n_conn, nm = nc + nb;
    viorb_correct_loop_map D = *map;
    D.kf_start = B.up(map->kf_start, nb + 1); D.kf_by_key = B.up(map->kf_by_key, nk); D.kp_start = B.up(map->kp_start, nk + 1); D.kp_point = B.up(map->kp_point, ni);
    D.pt_start = B.up(map->pt_start, nb + 1); D.pt_bad = B.up(map->pt_bad, np); D.obs_start = B.up(map->obs_start, np + 1); D.obs = B.up(map->obs, no);
    D.pose12 = B.up(map->pose12, nk * 12); D.pts_f = B.up(map->pts_f, np * 8); D.pt_ref = B.up(map->pt_ref, np); D.pt_corrected_by = B.up(map->pt_corrected_by, np);
    D.cur_kf = B.up(map->cur_kf, nb); D.cur_id = B.up(map->cur_id, nb); D.Scw8 = B.up(map->Scw8, nb * 8);
    D.conn_start = B.up(map->conn_start, nb + 1); D.conn_kf = B.up(map->conn_kf, nc);
    viorb_correct_loop_result O;
    O.status = B.zeros<int32_t>(nb); O.n_member = B.zeros<int32_t>(nb); O.member_kf = B.zeros<int32_t>(nm); O.Scw_f12 = B.zeros<float>(nm * 12);
    O.Scw_out = B.zeros<double>(nk * 8); O.Smeas_out = B.zeros<double>(nk * 8); O.pose12_out = B.zeros<float>(nk * 12); O.Ow_out = B.zeros<float>(nk * 3);
    O.pts_f_out = B.zeros<float>(np * 8); O.pt_corrected_by_out = B.zeros<int32_t>(np); O.pt_corrected_ref_out = B.zeros<int32_t>(np); O.pt_touched = B.zeros<uint8_t>(np);
    const size_t wb = viorb_correct_loop_workspace_bytes(map->batch, map->n_kf, map->n_pt, map->n_obs);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_correct_loop_device(&D, cam, &O, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    // a refused stream writes nothing but its status: its ranges of the caller's arrays stay as they are. The key frames, points and members
    // of an accepted stream lie at kf_start / pt_start / conn_start[b] + b, which the validator keeps apart from every other accepted stream's.
    std::vector<int32_t> status(nb), mstart(nb + 1);
    VIORB_TRY(download(status.data(), O.status, nb));
    std::copy(status.begin(), status.end(), result->status);
    for (size_t b = 0; b <= nb; b++) mstart[b] = map->conn_start[b] + (int32_t)b;
    std::vector<unsigned char> tmp;
    struct Rows { void* host; const void* dev; const int32_t* start; size_t n, bytes; };
    const Rows rows[] = {{result->n_member, O.n_member, nullptr, nb, 4}, {result->member_kf, O.member_kf, mstart.data(), nm, 4}, {result->Scw_f12, O.Scw_f12, mstart.data(), nm, 48},
                         {result->Scw_out, O.Scw_out, map->kf_start, nk, 64}, {result->Smeas_out, O.Smeas_out, map->kf_start, nk, 64},
                         {result->pose12_out, O.pose12_out, map->kf_start, nk, 48}, {result->Ow_out, O.Ow_out, map->kf_start, nk, 12},
                         {result->pts_f_out, O.pts_f_out, map->pt_start, np, 32}, {result->pt_corrected_by_out, O.pt_corrected_by_out, map->pt_start, np, 4},
                         {result->pt_corrected_ref_out, O.pt_corrected_ref_out, map->pt_start, np, 4}, {result->pt_touched, O.pt_touched, map->pt_start, np, 1}};
    for (const Rows& r : rows) {
        tmp.resize(r.n * r.bytes);
        VIORB_TRY(download(tmp.data(), static_cast<const unsigned char*>(r.dev), tmp.size()));
        for (size_t b = 0; b < nb; b++) {
            if (status[b] == VIORB_ERR_INVALID_ARG) continue;
            const size_t i0 = r.start ? (size_t)r.start[b] : b, i1 = r.start ? (size_t)r.start[b + 1] : b + 1;
            std::copy(tmp.begin() + i0 * r.bytes, tmp.begin() + i1 * r.bytes, static_cast<unsigned char*>(r.host) + i0 * r.bytes);
        }
    }
    return VIORB_OK;
}

// ---- host-only test hook: map_correct_core.h compiled for the host -----------------------------------------------------------------------
int viorb_debug_correct_loop_host(const viorb_correct_loop_map* map, const viorb_mapping_camera* cam, const viorb_correct_loop_result* result) {
    VIORB_TRY(cl_check(map, cam, result));
    const size_t nk = (size_t)map->n_kf + 1, np = (size_t)map->n_pt + 1, no = (size_t)map->n_obs + 1;
    std::vector<int32_t> key(nk), memb(nk), claim(np), terms(no * 3), info(map->batch);
    std::vector<float> Ow(nk * 3);
    std::vector<double> Swi(nk * 8);
    ClWork W;
    W.key = key.data(); W.memb = memb.data(); W.claim = claim.data(); W.Ow_in = Ow.data(); W.Swi = Swi.data(); W.terms = terms.data(); W.info = info.data();
    cl_run_host(cl_map(*map, *cam), W, cl_out(*result));
    return VIORB_OK;
}

} // extern "C"
