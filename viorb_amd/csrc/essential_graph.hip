// viorb_amd/csrc/essential_graph.hip — Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:4313-4587, BlockSolver_7_3) on the
// device: every key frame of the map as a Sim3 (7), one EdgeSim3 per edge of the essential graph, one optimize(nIterations) of g2o's
// Levenberg from lambda = 1e-16, then the write-back of key-frame poses and map points. There are no points in the solve and no Schur
// complement: the system H + lambda I of order n = 7 * (free key frames) is assembled directly, dense in global memory, and factored by
// the blocked Cholesky of the global bundle adjustments; the Levenberg control is theirs too (gba_run through global_ba_dev.h, with
// np = ne = 0 for its own point / observation bookkeeping). What is here is the arithmetic of 7-dimensional blocks with 7-row edges:
//
//   once            k_eg_setup (free ranks, argument checks, the measurement Sji = Sjw * Swi of every edge, vertex degrees),
//                   k_eg_csr_offsets / k_eg_csr_fill / k_eg_csr_sort (the edge ends of every vertex, in edge order)
//   per iteration   k_eg_linearise (16 lanes per edge: 14 columns of g2o's numeric Jacobian, then the 14 x 14 J^T J and J^T e of the edge),
//                   k_eg_hpp (one wavefront per free vertex over its list: the 7 x 7 diagonal block and bp)
//   per trial       k_eg_init_reduced (S = H + lambda I in 7-stride blocks, off-diagonal blocks by FP64 atomics, right-hand side), the
//                   shared Cholesky chain, k_eg_update (Sim3(dx) * estimate + the gain ratio's denominator), k_eg_errors (chi2)
//   after           k_eg_recover ([R | t / s] of every key frame, correctedSwr.map(Srw.map(P)) of every point)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "global_ba_dev.h"
#include "essential_graph_core.h"

namespace viorb {

// the solve's own arrays; GbaDev::ext points at it on the host, the kernels take it by value
struct EgDev {
    int ne, np, fix_scale;
    const double *Scw, *Smeas;          // [nk][8] the inputs (GbaDev::kf is the working copy of Scw)
    const int32_t* e_idx;               // [ne][2] (vertex 0 = i, vertex 1 = j)
    const uint8_t* e_corr;              // [ne]
    const float* pts;                   // [np][3]
    const int32_t* pt_ref;              // [np]
    int *cnt, *start, *tmp, *list;      // [nk] degree / fill cursor, [nk + 1], [2 ne], [2 ne]: entry = 2 * edge + side
    double *meas, *err;                 // [ne][8], [ne][7]
    double *Hii, *Hij, *Hjj, *b;        // [ne][49] Ji^T Ji, Ji^T Jj, Jj^T Jj; [ne][14] Ji^T e, Jj^T e
};

static size_t eg_layout(EgDev& E, void* base, int nk, int ne, size_t* clear_bytes) {
    WorkspaceLayout L(base);
    L.take(&E.cnt, nk);
    if (clear_bytes) *clear_bytes = L.end();
    L.take(&E.start, (size_t)nk + 1); L.take(&E.tmp, 2 * (size_t)ne); L.take(&E.list, 2 * (size_t)ne);
    L.take(&E.meas, 8 * (size_t)ne); L.take(&E.err, 7 * (size_t)ne);
    L.take(&E.Hii, 49 * (size_t)ne); L.take(&E.Hij, 49 * (size_t)ne); L.take(&E.Hjj, 49 * (size_t)ne); L.take(&E.b, 14 * (size_t)ne);
    return L.end();
}

// one lane per vertex, edge and point; lane 0: the free ranks and the gauge
__global__ __launch_bounds__(256) void k_eg_setup(GbaDev D, EgDev E) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q == 0) {
        int r = 0;
        for (int i = 0; i < D.nk; i++) D.fidx[i] = D.fixed[i] ? -1 : r++;
        D.status[GBA_ST_NFREE] = r;
        if (r == D.nk) atomicOr(&D.status[GBA_ST_INVALID], GBA_BAD_EG_GAUGE);
    }
    if (q < D.nk && !(eg_pose_ok(E.Scw + 8 * (size_t)q) && eg_pose_ok(E.Smeas + 8 * (size_t)q))) atomicOr(&D.status[GBA_ST_INVALID], GBA_BAD_EG_POSE);
    if (q < E.np && !(E.pt_ref[q] >= -1 && E.pt_ref[q] < D.nk)) atomicOr(&D.status[GBA_ST_INVALID], GBA_BAD_EG_REF);
    if (q < E.ne) {
        const int i = E.e_idx[2 * q], j = E.e_idx[2 * q + 1];
        if (!eg_edge_ok(i, j, D.nk)) { atomicOr(&D.status[GBA_ST_INVALID], GBA_BAD_EG_EDGE); return; }
        const double* A = E.e_corr[q] ? E.Scw : E.Smeas;
        sim3_st(E.meas + 8 * (size_t)q, eg_measurement(sim3_ld(A + 8 * (size_t)i), sim3_ld(A + 8 * (size_t)j)));
        atomicAdd(&E.cnt[i], 1); atomicAdd(&E.cnt[j], 1);
    }
}
__global__ void k_eg_csr_offsets(GbaDev D, EgDev E) {
    if (threadIdx.x || blockIdx.x) return;
    int s = 0;
    for (int i = 0; i < D.nk; i++) { E.start[i] = s; s += E.cnt[i]; E.cnt[i] = 0; }
    E.start[D.nk] = s;
}
__global__ __launch_bounds__(256) void k_eg_csr_fill(GbaDev D, EgDev E) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= E.ne) return;
    const int i = E.e_idx[2 * k], j = E.e_idx[2 * k + 1];
    if (!eg_edge_ok(i, j, D.nk)) return;                   // flagged by k_eg_setup and not counted there
    E.tmp[E.start[i] + atomicAdd(&E.cnt[i], 1)] = 2 * k;
    E.tmp[E.start[j] + atomicAdd(&E.cnt[j], 1)] = 2 * k + 1;
}
// the fill order depends on the atomics' arrival: rank-sort every vertex's list so that its sums run in edge order
__global__ __launch_bounds__(64) void k_eg_csr_sort(GbaDev D, EgDev E) {
    const int s = E.start[blockIdx.x], m = E.start[blockIdx.x + 1] - s;
    for (int q = threadIdx.x; q < m; q += blockDim.x) {
        const int v = E.tmp[s + q];
        int r = 0;
        for (int j = 0; j < m; j++) r += E.tmp[s + j] < v;
        E.list[s + r] = v;
    }
}

__global__ __launch_bounds__(256) void k_eg_errors(GbaDev D, EgDev E) {
    __shared__ double s_red[4];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    double c = 0;
    if (k < E.ne) {
        double e[7];
        eg_error(sim3_ld(E.meas + 8 * (size_t)k), sim3_ld(D.kf + 8 * (size_t)E.e_idx[2 * k]), sim3_ld(D.kf + 8 * (size_t)E.e_idx[2 * k + 1]), e);
#pragma unroll
        for (int r = 0; r < 7; r++) { E.err[7 * (size_t)k + r] = e[r]; c += e[r] * e[r]; }
    }
    c = ba_block_sum(c, s_red);
    if (threadIdx.x == 0 && c != 0.0) unsafeAtomicAdd(&D.scal[GBA_S_CHI], c);
}

// 16 lanes per edge, 16 edges per workgroup. Lane c < 14 of a group owns column c of [Ji | Jj]: it forms the +delta and -delta estimates
// of its vertex and evaluates the error twice (a fixed vertex has no Jacobian: zeros). The columns meet in LDS; lane c then forms row c
// of the 14 x 14 J^T J (rows 0..6: Hii | Hij, rows 7..13: Hjj) and entry c of J^T e. err[] is that of the current state.
__global__ __launch_bounds__(256) void k_eg_linearise(GbaDev D, EgDev E) {
    __shared__ double sJ[16][14][7];
    const int g = threadIdx.x >> 4, c = threadIdx.x & 15, k = blockIdx.x * 16 + g;
    const bool act = k < E.ne && c < 14;
    double col[7] = {0, 0, 0, 0, 0, 0, 0};
    if (act) {
        const int i = E.e_idx[2 * k], j = E.e_idx[2 * k + 1], side = c >= 7 ? 1 : 0;
        if (D.fidx[side ? j : i] >= 0)
            eg_jac_column(sim3_ld(E.meas + 8 * (size_t)k), sim3_ld(D.kf + 8 * (size_t)i), sim3_ld(D.kf + 8 * (size_t)j), side, c - 7 * side, E.fix_scale != 0, col);
    }
    if (c < 14) {
#pragma unroll
        for (int r = 0; r < 7; r++) sJ[g][c][r] = col[r];
    }
    __syncthreads();
    if (!act) return;
    double bs = 0;
#pragma unroll
    for (int r = 0; r < 7; r++) bs += col[r] * E.err[7 * (size_t)k + r];
    E.b[14 * (size_t)k + c] = bs;
    for (int kk = (c < 7 ? 0 : 7); kk < 14; kk++) {
        double m = 0;
#pragma unroll
        for (int r = 0; r < 7; r++) m += col[r] * sJ[g][kk][r];
        if (c < 7) (kk < 7 ? E.Hii : E.Hij)[49 * (size_t)k + 7 * c + (kk < 7 ? kk : kk - 7)] = m;
        else E.Hjj[49 * (size_t)k + 7 * (c - 7) + (kk - 7)] = m;
    }
}

// one wavefront per vertex: lanes 0..48 the diagonal block, lanes 49..55 bp = -sum J^T e, each over the vertex's list in edge order
__global__ __launch_bounds__(64) void k_eg_hpp(GbaDev D, EgDev E) {
    const int i = blockIdx.x, t = threadIdx.x, r = D.fidx[i];
    if (r < 0 || t >= 56) return;
    double v = 0;
    for (int q = E.start[i]; q < E.start[i + 1]; q++) {
        const int ent = E.list[q], k = ent >> 1, side = ent & 1;
        v += t < 49 ? (side ? E.Hjj : E.Hii)[49 * (size_t)k + t] : E.b[14 * (size_t)k + 7 * side + (t - 49)];
    }
    if (t < 49) D.Hd[49 * (size_t)r + t] = v; else D.bp[7 * (size_t)r + (t - 49)] = -v;
}

// S was cleared by a memset. Blocks [0, nk): the diagonal block of vertex i (identity for a free vertex without an edge, which g2o leaves
// out of the active set); [nk, nk + ne): the block Ji^T Jj of an edge between two free vertices into the lower triangle at (higher
// rank, lower rank), transposed where j has the higher rank, by FP64 atomics since two edges may join one pair; behind them: the
// right-hand side and the identity on the padding.
__global__ __launch_bounds__(64) void k_eg_init_reduced(GbaDev D, EgDev E, double lambda) {
    const int t = threadIdx.x, ld = D.ld, blk = blockIdx.x;
    if (blk < D.nk) {
        const int r = D.fidx[blk];
        if (r < 0 || t >= 49) return;
        const int a = t / 7, b = t % 7;
        const bool lone = E.start[blk + 1] == E.start[blk];
        D.S[(size_t)(7 * r + a) * ld + 7 * r + b] = lone ? (a == b ? 1.0 : 0.0) : D.Hd[49 * (size_t)r + t] + (a == b ? lambda : 0.0);
        return;
    }
    if (blk < D.nk + E.ne) {
        const int k = blk - D.nk, ri = D.fidx[E.e_idx[2 * k]], rj = D.fidx[E.e_idx[2 * k + 1]];
        if (ri < 0 || rj < 0 || t >= 49) return;
        const int a = t / 7, b = t % 7;
        double* dst = ri > rj ? D.S + (size_t)(7 * ri + a) * ld + 7 * rj + b : D.S + (size_t)(7 * rj + b) * ld + 7 * ri + a;
        unsafeAtomicAdd(dst, E.Hij[49 * (size_t)k + t]);
        return;
    }
    const int q = (blk - D.nk - E.ne) * 64 + t;
    if (q >= ld) return;
    D.rhs[q] = q < D.n ? D.bp[q] : 0.0;
    if (q >= D.n) D.S[(size_t)q * ld + q] = 1.0;
}

// oplus of every free vertex that has an edge (VertexSim3Expmap::oplusImpl) and scale = sum x (lambda x + b)
__global__ __launch_bounds__(256) void k_eg_update(GbaDev D, EgDev E, double lambda) {
    __shared__ double s_red[4];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    double sc = 0;
    if (D.scal[GBA_S_FAIL] == 0.0 && q < D.nk && D.fidx[q] >= 0 && E.start[q + 1] > E.start[q]) {
        const double* x = D.xp + 7 * (size_t)D.fidx[q]; const double* b = D.bp + 7 * (size_t)D.fidx[q];
        double u[7];
#pragma unroll
        for (int a = 0; a < 7; a++) { u[a] = x[a]; sc += u[a] * (lambda * u[a] + b[a]); }
        sim3_st(D.kf + 8 * (size_t)q, sim3_oplus(sim3_ld(D.kf + 8 * (size_t)q), u, E.fix_scale != 0));
    }
    sc = ba_block_sum(sc, s_red);
    if (threadIdx.x == 0 && sc != 0.0) unsafeAtomicAdd(&D.scal[GBA_S_SCALE], sc);
}

// one lane per key frame (12 doubles) and per point
__global__ __launch_bounds__(256) void k_eg_recover(GbaDev D, EgDev E, double* Tcw_out, float* points_out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < D.nk) {
        double T[12];
        eg_recover_pose(sim3_ld(D.kf + 8 * (size_t)q), T);
#pragma unroll
        for (int a = 0; a < 12; a++) Tcw_out[12 * (size_t)q + a] = T[a];
    }
    if (q < E.np) {
        const int r = E.pt_ref[q];
        const float* P = E.pts + 3 * (size_t)q; float* O = points_out + 3 * (size_t)q;
        if (r < 0) { O[0] = P[0]; O[1] = P[1]; O[2] = P[2]; }
        else eg_recover_point(sim3_ld(E.Scw + 8 * (size_t)r), sim3_ld(D.kf + 8 * (size_t)r), P, O);
    }
}

namespace {
const EgDev& eg_of(const GbaDev& D) { return *static_cast<const EgDev*>(D.ext); }
int eg_setup(const GbaDev& D, hipStream_t st) {
    const EgDev& E = eg_of(D);
    VIORB_LAUNCH(k_eg_setup, gba_blocks(std::max(D.nk, std::max(E.ne, E.np)), 256), 256, 0, st, D, E);
    VIORB_LAUNCH(k_eg_csr_offsets, 1, 64, 0, st, D, E);
    if (E.ne) VIORB_LAUNCH(k_eg_csr_fill, gba_blocks(E.ne, 256), 256, 0, st, D, E);
    VIORB_LAUNCH(k_eg_csr_sort, D.nk, 64, 0, st, D, E);
    return VIORB_OK;
}
int eg_errors(const GbaDev& D, hipStream_t st) {
    const EgDev& E = eg_of(D);
    if (E.ne) VIORB_LAUNCH(k_eg_errors, gba_blocks(E.ne, 256), 256, 0, st, D, E);
    return VIORB_OK;
}
int eg_linearise(const GbaDev& D, hipStream_t st) {
    const EgDev& E = eg_of(D);
    if (E.ne) VIORB_LAUNCH(k_eg_linearise, gba_blocks(E.ne, 16), 256, 0, st, D, E);
    VIORB_LAUNCH(k_eg_hpp, D.nk, 64, 0, st, D, E);
    return VIORB_OK;
}
int eg_reduce(const GbaDev& D, double lambda, hipStream_t st) {
    const EgDev& E = eg_of(D);
    VIORB_LAUNCH(k_eg_init_reduced, D.nk + E.ne + gba_blocks(D.ld, 64), 64, 0, st, D, E, lambda);
    return VIORB_OK;
}
int eg_step(const GbaDev& D, double lambda, hipStream_t st) {
    VIORB_LAUNCH(k_eg_update, gba_blocks(D.nk, 256), 256, 0, st, D, eg_of(D), lambda);
    return VIORB_OK;
}
// setUserLambdaInit(1e-16) (src/Optimizer.cc:4327)
const GbaOps g_eg_ops = {EG_MAX_FREE_KF, eg_setup, eg_errors, eg_linearise, eg_reduce, eg_step, 1e-16};

void eg_shape(GbaDev& D, int nk) {
    D.nk = nk; D.np = 0; D.ne = 0; D.blk = 7; D.kf_w = 8; D.obs_w = 1; D.rows = 1;
    D.nfree = 0; D.n = 0; D.ld = GBA_NB;
}
int eg_check_args(const viorb_eg_config* cfg, const double* Scw, const double* Smeas, const uint8_t* fixed, int nk, const int32_t* edge_idx,
                  const uint8_t* edge_corrected, int ne, const float* points, const int32_t* point_ref, int np, const double* Scw_out,
                  const double* Tcw_out, const float* points_out, const double* info) {
    VIORB_REQUIRE(cfg != nullptr, "cfg is NULL");
    VIORB_REQUIRE(cfg->iterations >= 0 && (cfg->fix_scale == 0 || cfg->fix_scale == 1), "iterations >= 0, fix_scale 0 or 1");
    VIORB_REQUIRE(nk >= 1 && ne >= 0 && np >= 0, "nk >= 1, ne >= 0, np >= 0");
    VIORB_REQUIRE(Scw && Smeas && fixed && Scw_out && Tcw_out && info, "NULL argument");
    VIORB_REQUIRE((ne == 0 || (edge_idx && edge_corrected)) && (np == 0 || (points && point_ref && points_out)), "NULL edge or point array");
    return VIORB_OK;
}
// the solve and the write-back on device-resident arrays; D.kf = Scw_out already holds Scw
int eg_run(const viorb_eg_config* cfg, GbaDev& D, EgDev& E, int nk, double* Tcw_out, float* points_out, void* workspace, size_t workspace_bytes,
           double* pinned, double info[6], hipStream_t st) {
    size_t clear_bytes = 0;
    const size_t eg_bytes = eg_layout(E, workspace, nk, E.ne, &clear_bytes);
    if (eg_bytes > workspace_bytes) { set_error("essential graph: workspace of %zu bytes, %zu needed", workspace_bytes, eg_bytes); return VIORB_ERR_CAPACITY; }
    VIORB_HIP_TRY(hipMemsetAsync(workspace, 0, clear_bytes, st));
    D.ext = &E;
    const viorb_gba_config gcfg = {cfg->iterations, 0};
    VIORB_TRY(gba_run(&gcfg, D, g_eg_ops, static_cast<uint8_t*>(workspace) + eg_bytes, workspace_bytes - eg_bytes, nullptr, pinned, info, st));
    VIORB_LAUNCH(k_eg_recover, gba_blocks(std::max(nk, E.np), 256), 256, 0, st, D, E, Tcw_out, points_out);
    return VIORB_OK;
}
} // namespace
} // namespace viorb

using namespace viorb;

extern "C" size_t viorb_essential_graph_workspace_bytes(int nk, int ne, int np) {
    if (nk < 1 || ne < 0 || np < 0) return 0;
    GbaDev D{}; EgDev E{};
    eg_shape(D, nk);
    return eg_layout(E, nullptr, nk, ne, nullptr) + gba_layout(D, nullptr, std::min(nk, EG_MAX_FREE_KF), nullptr);
}

extern "C" int viorb_optimize_essential_graph_device(const viorb_eg_config* cfg, const double* Scw, const double* Smeas, const uint8_t* fixed, int nk,
                                                     const int32_t* edge_idx, const uint8_t* edge_corrected, int ne, const float* points,
                                                     const int32_t* point_ref, int np, double* Scw_out, double* Tcw_out, float* points_out,
                                                     double info[6], void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(eg_check_args(cfg, Scw, Smeas, fixed, nk, edge_idx, edge_corrected, ne, points, point_ref, np, Scw_out, Tcw_out, points_out, info));
    VIORB_REQUIRE(workspace != nullptr, "NULL argument");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < 6; k++) info[k] = 0;
    gba_trials().clear();
    VIORB_HIP_TRY(hipMemcpyAsync(Scw_out, Scw, (size_t)nk * 8 * sizeof(double), hipMemcpyDeviceToDevice, st));
    GbaDev D{}; EgDev E{};
    eg_shape(D, nk);
    D.kf = Scw_out; D.fixed = fixed;
    E.ne = ne; E.np = np; E.fix_scale = cfg->fix_scale; E.Scw = Scw; E.Smeas = Smeas; E.e_idx = edge_idx; E.e_corr = edge_corrected; E.pts = points; E.pt_ref = point_ref;
    double* pinned = nullptr;
    VIORB_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&pinned), 16 * sizeof(double)));
    const int rc = eg_run(cfg, D, E, nk, Tcw_out, points_out, workspace, workspace_bytes, pinned, info, st);
    const hipError_t e = hipStreamSynchronize(st);
    (void)hipHostFree(pinned);
    if (rc == VIORB_OK && e != hipSuccess) { set_error("essential graph: %s", hipGetErrorString(e)); return VIORB_ERR_HIP; }
    return rc;
}

extern "C" int viorb_optimize_essential_graph(const viorb_eg_config* cfg, const double* Scw, const double* Smeas, const uint8_t* fixed, int nk,
                                              const int32_t* edge_idx, const uint8_t* edge_corrected, int ne, const float* points,
                                              const int32_t* point_ref, int np, double* Scw_out, double* Tcw_out, float* points_out, double info[6]) {
    VIORB_TRY(eg_check_args(cfg, Scw, Smeas, fixed, nk, edge_idx, edge_corrected, ne, points, point_ref, np, Scw_out, Tcw_out, points_out, info));
    // the checks of the device form's setup kernel, on the host and before any GPU call
    int nfree = 0;
    for (int i = 0; i < nk; i++) {
        nfree += fixed[i] ? 0 : 1;
        VIORB_REQUIRE(eg_pose_ok(Scw + 8 * (size_t)i) && eg_pose_ok(Smeas + 8 * (size_t)i), "a Sim3 pose is not finite or has a scale <= 0");
    }
    VIORB_REQUIRE(nfree < nk, "no fixed vertex: with lambda = 1e-16 nothing holds the gauge");
    for (int k = 0; k < ne; k++) VIORB_REQUIRE(eg_edge_ok(edge_idx[2 * k], edge_idx[2 * k + 1], nk), "edge index out of range or i == j");
    for (int p = 0; p < np; p++) VIORB_REQUIRE(point_ref[p] >= -1 && point_ref[p] < nk, "point_ref outside -1..nk-1");
    if (nfree > EG_MAX_FREE_KF) { set_error("essential graph: %d free key frames, at most %d", nfree, EG_MAX_FREE_KF); return VIORB_ERR_CAPACITY; }
    for (int k = 0; k < 6; k++) info[k] = 0;
    gba_trials().clear();
    VIORB_TRY(require_device());
    GbaArena lease;
    if (!lease.ready()) { set_error("essential graph: no stream"); return VIORB_ERR_HIP; }
    hipStream_t st = lease.c->st;
    // arena = inputs and outputs | workspace
    double *d_scw, *d_smeas, *d_out, *d_tcw; float *d_pts, *d_pout; int32_t *d_eidx, *d_ref; uint8_t *d_fixed, *d_corr;
    auto lay = [&](WorkspaceLayout& L) {
        L.take(&d_scw, (size_t)nk * 8); L.take(&d_smeas, (size_t)nk * 8); L.take(&d_out, (size_t)nk * 8); L.take(&d_tcw, (size_t)nk * 12);
        L.take(&d_pts, (size_t)np * 3); L.take(&d_pout, (size_t)np * 3); L.take(&d_eidx, (size_t)ne * 2); L.take(&d_ref, np);
        L.take(&d_fixed, nk); L.take(&d_corr, ne);
        L.take(static_cast<double**>(nullptr), 0);
    };
    WorkspaceLayout in(nullptr);
    lay(in);
    const size_t in_bytes = in.end();
    GbaDev D{}; EgDev E{};
    eg_shape(D, nk);
    const size_t ws_bytes = eg_layout(E, nullptr, nk, ne, nullptr) + gba_layout(D, nullptr, nfree, nullptr);
    if (!lease.reserve(in_bytes + ws_bytes)) { set_error("essential graph: hipMalloc of %zu bytes failed", in_bytes + ws_bytes); return VIORB_ERR_HIP; }
    WorkspaceLayout at(lease.c->arena);
    lay(at);
    void* ws = static_cast<uint8_t*>(lease.c->arena) + in_bytes;
    VIORB_HIP_TRY(hipMemcpyAsync(d_scw, Scw, (size_t)nk * 8 * sizeof(double), hipMemcpyHostToDevice, st));
    VIORB_HIP_TRY(hipMemcpyAsync(d_out, Scw, (size_t)nk * 8 * sizeof(double), hipMemcpyHostToDevice, st));
    VIORB_HIP_TRY(hipMemcpyAsync(d_smeas, Smeas, (size_t)nk * 8 * sizeof(double), hipMemcpyHostToDevice, st));
    VIORB_HIP_TRY(hipMemcpyAsync(d_fixed, fixed, (size_t)nk, hipMemcpyHostToDevice, st));
    if (ne) {
        VIORB_HIP_TRY(hipMemcpyAsync(d_eidx, edge_idx, (size_t)ne * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
        VIORB_HIP_TRY(hipMemcpyAsync(d_corr, edge_corrected, (size_t)ne, hipMemcpyHostToDevice, st));
    }
    if (np) {
        VIORB_HIP_TRY(hipMemcpyAsync(d_pts, points, (size_t)np * 3 * sizeof(float), hipMemcpyHostToDevice, st));
        VIORB_HIP_TRY(hipMemcpyAsync(d_ref, point_ref, (size_t)np * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    D.kf = d_out; D.fixed = d_fixed;
    E.ne = ne; E.np = np; E.fix_scale = cfg->fix_scale; E.Scw = d_scw; E.Smeas = d_smeas; E.e_idx = d_eidx; E.e_corr = d_corr; E.pts = d_pts; E.pt_ref = d_ref;
    VIORB_TRY(eg_run(cfg, D, E, nk, d_tcw, d_pout, ws, ws_bytes, lease.c->pinned, info, st));
    VIORB_HIP_TRY(hipMemcpyAsync(Scw_out, d_out, (size_t)nk * 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    VIORB_HIP_TRY(hipMemcpyAsync(Tcw_out, d_tcw, (size_t)nk * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (np) VIORB_HIP_TRY(hipMemcpyAsync(points_out, d_pout, (size_t)np * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    VIORB_HIP_TRY(hipStreamSynchronize(st));
    return VIORB_OK;
}

// Test hooks without a device: essential_graph_core.h compiled for the host.
extern "C" int viorb_debug_sim3_log(const double* S8, double* out7) {
    VIORB_REQUIRE(S8 && out7, "NULL argument");
    sim3_log(sim3_ld(S8), out7);
    return VIORB_OK;
}
extern "C" int viorb_debug_essential_graph_edge(const double* Si8, const double* Sj8, const double* C8, int fix_scale, int fixed_i, int fixed_j,
                                                double* e7, double* Ji49, double* Jj49) {
    VIORB_REQUIRE(Si8 && Sj8 && C8 && e7 && Ji49 && Jj49, "NULL argument");
    eg_edge(sim3_ld(Si8), sim3_ld(Sj8), sim3_ld(C8), fix_scale != 0, fixed_i != 0, fixed_j != 0, e7, Ji49, Jj49);
    return VIORB_OK;
}
