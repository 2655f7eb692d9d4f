// viorb_amd/csrc/global_ba_se3.hip — Optimizer::GlobalBundleAdjustemnt / Optimizer::BundleAdjustment (reference src/Optimizer.cc:3551-3747,
// BlockSolver_6_3) on the device: every key frame of the map as an SE3 pose (6), marginalised points, one EdgeSE3ProjectXYZ (2 rows) or
// EdgeStereoSE3ProjectXYZ (3 rows) per observation, one optimize(nIterations) of g2o's Levenberg on the Schur complement of the point
// block. The reduced matrix S of order n = 6 * (free key frames) is dense in global memory; its factorisation, the graph bookkeeping
// and the Levenberg control are those of the NavState solve (global_ba.hip, reached through global_ba_dev.h). What is here is the
// arithmetic of 6-dimensional pose blocks with 2- and 3-row edges:
//
//   per iteration   k_gse3_lin_edges (one thread per observation: error rows, Jacobians, robust weight by edge type, W block),
//                   k_gse3_hll (per point: Hll, bl, in edge order), k_gse3_hpp (one workgroup per free key frame over the by-key-frame
//                   edge list: its 6 x 6 block and bp)
//   per trial       Dinv (shared), k_gse3_init_reduced (S = Hpp + lambda I in 6-stride blocks, right-hand side), k_gse3_schur (one
//                   wavefront per point, all pairs of its free observers, FP64 hardware atomics into the lower triangle of S), the shared
//                   Cholesky chain, k_gse3_backsub (point increments), k_gse3_update (SE3Quat::exp(dx) * estimate + the gain ratio's
//                   denominator), k_gse3_errors (robust chi2).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "global_ba_dev.h"
#include "global_ba_se3_core.h"

namespace viorb {

// one workgroup: free ranks; every thread: a stereo edge needs bf > 0
__global__ __launch_bounds__(256) void k_gse3_setup(GbaDev D) {
    const int t = threadIdx.x;
    if (t == 0) {
        int r = 0;
        for (int i = 0; i < D.nk; i++) D.fidx[i] = D.fixed[i] ? -1 : r++;
        D.status[GBA_ST_NFREE] = r;
    }
    bool bad = false;
    for (int k = t; k < D.ne; k += blockDim.x) bad |= !gba_se3_obs_ok(D.e_obs + 4 * (size_t)k, D.cam[4]);
    if (bad) atomicOr(&D.status[GBA_ST_INVALID], GBA_BAD_BF);
}

__global__ __launch_bounds__(256) void k_gse3_errors(GbaDev D) {
    __shared__ double s_red[4];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    double c = 0;
    if (k < D.ne) {
        const double* ob = D.e_obs + 4 * (size_t)k;
        double e[3];
        gba_se3_error(D.kf + (size_t)D.e_idx[2 * k + 1] * 7, D.pt + (size_t)D.e_idx[2 * k] * 3, ob, D.cam, e);
        D.err[3 * (size_t)k] = e[0]; D.err[3 * (size_t)k + 1] = e[1]; D.err[3 * (size_t)k + 2] = e[2];
        double r1;
        ba_robust(D.robust, ob[3] * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]), gba_se3_delta(ob), &c, &r1);
    }
    c = ba_block_sum(c, s_red);
    if (threadIdx.x == 0 && c != 0.0) unsafeAtomicAdd(&D.scal[GBA_S_CHI], c);
}

// err[] is that of the current state (k_gse3_errors ran on it)
__global__ __launch_bounds__(256) void k_gse3_lin_edges(GbaDev D) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.ne) return;
    const double* ob = D.e_obs + 4 * (size_t)k;
    double Jp[9], Jk[18];
    gba_se3_jac(D.kf + (size_t)D.e_idx[2 * k + 1] * 7, D.pt + (size_t)D.e_idx[2 * k] * 3, ob, D.cam, Jp, Jk);
    const double e0 = D.err[3 * (size_t)k], e1 = D.err[3 * (size_t)k + 1], e2 = D.err[3 * (size_t)k + 2];
    double r0, r1;
    ba_robust(D.robust, ob[3] * (e0 * e0 + e1 * e1 + e2 * e2), gba_se3_delta(ob), &r0, &r1);
    const double w = r1 * ob[3];
    D.wgt[k] = w;
    double* Jpo = D.Jp + 9 * (size_t)k; double2* Jko = reinterpret_cast<double2*>(D.Jk + 18 * (size_t)k);
    double2* Wo = reinterpret_cast<double2*>(D.We + 18 * (size_t)k);
#pragma unroll
    for (int a = 0; a < 9; a++) Jpo[a] = Jp[a];
#pragma unroll
    for (int a = 0; a < 9; a++) Jko[a] = make_double2(Jk[2 * a], Jk[2 * a + 1]);
    double We[18];
    ba_w_block<3>(w, Jk, Jp, We);
#pragma unroll
    for (int a = 0; a < 9; a++) Wo[a] = make_double2(We[2 * a], We[2 * a + 1]);
}

__global__ __launch_bounds__(256) void k_gse3_hll(GbaDev D) { gba_hll_body<3>(D); }

// one workgroup per key frame: the 6 x 6 diagonal block (21 sums) and bp (6 sums) of a free one. A thread takes every 256th entry of the
// key frame's edge list (sorted by edge number), so the order of the sums is fixed by the graph.
__global__ __launch_bounds__(256) void k_gse3_hpp(GbaDev D) {
    __shared__ double s_red[4][27];
    const int i = blockIdx.x, t = threadIdx.x, r = D.fidx[i];
    if (r < 0) return;
    double a[27];
#pragma unroll
    for (int k = 0; k < 27; k++) a[k] = 0;
    for (int q = D.kf_start[i] + t; q < D.kf_start[i + 1]; q += blockDim.x) {
        const int k = D.kf_list[q];
        ba_kf_add<3>(a, D.wgt[k], D.Jk + (size_t)18 * k, D.err + 3 * (size_t)k);
    }
    ba_kf_reduce(a, s_red);
    if (t < 36) D.Hd[(size_t)r * 36 + t] = ba_kf_sum(s_red, ba_kf_tri(t / 6, t % 6));
    if (t < 6) D.bp[6 * r + t] = ba_kf_sum(s_red, 21 + t);
}

// S was cleared by a memset; blocks [0, nk): the diagonal block of key frame i; the blocks behind them: right-hand side and the
// identity on the padding
__global__ __launch_bounds__(256) void k_gse3_init_reduced(GbaDev D, double lambda) {
    const int t = threadIdx.x, ld = D.ld;
    if ((int)blockIdx.x < D.nk) {
        const int r = D.fidx[blockIdx.x];
        if (r < 0 || t >= 36) return;
        const int a = t / 6, b = t % 6;
        D.S[(size_t)(6 * r + a) * ld + 6 * r + b] = D.Hd[(size_t)r * 36 + t] + (a == b ? lambda : 0.0);
        return;
    }
    for (int q = (blockIdx.x - D.nk) * blockDim.x + t; q < ld; q += (gridDim.x - D.nk) * blockDim.x) {
        D.rhs[q] = q < D.n ? D.bp[q] : 0.0;
        if (q >= D.n) D.S[(size_t)q * ld + q] = 1.0;
    }
}

__global__ __launch_bounds__(64) void k_gse3_schur(GbaDev D) { gba_schur_body<6>(D); }
__global__ __launch_bounds__(256) void k_gse3_backsub(GbaDev D) { gba_backsub_body<6>(D); }
// oplus of every vertex (VertexSE3Expmap::oplusImpl: SE3Quat::exp(update) * estimate; point += xl) and scale = sum x (lambda x + b)
__global__ __launch_bounds__(256) void k_gse3_update(GbaDev D, double lambda) {
    __shared__ double s_red[4];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    double sc = 0;
    if (D.scal[GBA_S_FAIL] == 0.0) {
        if (q < D.nk && D.fidx[q] >= 0) {
            const double* x = D.xp + 6 * (size_t)D.fidx[q]; const double* b = D.bp + 6 * (size_t)D.fidx[q];
            double* k7 = D.kf + (size_t)q * 7;
            double u[6];
            for (int a = 0; a < 6; a++) { u[a] = x[a]; sc += u[a] * (lambda * u[a] + b[a]); }
            se3_oplus7(k7, u);
        }
        if (q < D.np) for (int a = 0; a < 3; a++) { const double x = D.xl[3 * (size_t)q + a]; sc += x * (lambda * x + D.bl[3 * (size_t)q + a]); D.pt[3 * (size_t)q + a] += x; }
    }
    sc = ba_block_sum(sc, s_red);
    if (threadIdx.x == 0 && sc != 0.0) unsafeAtomicAdd(&D.scal[GBA_S_SCALE], sc);
}

namespace {
int gse3_setup(const GbaDev& D, hipStream_t st) {
    VIORB_LAUNCH(k_gse3_setup, 1, 256, 0, st, D);
    return VIORB_OK;
}
int gse3_errors(const GbaDev& D, hipStream_t st) {
    if (D.ne) VIORB_LAUNCH(k_gse3_errors, gba_blocks(D.ne, 256), 256, 0, st, D);
    return VIORB_OK;
}
int gse3_linearise(const GbaDev& D, hipStream_t st) {
    if (D.ne) VIORB_LAUNCH(k_gse3_lin_edges, gba_blocks(D.ne, 256), 256, 0, st, D);
    if (D.np) VIORB_LAUNCH(k_gse3_hll, gba_blocks(D.np, 256), 256, 0, st, D);
    VIORB_LAUNCH(k_gse3_hpp, D.nk, 256, 0, st, D);
    return VIORB_OK;
}
int gse3_reduce(const GbaDev& D, double lambda, hipStream_t st) {
    VIORB_TRY(gba_point_inverses(D, lambda, st));
    VIORB_LAUNCH(k_gse3_init_reduced, D.nk + gba_blocks(D.ld, 256), 256, 0, st, D, lambda);
    if (D.np && D.ne) VIORB_LAUNCH(k_gse3_schur, D.np, 64, 0, st, D);
    return VIORB_OK;
}
int gse3_step(const GbaDev& D, double lambda, hipStream_t st) {
    if (D.np) VIORB_LAUNCH(k_gse3_backsub, gba_blocks(D.np, 256), 256, 0, st, D);
    VIORB_LAUNCH(k_gse3_update, gba_blocks(std::max(D.nk, D.np), 256), 256, 0, st, D, lambda);
    return VIORB_OK;
}
const GbaOps g_gse3_ops = {GBA_SE3_MAX_FREE_KF, gse3_setup, gse3_errors, gse3_linearise, gse3_reduce, gse3_step, 0.0};

void gse3_shape(GbaDev& D, int nk, int np, int ne) {
    D.nk = nk; D.np = np; D.ne = ne; D.blk = 6; D.kf_w = 7; D.obs_w = 4; D.rows = 3;
    D.nfree = 0; D.n = 0; D.ld = GBA_NB;
}
int gse3_check_pointers(const double* kfs, const uint8_t* fixed, const double* points, int np, const int32_t* edge_idx, const double* edge_obs, int ne,
                        const double* intr5, const double* kfs_out, const double* points_out, const uint8_t* point_included, const double* info) {
    VIORB_REQUIRE(kfs && fixed && intr5 && kfs_out && info, "NULL argument");
    VIORB_REQUIRE((np == 0 || (points && points_out && point_included)) && (ne == 0 || (edge_idx && edge_obs && np > 0)), "NULL point or edge array");
    return VIORB_OK;
}
} // namespace
} // namespace viorb

using namespace viorb;

extern "C" size_t viorb_global_ba_se3_workspace_bytes(int nk, int np, int ne) {
    if (nk < 1 || np < 0 || ne < 0) return 0;
    GbaDev D{};
    gse3_shape(D, nk, np, ne);
    return gba_layout(D, nullptr, std::min(nk, GBA_SE3_MAX_FREE_KF), nullptr);
}

extern "C" int viorb_global_ba_se3_device(const viorb_gba_config* cfg, const double* kfs, int nk, const uint8_t* fixed, const double* points, int np,
                                          const int32_t* edge_idx, const double* edge_obs, int ne, const double intr5[5], const volatile int* stop,
                                          double* kfs_out, double* points_out, uint8_t* point_included, double info[6], void* workspace,
                                          size_t workspace_bytes, void* stream) {
    if (int rc = gba_check_config(cfg, nk, np, ne)) return rc;
    VIORB_TRY(gse3_check_pointers(kfs, fixed, points, np, edge_idx, edge_obs, ne, intr5, kfs_out, points_out, point_included, info));
    VIORB_REQUIRE(workspace != nullptr, "NULL argument");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < 6; k++) info[k] = 0;
    gba_trials().clear();
    VIORB_HIP_TRY(hipMemcpyAsync(kfs_out, kfs, (size_t)nk * 7 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (np) VIORB_HIP_TRY(hipMemcpyAsync(points_out, points, (size_t)np * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    GbaDev D{};
    gse3_shape(D, nk, np, ne); D.robust = cfg->robust;
    D.kf = kfs_out; D.pt = points_out; D.fixed = fixed; D.e_idx = edge_idx; D.e_obs = edge_obs; D.included = point_included;
    for (int k = 0; k < 5; k++) D.cam[k] = intr5[k];
    if (stop && *stop) {                     // the reference's optimize() returns before its first iteration: everything stays
        if (np) VIORB_HIP_TRY(hipMemsetAsync(point_included, 0, np, st));
        VIORB_TRY(gba_mark_included(D, st));
        VIORB_HIP_TRY(hipStreamSynchronize(st));
        return VIORB_OK;
    }
    double* pinned = nullptr;
    VIORB_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&pinned), 16 * sizeof(double)));
    const int rc = gba_run(cfg, D, g_gse3_ops, workspace, workspace_bytes, stop, pinned, info, st);
    const hipError_t e = hipStreamSynchronize(st);
    (void)hipHostFree(pinned);
    if (rc == VIORB_OK && e != hipSuccess) { set_error("global BA: %s", hipGetErrorString(e)); return VIORB_ERR_HIP; }
    return rc;
}

extern "C" int viorb_global_ba_se3(const viorb_gba_config* cfg, const double* kfs, int nk, const uint8_t* fixed, const double* points, int np,
                                   const int32_t* edge_idx, const double* edge_obs, int ne, const double intr5[5], const volatile int* stop,
                                   double* kfs_out, double* points_out, uint8_t* point_included, double info[6]) {
    if (int rc = gba_check_config(cfg, nk, np, ne)) return rc;
    VIORB_TRY(gse3_check_pointers(kfs, fixed, points, np, edge_idx, edge_obs, ne, intr5, kfs_out, points_out, point_included, info));
    // the checks of the device form's setup kernels, on the host and before any GPU call
    int nfree = 0;
    for (int i = 0; i < nk; i++) nfree += fixed[i] ? 0 : 1;
    for (int k = 0; k < ne; k++)
        VIORB_REQUIRE(gba_edge_ok(edge_idx[2 * k], edge_idx[2 * k + 1], k ? edge_idx[2 * k - 2] : 0, np, nk), "edge index out of range or edges not sorted by point");
    for (int k = 0; k < ne; k++) {
        VIORB_REQUIRE(edge_obs[4 * (size_t)k + 3] > 0.0, "edge_obs[k][3] (invSigma2) must be positive");
        VIORB_REQUIRE(gba_se3_obs_ok(edge_obs + 4 * (size_t)k, intr5[4]), "a stereo edge (uRight >= 0) needs bf > 0");
    }
    if (nfree > GBA_SE3_MAX_FREE_KF) { set_error("global BA: %d free key frames, at most %d", nfree, GBA_SE3_MAX_FREE_KF); return VIORB_ERR_CAPACITY; }
    for (int k = 0; k < 6; k++) info[k] = 0;
    gba_trials().clear();
    if (stop && *stop) {
        memcpy(kfs_out, kfs, (size_t)nk * 7 * sizeof(double));
        if (np) { memcpy(points_out, points, (size_t)np * 3 * sizeof(double)); memset(point_included, 0, np); }
        for (int k = 0; k < ne; k++) point_included[edge_idx[2 * k]] = 1;
        return VIORB_OK;
    }
    VIORB_TRY(require_device());
    GbaArena lease;
    if (!lease.ready()) { set_error("global BA: no stream"); return VIORB_ERR_HIP; }
    hipStream_t st = lease.c->st;
    // arena = inputs | states | workspace
    GbaDev D{};
    WorkspaceLayout in(nullptr);
    double *d_kf, *d_pt, *d_obs; int32_t* d_eidx; uint8_t *d_fixed, *d_inc;
    auto lay = [&](WorkspaceLayout& L) {
        L.take(&d_kf, (size_t)nk * 7); L.take(&d_pt, (size_t)np * 3); L.take(&d_obs, (size_t)ne * 4);
        L.take(&d_eidx, (size_t)ne * 2); L.take(&d_fixed, nk); L.take(&d_inc, np);
        L.take(static_cast<double**>(nullptr), 0);
    };
    lay(in);
    const size_t in_bytes = in.end();
    gse3_shape(D, nk, np, ne); D.robust = cfg->robust;
    const size_t ws_bytes = gba_layout(D, nullptr, nfree, nullptr);
    if (!lease.reserve(in_bytes + ws_bytes)) { set_error("global BA: hipMalloc of %zu bytes failed", in_bytes + ws_bytes); return VIORB_ERR_HIP; }
    WorkspaceLayout at(lease.c->arena);
    lay(at);
    void* ws = static_cast<uint8_t*>(lease.c->arena) + in_bytes;
    VIORB_HIP_TRY(hipMemcpyAsync(d_kf, kfs, (size_t)nk * 7 * sizeof(double), hipMemcpyHostToDevice, st));
    VIORB_HIP_TRY(hipMemcpyAsync(d_fixed, fixed, (size_t)nk, hipMemcpyHostToDevice, st));
    if (np) VIORB_HIP_TRY(hipMemcpyAsync(d_pt, points, (size_t)np * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (ne) {
        VIORB_HIP_TRY(hipMemcpyAsync(d_eidx, edge_idx, (size_t)ne * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
        VIORB_HIP_TRY(hipMemcpyAsync(d_obs, edge_obs, (size_t)ne * 4 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (np) VIORB_HIP_TRY(hipMemsetAsync(d_inc, 0, np, st));
    D.kf = d_kf; D.pt = d_pt; D.fixed = d_fixed; D.e_idx = d_eidx; D.e_obs = d_obs; D.included = d_inc;
    for (int k = 0; k < 5; k++) D.cam[k] = intr5[k];
    const int rc = gba_run(cfg, D, g_gse3_ops, ws, ws_bytes, stop, lease.c->pinned, info, st);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipMemcpyAsync(kfs_out, d_kf, (size_t)nk * 7 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (np) {
        VIORB_HIP_TRY(hipMemcpyAsync(points_out, d_pt, (size_t)np * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        VIORB_HIP_TRY(hipMemcpyAsync(point_included, d_inc, np, hipMemcpyDeviceToHost, st));
    }
    VIORB_HIP_TRY(hipStreamSynchronize(st));
    return VIORB_OK;
}

// Test hook without a device: gba_se3_error and ba_se3_jac (ba_core.h: the window solve's Jacobians too) compiled for the host. One edge's error e3, Jp9 = d e / d point [3][3], Jk18 = d e / d
// (omega, upsilon) [3][6] (third rows zero on a monocular edge); returns the edge's dimension, 2 or 3.
extern "C" int viorb_debug_gba_se3_edge(const double* kf7, const double* pt3, const double* obs4, const double* intr5, double* e3, double* Jp9,
                                        double* Jk18) {
    VIORB_REQUIRE(kf7 && pt3 && obs4 && intr5 && e3 && Jp9 && Jk18, "NULL argument");
    gba_se3_jac(kf7, pt3, obs4, intr5, Jp9, Jk18);
    return gba_se3_error(kf7, pt3, obs4, intr5, e3);
}
