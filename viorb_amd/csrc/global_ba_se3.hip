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
        gba_robust(D.robust, ob[3] * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]), gba_se3_delta(ob), &c, &r1);
    }
    c = gba_block_sum(c, s_red);
    if (threadIdx.x == 0 && c != 0.0) unsafeAtomicAdd(&D.scal[GBA_S_CHI], c);
}

// err[] is that of the current state (k_gse3_errors ran on it); the error computed here with the Jacobians is the same value
__global__ __launch_bounds__(256) void k_gse3_lin_edges(GbaDev D) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.ne) return;
    const double* ob = D.e_obs + 4 * (size_t)k;
    double e[3], Jp[9], Jk[18];
    gba_se3_lin(D.kf + (size_t)D.e_idx[2 * k + 1] * 7, D.pt + (size_t)D.e_idx[2 * k] * 3, ob, D.cam, e, Jp, Jk);
    const double e0 = D.err[3 * (size_t)k], e1 = D.err[3 * (size_t)k + 1], e2 = D.err[3 * (size_t)k + 2];
    double r0, r1;
    gba_robust(D.robust, ob[3] * (e0 * e0 + e1 * e1 + e2 * e2), gba_se3_delta(ob), &r0, &r1);
    const double w = r1 * ob[3];
    D.wgt[k] = w;
    double* Jpo = D.Jp + 9 * (size_t)k; double2* Jko = reinterpret_cast<double2*>(D.Jk + 18 * (size_t)k);
    double2* Wo = reinterpret_cast<double2*>(D.We + 18 * (size_t)k);
#pragma unroll
    for (int a = 0; a < 9; a++) Jpo[a] = Jp[a];
#pragma unroll
    for (int a = 0; a < 9; a++) Jko[a] = make_double2(Jk[2 * a], Jk[2 * a + 1]);
    double We[18];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) We[3 * r + c] = w * (Jk[r] * Jp[c] + Jk[6 + r] * Jp[3 + c] + Jk[12 + r] * Jp[6 + c]);
#pragma unroll
    for (int a = 0; a < 9; a++) Wo[a] = make_double2(We[2 * a], We[2 * a + 1]);
}

__global__ __launch_bounds__(256) void k_gse3_hll(GbaDev D) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.np) return;
    double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    for (int k = D.pt_start[p]; k < D.pt_start[p + 1]; k++) {
        const double* J = D.Jp + 9 * (size_t)k; const double* e = D.err + 3 * (size_t)k;
        const double w = D.wgt[k];
        H[0] += w * (J[0] * J[0] + J[3] * J[3] + J[6] * J[6]); H[1] += w * (J[0] * J[1] + J[3] * J[4] + J[6] * J[7]); H[2] += w * (J[0] * J[2] + J[3] * J[5] + J[6] * J[8]);
        H[3] += w * (J[1] * J[1] + J[4] * J[4] + J[7] * J[7]); H[4] += w * (J[1] * J[2] + J[4] * J[5] + J[7] * J[8]); H[5] += w * (J[2] * J[2] + J[5] * J[5] + J[8] * J[8]);
        for (int a = 0; a < 3; a++) b[a] -= w * (J[a] * e[0] + J[3 + a] * e[1] + J[6 + a] * e[2]);
    }
    double* Ho = D.Hll + (size_t)p * 9;
    Ho[0] = H[0]; Ho[1] = H[1]; Ho[2] = H[2]; Ho[3] = H[1]; Ho[4] = H[3]; Ho[5] = H[4]; Ho[6] = H[2]; Ho[7] = H[4]; Ho[8] = H[5];
    for (int a = 0; a < 3; a++) D.bl[(size_t)p * 3 + a] = b[a];
    D.included[p] = D.pt_start[p + 1] > D.pt_start[p];            // a point without an edge is not a vertex (src/Optimizer.cc:3685-3693)
}

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
        const double* J = D.Jk + (size_t)18 * k; const double w = D.wgt[k];
#pragma unroll
        for (int row = 0; row < 3; row++) {
            const double* Jr = J + 6 * row; const double er = D.err[3 * (size_t)k + row];
            int c = 0;
#pragma unroll
            for (int rr = 0; rr < 6; rr++)
#pragma unroll
                for (int cc = rr; cc < 6; cc++) a[c++] += w * (Jr[rr] * Jr[cc]);
#pragma unroll
            for (int rr = 0; rr < 6; rr++) a[21 + rr] -= w * (Jr[rr] * er);
        }
    }
#pragma unroll
    for (int k = 0; k < 27; k++) {
        double v = a[k];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
        if ((t & 63) == 0) s_red[t >> 6][k] = v;
    }
    __syncthreads();
    if (t < 36) {
        const int rr = t / 6, cc = t % 6, lo = rr < cc ? rr : cc, hi = rr < cc ? cc : rr, k = lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
        D.Hd[(size_t)r * 36 + t] = s_red[0][k] + s_red[1][k] + s_red[2][k] + s_red[3][k];
    }
    if (t < 6) D.bp[6 * r + t] = s_red[0][21 + t] + s_red[1][21 + t] + s_red[2][21 + t] + s_red[3][21 + t];
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

// Schur complement of the point block (block_solver.hpp:381-432): one wavefront per point walks the ordered pairs (a, b) of its
// observers; the pair with rank(a) > rank(b) owns block (a, b) of the lower triangle, a pair on one key frame the lower triangle of its
// diagonal block. S_ab -= W_a Dinv W_b^T, bs_a -= W_a Dinv bl (W = wgt Jk^T Jp, 6 x 3).
__global__ __launch_bounds__(64) void k_gse3_schur(GbaDev D) {
    const int p = blockIdx.x, s = D.pt_start[p], m = D.pt_start[p + 1] - s, ld = D.ld;
    if (m == 0) return;
    double Di[9], db[3];
    for (int a = 0; a < 9; a++) Di[a] = D.Dinv[(size_t)p * 9 + a];
    for (int a = 0; a < 3; a++) db[a] = D.db[(size_t)p * 3 + a];
    for (int q = threadIdx.x; q < m * m; q += 64) {
        const int a = s + q / m, b = s + q % m;
        const int fa = D.fidx[D.e_idx[2 * a + 1]], fb = D.fidx[D.e_idx[2 * b + 1]];
        if (fa < 0 || fb < 0 || fa < fb) continue;
        double Wa[18], Wb[18], BD[18];
#pragma unroll
        for (int k = 0; k < 18; k++) { Wa[k] = D.We[18 * (size_t)a + k]; Wb[k] = D.We[18 * (size_t)b + k]; }
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) BD[3 * r + c] = Wa[3 * r] * Di[c] + Wa[3 * r + 1] * Di[3 + c] + Wa[3 * r + 2] * Di[6 + c];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double* row = D.S + (size_t)(6 * fa + r) * ld + 6 * fb;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                if (fa == fb && c > r) continue;
                unsafeAtomicAdd(&row[c], -(BD[3 * r] * Wb[3 * c] + BD[3 * r + 1] * Wb[3 * c + 1] + BD[3 * r + 2] * Wb[3 * c + 2]));
            }
            if (a == b) unsafeAtomicAdd(&D.rhs[6 * fa + r], -(Wa[3 * r] * db[0] + Wa[3 * r + 1] * db[1] + Wa[3 * r + 2] * db[2]));
        }
    }
}

__global__ __launch_bounds__(256) void k_gse3_backsub(GbaDev D) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.np) return;
    if (D.scal[GBA_S_FAIL] != 0.0) return;
    double cl[3] = {D.bl[3 * (size_t)p], D.bl[3 * (size_t)p + 1], D.bl[3 * (size_t)p + 2]};
    for (int k = D.pt_start[p]; k < D.pt_start[p + 1]; k++) {
        const int r = D.fidx[D.e_idx[2 * k + 1]];
        if (r < 0) continue;
        const double* W = D.We + 18 * (size_t)k; const double* x = D.xp + 6 * (size_t)r;
        for (int c = 0; c < 3; c++) { double s = 0; for (int a = 0; a < 6; a++) s += W[3 * a + c] * x[a]; cl[c] -= s; }
    }
    const double* Di = D.Dinv + (size_t)p * 9;
    for (int a = 0; a < 3; a++) D.xl[3 * (size_t)p + a] = Di[3 * a] * cl[0] + Di[3 * a + 1] * cl[1] + Di[3 * a + 2] * cl[2];
}
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
            gba_st_se3(k7, se3_mul(se3_exp(u), gba_ld_se3(k7)));
        }
        if (q < D.np) for (int a = 0; a < 3; a++) { const double x = D.xl[3 * (size_t)q + a]; sc += x * (lambda * x + D.bl[3 * (size_t)q + a]); D.pt[3 * (size_t)q + a] += x; }
    }
    sc = gba_block_sum(sc, s_red);
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
const GbaOps g_gse3_ops = {GBA_SE3_MAX_FREE_KF, gse3_setup, gse3_errors, gse3_linearise, gse3_reduce, gse3_step};

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

// Test hook without a device: global_ba_se3_core.h compiled for the host. One edge's error e3, Jp9 = d e / d point [3][3], Jk18 = d e / d
// (omega, upsilon) [3][6] (third rows zero on a monocular edge); returns the edge's dimension, 2 or 3.
extern "C" int viorb_debug_gba_se3_edge(const double* kf7, const double* pt3, const double* obs4, const double* intr5, double* e3, double* Jp9,
                                        double* Jk18) {
    VIORB_REQUIRE(kf7 && pt3 && obs4 && intr5 && e3 && Jp9 && Jk18, "NULL argument");
    return gba_se3_lin(kf7, pt3, obs4, intr5, e3, Jp9, Jk18);
}
