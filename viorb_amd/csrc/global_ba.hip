// viorb_amd/csrc/global_ba.hip — Optimizer::GlobalBundleAdjustmentNavState (reference src/Optimizer.cc:50-320) on the device: every key
// frame of the map as a PVR (9) + accelerometer-bias (3) block, marginalised points, one EdgeNavStatePVR + EdgeNavStateBias per key
// frame with a predecessor, one EdgeNavStatePVRPointXYZ per observation, one optimize(nIterations) of g2o's Levenberg on the Schur
// complement of the point block. The window solve of local_ba.hip factors its reduced system inside one workgroup (n_local <= 20);
// here the reduced matrix S of order n = 12 * (free key frames) is dense in global memory and is factored by a chain of launches:
//
//   per iteration   k_gba_lin_edges (one thread per observation: Jacobians, robust weight, W block), k_gba_hll (per point: Hll, bl),
//                   k_gba_hpp (one workgroup per free key frame over the by-key-frame edge list: its 6 x 6 block and bp),
//                   k_gba_imu (one wavefront per IMU / bias factor: 21 x 21 terms into the 12-stride blocks of both key frames)
//   per trial       k_gba_dinv, k_gba_init_reduced (S = Hpp + lambda I as blocks, right-hand side), k_gba_schur (one wavefront per point,
//                   all pairs of its observers, FP64 hardware atomics into the lower triangle of S),
//                   the Cholesky: for every block column kb  k_gba_potrf (64 x 64 tile, one wavefront, vector pipe, LDS) -> k_gba_trsm (panel below it,
//                   one row per lane) -> k_gba_syrk (trailing lower triangle, v_mfma_f64_16x16x4_f64, 64 x 64 tile per workgroup);
//                   the right-hand side rides along as one more row of the panel, so L y = bs is done when the factor is;
//                   k_gba_bwd per block column (L^T x = y), k_gba_backsub (point increments), k_gba_update (retraction + the gain
//                   ratio's denominator), k_gba_errors + k_gba_imu_errors (robust chi2).
// Workgroups never wait on each other inside a kernel; the steps are ordered by the stream. The Levenberg control runs on the host and
// reads 3 doubles per trial (chi2, scale, pivot status). The graph bookkeeping (point and key-frame edge lists, free-key-frame ranks,
// IMU information matrices, argument checks of the device form) is built on the device before the first iteration.
// The graph bookkeeping, k_gba_dinv, k_gba_max_diag, the Cholesky chain and the Levenberg loop (gba_run) also serve the vision-only solve of
// global_ba_se3.hip, which plugs its own launches in through GbaOps (global_ba_dev.h); the sizes that differ between the two come from GbaDev.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "global_ba_dev.h"

namespace viorb {

typedef double gba_v4d __attribute__((ext_vector_type(4)));

// ---- graph bookkeeping ----------------------------------------------------------------------------------------------------------------
// one workgroup: predecessor check, free ranks, information matrices of the IMU factors
__global__ __launch_bounds__(256) void k_gba_setup(GbaDev D) {
    const int t = threadIdx.x;
    if (t == 0) {
        int r = 0;
        for (int i = 0; i < D.nk; i++) D.fidx[i] = D.fixed[i] ? -1 : r++;
        D.status[GBA_ST_NFREE] = r;
    }
    for (int i = t; i < D.nk; i += blockDim.x) {
        D.kf_cur[i] = 0;
        if (!gba_prev_ok(D.prev[i], i)) { atomicOr(&D.status[GBA_ST_INVALID], 1); continue; }
        if (D.prev[i] < 0) continue;
        if (!gba_inverse9(D.preint + (size_t)i * 142 + 60, D.info_pvr + (size_t)i * 81)) atomicOr(&D.status[GBA_ST_INVALID], 4);
    }
}
// one thread per edge: index checks, the by-point offsets, the per-key-frame counts
__global__ __launch_bounds__(256) void k_gba_edges_scan(GbaDev D) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.ne) return;
    const int p = D.e_idx[2 * k], f = D.e_idx[2 * k + 1], before = k ? D.e_idx[2 * k - 2] : 0;
    if (!gba_edge_ok(p, f, before, D.np, D.nk) || before < 0 || before >= D.np) { atomicOr(&D.status[GBA_ST_INVALID], 2); return; }
    if (!(D.e_obs[(size_t)D.obs_w * k + D.obs_w - 1] > 0.0)) atomicOr(&D.status[GBA_ST_INVALID], GBA_BAD_SIGMA);
    for (int q = (k ? before + 1 : 0); q <= p; q++) D.pt_start[q] = k;
    if (k == D.ne - 1) for (int q = p + 1; q <= D.np; q++) D.pt_start[q] = D.ne;
    atomicAdd(&D.kf_cur[f], 1);
}
__global__ void k_gba_kf_offsets(GbaDev D) {
    if (threadIdx.x || blockIdx.x) return;
    int s = 0;
    for (int i = 0; i < D.nk; i++) { D.kf_start[i] = s; s += D.kf_cur[i]; D.kf_cur[i] = 0; }
    D.kf_start[D.nk] = s;
}
__global__ __launch_bounds__(256) void k_gba_kf_fill(GbaDev D) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.ne) return;
    const int f = D.e_idx[2 * k + 1];
    D.kf_tmp[D.kf_start[f] + atomicAdd(&D.kf_cur[f], 1)] = k;
}
// the fill order depends on the atomics' arrival: rank-sort every key frame's list so that its sums run in edge order
__global__ __launch_bounds__(256) void k_gba_kf_sort(GbaDev D) {
    const int s = D.kf_start[blockIdx.x], m = D.kf_start[blockIdx.x + 1] - s;
    for (int q = threadIdx.x; q < m; q += blockDim.x) {
        const int v = D.kf_tmp[s + q];
        int r = 0;
        for (int j = 0; j < m; j++) r += D.kf_tmp[s + j] < v;
        D.kf_list[s + r] = v;
    }
}

// point_included without a solve (a stop flag raised before the call): a point with an edge is a vertex
__global__ __launch_bounds__(256) void k_gba_included(GbaDev D) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < D.ne && D.e_idx[2 * k] >= 0 && D.e_idx[2 * k] < D.np) D.included[D.e_idx[2 * k]] = 1;
}

// ---- errors and linearisation -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gba_errors(GbaDev D) {
    __shared__ double s_red[4];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    double c = 0;
    if (k < D.ne) {
        const cam_t K = ld_cam(D.cam);
        double e[2];
        ba_nav_error(K, ba_nav_geom(K, D.kf + (size_t)D.e_idx[2 * k + 1] * 22, D.pt + (size_t)D.e_idx[2 * k] * 3).Pc, D.e_obs + 3 * (size_t)k, e);
        D.err[2 * k] = e[0]; D.err[2 * k + 1] = e[1];
        double r1;
        ba_robust(D.robust, D.e_obs[3 * (size_t)k + 2] * (e[0] * e[0] + e[1] * e[1]), ba_delta_mono_map(), &c, &r1);
    }
    c = ba_block_sum(c, s_red);
    if (threadIdx.x == 0 && c != 0.0) unsafeAtomicAdd(&D.scal[GBA_S_CHI], c);
}
__global__ __launch_bounds__(256) void k_gba_imu_errors(GbaDev D) {
    __shared__ double s_red[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double c = 0;
    if (i < D.nk && D.prev[i] >= 0) {
        double e[9], rho[2]; d3 eb;
        ba_imu_chi2(D.kf + (size_t)i * 22, D.kf + (size_t)D.prev[i] * 22, D.preint + (size_t)i * 142, D.info_pvr + (size_t)i * 81, ld3(D.gw), GBA_ACC_BIAS_RW2,
                    D.robust, e, &eb, rho);
        c = rho[0]; c += rho[1];
    }
    c = ba_block_sum(c, s_red);
    if (threadIdx.x == 0 && c != 0.0) unsafeAtomicAdd(&D.scal[GBA_S_CHI], c);
}
__global__ __launch_bounds__(256) void k_gba_lin_edges(GbaDev D) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.ne) return;
    const cam_t K = ld_cam(D.cam);
    double Jp[6], Jk[12];
    ba_nav_jac(K, ba_nav_geom(K, D.kf + (size_t)D.e_idx[2 * k + 1] * 22, D.pt + (size_t)D.e_idx[2 * k] * 3), Jp, Jk);
    const double e0 = D.err[2 * k], e1 = D.err[2 * k + 1], is2 = D.e_obs[3 * (size_t)k + 2];
    double r0, r1;
    ba_robust(D.robust, is2 * (e0 * e0 + e1 * e1), ba_delta_mono_map(), &r0, &r1);
    const double w = r1 * is2;
    D.wgt[k] = w;
    double2* Jpo = reinterpret_cast<double2*>(D.Jp + 6 * (size_t)k); double2* Jko = reinterpret_cast<double2*>(D.Jk + 12 * (size_t)k);
    double2* Wo = reinterpret_cast<double2*>(D.We + 18 * (size_t)k);
#pragma unroll
    for (int a = 0; a < 3; a++) Jpo[a] = make_double2(Jp[2 * a], Jp[2 * a + 1]);
#pragma unroll
    for (int a = 0; a < 6; a++) Jko[a] = make_double2(Jk[2 * a], Jk[2 * a + 1]);
    double We[18];
    ba_w_block<2>(w, Jk, Jp, We);
#pragma unroll
    for (int a = 0; a < 9; a++) Wo[a] = make_double2(We[2 * a], We[2 * a + 1]);
}
__global__ __launch_bounds__(256) void k_gba_hll(GbaDev D) { gba_hll_body<2>(D); }
// one workgroup per key frame: writes the whole 12 x 12 diagonal block and bp of a free one (the IMU kernel adds to them afterwards) and
// clears its predecessor block
__global__ __launch_bounds__(256) void k_gba_hpp(GbaDev D) {
    __shared__ double s_red[4][27];
    const int i = blockIdx.x, t = threadIdx.x, r = D.fidx[i];
    if (t < 144) D.Ho[(size_t)i * 144 + t] = 0.0;
    if (r < 0) return;
    double a[27];
#pragma unroll
    for (int k = 0; k < 27; k++) a[k] = 0;
    for (int q = D.kf_start[i] + t; q < D.kf_start[i + 1]; q += blockDim.x) {
        const int k = D.kf_list[q];
        ba_kf_add<2>(a, D.wgt[k], D.Jk + (size_t)12 * k, D.err + 2 * k);
    }
    ba_kf_reduce(a, s_red);
    if (t < 144) {
        const int rr = t / 12, cc = t % 12;
        // index of (min, max) in the packed upper triangle of the 6 x 6 block, for the coordinates an observation touches
        const int a6 = rr < 3 ? rr : (rr >= 6 && rr < 9 ? rr - 3 : -1), b6 = cc < 3 ? cc : (cc >= 6 && cc < 9 ? cc - 3 : -1);
        D.Hd[(size_t)r * 144 + t] = a6 >= 0 && b6 >= 0 ? ba_kf_sum(s_red, ba_kf_tri(a6, b6)) : 0.0;
    }
    if (t < 12) {
        const int a6 = t < 3 ? t : (t >= 6 && t < 9 ? t - 3 : -1);
        D.bp[12 * r + t] = a6 >= 0 ? ba_kf_sum(s_red, 21 + a6) : 0.0;
    }
}
// one wavefront per key frame i with a predecessor j: EdgeNavStatePVR on (PVR j, PVR i, bias j) and EdgeNavStateBias on (bias j, bias i).
// Column c of the 9 x 21 Jacobian belongs to key frame j (0..8 -> 0..8, 18..20 -> 9..11) or i (9..17 -> 0..8); a fixed key frame's columns drop out.
__global__ __launch_bounds__(64) void k_gba_imu(GbaDev D) {
    __shared__ double J[9 * 21], OJ[9 * 21], e[9];
    __shared__ double s_w;
    const int i = blockIdx.x, t = threadIdx.x, j = D.prev[i];
    if (j < 0) return;
    const int ri = D.fidx[i], rj = D.fidx[j];
    if (ri < 0 && rj < 0) return;                       // between two fixed key frames: chi2 only
    const double* ki = D.kf + (size_t)i * 22; const double* kj = D.kf + (size_t)j * 22;
    const double* info = D.info_pvr + (size_t)i * 81;
    if (t == 0) {
        d3 eb; double w_pvr, wb;
        ba_imu_weights(ki, kj, D.preint + (size_t)i * 142, info, ld3(D.gw), GBA_ACC_BIAS_RW2, D.robust, e, J, &w_pvr, &eb, &wb);
        s_w = w_pvr;
        const double ev[3] = {eb.x, eb.y, eb.z};
        for (int c = 0; c < 3; c++) {
            const int d = (9 + c) * 12 + 9 + c;
            if (ri >= 0) { unsafeAtomicAdd(&D.Hd[(size_t)ri * 144 + d], wb); unsafeAtomicAdd(&D.bp[12 * ri + 9 + c], -wb * ev[c]); }
            if (rj >= 0) { unsafeAtomicAdd(&D.Hd[(size_t)rj * 144 + d], wb); unsafeAtomicAdd(&D.bp[12 * rj + 9 + c], wb * ev[c]); }
            if (ri >= 0 && rj >= 0) D.Ho[(size_t)i * 144 + d] = -wb;      // this factor is the only writer of block (i, j)
        }
    }
    __syncthreads();
    ba_omega_j(info, J, OJ, t, 64);
    __syncthreads();
    const double w = s_w;
    for (int q = t; q < 441 + 21; q += 64) {
        const int r = q < 441 ? q / 21 : q - 441, c = q < 441 ? q % 21 : 0;
        const bool r_in_i = r >= 9 && r < 18, c_in_i = c >= 9 && c < 18;
        const int lr = r < 9 ? r : (r < 18 ? r - 9 : r - 9), lc = c < 9 ? c : (c < 18 ? c - 9 : c - 9);   // 18..20 -> 9..11 of j
        const int kr = r_in_i ? ri : rj, kc = c_in_i ? ri : rj;
        if (kr < 0) continue;
        if (q >= 441) { double s = 0; for (int k = 0; k < 9; k++) s += OJ[k * 21 + r] * e[k]; unsafeAtomicAdd(&D.bp[12 * kr + lr], -w * s); continue; }
        if (kc < 0) continue;
        double s = 0;
        for (int k = 0; k < 9; k++) s += J[k * 21 + r] * OJ[k * 21 + c];
        if (r_in_i == c_in_i) unsafeAtomicAdd(&D.Hd[(size_t)kr * 144 + lr * 12 + lc], w * s);
        else if (r_in_i) D.Ho[(size_t)i * 144 + lr * 12 + lc] = w * s;      // rows of i, columns of j: below the diagonal of S (prev[i] < i); no bias-bias entry here
    }
}
__global__ __launch_bounds__(256) void k_gba_max_diag(GbaDev D) {
    __shared__ double s_red[4];
    double m = 0;
    const int n = D.n, blk = D.blk;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n + 3 * D.np; q += gridDim.x * blockDim.x)
        m = fmax(m, fabs(q < n ? D.Hd[(size_t)(q / blk) * blk * blk + (q % blk) * (blk + 1)] : D.Hll[(size_t)((q - n) / 3) * 9 + ((q - n) % 3) * 4]));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)          // fmax over non-negative doubles == max over their bit patterns as unsigned integers
        atomicMax(reinterpret_cast<unsigned long long*>(&D.scal[GBA_S_MAXDIAG]), (unsigned long long)__double_as_longlong(fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]))));
}

// ---- one Levenberg trial: reduced system -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gba_dinv(GbaDev D, double lambda) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.np) return;
    double* Di = D.Dinv + (size_t)p * 9;
    if (D.pt_start[p + 1] == D.pt_start[p]) { for (int a = 0; a < 9; a++) Di[a] = 0.0; for (int a = 0; a < 3; a++) D.db[3 * (size_t)p + a] = 0.0; return; }
    ba_point_inverse(D.Hll + (size_t)p * 9, lambda, D.bl + 3 * (size_t)p, Di, D.db + 3 * (size_t)p);
}
// S was cleared by a memset; blocks [0, nk): the blocks of key frame i; the blocks behind them: right-hand side and the identity on the padding
__global__ __launch_bounds__(256) void k_gba_init_reduced(GbaDev D, double lambda) {
    const int t = threadIdx.x, ld = D.ld;
    if ((int)blockIdx.x < D.nk) {
        const int i = blockIdx.x, r = D.fidx[i];
        if (r < 0 || t >= 144) return;
        const int a = t / 12, b = t % 12;
        D.S[(size_t)(12 * r + a) * ld + 12 * r + b] = D.Hd[(size_t)r * 144 + t] + (a == b ? lambda : 0.0);
        const int j = D.prev[i], rj = j >= 0 ? D.fidx[j] : -1;
        if (rj >= 0) D.S[(size_t)(12 * r + a) * ld + 12 * rj + b] = D.Ho[(size_t)i * 144 + t];
        return;
    }
    for (int q = (blockIdx.x - D.nk) * blockDim.x + t; q < ld; q += (gridDim.x - D.nk) * blockDim.x) {
        D.rhs[q] = q < D.n ? D.bp[q] : 0.0;
        if (q >= D.n) D.S[(size_t)q * ld + q] = 1.0;
    }
}
__global__ __launch_bounds__(64) void k_gba_schur(GbaDev D) { gba_schur_body<12>(D); }

// ---- blocked right-looking Cholesky of the lower triangle of S (row-major, leading dimension ld, a multiple of GBA_NB), in place ------
#define GBA_LDS 65        // tile rows in LDS, padded against bank conflicts of column walks
// factor of the diagonal tile kb. A pivot that is not positive and finite fails the trial like the reference's LLT (Eigen info()):
// scal[GBA_S_FAIL] = 1 and every later kernel of the chain returns at once.
__global__ __launch_bounds__(64) void k_gba_potrf(GbaDev D, int kb) {
    __shared__ double s[GBA_NB][GBA_LDS];
    if (D.scal[GBA_S_FAIL] != 0.0) return;
    const int t = threadIdx.x, ld = D.ld;
    double* A = D.S + ((size_t)kb * GBA_NB) * ld + (size_t)kb * GBA_NB;
    for (int q = t; q < GBA_NB * GBA_NB; q += 64) { const int r = q / GBA_NB, c = q % GBA_NB; s[r][c] = c <= r ? A[(size_t)r * ld + c] : 0.0; }
    __syncthreads();
    // left-looking, one row per lane: the dot product of rows r and j is summed from zero (fused) and subtracted once, so that every
    // element is rounded at its own magnitude once per column instead of once per term
    for (int j = 0; j < GBA_NB; j++) {
        double s0 = 0.0, s1 = 0.0;
        if (t >= j) {
            int k = 0;
            for (; k + 1 < j; k += 2) { s0 = fma(s[t][k], s[j][k], s0); s1 = fma(s[t][k + 1], s[j][k + 1], s1); }
            if (k < j) s0 = fma(s[t][k], s[j][k], s0);
        }
        const double v = s[t][j] - (s0 + s1);
        __syncthreads();
        if (t == j) s[j][j] = v;
        __syncthreads();
        const double d = s[j][j];
        if (!(d > 0.0) || !(d < DBL_MAX)) { if (t == 0) D.scal[GBA_S_FAIL] = 1.0; return; }     // the same value in every lane
        const double ljj = sqrt(d);
        __syncthreads();
        if (t == j) s[j][j] = ljj; else if (t > j) s[t][j] = v / ljj;
        __syncthreads();
    }
    for (int q = t; q < GBA_NB * GBA_NB; q += 64) { const int r = q / GBA_NB, c = q % GBA_NB; if (c <= r) A[(size_t)r * ld + c] = s[r][c]; }
}
// panel below the diagonal tile: X L11^T = A21, one row per lane, the row in registers; the last workgroup solves the right-hand side's
// block (L11 y = bs) as one more row
__global__ __launch_bounds__(64) void k_gba_trsm(GbaDev D, int kb, int T) {
    __shared__ double sL[GBA_NB][GBA_LDS], sx[GBA_NB][GBA_LDS];
    if (D.scal[GBA_S_FAIL] != 0.0) return;
    const int t = threadIdx.x, ld = D.ld;
    const bool is_rhs = (int)blockIdx.x == T - kb - 1;
    const double* L = D.S + ((size_t)kb * GBA_NB) * ld + (size_t)kb * GBA_NB;
    double* X = is_rhs ? D.rhs + (size_t)kb * GBA_NB : D.S + ((size_t)(kb + 1 + blockIdx.x) * GBA_NB) * ld + (size_t)kb * GBA_NB;
    const int rows = is_rhs ? 1 : GBA_NB;
    for (int q = t; q < GBA_NB * GBA_NB; q += 64) { const int r = q / GBA_NB, c = q % GBA_NB; sL[r][c] = L[(size_t)r * ld + c]; if (r < rows) sx[r][c] = X[(size_t)r * ld + c]; }
    __syncthreads();
    if (t < rows) {
        double x[GBA_NB];
#pragma unroll
        for (int c = 0; c < GBA_NB; c++) x[c] = sx[t][c];
#pragma unroll
        for (int j = 0; j < GBA_NB; j++) {          // x_j = (a_j - sum_{k<j} x_k L_jk) / L_jj, the sum from zero in four fused chains
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
            for (int k = 0; k < j; k++) {
                if ((k & 3) == 0) s0 = fma(x[k], sL[j][k], s0); else if ((k & 3) == 1) s1 = fma(x[k], sL[j][k], s1);
                else if ((k & 3) == 2) s2 = fma(x[k], sL[j][k], s2); else s3 = fma(x[k], sL[j][k], s3);
            }
            x[j] = (x[j] - ((s0 + s1) + (s2 + s3))) / sL[j][j];
        }
#pragma unroll
        for (int c = 0; c < GBA_NB; c++) sx[t][c] = x[c];
    }
    __syncthreads();
    for (int q = t; q < rows * GBA_NB; q += 64) { const int r = q / GBA_NB, c = q % GBA_NB; X[(size_t)r * ld + c] = sx[r][c]; }
}
// trailing update C_ij -= P_i P_j^T over the tiles i >= j behind block column kb (P = the panel k_gba_trsm left, 64 columns): one 64 x 64
// tile per workgroup, one 32 x 32 quadrant (2 x 2 MFMA tiles) per wave, 16 k-steps of v_mfma_f64_16x16x4_f64 (A[i][k]: lane 16k+i,
// B[k][j] = P_j[j][k]: lane 16k+j, result row = lane/16 + 4*reg, col = lane%16). The panels are staged in LDS, 32 columns per pass, with a row stride of 34
// doubles: the 16 rows x 2 columns a half-wave reads land in 32 different 8-byte slots. blockIdx.y == tiles: the right-hand side's row,
// bs_j -= P_j y (one lane per row).
#define GBA_PK 32         // panel columns staged per pass
#define GBA_PLD 34
__global__ __launch_bounds__(256) void k_gba_syrk(GbaDev D, int kb, int tiles) {
    __shared__ __attribute__((aligned(16))) double sA[GBA_NB][GBA_PLD], sB[GBA_NB][GBA_PLD];
    if (D.scal[GBA_S_FAIL] != 0.0) return;
    const int jj = blockIdx.x, ii = blockIdx.y, t = threadIdx.x, ld = D.ld;
    if (jj > ii) return;
    const size_t k0 = (size_t)kb * GBA_NB, j0 = (size_t)(kb + 1 + jj) * GBA_NB, i0 = (size_t)(kb + 1 + ii) * GBA_NB;
    if (ii == tiles) {
        if (t >= GBA_NB) return;
        const double* P = D.S + (j0 + t) * ld + k0; const double* y = D.rhs + k0;
        double s = 0;
        for (int k = 0; k < GBA_NB; k++) s = fma(P[k], y[k], s);
        D.rhs[j0 + t] -= s;
        return;
    }
    const int w = t >> 6, l = t & 63, wr = w >> 1, wc = w & 1;
    const bool diag = ii == jj;
    // the products are summed from zero and subtracted from the tile once: one rounding at the tile's magnitude per block column
    gba_v4d acc[2][2], cin[2][2];
    const bool active = !(diag && wc > wr);         // the quadrant above the diagonal is never read
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) { acc[a][b][r] = 0.0; cin[a][b][r] = active ? D.S[(i0 + 32 * wr + 16 * a + (l >> 4) + 4 * r) * ld + j0 + 32 * wc + 16 * b + (l & 15)] : 0.0; }
    const double (*pB)[GBA_PLD] = diag ? sA : sB;
    for (int h = 0; h < GBA_NB / GBA_PK; h++) {
        if (h) __syncthreads();
        for (int q = t; q < GBA_NB * GBA_PK / 2; q += 256) {
            const int r = q / (GBA_PK / 2), c = 2 * (q % (GBA_PK / 2));
            *reinterpret_cast<double2*>(&sA[r][c]) = *reinterpret_cast<const double2*>(D.S + (i0 + r) * ld + k0 + h * GBA_PK + c);
            if (!diag) *reinterpret_cast<double2*>(&sB[r][c]) = *reinterpret_cast<const double2*>(D.S + (j0 + r) * ld + k0 + h * GBA_PK + c);
        }
        __syncthreads();
        if (active)
#pragma unroll
            for (int kc = 0; kc < GBA_PK / 4; kc++) {
                const int kk = 4 * kc + (l >> 4);
                const double a0 = sA[32 * wr + (l & 15)][kk], a1 = sA[32 * wr + 16 + (l & 15)][kk];
                const double b0 = pB[32 * wc + (l & 15)][kk], b1 = pB[32 * wc + 16 + (l & 15)][kk];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
    }
    if (!active) return;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) D.S[(i0 + 32 * wr + 16 * a + (l >> 4) + 4 * r) * ld + j0 + 32 * wc + 16 * b + (l & 15)] = cin[a][b][r] - acc[a][b][r];
}
// backward substitution L^T x = y, block column kb (from the last to the first): every workgroup solves the 64 unknowns of the block
// from the finished y_kb (right-looking, in LDS), then takes 256 of the columns to its left: y_c -= sum_r L[kb rows r][c] x_r.
__global__ __launch_bounds__(256) void k_gba_bwd(GbaDev D, int kb) {
    __shared__ double sL[GBA_NB][GBA_LDS], sy[GBA_NB];
    if (D.scal[GBA_S_FAIL] != 0.0) return;
    const int t = threadIdx.x, ld = D.ld;
    const size_t k0 = (size_t)kb * GBA_NB;
    const double* L = D.S + k0 * ld + k0;
    for (int q = t; q < GBA_NB * GBA_NB; q += 256) { const int r = q / GBA_NB, c = q % GBA_NB; sL[r][c] = L[(size_t)r * ld + c]; }
    if (t < GBA_NB) sy[t] = D.rhs[k0 + t];
    __syncthreads();
    for (int j = GBA_NB - 1; j >= 0; j--) {
        if (t == j) sy[j] = sy[j] / sL[j][j];
        __syncthreads();
        if (t < j) sy[t] = fma(-sL[j][t], sy[j], sy[t]);
        __syncthreads();
    }
    if (blockIdx.x == 0 && t < GBA_NB) D.xp[k0 + t] = sy[t];
    const size_t c = (size_t)blockIdx.x * 256 + t;
    if (c >= k0) return;
    double s = 0;
    for (int r = 0; r < GBA_NB; r++) s = fma(D.S[(k0 + r) * ld + c], sy[r], s);
    D.rhs[c] -= s;
}

// ---- increments, retraction, restore ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gba_backsub(GbaDev D) { gba_backsub_body<12>(D); }
// oplus of every vertex (NavState::IncSmallPVR / IncSmallBias, point += xl) and scale = sum x (lambda x + b) of the gain ratio
__global__ __launch_bounds__(256) void k_gba_update(GbaDev D, double lambda) {
    __shared__ double s_red[4];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    double sc = 0;
    if (D.scal[GBA_S_FAIL] == 0.0) {
        if (q < D.nk && D.fidx[q] >= 0) {
            const double* x = D.xp + 12 * (size_t)D.fidx[q]; const double* b = D.bp + 12 * (size_t)D.fidx[q];
            double* ns = D.kf + (size_t)q * 22;
            double u[12];
            for (int a = 0; a < 12; a++) { u[a] = x[a]; sc += u[a] * (lambda * u[a] + b[a]); }
            st_pvr(ns, inc_small_pvr(ld_pvr(ns), u));
            for (int a = 0; a < 3; a++) ns[19 + a] += u[9 + a];
        }
        if (q < D.np) for (int a = 0; a < 3; a++) { const double x = D.xl[3 * (size_t)q + a]; sc += x * (lambda * x + D.bl[3 * (size_t)q + a]); D.pt[3 * (size_t)q + a] += x; }
    }
    sc = ba_block_sum(sc, s_red);
    if (threadIdx.x == 0 && sc != 0.0) unsafeAtomicAdd(&D.scal[GBA_S_SCALE], sc);
}

std::vector<uint8_t>& gba_trials() { thread_local std::vector<uint8_t> t; return t; }

size_t gba_layout(GbaDev& D, void* base, int nfree, size_t* clear_bytes) {
    const int nk = D.nk, np = D.np, ne = D.ne, blk = D.blk, rows = D.rows;
    const bool imu = blk == 12;
    WorkspaceLayout L(base);
    L.take(&D.scal, GBA_S_N); L.take(&D.status, GBA_ST_N);
    L.take(&D.pt_start, (size_t)np + 1); L.take(&D.kf_cur, nk);           // cleared together with scal / status: see gba_run
    if (clear_bytes) *clear_bytes = L.off;
    L.take(&D.kf_bak, (size_t)nk * D.kf_w); L.take(&D.pt_bak, (size_t)np * 3);
    L.take(&D.fidx, nk); L.take(&D.kf_start, (size_t)nk + 1); L.take(&D.kf_tmp, ne); L.take(&D.kf_list, ne);
    L.take(&D.info_pvr, imu ? (size_t)nk * 81 : 0);
    L.take(&D.err, (size_t)ne * rows); L.take(&D.Jp, (size_t)ne * 3 * rows); L.take(&D.Jk, (size_t)ne * 6 * rows); L.take(&D.wgt, ne); L.take(&D.We, (size_t)ne * 18);
    L.take(&D.Hll, (size_t)np * 9); L.take(&D.bl, (size_t)np * 3); L.take(&D.Dinv, (size_t)np * 9); L.take(&D.db, (size_t)np * 3); L.take(&D.xl, (size_t)np * 3);
    L.take(&D.Hd, (size_t)nk * blk * blk); L.take(&D.Ho, imu ? (size_t)nk * 144 : 0); L.take(&D.bp, (size_t)nk * blk);
    L.take(&D.rhs, (size_t)gba_ld(blk * nk)); L.take(&D.xp, (size_t)gba_ld(blk * nk));
    L.take(static_cast<double**>(nullptr), 0);
    const size_t head = L.end();
    if (nfree < 0) return head;
    const size_t ld = gba_ld(blk * nfree);
    D.S = reinterpret_cast<double*>(static_cast<uint8_t*>(base) + head);
    return head + ld * ld * sizeof(double);
}

// the factorisation chain + both substitutions; S and rhs hold the system, xp receives the solution
int gba_factor_solve(const GbaDev& D, hipStream_t st, bool solve) {
    const int T = D.ld / GBA_NB;
    for (int kb = 0; kb < T; kb++) {
        VIORB_LAUNCH(k_gba_potrf, 1, 64, 0, st, D, kb);
        VIORB_LAUNCH(k_gba_trsm, T - kb, 64, 0, st, D, kb, T);
        if (kb + 1 < T) VIORB_LAUNCH(k_gba_syrk, dim3(T - kb - 1, T - kb), 256, 0, st, D, kb, T - kb - 1);
    }
    if (solve) for (int kb = T - 1; kb >= 0; kb--) VIORB_LAUNCH(k_gba_bwd, gba_blocks((size_t)kb * GBA_NB, 256), 256, 0, st, D, kb);
    return VIORB_OK;
}

int gba_point_inverses(const GbaDev& D, double lambda, hipStream_t st) {
    if (D.np) VIORB_LAUNCH(k_gba_dinv, gba_blocks(D.np, 256), 256, 0, st, D, lambda);
    return VIORB_OK;
}
int gba_mark_included(const GbaDev& D, hipStream_t st) {
    if (D.ne) VIORB_LAUNCH(k_gba_included, gba_blocks(D.ne, 256), 256, 0, st, D);
    return VIORB_OK;
}

namespace {
int gba_setup(const GbaDev& D, hipStream_t st) {
    VIORB_LAUNCH(k_gba_setup, 1, 256, 0, st, D);
    return VIORB_OK;
}
int gba_errors(const GbaDev& D, hipStream_t st) {
    if (D.ne) VIORB_LAUNCH(k_gba_errors, gba_blocks(D.ne, 256), 256, 0, st, D);
    VIORB_LAUNCH(k_gba_imu_errors, gba_blocks(D.nk, 256), 256, 0, st, D);
    return VIORB_OK;
}
int gba_linearise(const GbaDev& D, hipStream_t st) {
    if (D.ne) VIORB_LAUNCH(k_gba_lin_edges, gba_blocks(D.ne, 256), 256, 0, st, D);
    if (D.np) VIORB_LAUNCH(k_gba_hll, gba_blocks(D.np, 256), 256, 0, st, D);
    VIORB_LAUNCH(k_gba_hpp, D.nk, 256, 0, st, D);
    VIORB_LAUNCH(k_gba_imu, D.nk, 64, 0, st, D);
    return VIORB_OK;
}
int gba_reduce(const GbaDev& D, double lambda, hipStream_t st) {
    VIORB_TRY(gba_point_inverses(D, lambda, st));
    VIORB_LAUNCH(k_gba_init_reduced, D.nk + gba_blocks(D.ld, 256), 256, 0, st, D, lambda);
    if (D.np && D.ne) VIORB_LAUNCH(k_gba_schur, D.np, 64, 0, st, D);
    return VIORB_OK;
}
int gba_step(const GbaDev& D, double lambda, hipStream_t st) {
    if (D.np) VIORB_LAUNCH(k_gba_backsub, gba_blocks(D.np, 256), 256, 0, st, D);
    VIORB_LAUNCH(k_gba_update, gba_blocks(std::max(D.nk, D.np), 256), 256, 0, st, D, lambda);
    return VIORB_OK;
}
const GbaOps g_gba_navstate_ops = {GBA_MAX_FREE_KF, gba_setup, gba_errors, gba_linearise, gba_reduce, gba_step, 0.0};
void gba_navstate_shape(GbaDev& D, int nk, int np, int ne) { D.nk = nk; D.np = np; D.ne = ne; D.blk = 12; D.kf_w = 22; D.obs_w = 3; D.rows = 2; }
} // namespace

// The solve proper on device-resident inputs. `pinned`: 16 page-locked doubles. kf / pt (the working states) are kfs_out / points_out.
int gba_run(const viorb_gba_config* cfg, GbaDev& D, const GbaOps& ops, void* workspace, size_t workspace_bytes, const volatile int* stop,
            double* pinned, double info[6], hipStream_t st) {
    size_t clear_bytes = 0;
    const size_t head = gba_layout(D, workspace, -1, &clear_bytes);
    if (head > workspace_bytes) { set_error("global BA: workspace of %zu bytes, %zu needed", workspace_bytes, head); return VIORB_ERR_CAPACITY; }
    VIORB_HIP_TRY(hipMemsetAsync(workspace, 0, clear_bytes, st));
    VIORB_TRY(ops.setup(D, st));
    if (D.ne) VIORB_LAUNCH(k_gba_edges_scan, gba_blocks(D.ne, 256), 256, 0, st, D);
    VIORB_HIP_TRY(hipMemcpyAsync(pinned, D.status, GBA_ST_N * sizeof(int), hipMemcpyDeviceToHost, st));
    VIORB_HIP_TRY(hipStreamSynchronize(st));
    const int* hst = reinterpret_cast<const int*>(pinned);
    if (hst[GBA_ST_INVALID]) {
        const int bad = hst[GBA_ST_INVALID];
        set_error("invalid argument: global BA graph (%s%s%s%s%s%s%s%s%s)", (bad & GBA_BAD_PREV) ? " prev[i] >= i" : "", (bad & GBA_BAD_EDGE) ? " edge index out of range or edges not sorted by point" : "",
                  (bad & GBA_BAD_COV) ? " singular pre-integration covariance" : "", (bad & GBA_BAD_SIGMA) ? " invSigma2 <= 0" : "", (bad & GBA_BAD_BF) ? " stereo edge with bf <= 0" : "",
                  (bad & GBA_BAD_EG_EDGE) ? " Sim3 edge index out of range or i == j" : "", (bad & GBA_BAD_EG_POSE) ? " Sim3 pose not finite or scale <= 0" : "",
                  (bad & GBA_BAD_EG_GAUGE) ? " no fixed vertex" : "", (bad & GBA_BAD_EG_REF) ? " point_ref out of range" : "");
        return VIORB_ERR_INVALID_ARG;
    }
    D.nfree = hst[GBA_ST_NFREE]; D.n = D.blk * D.nfree; D.ld = gba_ld(D.n);
    if (D.nfree > ops.max_free) { set_error("global BA: %d free key frames, at most %d", D.nfree, ops.max_free); return VIORB_ERR_CAPACITY; }
    const size_t total = gba_layout(D, workspace, D.nfree, nullptr);
    if (total > workspace_bytes) { set_error("global BA: workspace of %zu bytes, %zu needed", workspace_bytes, total); return VIORB_ERR_CAPACITY; }
    if (D.ne) {
        VIORB_LAUNCH(k_gba_kf_offsets, 1, 64, 0, st, D);
        VIORB_LAUNCH(k_gba_kf_fill, gba_blocks(D.ne, 256), 256, 0, st, D);
        VIORB_LAUNCH(k_gba_kf_sort, D.nk, 256, 0, st, D);
    } else VIORB_HIP_TRY(hipMemsetAsync(D.kf_start, 0, ((size_t)D.nk + 1) * sizeof(int), st));

    auto stopped = [&]() { return stop && *stop; };
    auto read_scal = [&]() -> int {
        VIORB_HIP_TRY(hipMemcpyAsync(pinned, D.scal, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
        VIORB_HIP_TRY(hipStreamSynchronize(st));
        return VIORB_OK;
    };
    const size_t S_bytes = (size_t)D.ld * D.ld * sizeof(double);
    VIORB_TRY(ops.errors(D, st));
    VIORB_TRY(ops.linearise(D, st));
    VIORB_LAUNCH(k_gba_max_diag, gba_blocks((size_t)D.n + 3 * (size_t)D.np, 256 * 8), 256, 0, st, D);
    if (int rc = read_scal()) return rc;
    double cur = pinned[GBA_S_CHI], lambda = ops.lambda_init > 0 ? ops.lambda_init : lm_lambda_init(pinned[GBA_S_MAXDIAG]), ni = 2;
    const double chi_before = cur;
    int its = 0, trials = 0, nfail = 0, nbad = 0;
    gba_trials().clear();
    bool stale = false;
    for (int it = 0; it < cfg->iterations && !stopped(); it++) {
        if (it > 0) {                                      // err[] is that of the accepted trial = the current state
            if (stale) { VIORB_TRY(ops.errors(D, st)); stale = false; }   // unless the last trial was rejected and restored
            VIORB_TRY(ops.linearise(D, st));
        }
        const double ini = cur;
        VIORB_HIP_TRY(hipMemcpyAsync(D.kf_bak, D.kf, (size_t)D.nk * D.kf_w * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (D.np) VIORB_HIP_TRY(hipMemcpyAsync(D.pt_bak, D.pt, (size_t)D.np * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
        double rho = 0; int qmax = 0;
        do {
            VIORB_HIP_TRY(hipMemsetAsync(D.scal, 0, 3 * sizeof(double), st));
            VIORB_HIP_TRY(hipMemsetAsync(D.S, 0, S_bytes, st));
            VIORB_TRY(ops.reduce(D, lambda, st));
            VIORB_TRY(gba_factor_solve(D, st, true));
            VIORB_TRY(ops.step(D, lambda, st));
            VIORB_TRY(ops.errors(D, st));
            if (int rc = read_scal()) return rc;
            const bool ok = pinned[GBA_S_FAIL] == 0.0;
            if (!ok) nfail++;
            const double tmp = lm_trial_chi2(ok, pinned[GBA_S_CHI]);
            rho = lm_rho(cur, tmp, ok ? pinned[GBA_S_SCALE] : 0.0);
            const bool accepted = lm_accepted(rho, tmp);
            if (accepted) { lm_good_step(lambda, ni, lm_cube_pow(2 * rho - 1)); cur = tmp; } else lm_bad_step(lambda, ni);
            stale = !accepted;
            gba_trials().push_back(accepted ? 1 : 0);
            if (!accepted) {
                VIORB_HIP_TRY(hipMemcpyAsync(D.kf, D.kf_bak, (size_t)D.nk * D.kf_w * sizeof(double), hipMemcpyDeviceToDevice, st));
                if (D.np) VIORB_HIP_TRY(hipMemcpyAsync(D.pt, D.pt_bak, (size_t)D.np * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
            }
            qmax++; trials++;
        } while (lm_retry(rho, qmax) && !stopped());
        its++;
        if (lm_iteration_stops(rho, qmax, ini, cur, nbad)) break;
    }
    info[0] = chi_before; info[1] = cur; info[2] = its; info[3] = trials; info[4] = lambda; info[5] = nfail;
    return VIORB_OK;
}

int gba_check_config(const viorb_gba_config* cfg, int nk, int np, int ne) {
    VIORB_REQUIRE(cfg != nullptr, "cfg is NULL");
    VIORB_REQUIRE(cfg->iterations >= 0 && (cfg->robust == 0 || cfg->robust == 1), "iterations >= 0, robust 0 or 1");
    VIORB_REQUIRE(nk >= 1 && np >= 0 && ne >= 0, "nk >= 1, np >= 0, ne >= 0");
    return VIORB_OK;
}
} // namespace viorb

using namespace viorb;

extern "C" size_t viorb_global_ba_navstate_workspace_bytes(int nk, int np, int ne) {
    if (nk < 1 || np < 0 || ne < 0) return 0;
    GbaDev D{};
    gba_navstate_shape(D, nk, np, ne);
    return gba_layout(D, nullptr, std::min(nk, GBA_MAX_FREE_KF), nullptr);
}

extern "C" int viorb_global_ba_navstate_device(const viorb_gba_config* cfg, const double* kfs, int nk, const int32_t* prev, const uint8_t* fixed,
                                               const double* preint, const double* points, int np, const int32_t* edge_idx, const double* edge_obs,
                                               int ne, const double gw[3], const double cam[16], const volatile int* stop, double* kfs_out,
                                               double* points_out, uint8_t* point_included, double info[6], void* workspace,
                                               size_t workspace_bytes, void* stream) {
    if (int rc = gba_check_config(cfg, nk, np, ne)) return rc;
    VIORB_REQUIRE(kfs && prev && fixed && preint && gw && cam && kfs_out && info && workspace, "NULL argument");
    VIORB_REQUIRE((np == 0 || (points && points_out && point_included)) && (ne == 0 || (edge_idx && edge_obs && np > 0)), "NULL point or edge array");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < 6; k++) info[k] = 0;
    gba_trials().clear();
    VIORB_HIP_TRY(hipMemcpyAsync(kfs_out, kfs, (size_t)nk * 22 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (np) VIORB_HIP_TRY(hipMemcpyAsync(points_out, points, (size_t)np * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    GbaDev D{};
    gba_navstate_shape(D, nk, np, ne); D.nfree = 0; D.n = 0; D.ld = GBA_NB; D.robust = cfg->robust;
    D.kf = kfs_out; D.pt = points_out; D.prev = prev; D.fixed = fixed; D.e_idx = edge_idx; D.e_obs = edge_obs; D.preint = preint; D.included = point_included;
    for (int k = 0; k < 16; k++) D.cam[k] = cam[k];
    for (int k = 0; k < 3; k++) D.gw[k] = gw[k];
    if (stop && *stop) {                     // the reference's optimize() returns before its first iteration: everything stays
        if (np) VIORB_HIP_TRY(hipMemsetAsync(point_included, 0, np, st));
        VIORB_TRY(gba_mark_included(D, st));
        VIORB_HIP_TRY(hipStreamSynchronize(st));
        return VIORB_OK;
    }
    double* pinned = nullptr;
    VIORB_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&pinned), 16 * sizeof(double)));
    const int rc = gba_run(cfg, D, g_gba_navstate_ops, workspace, workspace_bytes, stop, pinned, info, st);
    const hipError_t e = hipStreamSynchronize(st);
    (void)hipHostFree(pinned);
    if (rc == VIORB_OK && e != hipSuccess) { set_error("global BA: %s", hipGetErrorString(e)); return VIORB_ERR_HIP; }
    return rc;
}

extern "C" int viorb_global_ba_navstate(const viorb_gba_config* cfg, const double* kfs, int nk, const int32_t* prev, const uint8_t* fixed,
                                        const double* preint, const double* points, int np, const int32_t* edge_idx, const double* edge_obs, int ne,
                                        const double gw[3], const double cam[16], const volatile int* stop, double* kfs_out, double* points_out,
                                        uint8_t* point_included, double info[6]) {
    if (int rc = gba_check_config(cfg, nk, np, ne)) return rc;
    VIORB_REQUIRE(kfs && prev && fixed && preint && gw && cam && kfs_out && info, "NULL argument");
    VIORB_REQUIRE((np == 0 || (points && points_out && point_included)) && (ne == 0 || (edge_idx && edge_obs && np > 0)), "NULL point or edge array");
    // the checks of the device form's setup kernels, on the host and before any GPU call
    int nfree = 0;
    for (int i = 0; i < nk; i++) { VIORB_REQUIRE(gba_prev_ok(prev[i], i), "prev[i] must be -1 or an earlier key frame (prev[i] < i)"); nfree += fixed[i] ? 0 : 1; }
    for (int k = 0; k < ne; k++)
        VIORB_REQUIRE(gba_edge_ok(edge_idx[2 * k], edge_idx[2 * k + 1], k ? edge_idx[2 * k - 2] : 0, np, nk), "edge index out of range or edges not sorted by point");
    for (int k = 0; k < ne; k++) VIORB_REQUIRE(edge_obs[3 * k + 2] > 0.0, "edge_obs[k][2] (invSigma2) must be positive; a stereo observation cannot be expressed");
    for (int i = 0; i < nk; i++) if (prev[i] >= 0) { double inv[81]; VIORB_REQUIRE(gba_inverse9(preint + (size_t)i * 142 + 60, inv), "singular pre-integration covariance"); }
    if (nfree > GBA_MAX_FREE_KF) { set_error("global BA: %d free key frames, at most %d", nfree, GBA_MAX_FREE_KF); return VIORB_ERR_CAPACITY; }
    for (int k = 0; k < 6; k++) info[k] = 0;
    gba_trials().clear();
    if (stop && *stop) {
        memcpy(kfs_out, kfs, (size_t)nk * 22 * sizeof(double));
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
    double *d_kf, *d_pt, *d_preint, *d_obs; int32_t *d_prev, *d_eidx; uint8_t *d_fixed, *d_inc;
    auto lay = [&](WorkspaceLayout& L) {
        L.take(&d_kf, (size_t)nk * 22); L.take(&d_pt, (size_t)np * 3); L.take(&d_preint, (size_t)nk * 142); L.take(&d_obs, (size_t)ne * 3);
        L.take(&d_prev, nk); L.take(&d_eidx, (size_t)ne * 2); L.take(&d_fixed, nk); L.take(&d_inc, np);
        L.take(static_cast<double**>(nullptr), 0);
    };
    lay(in);
    const size_t in_bytes = in.end();
    gba_navstate_shape(D, nk, np, ne);
    const size_t ws_bytes = gba_layout(D, nullptr, nfree, nullptr);
    if (!lease.reserve(in_bytes + ws_bytes)) { set_error("global BA: hipMalloc of %zu bytes failed", in_bytes + ws_bytes); return VIORB_ERR_HIP; }
    WorkspaceLayout at(lease.c->arena);
    lay(at);
    void* ws = static_cast<uint8_t*>(lease.c->arena) + in_bytes;
    VIORB_HIP_TRY(hipMemcpyAsync(d_kf, kfs, (size_t)nk * 22 * sizeof(double), hipMemcpyHostToDevice, st));
    VIORB_HIP_TRY(hipMemcpyAsync(d_preint, preint, (size_t)nk * 142 * sizeof(double), hipMemcpyHostToDevice, st));
    VIORB_HIP_TRY(hipMemcpyAsync(d_prev, prev, (size_t)nk * sizeof(int32_t), hipMemcpyHostToDevice, st));
    VIORB_HIP_TRY(hipMemcpyAsync(d_fixed, fixed, (size_t)nk, hipMemcpyHostToDevice, st));
    if (np) VIORB_HIP_TRY(hipMemcpyAsync(d_pt, points, (size_t)np * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (ne) {
        VIORB_HIP_TRY(hipMemcpyAsync(d_eidx, edge_idx, (size_t)ne * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
        VIORB_HIP_TRY(hipMemcpyAsync(d_obs, edge_obs, (size_t)ne * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (np) VIORB_HIP_TRY(hipMemsetAsync(d_inc, 0, np, st));
    gba_navstate_shape(D, nk, np, ne); D.nfree = 0; D.n = 0; D.ld = GBA_NB; D.robust = cfg->robust;
    D.kf = d_kf; D.pt = d_pt; D.prev = d_prev; D.fixed = d_fixed; D.e_idx = d_eidx; D.e_obs = d_obs; D.preint = d_preint; D.included = d_inc;
    for (int k = 0; k < 16; k++) D.cam[k] = cam[k];
    for (int k = 0; k < 3; k++) D.gw[k] = gw[k];
    const int rc = gba_run(cfg, D, g_gba_navstate_ops, ws, ws_bytes, stop, lease.c->pinned, info, st);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipMemcpyAsync(kfs_out, d_kf, (size_t)nk * 22 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (np) {
        VIORB_HIP_TRY(hipMemcpyAsync(points_out, d_pt, (size_t)np * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        VIORB_HIP_TRY(hipMemcpyAsync(point_included, d_inc, np, hipMemcpyDeviceToHost, st));
    }
    VIORB_HIP_TRY(hipStreamSynchronize(st));
    return VIORB_OK;
}

// Test hook: the blocked Cholesky alone. A [n][n] row-major symmetric (the lower triangle is read), L [n][n] receives the factor (upper
// triangle zero); *ok = 0 when a pivot was not positive and finite (L is then left untouched).
extern "C" int viorb_debug_gba_cholesky(const double* A, int n, double* L, int32_t* ok) {
    VIORB_REQUIRE(A && L && ok && n >= 1 && n <= 12 * GBA_MAX_FREE_KF, "A, L, ok; 1 <= n <= 24576");
    VIORB_TRY(require_device());
    GbaArena lease;
    if (!lease.ready()) { set_error("global BA: no stream"); return VIORB_ERR_HIP; }
    hipStream_t st = lease.c->st;
    const size_t ld = gba_ld(n), S_bytes = ld * ld * sizeof(double);
    if (!lease.reserve(S_bytes + ld * sizeof(double) + 256)) { set_error("global BA: hipMalloc of %zu bytes failed", S_bytes); return VIORB_ERR_HIP; }
    GbaDev D{};
    D.n = n; D.ld = (int)ld; D.S = static_cast<double*>(lease.c->arena); D.rhs = D.S + ld * ld; D.scal = D.rhs + ld; D.xp = nullptr;
    VIORB_HIP_TRY(hipMemsetAsync(D.S, 0, S_bytes + ld * sizeof(double) + GBA_S_N * sizeof(double), st));
    VIORB_HIP_TRY(hipMemcpy2DAsync(D.S, ld * sizeof(double), A, (size_t)n * sizeof(double), (size_t)n * sizeof(double), n, hipMemcpyHostToDevice, st));
    std::vector<double> ones(ld - n, 1.0);
    if (ld > (size_t)n) VIORB_HIP_TRY(hipMemcpy2DAsync(D.S + (size_t)n * ld + n, (ld + 1) * sizeof(double), ones.data(), sizeof(double), sizeof(double), ld - n, hipMemcpyHostToDevice, st));
    VIORB_TRY(gba_factor_solve(D, st, false));
    VIORB_HIP_TRY(hipMemcpyAsync(lease.c->pinned, D.scal, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    VIORB_HIP_TRY(hipStreamSynchronize(st));
    *ok = lease.c->pinned[GBA_S_FAIL] == 0.0;
    if (!*ok) return VIORB_OK;
    VIORB_HIP_TRY(hipMemcpy2D(L, (size_t)n * sizeof(double), D.S, ld * sizeof(double), (size_t)n * sizeof(double), n, hipMemcpyDeviceToHost));
    for (int r = 0; r < n; r++) for (int c = r + 1; c < n; c++) L[(size_t)r * n + c] = 0.0;
    return VIORB_OK;
}

// Test hook: accept (1) / reject (0) of the trials of the calling thread's last viorb_global_ba_navstate[_device] call, in order; *n = their
// number (at most cap are written).
extern "C" int viorb_debug_gba_last_trials(uint8_t* accepted, int cap, int* n) {
    VIORB_REQUIRE(n && cap >= 0 && (cap == 0 || accepted), "accepted[cap], n");
    *n = (int)gba_trials().size();
    for (int k = 0; k < *n && k < cap; k++) accepted[k] = gba_trials()[k];
    return VIORB_OK;
}
