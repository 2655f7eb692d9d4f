// viorb_amd/csrc/local_ba.hip — Optimizer::LocalBundleAdjustmentNavState (reference src/Optimizer.cc:1690-2241) on the GPU.
//
// Graph: W local key frames with free PVR(9)+Bias(3) vertices, fixed key frames, marginalised 3-D points, one IMU factor
// (src/IMU/g2otypes.cpp:8-229, information = cov^-1, not inflated: Optimizer.cc:1901-1902) and one bias factor per local
// key frame, one EdgeNavStatePVRPointXYZ (src/IMU/g2otypes.h:129-203, g2otypes.cpp:299-354) per observation.
// Solver: g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:61-189) with the Schur complement of the point
// block (block_solver.hpp:367-486), 5 + 10 iterations with the chi2 / depth gate in between.
//
// Device code (all FP64), as bodies that the single window's launches (k_ba_*) and the lock-step batch's (k_bab_*) share: errors (per
// edge residuals + robust chi2), the linearisation (one thread per edge, or per point: Jacobians, weights, W blocks, Hll, bl), hpp (one
// workgroup per local key frame: its 6x6 (P,Phi) block), imu (one workgroup per IMU factor), dinv (one thread per point:
// (Hll + lambda I)^-1), schur (one wavefront per key-frame pair: its 6x6 block of -W D^-1 W^T gathered over the points both key frames
// observe, no atomics), chol_solve (dense Cholesky of the <= 240x240 reduced system by one 512-thread workgroup, register tiles +
// v_mfma_f64_16x16x4), backsub8_update. The LM control flow (accept / reject, restore and retry, lambda schedule, stop rules, the phase
// change) runs on the device, in the window's control block (lba_ctl.h); the host reads the block once per chunk of trials / few rounds.
#include <hip/hip_runtime.h>
#include <memory>
#include <string>
#include <atomic>
#include <thread>
#include <vector>
#include <algorithm>
#include <cmath>
#include "viorb_common.h"
#include "ba_core.h"
#include "lba_ctl.h"

namespace viorb {

struct BaDev {
    int W, NK, NP, NE, np, ld, prev_kf;
    int pose_dim, rows, kf_stride;  // unknowns per key frame (12: PVR+bias, 6: SE3), residual rows per edge (2, or 3 with stereo), doubles per key-frame state
    // layouts as NavState window / SE3 window where they differ (kf_stride 22 / 7, rows 2 / 3)
    double *kf, *kf_bak;            // [NK][22] navstate / [NK][7] qx qy qz qw tx ty tz of Tcw
    double *pt, *pt_bak;            // [NP][3]
    const int *e_pt, *e_kf;         // [NE]
    const double *e_obs;            // [NE][3] u v invSigma2 / [NE][4] u v uRight invSigma2 (uRight < 0: mono)
    uint8_t* level;                 // [NE]
    double *err, *Jp, *Jk, *wgt;    // [NE][rows], [NE][3 rows], [NE][6 rows], [NE]
    double *We;                     // [NE][6][3] = wgt * Jk^T Jp, the edge's block of W (block_solver.hpp's Hpl), written with the linearisation
    int *pr_start, *pr_ent;         // CSR over the key-frame pairs (a >= b, pair a (a + 1) / 2 + b): (edge of a, edge of b) of every point both observe (k_ba_pairs_*)
    const int *pt_start;            // [NP+1]
    const int *kf_start, *kf_list;  // CSR of the edges of each local key frame
    double *Hll, *bl, *Dinv, *db;   // [NP][9], [NP][3], [NP][9], [NP][3] = Dinv bl
    double *Hpp, *bp, *S, *bs, *xp, *xl;
    const double *preint, *info_pvr; // [W][142], [W][81] (NavState window)
    double *e_pvr, *e_b;            // [W][9], [W][3] (NavState window)
    double *scal;                   // [8]: 0 chi2, 1 scale, 2 ok, 3 max diag
    double *ctl;                    // the window's control block (lba_ctl.h): kernels return at once while ctl[BA_B_GATE] != 0
    int *ticket;                    // block counter of k_ba_f_errors_decide (the last block to add its chi2 takes the trial's decision)
    int use_ctl;                    // 1 in both drivers: the two lines above, and lambda from ctl[BA_CTL_LAMBDA]
    const unsigned long long* abort_host;   // page-locked word the waiting host thread sets when the caller's pbStopFlag goes up (nullptr: no flag)
    double cam[16], gw[3];          // NavState window: cam[16], gw; SE3 window: cam[0..4] = fx fy cx cy bf
    double acc_bias_rw2;
};

// Once an optimize() call is over (ctl[BA_B_GATE] != 0) every solver kernel still in the stream returns at once: the single window's host
// enqueues trials ahead of the decisions (BaSolve::run); in the lock-step batch the word is 0 whenever these bodies run (k_bab_phase).
__device__ __forceinline__ bool ba_skip(const BaDev& D) { return D.use_ctl && D.ctl[BA_B_GATE] != 0.0; }
// g2o polls terminate() once per iteration and once per LM trial (optimization_algorithm_levenberg.cpp / sparse_optimizer.cpp:354-432); the
// device-side LM control does the same through a system-scope load of the mirrored flag, so an abort costs at most the trial in flight
__device__ __forceinline__ bool ba_abort_requested(const BaDev& D) {
    return D.abort_host && __hip_atomic_load(D.abort_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0ull;
}
__device__ __forceinline__ double ba_lambda(const BaDev& D, double arg) { return D.use_ctl ? D.ctl[BA_CTL_LAMBDA] : arg; }

__device__ __forceinline__ nav_geom ba_edge_geom(const BaDev& D, int k, const cam_t& K) {
    return ba_nav_geom(K, D.kf + (size_t)D.e_kf[k] * 22, D.pt + (size_t)D.e_pt[k] * 3);
}
__device__ __forceinline__ int ba_pred(const BaDev& D, int i) { return i == 0 ? D.prev_kf : i - 1; }
__device__ __forceinline__ int ba_loc(const BaDev& D, int r) { return loc6(D.pose_dim, r); }

// residuals of the active edges + robust chi2 (mono kernel optional) + IMU / bias factors
__device__ __forceinline__ void k_ba_errors_body(const BaDev& D, int mono_kernel) {
    if (ba_skip(D)) return;
    __shared__ double s_red[8];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    double c = 0;
    if (k < D.NE && D.level[k] == 0) {
        const cam_t K = ld_cam(D.cam);
        double e[2], r1;
        ba_nav_error(K, ba_edge_geom(D, k, K).Pc, D.e_obs + 3 * k, e);
        D.err[2 * k] = e[0]; D.err[2 * k + 1] = e[1];
        ba_robust(mono_kernel, D.e_obs[3 * k + 2] * (e[0] * e[0] + e[1] * e[1]), ba_delta_mono_window(), &c, &r1);
    }
    if (blockIdx.x == 0 && threadIdx.x < D.W) {               // W <= blockDim.x
        const int i = threadIdx.x, j = ba_pred(D, i);
        if (j >= 0) {
            double e[9], rho[2]; d3 eb;                       // the window always applies the Huber kernel to these two factors
            ba_imu_chi2(D.kf + (size_t)i * 22, D.kf + (size_t)j * 22, D.preint + (size_t)i * 142, D.info_pvr + i * 81, ld3(D.gw), D.acc_bias_rw2, 1, e, &eb, rho);
            for (int a = 0; a < 9; a++) D.e_pvr[i * 9 + a] = e[a];
            st3(D.e_b + i * 3, eb);
            c += rho[0]; c += rho[1];
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += s_red[w]; atomicAdd(&D.scal[0], t); }
}

// The NavState linearisation with one thread per EDGE (Jacobians, weight, W block); the point blocks Hll, bl are summed afterwards by one
// thread per point from the stored Jacobians (k_ba_hll_body), in the order of the point's edges. A single window has 2000 points = 8
// workgroups with one thread per point (the form k_ba_se3_lin_points_body still has) but 43 with one per edge.
__device__ __forceinline__ void k_ba_lin_edges_body(const BaDev& D, int mono_kernel) {
    if (ba_skip(D)) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.NE || D.level[k] != 0) return;
    const cam_t K = ld_cam(D.cam);
    double Jp[6], Jk[12];
    ba_nav_jac(K, ba_edge_geom(D, k, K), Jp, Jk);
    const double e0 = D.err[2 * k], e1 = D.err[2 * k + 1], is2 = D.e_obs[3 * k + 2];
    double r0, r1;
    ba_robust(mono_kernel, is2 * (e0 * e0 + e1 * e1), ba_delta_mono_window(), &r0, &r1);
    const double w = r1 * is2;
    D.wgt[k] = w;
    // 16-byte stores (the blocks are 48, 96 and 144 bytes: 16-byte aligned): the kernel is bound by the number of per-lane memory operations
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
__device__ __forceinline__ void k_ba_hll_body(const BaDev& D, int bid) {
    if (ba_skip(D)) return;
    const int p = bid * blockDim.x + threadIdx.x;
    if (p >= D.NP) return;
    double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    for (int k = D.pt_start[p]; k < D.pt_start[p + 1]; k++) {
        if (D.level[k] != 0) continue;
        ba_point_add<2>(H, b, D.wgt[k], D.Jp + 6 * (size_t)k, D.err + 2 * k);
    }
    ba_point_store(D.Hll + (size_t)p * 9, D.bl + (size_t)p * 3, H, b);
}

// one workgroup per local key frame: sum of Jk^T w Jk / Jk^T w e over its active edges -> the 6x6 reprojection block of Hpp, bp
__device__ __forceinline__ void k_ba_hpp_body(const BaDev& D, int i = blockIdx.x) {
    if (ba_skip(D)) return;
    __shared__ double s_red[4][27];
    const int t = threadIdx.x, rows = D.rows;
    double a[27];
#pragma unroll
    for (int k = 0; k < 27; k++) a[k] = 0;
    for (int q = D.kf_start[i] + t; q < D.kf_start[i + 1]; q += blockDim.x) {
        const int k = D.kf_list[q];
        if (D.level[k] != 0) continue;
        const double* J = D.Jk + (size_t)6 * rows * k; const double* e = D.err + (size_t)rows * k; const double w = D.wgt[k];
        for (int row = 0; row < rows; row++) ba_kf_add_row(a, w, J + 6 * row, e[row]);
    }
    ba_kf_reduce(a, s_red);
    if (t < 27) {
        const double v = ba_kf_sum(s_red, t);
        const int base = D.pose_dim * i, n = D.np;
        if (t < 21) {
            int kk = 0, rr = 0, cc = 0;
            for (int r = 0; r < 6; r++) for (int c = r; c < 6; c++) { if (kk == t) { rr = r; cc = c; } kk++; }
            atomicAdd(&D.Hpp[(size_t)(base + ba_loc(D, rr)) * n + base + ba_loc(D, cc)], v);
            if (rr != cc) atomicAdd(&D.Hpp[(size_t)(base + ba_loc(D, cc)) * n + base + ba_loc(D, rr)], v);
        } else atomicAdd(&D.bp[base + ba_loc(D, t - 21)], v);
    }
}

// one workgroup per local key frame i: IMU factor (pred(i) -> i) and bias factor
__device__ __forceinline__ void k_ba_imu_body(const BaDev& D, int i = blockIdx.x) {
    if (ba_skip(D)) return;
    __shared__ double J[9 * 21], OJ[9 * 21], e[9];
    __shared__ int map[21];
    __shared__ double s_w;
    const int t = threadIdx.x, j = ba_pred(D, i), n = D.np;
    if (j < 0) return;
    const double* ki = D.kf + (size_t)i * 22; const double* kj = D.kf + (size_t)j * 22;
    if (t == 0) {
        d3 eb; double w_pvr, wb;                              // the window always applies the Huber kernel to these two factors
        ba_imu_weights(ki, kj, D.preint + (size_t)i * 142, D.info_pvr + i * 81, ld3(D.gw), D.acc_bias_rw2, 1, e, J, &w_pvr, &eb, &wb);
        s_w = w_pvr;
        for (int c = 0; c < 9; c++) { map[c] = j < D.W ? 12 * j + c : -1; map[9 + c] = 12 * i + c; }
        for (int c = 0; c < 3; c++) map[18 + c] = j < D.W ? 12 * j + 9 + c : -1;
        // bias factor
        const double ev[3] = {eb.x, eb.y, eb.z};
        for (int c = 0; c < 3; c++) {
            const int ic = 12 * i + 9 + c, jc = j < D.W ? 12 * j + 9 + c : -1;
            atomicAdd(&D.Hpp[(size_t)ic * n + ic], wb); atomicAdd(&D.bp[ic], -wb * ev[c]);
            if (jc >= 0) { atomicAdd(&D.Hpp[(size_t)jc * n + jc], wb); atomicAdd(&D.Hpp[(size_t)ic * n + jc], -wb); atomicAdd(&D.Hpp[(size_t)jc * n + ic], -wb); atomicAdd(&D.bp[jc], wb * ev[c]); }
        }
    }
    __syncthreads();
    ba_omega_j(D.info_pvr + i * 81, J, OJ, t, blockDim.x);
    __syncthreads();
    const double w = s_w;
    for (int q = t; q < 441 + 21; q += blockDim.x) {
        if (q < 441) { const int r = q / 21, c = q % 21; if (map[r] >= 0 && map[c] >= 0) { double s = 0; for (int k = 0; k < 9; k++) s += J[k * 21 + r] * OJ[k * 21 + c]; atomicAdd(&D.Hpp[(size_t)map[r] * n + map[c]], w * s); } }
        else { const int r = q - 441; if (map[r] >= 0) { double s = 0; for (int k = 0; k < 9; k++) s += OJ[k * 21 + r] * e[k]; atomicAdd(&D.bp[map[r]], -w * s); } }
    }
}

// S = Hpp + lambda I, bs = bp, written with the padded leading dimension ld (a multiple of 16: identity on the padding)
__device__ __forceinline__ void k_ba_init_reduced_body(const BaDev& D, double lambda_arg) {
    if (ba_skip(D)) return;
    const double lambda = ba_lambda(D, lambda_arg);
    const int q = blockIdx.x * blockDim.x + threadIdx.x, n = D.np, ld = D.ld;
    if (q < ld * ld) {
        const int i = q / ld, j = q - i * ld;
        D.S[q] = (i < n && j < n) ? D.Hpp[(size_t)i * n + j] + (i == j ? lambda : 0.0) : (i == j ? 1.0 : 0.0);
    }
    if (q < ld) D.bs[q] = q < n ? D.bp[q] : 0.0;
}
__device__ __forceinline__ void k_ba_max_diag_body(const BaDev& D) {
    if (ba_skip(D)) return;
    __shared__ double s_red[4];
    double m = 0;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < D.np + 3 * D.NP; q += gridDim.x * blockDim.x)
        m = fmax(m, fabs(q < D.np ? D.Hpp[(size_t)q * D.np + q] : D.Hll[(size_t)((q - D.np) / 3) * 9 + ((q - D.np) % 3) * 4]));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
        // fmax over non-negative doubles == max over their bit patterns as unsigned integers
        atomicMax(reinterpret_cast<unsigned long long*>(&D.scal[3]), (unsigned long long)__double_as_longlong(t));
    }
}

// one thread per point: Dinv = (Hll + lambda I)^-1 and Dinv * bl
__device__ __forceinline__ void k_ba_dinv_body(const BaDev& D, double lambda_arg, int bid = blockIdx.x) {
    if (ba_skip(D)) return;
    const double lambda = ba_lambda(D, lambda_arg);
    const int p = bid * blockDim.x + threadIdx.x;
    if (p >= D.NP) return;
    ba_point_inverse(D.Hll + (size_t)p * 9, lambda, D.bl + 3 * p, D.Dinv + (size_t)p * 9, D.db + 3 * p);
}
// Schur complement of the point block (block_solver.hpp:381-432), gathered per key-frame PAIR: wavefront (a, b), a >= b, owns the 6 x 6 block
// S[a][b] -= sum_p (W_pa Dinv_p) W_pb^T over the points p both observe (W = wgt Jk^T Jp from the linearisation, Dinv from k_ba_dinv; the
// Cholesky never reads above the diagonal) and, on the diagonal pairs, bs[a] -= sum_p W_pa Dinv_p bl_p. The pair's list of (edge of a,
// edge of b) comes from the host (ba_build_pairs: the graph is fixed over the solve; an edge gated out after the first phase is skipped by
// its level). One lane per list entry: both W blocks and Dinv as 16-byte loads, 162 FMA, 36 (+ 6) running sums in registers; the lanes' sums
// meet through an LDS transpose (row k = the 64 lanes' k-th sums, padded against bank conflicts), lane k adds row k and updates its
// element. One writer per block: no atomics, neither in LDS nor on S. (The round-2 form walked a key frame's observations with one thread
// each and added every product to an LDS block row by ds_add_f64 — 256 threads on the 36 addresses of each partner block: 0.6 atomics
// per cycle and CU, 475 us for 128 windows.)
#define BA_SCHUR_VALS 42
__device__ __forceinline__ void k_ba_schur_body(const BaDev& D, int pid) {
    if (ba_skip(D)) return;
    __shared__ double s_t[BA_SCHUR_VALS][65];
    const int lane = threadIdx.x;
    int a = (int)((sqrt(8.0 * (double)pid + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > pid) a--;
    while ((a + 1) * (a + 2) / 2 <= pid) a++;
    const int b = pid - a * (a + 1) / 2;
    const int e0 = D.pr_start[pid], e1 = D.pr_start[pid + 1];
    double acc[BA_SCHUR_VALS];
#pragma unroll
    for (int k = 0; k < BA_SCHUR_VALS; k++) acc[k] = 0.0;
    for (int i = e0 + lane; i < e1; i += 64) {
        const int2 ent = reinterpret_cast<const int2*>(D.pr_ent)[i];
        const int ea = ent.x, eb = ent.y;
        if (D.level[ea] != 0 || D.level[eb] != 0) continue;
        const int p = D.e_pt[ea];
        double wa[18], wb[18], di[9];
        {
            const double2* A2 = reinterpret_cast<const double2*>(D.We + (size_t)18 * ea); const double2* B2 = reinterpret_cast<const double2*>(D.We + (size_t)18 * eb);
#pragma unroll
            for (int k = 0; k < 9; k++) { const double2 u = A2[k], v = B2[k]; wa[2 * k] = u.x; wa[2 * k + 1] = u.y; wb[2 * k] = v.x; wb[2 * k + 1] = v.y; }
            const double* Dp = D.Dinv + (size_t)9 * p;
#pragma unroll
            for (int k = 0; k < 9; k++) di[k] = Dp[k];
        }
        double y[18];
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) y[3 * r + c] = wa[3 * r] * di[3 * c] + wa[3 * r + 1] * di[3 * c + 1] + wa[3 * r + 2] * di[3 * c + 2];
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) acc[6 * r + c] += y[3 * r] * wb[3 * c] + y[3 * r + 1] * wb[3 * c + 1] + y[3 * r + 2] * wb[3 * c + 2];
        if (ea == eb) {                                              // once per observation of a: W_pa (Dinv_p bl_p)
            const double d0 = D.db[3 * p], d1 = D.db[3 * p + 1], d2 = D.db[3 * p + 2];
#pragma unroll
            for (int r = 0; r < 6; r++) acc[36 + r] += wa[3 * r] * d0 + wa[3 * r + 1] * d1 + wa[3 * r + 2] * d2;
        }
    }
#pragma unroll
    for (int k = 0; k < BA_SCHUR_VALS; k++) s_t[k][lane] = acc[k];
    __syncthreads();
    if (lane < BA_SCHUR_VALS) {
        double v = 0.0;
#pragma unroll 16
        for (int l = 0; l < 64; l++) v += s_t[lane][l];
        const int pd = D.pose_dim;
        if (lane < 36) {
            const int row = pd * a + ba_loc(D, lane / 6), col = pd * b + ba_loc(D, lane % 6);
            if (col <= row && v != 0.0) D.S[(size_t)row * D.ld + col] -= v;
        } else if (a == b) D.bs[pd * a + ba_loc(D, lane - 36)] -= v;
    }
}

// Dense Cholesky solve S xp = bs of the reduced system by ONE 512-thread workgroup, blocked by 16 (n <= 240, padded to ld): the lower
// block triangle lives in the registers of seven waves as 16x16 tiles in the layout of v_mfma_f64_16x16x4_f64 (operands A[i][k]: lane
// 16k+i, B[k][j]: lane 16k+j; result row = lane/16 + 4*reg, col = lane%16 — probed on gfx950, tools/ubench/mfma_f64_layout.hip), the
// eighth wave factors the 16x16 diagonal blocks one block column ahead (see the body). The right-hand side lives in LDS and its forward
// substitution L y = bs rides along with the panels; the backward substitution uses the inverted diagonal blocks and is a 16x16 mat-vec
// + a rank-16 update per block. scal[2] = 1 on success; a pivot that is not positive and finite fails the solve like the reference's
// LLT (linear_solver_eigen.h / Eigen info()).
typedef double v4d __attribute__((ext_vector_type(4)));
#define BA_CHOL_THREADS 512                  // 8 waves: 7 tile owners + the factor wave
#define BA_CHOL_WAVES (BA_CHOL_THREADS / 64)
#define BA_CHOL_OWNERS (BA_CHOL_WAVES - 1)
#define BA_MAX_TILES_PER_WAVE 18             // ceil((15 * 16 / 2) / 7) register tiles (144 registers) per owner wave at ld = 240 (the lower block triangle; the right-hand side lives in LDS)
// lane broadcast of a double and a full-precision reciprocal square root (hardware estimate + two Newton steps) for the factorisation's
// diagonal blocks
__device__ __forceinline__ double ba_readlane(double v, int l) {
    union { double d; int i[2]; } u; u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], l); u.i[1] = __builtin_amdgcn_readlane(u.i[1], l);
    return u.d;
}
__device__ __forceinline__ double ba_rsqrt(double d) {
    double y = __builtin_amdgcn_rsq(d);
    y = fma(0.5 * y, fma(-(d * y), y, 1.0), y);
    y = fma(0.5 * y, fma(-(d * y), y, 1.0), y);
    return y;
}
#ifdef VIORB_CHOL_TIMING
#define CT_LAP(i) do { if ((threadIdx.x & 63) == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); ct_[i] += now_ - ct_last; ct_last = now_; } } while (0)     /* per wave, no barrier of its own */
#else
#define CT_LAP(i) do { } while (0)
#endif
// dynamic LDS of the Cholesky kernels: two panel buffers [256][17], the inverted diagonal block, the next diagonal tile, y
#define BA_CHOL_LDS_BYTES ((2 * 256 * 17 + 2 * 16 * 17 + 256) * sizeof(double))
__device__ __forceinline__ void k_ba_chol_solve_body(const BaDev& D, double* s_dyn) {
    if (ba_skip(D)) return;
#ifdef VIORB_CHOL_TIMING
    unsigned long long ct_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ct_last = __builtin_amdgcn_s_memtime();
#endif
    typedef double row17[17];
    row17* s_P0 = reinterpret_cast<row17*>(s_dyn);               // [256][17] panel of an even block column
    row17* s_P1 = s_P0 + 256;                                    // ... of an odd one
    row17* s_L = s_P1 + 256;                                     // [16][17] L11^-1 of the current block column
    row17* s_D = s_L + 16;                                       // [16][17] the next diagonal tile, as published
    double* s_y = reinterpret_cast<double*>(s_D + 16);           // [256]
    __shared__ int s_ok;
    const int n = D.np, ld = D.ld, nb = ld >> 4, t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int rows = ld + 16;                                    // + the block row that carries bs^T in its first row
    double* A = D.S;
    double* inv = A + (size_t)rows * ld;                         // [nb][16][16] inverted diagonal blocks
    if (t == 0) s_ok = 1;
    for (int i = t; i < 256; i += blockDim.x) s_y[i] = i < ld ? D.bs[i] : 0.0;             // the right-hand side; the forward substitution rides along with the panels
    // Two roles. Waves 0 .. BA_CHOL_OWNERS-1 own the lower block triangle in REGISTERS for the whole factorisation:
    // tile idx = wv + BA_CHOL_OWNERS u of the row-major enumeration (I, J <= I) is slot u of wave
    // wv, 4 doubles per lane in the MFMA accumulator layout (row = lane / 16 + 4 reg, col = lane % 16). The last wave owns nothing and
    // factors the diagonal blocks, ONE BLOCK COLUMN AHEAD of the owners. Per block column kb, three phases between barriers:
    //   P   the owners multiply their panel tiles of column kb by L11^-T (v_mfma_f64_16x16x4; operands in LDS) -> L21, final;
    //   3a  they apply panel kb's rank-16 update to their tiles of column kb + 1 FIRST and publish those to LDS (diagonal tile, next panel);
    //   3b  they update the rest of the trailing matrix WHILE the factor wave turns the published diagonal tile into L11 and L11^-1.
    // No global-memory round trip inside the loop; the factorisation of a diagonal block (a chain of 16 dependent 1/sqrt) hides behind
    // the trailing update. The two roles run separate loops with the same barriers, so the factor wave's ~100 live registers (block row,
    // inverse row, broadcasts) and the owners' 160 accumulator registers never have to fit one allocation. L and the solved rhs row are
    // written to global memory for the backward substitution.
    auto factor_block = [&](int kb) {
        // Lane li holds row li of the (symmetrised) block. A column step's dependent chain is pivot -> 1/sqrt (rsq + two Newton steps) ->
        // s = a_ij / d -> up to 15 independent FMAs; the broadcast of row j (v_readlane from lane j's registers: A[j][k] = A[k][j] is the
        // multiplier column k needs) does not depend on it. L11^-1 follows by a right-looking forward substitution with lane c on column
        // c: L goes through LDS once and comes back as broadcast reads that do not depend on the substitution's chain (two dependent
        // operations per row). (Building the inverse inside the factorisation loop doubled its v_readlane traffic: 8.8 k cycles per
        // block; row broadcasts through LDS inside the loop 11.8 k; the first form, broadcasting l_kj after the chain, 6.5 k without inverse.)
        const int li = lane & 15, k0 = kb << 4;
        double a[16], rinv[16];
#pragma unroll
        for (int c = 0; c < 16; c++) a[c] = c <= li ? s_D[li][c] : s_D[c][li];
        bool good = true;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const double d = ba_readlane(a[j], j);
            double u[16];
#pragma unroll
            for (int k = j + 1; k < 16; k++) u[k] = ba_readlane(a[k], j);
            const bool gj = (d > 0) && isfinite(d);
            good = good && gj;
            const double ri = ba_rsqrt(gj ? d : 1.0);
            rinv[j] = ri;
            const double sj = a[j] * (ri * ri);                                         // l_ij / l_jj
            a[j] = a[j] * ri;                                                           // l_ij (rows >= j; the rest never reaches a result)
#pragma unroll
            for (int k = j + 1; k < 16; k++) a[k] = fma(-sj, u[k], a[k]);
        }
        if (!good && lane == 0) s_ok = 0;
        if (lane < 16) {
#pragma unroll
            for (int c = 0; c < 16; c++) {
                s_D[li][c] = a[c];                                                      // L11 (lower triangle valid)
                if (c <= li) A[(size_t)(k0 + li) * ld + k0 + c] = a[c];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // X = L11^-1, column li per lane: x_u = acc_u / l_uu, then acc_i -= l_iu x_u for the rows below
        double x[16];
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = i == li ? 1.0 : 0.0;
#pragma unroll
        for (int u = 0; u < 16; u++) {
            x[u] *= rinv[u];
#pragma unroll
            for (int i = u + 1; i < 16; i++) x[i] = fma(-s_D[i][u], x[u], x[i]);
        }
        if (lane < 16) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                s_L[i][li] = x[i];                                                      // L11^-1 (lower triangular: x[i] = 0 for i < li)
                inv[(size_t)kb * 256 + i * 16 + li] = x[i];                             // for the backward substitution
            }
        }
    };
    if (wv == BA_CHOL_OWNERS) {
        __syncthreads();                                         // column 0 is published
        factor_block(0);
        __syncthreads();
        for (int kb = 0; kb < nb; kb++) {
            __syncthreads();                                     // (owners: P)
            __syncthreads();                                     // (owners: 3a) — the next diagonal tile is in s_D
            CT_LAP(1);
            if (kb + 1 < nb) factor_block(kb + 1);
            CT_LAP(2);
            __syncthreads();                                     // (owners: 3b)
            CT_LAP(3);
        }
    } else {
        v4d acc[BA_MAX_TILES_PER_WAVE]; int tI[BA_MAX_TILES_PER_WAVE], tJ[BA_MAX_TILES_PER_WAVE];
        const int ntiles_all = nb * (nb + 1) / 2;
#pragma unroll
        for (int u = 0; u < BA_MAX_TILES_PER_WAVE; u++) {
            const int idx = wv + BA_CHOL_OWNERS * u;
            tI[u] = -1; tJ[u] = -1;
            acc[u] = (v4d){0.0, 0.0, 0.0, 0.0};
            if (idx < ntiles_all) {
                int I = 0, rem = idx;
                while (rem > I) { rem -= I + 1; I++; }
                const int J = rem;
                tI[u] = I; tJ[u] = J;
#pragma unroll
                for (int r = 0; r < 4; r++) acc[u][r] = A[(size_t)(I * 16 + (lane >> 4) + 4 * r) * ld + J * 16 + (lane & 15)];
            }
        }
        // publish the tiles of block column c: the diagonal tile to s_D, the tiles below it to the panel buffer of that column's parity
        auto publish = [&](int c) {
            row17* Pn = (c & 1) ? s_P1 : s_P0;
#pragma unroll
            for (int u = 0; u < BA_MAX_TILES_PER_WAVE; u++) {
                if (tJ[u] != c) continue;
                if (tI[u] == c) {
#pragma unroll
                    for (int r = 0; r < 4; r++) s_D[(lane >> 4) + 4 * r][lane & 15] = acc[u][r];
                } else {
                    const int rb = (tI[u] - c - 1) * 16;
#pragma unroll
                    for (int r = 0; r < 4; r++) Pn[rb + (lane >> 4) + 4 * r][lane & 15] = acc[u][r];
                }
            }
        };
        publish(0);
        __syncthreads();
        __syncthreads();                                         // (factor wave: block 0)
        double yn = 0;
        for (int kb = 0; kb < nb; kb++) {
            const int k0 = kb << 4;
            row17* Pc = (kb & 1) ? s_P1 : s_P0;
            // P: L21 = A21 L11^-T per owned tile of block column kb of block column kb: A operand = the published tile, B[k][j] =
            //    L11^-1[j][k]; the result overwrites the tile's rows of the panel buffer (they belong to this wave alone in this phase). (A thread per row solving against L11 was a chain of 120 dependent FMAs fed by
            //    LDS reads: 7.3 k cycles per panel.)
#pragma unroll
            for (int u = 0; u < BA_MAX_TILES_PER_WAVE; u++) {
                if (tJ[u] != kb || tI[u] == kb) continue;
                const int rb = (tI[u] - kb - 1) * 16;
                v4d xt = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kc = 0; kc < 4; kc++)
                    xt = __builtin_amdgcn_mfma_f64_16x16x4f64(Pc[rb + (lane & 15)][4 * kc + (lane >> 4)], s_L[lane & 15][4 * kc + (lane >> 4)], xt, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; r++) Pc[rb + (lane >> 4) + 4 * r][lane & 15] = xt[r];
            }
            if (t < 16) {                                        // forward substitution of the right-hand side: y_kb <- L11^-1 y_kb
                double yk = 0;
#pragma unroll
                for (int c = 0; c < 16; c++) yk += s_L[t][c] * s_y[k0 + c];
                yn = yk;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (t < 16) s_y[k0 + t] = yn;
            CT_LAP(1);
            __syncthreads();
            // 3a: y_I -= L21_I y_kb for the rows below (one thread per row of the panel), the rank-16 update of the tiles of block column kb + 1,
            //     then their publication
            if (t < ld - k0 - 16) {
                double yv = s_y[k0 + 16 + t];
                double* Arow = A + (size_t)(k0 + 16 + t) * ld + k0;      // L21 goes to global memory here, a row per thread (per-tile stores in P kept
#pragma unroll                                                           // 4 hoisted 64-bit addresses per tile alive: spills)
                for (int c = 0; c < 16; c++) { const double l = Pc[t][c]; yv -= l * s_y[k0 + c]; Arow[c] = l; }
                s_y[k0 + 16 + t] = yv;
            }
#pragma unroll
            for (int u = 0; u < BA_MAX_TILES_PER_WAVE; u++) {
                if (tJ[u] != kb + 1) continue;                   // tJ > kb implies tI > kb
                const int Io = (tI[u] - kb - 1) * 16 + (lane & 15), Jo = (tJ[u] - kb - 1) * 16 + (lane & 15);
#pragma unroll
                for (int kc = 0; kc < 4; kc++)
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Pc[Io][4 * kc + (lane >> 4)], Pc[Jo][4 * kc + (lane >> 4)], acc[u], 0, 0, 0);
            }
            if (kb + 1 < nb) publish(kb + 1);
            CT_LAP(2);
            __syncthreads();
            // 3b: the rest of the trailing matrix, beside the factor wave
#pragma unroll
            for (int u = 0; u < BA_MAX_TILES_PER_WAVE; u++) {
                if (tJ[u] <= kb + 1) continue;
                const int Io = (tI[u] - kb - 1) * 16 + (lane & 15), Jo = (tJ[u] - kb - 1) * 16 + (lane & 15);
#pragma unroll
                for (int kc = 0; kc < 4; kc++)
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Pc[Io][4 * kc + (lane >> 4)], Pc[Jo][4 * kc + (lane >> 4)], acc[u], 0, 0, 0);
            }
            CT_LAP(3);
            __syncthreads();
            CT_LAP(4);
        }
    }
    __syncthreads();
    CT_LAP(0);
    // y = L^-1 bs now sits in s_y; backward substitution L^T x = y, 16 unknowns at a time
    for (int kb = nb - 1; kb >= 0; kb--) {
        const int k0 = kb << 4;
        double xi = 0;
        if (t < 16) {                                            // x_blk = L11^-T y_blk
#pragma unroll
            for (int c = 0; c < 16; c++) xi += inv[(size_t)kb * 256 + c * 16 + t] * s_y[k0 + c];
        }
        __syncthreads();
        if (t < 16) s_y[k0 + t] = xi;
        __syncthreads();
        if (t < k0) {
            double v = s_y[t];
#pragma unroll
            for (int c = 0; c < 16; c++) v -= A[(size_t)(k0 + c) * ld + t] * s_y[k0 + c];
            s_y[t] = v;
        }
        __syncthreads();
    }
    CT_LAP(5);
    for (int i = t; i < n; i += blockDim.x) D.xp[i] = s_ok ? s_y[i] : 0.0;
#ifdef VIORB_CHOL_TIMING
    if (lane == 0 && (wv == 0 || wv == BA_CHOL_OWNERS) && blockIdx.x == 0) printf("chol cycles wave %d: [0] %llu [1] %llu [2] %llu [3] %llu [4] %llu [5] %llu [6] %llu\n", wv, ct_[0], ct_[1], ct_[2], ct_[3], ct_[4], ct_[5], ct_[6]);
#endif
    if (t == 0) { D.scal[2] = s_ok ? 1.0 : 0.0; D.scal[1] = 0.0; D.scal[0] = 0.0; }      // [1], [0]: accumulators of the back-substitution and of the error pass, which follow
}

// a rejected trial: local key frames and points back to what k_ba_backsub8_update_body saved
__device__ __forceinline__ void k_ba_restore_body(const BaDev& D) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, stride = D.kf_stride;
    if (q < D.W) for (int c = 0; c < stride; c++) D.kf[(size_t)q * stride + c] = D.kf_bak[(size_t)q * stride + c];
    if (q < D.NP) for (int c = 0; c < 3; c++) D.pt[3 * q + c] = D.pt_bak[3 * q + c];
}

// chi2 / depth gate on every edge (stale error on excluded edges, fresh depth), Optimizer.cc:2037-2051 and :2105-2118
__device__ __forceinline__ void k_ba_gate_body(const BaDev& D, uint8_t* out, int set_level) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.NE) return;
    const d3 Pc = ba_edge_geom(D, k, ld_cam(D.cam)).Pc;
    const double chi = D.e_obs[3 * k + 2] * (D.err[2 * k] * D.err[2 * k] + D.err[2 * k + 1] * D.err[2 * k + 1]);
    const int bad = (chi > BA_GATE_CHI2_MONO || !(Pc.z > 0.0)) ? 1 : 0;
    if (set_level) { if (bad) D.level[k] = 1; } else out[k] = (uint8_t)bad;
}

// zero Hpp / bp (and the max-diagonal accumulator) for the linearisation of an iteration; first = 1 on the first iteration of a single
// window's phase (the lock-step round has launches of its own for that: k_bab_round_begin, k_bab_take_chi, k_bab_lambda0)
__device__ __forceinline__ void k_ba_clear_body(const BaDev& D, int first, int bid = blockIdx.x, int nblk = gridDim.x) {
    if (ba_skip(D)) return;
    const size_t n2 = (size_t)D.np * D.np;
    for (size_t q = (size_t)bid * blockDim.x + threadIdx.x; q < n2; q += (size_t)nblk * blockDim.x) D.Hpp[q] = 0.0;
    if (bid == 0) {
        for (int q = threadIdx.x; q < D.np; q += blockDim.x) D.bp[q] = 0.0;
        if (threadIdx.x == 0) {
            if (first) { D.scal[3] = 0.0; D.ctl[BA_CTL_CHI] = D.scal[0]; D.ctl[BA_CTL_NBAD] = 0.0; }   // chi2 of the phase's first computeActiveErrors
            D.ctl[BA_CTL_INICHI] = D.ctl[BA_CTL_CHI];
        }
    }
}

// ---- by-value kernels of the single-window driver (its fused launches follow the vision-only bodies below) ---------------------------
__global__ void k_ba_errors(BaDev D, int mono_kernel) { k_ba_errors_body(D, mono_kernel); }
__global__ void k_ba_max_diag(BaDev D) { k_ba_max_diag_body(D); }
__global__ __launch_bounds__(64) void k_ba_schur(BaDev D) { k_ba_schur_body(D, blockIdx.x); }
__global__ __launch_bounds__(BA_CHOL_THREADS) void k_ba_chol_solve(BaDev D) { extern __shared__ __attribute__((aligned(16))) double s_chol[]; k_ba_chol_solve_body(D, s_chol); }
__global__ void k_ba_restore(BaDev D) { k_ba_restore_body(D); }
__global__ void k_ba_gate(BaDev D, uint8_t* out, int set_level) { k_ba_gate_body(D, out, set_level); }
// the control block at the start of the solve and at its phase change: the host applies the same functions to its copy (BaSolve::run)
__global__ void k_ba_ctl_init(BaDev D) { if (threadIdx.x < BA_B_N) D.ctl[threadIdx.x] = lba_ctl_init(threadIdx.x); }
__global__ void k_ba_phase(BaDev D) { if (threadIdx.x == 0) lba_phase(D.ctl); }
// lambda_0, after k_ba_max_diag on the first iteration of a phase
__global__ void k_ba_lambda0(BaDev D) { if (!ba_skip(D) && blockIdx.x == 0 && threadIdx.x == 0) lba_lambda0(D.ctl, D.scal[3]); }

// ---- lock-step batch: one launch covers every window of a batch (blockIdx.y = window) ------------------------------------------------
// viorb_local_ba_navstate_batch used to give every window its own stream and host-driven LM loop; the streams share four hardware queues,
// so at most four windows' kernel chains really overlapped (436 windows/s for 64 W = 20 windows). Here all windows advance through the
// same ROUND of launches — [chi2 of a new phase] [linearise if the last trial was accepted] [lambda_0 on a phase's first iteration]
// [one LM trial] [decide] [restore a rejected trial] [phase gate] — and the per-window state machine of g2o's Levenberg loop
// (optimization_algorithm_levenberg.cpp:61-164) plus LocalBundleAdjustmentNavState's two optimize() calls (src/Optimizer.cc:2026-2099)
// lives in the window's control block on the device (lba_ctl.h). A round is 16 launches for the whole batch (the k_bab_f_* ones cover several solver steps by block range); the host only counts finished windows
// every few rounds.
#define BA_B_WINDOW() const BaDev& D = Dv[blockIdx.y]; const double* c = D.ctl; if (c[BA_B_DONE] != 0.0 || c[BA_B_ABORT] != 0.0) return
__global__ void k_bab_round_begin(const BaDev* __restrict__ Dv, int nwin) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwin) return;
    const BaDev& D = Dv[w]; double* c = D.ctl;
    if (c[BA_B_DONE] != 0.0 || c[BA_B_ABORT] != 0.0) return;
    if (c[BA_B_NEED_CHI] != 0.0) D.scal[0] = 0.0;                        // accumulator of the phase's first computeActiveErrors
    if (c[BA_B_NEED_LIN] != 0.0 && c[BA_B_FIRST] != 0.0) D.scal[3] = 0.0;  // accumulator of k_ba_max_diag
}
__global__ void k_bab_take_chi(const BaDev* __restrict__ Dv, int nwin) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwin) return;
    const BaDev& D = Dv[w]; double* c = D.ctl;
    if (c[BA_B_DONE] != 0.0 || c[BA_B_ABORT] != 0.0 || c[BA_B_NEED_CHI] == 0.0) return;
    c[BA_CTL_CHI] = D.scal[0]; c[BA_B_NEED_CHI] = 0.0;
}
__global__ void k_bab_max_diag(const BaDev* __restrict__ Dv) { BA_B_WINDOW(); if (c[BA_B_NEED_LIN] == 0.0 || c[BA_B_FIRST] == 0.0) return; k_ba_max_diag_body(D); }
__global__ void k_bab_lambda0(const BaDev* __restrict__ Dv, int nwin) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwin) return;
    const BaDev& D = Dv[w]; double* c = D.ctl;
    if (c[BA_B_DONE] != 0.0 || c[BA_B_ABORT] != 0.0 || c[BA_B_NEED_LIN] == 0.0) return;
    if (c[BA_B_FIRST] != 0.0) lba_lambda0(c, D.scal[3]);
    c[BA_B_NEED_LIN] = 0.0;
}
// The batch's grid is (pairs, windows) linearised and dealt so that all pairs of a window run on ONE XCD (workgroup ids go round-robin over the
// eight XCDs): a window's W blocks (1.6 MB at 10.9 k edges) are read by ~5 pairs each and stay in that XCD's L2 meanwhile.
__global__ __launch_bounds__(64) void k_bab_schur(const BaDev* __restrict__ Dv, int npairs, int nwin) {
    const int L = blockIdx.x, xcd = L & 7, s = L >> 3;
    const int win = (s / npairs) * 8 + xcd, pid = s - (s / npairs) * npairs;
    if (win >= nwin) return;
    const BaDev& D = Dv[win]; const double* c = D.ctl;
    if (c[BA_B_DONE] != 0.0 || c[BA_B_ABORT] != 0.0) return;
    if (pid >= D.W * (D.W + 1) / 2) return;
    k_ba_schur_body(D, pid);
}
__global__ __launch_bounds__(BA_CHOL_THREADS) void k_bab_chol_solve(const BaDev* __restrict__ Dv) { extern __shared__ __attribute__((aligned(16))) double s_chol[]; BA_B_WINDOW(); k_ba_chol_solve_body(D, s_chol); }
// the Levenberg decisions of one trial, per window (:129-161), and the end of an optimize() call
__global__ void k_bab_decide(const BaDev* __restrict__ Dv, int nwin) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwin) return;
    const BaDev& D = Dv[w]; double* c = D.ctl;
    if (c[BA_B_DONE] != 0.0) return;
    if (c[BA_B_ABORT] != 0.0) { c[BA_B_GATE] = 2.0; return; }            // the host saw the stop flag between rounds (this round's trial kernels were skipped): final gate on the state as it is
    lba_decide(c, D.scal[0], D.scal[1], D.scal[2], ba_abort_requested(D));   // a rejected trial is restored by k_bab_restore, before the gate
}
__global__ void k_bab_restore(const BaDev* __restrict__ Dv) { BA_B_WINDOW(); if (c[BA_B_RESTORE] == 0.0) return; k_ba_restore_body(D); }
// after the gate: phase 0 -> second optimize() without the mono kernel (src/Optimizer.cc:2037-2099), phase 1 -> the window is finished
__global__ void k_bab_phase(const BaDev* __restrict__ Dv, int nwin, int* __restrict__ n_done) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwin) return;
    const BaDev& D = Dv[w]; double* c = D.ctl;
    if (c[BA_B_DONE] != 0.0) return;
    if (lba_phase(c)) atomicAdd(n_done, 1);
}

// ---- vision-only LocalBundleAdjustment (reference src/Optimizer.cc:3980-4311): SE3 key frames (kf = qx qy qz qw tx ty tz of Tcw),
// EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ (Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:66-250). e_obs[k] = u v uRight invSigma2
// (uRight < 0: mono); cam[0..4] = fx fy cx cy bf. Three residual rows per edge (the third is zero for mono edges).
__device__ __forceinline__ void k_ba_se3_errors_body(const BaDev& D, int kernels) {
    if (ba_skip(D)) return;
    __shared__ double s_red[8];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    double c = 0;
    if (k < D.NE && D.level[k] == 0) {
        const double* ob = D.e_obs + 4 * (size_t)k;
        double e[3];
        se3_edge(se3_ld7(D.kf + (size_t)D.e_kf[k] * 7), ld3(D.pt + (size_t)D.e_pt[k] * 3), ob[0], ob[1], ob[2], D.cam[0], D.cam[1], D.cam[2], D.cam[3], D.cam[4], false, e, nullptr);
        D.err[3 * k] = e[0]; D.err[3 * k + 1] = e[1]; D.err[3 * k + 2] = e[2];
        const double chi = ob[3] * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        double r1;
        ba_robust(kernels, chi, ba_se3_stereo(ob) ? ba_delta_stereo() : ba_delta_mono_window(), &c, &r1);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += s_red[w]; atomicAdd(&D.scal[0], t); }
}
__device__ __forceinline__ void k_ba_se3_lin_points_body(const BaDev& D, int kernels) {
    if (ba_skip(D)) return;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.NP) return;
    double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    const double fx = D.cam[0], fy = D.cam[1], bf = D.cam[4];
    for (int k = D.pt_start[p]; k < D.pt_start[p + 1]; k++) {
        if (D.level[k] != 0) continue;
        const double* ob = D.e_obs + 4 * (size_t)k;
        const bool stereo = ba_se3_stereo(ob);
        double Jp[9], Jk[18];
        ba_se3_jac(se3_ld7(D.kf + (size_t)D.e_kf[k] * 7), ld3(D.pt + (size_t)p * 3), stereo, fx, fy, bf, Jp, Jk);
        const double e[3] = {D.err[3 * k], D.err[3 * k + 1], D.err[3 * k + 2]}, is2 = ob[3];
        double r0, r1;
        ba_robust(kernels, is2 * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]), stereo ? ba_delta_stereo() : ba_delta_mono_window(), &r0, &r1);
        const double w = r1 * is2;
        D.wgt[k] = w;
        for (int a = 0; a < 9; a++) D.Jp[9 * (size_t)k + a] = Jp[a];
        for (int a = 0; a < 18; a++) D.Jk[18 * (size_t)k + a] = Jk[a];
        ba_w_block<3>(w, Jk, Jp, D.We + 18 * (size_t)k);
        ba_point_add<3>(H, b, w, Jp, e);
    }
    ba_point_store(D.Hll + (size_t)p * 9, D.bl + (size_t)p * 3, H, b);
}
// chi2 (5.991 mono / 7.815 stereo, stale error on excluded edges) / depth gate, Optimizer.cc:4170-4200 and :4207-4235
__device__ __forceinline__ void k_ba_se3_gate_body(const BaDev& D, uint8_t* out, int set_level) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.NE) return;
    const double* ob = D.e_obs + 4 * (size_t)k;
    const d3 pc = se3_map(se3_ld7(D.kf + (size_t)D.e_kf[k] * 7), ld3(D.pt + (size_t)D.e_pt[k] * 3));
    const double chi = ob[3] * (D.err[3 * k] * D.err[3 * k] + D.err[3 * k + 1] * D.err[3 * k + 1] + D.err[3 * k + 2] * D.err[3 * k + 2]);
    const int bad = (chi > (ba_se3_stereo(ob) ? BA_GATE_CHI2_STEREO : BA_GATE_CHI2_MONO) || !(pc.z > 0.0)) ? 1 : 0;
    if (set_level) { if (bad) D.level[k] = 1; } else out[k] = (uint8_t)bad;
}
__global__ void k_ba_se3_errors(BaDev D, int kernels) { k_ba_se3_errors_body(D, kernels); }
__global__ void k_ba_se3_gate(BaDev D, uint8_t* out, int set_level) { k_ba_se3_gate_body(D, out, set_level); }

// ---- fused launches of the single window's slots (BaSolve::run): kernels with no dependency between them share a launch
// (by block range), the per-point back-substitution applies its own update, and the last block of the error pass takes the trial's
// decision — 8 launches per Levenberg trial. A single window is a chain of latency-bound launches of 5-25 us each: every launch removed
// is ~7 us of the ~230 us a trial takes. The host enqueues slots ahead of the decisions, so what a slot does is read from the control
// block: after an iteration has ended it linearises (its first two launches); after a rejected trial it is a retry — the first launch
// puts the estimate back instead and the second returns at once, the system of the last linearisation is solved again with the new
// lambda. (A rejected trial that ends its iteration without a Terminate — rho NaN — is handled like a retry: the linearisation at hand is
// the one of the restored estimate.)
enum { BA_SLOT_IDLE = 0, BA_SLOT_LINEARISE, BA_SLOT_RESTORE };
__device__ __forceinline__ int ba_slot(const BaDev& D) {
    const double* c = D.ctl;
    if (c[BA_B_GATE] != 0.0) return BA_SLOT_IDLE;                         // the phase is over
    if (c[BA_B_RESTORE] != 0.0) return BA_SLOT_RESTORE;
    return c[BA_B_NEED_LIN] != 0.0 ? BA_SLOT_LINEARISE : BA_SLOT_IDLE;
}
// gL blocks of the linearisation (at least as many as k_ba_restore_body needs), gC of the clear
template <int MODEL> __device__ __forceinline__ void k_ba_f_lin_clear_body(const BaDev& D, int mono_kernel, int gL, int gC) {
    const int slot = ba_slot(D);
    if (slot == BA_SLOT_RESTORE) { k_ba_restore_body(D); return; }
    if (slot != BA_SLOT_LINEARISE) return;
    if ((int)blockIdx.x >= gL) k_ba_clear_body(D, D.ctl[BA_B_FIRST] != 0.0, (int)blockIdx.x - gL, gC);
    else if (MODEL == 0) k_ba_lin_edges_body(D, mono_kernel);
    else k_ba_se3_lin_points_body(D, mono_kernel);
}
__global__ __launch_bounds__(256) void k_ba_f_lin_clear(BaDev D, int mono_kernel, int gL, int gC) { k_ba_f_lin_clear_body<1>(D, mono_kernel, gL, gC); }    // vision-only window: one thread per point
__global__ __launch_bounds__(256) void k_ba_f_line_clear(BaDev D, int mono_kernel, int gL, int gC) { k_ba_f_lin_clear_body<0>(D, mono_kernel, gL, gC); }   // NavState window: one thread per edge
__global__ __launch_bounds__(256) void k_ba_f_hpp_imu_hll(BaDev D) {
    if (ba_slot(D) != BA_SLOT_LINEARISE) return;
    const int b = blockIdx.x;
    if (b < D.W) k_ba_hpp_body(D, b); else if (b < 2 * D.W) k_ba_imu_body(D, b - D.W); else k_ba_hll_body(D, b - 2 * D.W);
}
__global__ __launch_bounds__(256) void k_ba_f_hpp(BaDev D) {                 // vision-only window (its linearisation wrote the point blocks itself)
    if (ba_slot(D) != BA_SLOT_LINEARISE) return;
    k_ba_hpp_body(D, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_ba_f_init_dinv(BaDev D, int gR) {
    if ((int)blockIdx.x < gR) k_ba_init_reduced_body(D, 0.0); else k_ba_dinv_body(D, 0.0, (int)blockIdx.x - gR);
}
// back-substitution of the point block with EIGHT lanes per point (one observation each per trip, shuffle reduction) + the update: the
// thread-per-point form was 8 workgroups for a 2000-point window and the latency of a lane walking its point's observations one after
// the other. xl = Dinv (bl - W^T xp) per point, the LM scale term sum x (lambda x + b), and the backup a rejected trial goes back to
__device__ __forceinline__ void k_ba_backsub8_update_body(const BaDev& D) {
    if (ba_skip(D)) return;
    const double lambda = ba_lambda(D, 0.0);
    __shared__ double s_red[4];
    const int g = blockIdx.x * blockDim.x + threadIdx.x, p = g >> 3, sub = g & 7;
    double a0 = 0, a1 = 0, a2 = 0;
    if (p < D.NP)
        for (int k = D.pt_start[p] + sub; k < D.pt_start[p + 1]; k += 8) {
            if (D.level[k] != 0 || D.e_kf[k] >= D.W) continue;
            const double* Wk = D.We + (size_t)18 * k;
            const int ba = D.pose_dim * D.e_kf[k];
#pragma unroll
            for (int r = 0; r < 6; r++) {
                const double x = D.xp[ba + ba_loc(D, r)];
                a0 += Wk[3 * r] * x; a1 += Wk[3 * r + 1] * x; a2 += Wk[3 * r + 2] * x;
            }
        }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) { a0 += __shfl_xor(a0, d); a1 += __shfl_xor(a1, d); a2 += __shfl_xor(a2, d); }
    double sc = 0;
    if (p < D.NP && sub == 0) {
        const double b0 = D.bl[3 * p], b1 = D.bl[3 * p + 1], b2 = D.bl[3 * p + 2];
        const double c0 = b0 - a0, c1 = b1 - a1, c2 = b2 - a2;
        const double* Di = D.Dinv + (size_t)p * 9;
        const double x0 = Di[0] * c0 + Di[1] * c1 + Di[2] * c2, x1 = Di[3] * c0 + Di[4] * c1 + Di[5] * c2, x2 = Di[6] * c0 + Di[7] * c1 + Di[8] * c2;
        D.xl[3 * p] = x0; D.xl[3 * p + 1] = x1; D.xl[3 * p + 2] = x2;
        sc = x0 * (lambda * x0 + b0) + x1 * (lambda * x1 + b1) + x2 * (lambda * x2 + b2);
        const double xs[3] = {x0, x1, x2};
        for (int c = 0; c < 3; c++) { D.pt_bak[3 * p + c] = D.pt[3 * p + c]; D.pt[3 * p + c] += xs[c]; }      // the backup a rejected trial goes back to (k_ba_restore_body)
    }
    if (blockIdx.x == 0) for (int q = threadIdx.x; q < D.np; q += blockDim.x) sc += D.xp[q] * (lambda * D.xp[q] + D.bp[q]);
    sc = ba_block_sum(sc, s_red);
    if (threadIdx.x == 0) atomicAdd(&D.scal[1], sc);
    if (g < D.W) {                                                       // the key frames, backup first
        if (D.pose_dim == 12) {
            double* k = D.kf + (size_t)g * 22;
            for (int c = 0; c < 22; c++) D.kf_bak[(size_t)g * 22 + c] = k[c];
            const pvr s = inc_small_pvr(ld_pvr(k), D.xp + 12 * g);
            st_pvr(k, s);
            for (int c = 0; c < 3; c++) k[19 + c] += D.xp[12 * g + 9 + c];
        } else {
            double* k = D.kf + (size_t)g * 7;
            for (int c = 0; c < 7; c++) D.kf_bak[(size_t)g * 7 + c] = k[c];
            se3_oplus7(k, D.xp + 6 * g);                                 // VertexSE3Expmap::oplusImpl: T <- exp(update) * T
        }
    }
}
__global__ __launch_bounds__(256) void k_ba_f_backsub8_update(BaDev D) { k_ba_backsub8_update_body(D); }
// ---- the lock-step batch's fused launches (blockIdx.y = window; the same bodies, gated by the window's control block) ----
__global__ __launch_bounds__(256) void k_bab_f_lin_clear(const BaDev* __restrict__ Dv, int gL, int gC) {   // gL = blocks of the linearisation: edges (NavState) or points (SE3)
    BA_B_WINDOW(); if (c[BA_B_NEED_LIN] == 0.0) return;
    if ((int)blockIdx.x < gL) { if (D.pose_dim == 12) k_ba_lin_edges_body(D, c[BA_B_MONO] != 0.0); else k_ba_se3_lin_points_body(D, c[BA_B_MONO] != 0.0); }
    else k_ba_clear_body(D, 0, (int)blockIdx.x - gL, gC);
}
__global__ __launch_bounds__(256) void k_bab_f_hpp_imu_hll(const BaDev* __restrict__ Dv, int Wmax) {
    BA_B_WINDOW(); if (c[BA_B_NEED_LIN] == 0.0) return;
    const int b = blockIdx.x;
    if (b < Wmax) { if (b < D.W) k_ba_hpp_body(D, b); }
    else if (b < 2 * Wmax) { if (b - Wmax < D.W && D.pose_dim == 12) k_ba_imu_body(D, b - Wmax); }
    else if (D.pose_dim == 12) k_ba_hll_body(D, b - 2 * Wmax);           // the SE3 linearisation (one thread per point) wrote its point blocks itself
}
__global__ __launch_bounds__(256) void k_bab_f_init_dinv(const BaDev* __restrict__ Dv, int gR) {
    BA_B_WINDOW();
    if ((int)blockIdx.x < gR) k_ba_init_reduced_body(D, 0.0); else k_ba_dinv_body(D, 0.0, (int)blockIdx.x - gR);
}
__global__ __launch_bounds__(256) void k_bab_f_backsub8_update(const BaDev* __restrict__ Dv) { BA_B_WINDOW(); k_ba_backsub8_update_body(D); }
// the single window's error pass; its last block takes the trial's decision (one thread) and so says what the next slot is
__global__ __launch_bounds__(256) void k_ba_f_errors_decide(BaDev D, int mono_kernel) {
    if (D.pose_dim == 12) k_ba_errors_body(D, mono_kernel); else k_ba_se3_errors_body(D, mono_kernel);
    __shared__ int s_last;
    if (threadIdx.x == 0) { __threadfence(); s_last = atomicAdd(D.ticket, 1) == (int)gridDim.x - 1; }
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        *D.ticket = 0; __threadfence();
        if (ba_skip(D)) return;
        double* c = D.ctl;
        c[BA_B_NEED_LIN] = 0.0; c[BA_B_RESTORE] = 0.0;                    // this slot's first launches have acted on them
        lba_decide(c, __hip_atomic_load(&D.scal[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), D.scal[1], D.scal[2], ba_abort_requested(D));
    }
}
// lock-step batch, the launches whose body depends on the kind of window (pose_dim 12: NavState, 6: vision-only SE3)
__global__ void k_bab_errors_chi(const BaDev* __restrict__ Dv) {
    BA_B_WINDOW(); if (c[BA_B_NEED_CHI] == 0.0) return;
    if (D.pose_dim == 12) k_ba_errors_body(D, c[BA_B_MONO] != 0.0); else k_ba_se3_errors_body(D, c[BA_B_MONO] != 0.0);
}
__global__ void k_bab_errors(const BaDev* __restrict__ Dv) {
    BA_B_WINDOW();
    if (D.pose_dim == 12) k_ba_errors_body(D, c[BA_B_MONO] != 0.0); else k_ba_se3_errors_body(D, c[BA_B_MONO] != 0.0);
}
// control blocks of a group's windows at the start of the solve (one launch instead of one small copy per window)
__global__ void k_bab_ctl_init(const BaDev* __restrict__ Dv) {
    double* c = Dv[blockIdx.x].ctl;
    const int t = threadIdx.x;
    if (t < BA_B_N) c[t] = lba_ctl_init(t);
}
// results of a group's windows into one device buffer (one copy back for the group instead of four per window): per window, at offs[4 w ..],
// key frames | points | erase flags | control block
__global__ void k_bab_pack(const BaDev* __restrict__ Dv, uint8_t* const* __restrict__ erase, uint8_t* __restrict__ out, const unsigned long long* __restrict__ offs) {
    const BaDev& D = Dv[blockIdx.y];
    const unsigned long long* o = offs + 4 * (size_t)blockIdx.y;
    const size_t nkf = (size_t)D.W * D.kf_stride, npt = (size_t)D.NP * 3, ner = (size_t)D.NE;
    double* okf = reinterpret_cast<double*>(out + o[0]); double* opt = reinterpret_cast<double*>(out + o[1]); uint8_t* oer = out + o[2]; double* oct = reinterpret_cast<double*>(out + o[3]);
    size_t n = ner > npt ? ner : npt; n = n > nkf ? n : nkf; n = n > (size_t)BA_B_N ? n : (size_t)BA_B_N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (i < ner) oer[i] = erase[blockIdx.y][i];
        if (i < nkf) okf[i] = D.kf[i];
        if (i < npt) opt[i] = D.pt[i];
        if (i < BA_B_N) oct[i] = D.ctl[i];
    }
}
__global__ void k_bab_gate(const BaDev* __restrict__ Dv, uint8_t* const* __restrict__ erase) {
    const BaDev& D = Dv[blockIdx.y]; const double* c = D.ctl;
    if (c[BA_B_DONE] != 0.0 || c[BA_B_GATE] == 0.0) return;
    if (D.pose_dim == 12) k_ba_gate_body(D, erase[blockIdx.y], c[BA_B_GATE] == 1.0 ? 1 : 0);
    else k_ba_se3_gate_body(D, erase[blockIdx.y], c[BA_B_GATE] == 1.0 ? 1 : 0);
}

} // namespace viorb

using namespace viorb;

namespace {
std::atomic<int> g_lba_device{-1};
// The device the window solves run on: viorb_local_ba_set_device(), else the calling thread's current HIP device (what
// torch.cuda.set_device(LOCAL_RANK) / hipSetDevice selected), so that under torchrun every rank's windows land on its own GPU.
static int lba_device() {
    int d = g_lba_device.load();
    if (d < 0 && hipGetDevice(&d) != hipSuccess) d = 0;
    return d;
}
// alloc() lays the arrays out in a host mirror (inputs copied, work arrays zero); commit() uploads the mirror into the context's
// arena in one copy and patches the recorded pointers.
struct BaBuf {
    // Inputs are laid out in a host mirror and uploaded in one copy; work arrays follow them in the arena and are only zeroed on the
    // device (uploading their zeros from the host was most of the per-window host time of a batch).
    struct Item { void** slot; size_t off; int kind; };            // 0 input, 1 zeroed work array, 2 work array that is written before it is read
    std::vector<Item> items;
    std::vector<uint8_t> mirror;
    size_t work_bytes = 0, raw_bytes = 0;
    template <class T> bool alloc(T** d, size_t n, const T* src = nullptr) {
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if (src) {
            const size_t off = (mirror.size() + 255) & ~(size_t)255;
            mirror.resize(off + bytes, 0);
            if (n) memcpy(mirror.data() + off, src, n * sizeof(T));
            items.push_back({reinterpret_cast<void**>(d), off, 0});
        } else {
            const size_t off = (work_bytes + 255) & ~(size_t)255;
            work_bytes = off + bytes;
            items.push_back({reinterpret_cast<void**>(d), off, 1});
        }
        *d = nullptr;
        return true;
    }
    // the large per-edge / per-point work arrays: every element a kernel reads has been written by an earlier kernel of the same solve
    // (zeroing them was 4 MB of memset per window, 8 % of a batch's stream time)
    template <class T> bool alloc_raw(T** d, size_t n) {
        const size_t off = (raw_bytes + 255) & ~(size_t)255;
        raw_bytes = off + std::max<size_t>(n, 1) * sizeof(T);
        items.push_back({reinterpret_cast<void**>(d), off, 2});
        *d = nullptr;
        return true;
    }
    bool commit(StreamCtx* c) {
        const size_t in_bytes = (mirror.size() + 255) & ~(size_t)255, zero_bytes = (work_bytes + 255) & ~(size_t)255, total = in_bytes + zero_bytes + raw_bytes;
        if (c->bytes < total) {
            if (c->arena) (void)hipFree(c->arena);
            c->arena = nullptr; c->bytes = 0;
            const size_t want = total + total / 4;
            if (hipMalloc(&c->arena, want) != hipSuccess) { c->arena = nullptr; return false; }
            c->bytes = want;
        }
        uint8_t* base = static_cast<uint8_t*>(c->arena);
        // The inputs go through the context's page-locked staging buffer: a truly asynchronous copy, and no synchronisation per window (a
        // pageable source made every upload a blocking staged copy + a stream synchronise: half of a batch's wall time was spent here).
        // The staging buffer belongs to the context, and a context serves one window at a time.
        if (!mirror.empty()) {
            if (c->stage_bytes < mirror.size()) {
                if (c->stage) (void)hipHostFree(c->stage);
                c->stage = nullptr; c->stage_bytes = 0;
                const size_t want = mirror.size() + mirror.size() / 4;
                if (hipHostMalloc(reinterpret_cast<void**>(&c->stage), want) != hipSuccess) { c->stage = nullptr; return false; }
                c->stage_bytes = want;
            }
            memcpy(c->stage, mirror.data(), mirror.size());
            if (hipMemcpyAsync(base, c->stage, mirror.size(), hipMemcpyHostToDevice, c->st) != hipSuccess) return false;
        }
        if (work_bytes && hipMemsetAsync(base + in_bytes, 0, work_bytes, c->st) != hipSuccess) return false;
        for (const Item& it : items) *it.slot = base + (it.kind == 0 ? it.off : (it.kind == 1 ? in_bytes + it.off : in_bytes + zero_bytes + it.off));
        return true;
    }
};
bool host_inverse9(const double* a_in, double* inv) {
    double a[81]; for (int i = 0; i < 81; i++) { a[i] = a_in[i]; inv[i] = (i / 9 == i % 9) ? 1.0 : 0.0; }
    for (int col = 0; col < 9; col++) {
        int p = col; double best = std::fabs(a[col * 9 + col]);
        for (int i = col + 1; i < 9; i++) if (std::fabs(a[i * 9 + col]) > best) { best = std::fabs(a[i * 9 + col]); p = i; }
        if (best == 0) return false;
        if (p != col) for (int j = 0; j < 9; j++) { std::swap(a[p * 9 + j], a[col * 9 + j]); std::swap(inv[p * 9 + j], inv[col * 9 + j]); }
        const double iv = 1.0 / a[col * 9 + col];
        for (int j = 0; j < 9; j++) { a[col * 9 + j] *= iv; inv[col * 9 + j] *= iv; }
        for (int i = 0; i < 9; i++) if (i != col) { const double f = a[i * 9 + col]; if (f == 0) continue; for (int j = 0; j < 9; j++) { a[i * 9 + j] -= f * a[col * 9 + j]; inv[i * 9 + j] -= f * inv[col * 9 + j]; } }
    }
    return true;
}
} // namespace

// One window on the host: optimize(5) -> gate / drop kernels -> optimize(10) -> erase flags (reference src/Optimizer.cc:2100-2160 and the
// vision-only twin; model 0: NavState window, 1: SE3 window). g2o's Levenberg loop itself (optimization_algorithm_levenberg.cpp:61-189)
// runs on the device, in the window's control block; the host enqueues trial slots ahead of it and reads the block after each chunk. It
// polls the stream instead of blocking in hipStreamSynchronize (whose wake-up costs more than the kernels of a trial take).
struct BaSolve;
static int ba_launch_pairs(const BaDev& D, hipStream_t st);      // the Schur complement's gather lists (k_ba_pairs_build, below)
static void ba_mirror_stop_flags(BaSolve* const* S, int n);
// Waits for the stream; meanwhile mirrors the callers' stop flags into the page-locked words the device-side LM control polls.
static hipError_t ba_wait(hipStream_t st, BaSolve* const* S = nullptr, int n = 0) {
    for (;;) {
        if (n) ba_mirror_stop_flags(S, n);
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
    }
}
// what a finished window's control block says about the solve
static void ba_info_from_ctl(const double* c, double info[6]) {
    info[0] = c[BA_B_CHI0]; info[1] = c[BA_B_CHI1]; info[2] = c[BA_B_ITS0]; info[3] = c[BA_B_ITS1];
    info[4] = c[BA_CTL_TRIALS]; info[5] = c[BA_CTL_REJECTS];
}
enum { BA_PIN_CTL = 8, BA_PIN_ABORT = 56 };                        // pinned[8..39]: the single window's copy of its control block; [48]: the batch's done counter; [56]: the mirrored stop flag (a 64-bit word)
struct BaSolve {
    StreamCtxLease lease;         // of the calling thread's current device: the caller has selected it (hipSetDevice(lba_device()))
    BaDev D; hipStream_t st = nullptr; double* h = nullptr;       // h: 64 page-locked doubles
    int model = 0; const volatile int* stop = nullptr; uint8_t* d_erase = nullptr;
    double* kfs_out = nullptr; double* points_out = nullptr; uint8_t* erase = nullptr; double* info = nullptr;
    enum State { ST_READY, ST_DONE } state = ST_READY;           // ST_DONE: the stop flag was up on entry, the outputs hold the inputs
    bool terminate() const { return stop && *stop; }
    // The single call. A slot is one Levenberg trial: 8 launches (k_ba_f_*), + k_ba_max_diag and k_ba_lambda0 on a phase's first. What a
    // slot does (linearise first, or restore and retry, or nothing because the phase is over) the device decides (ba_slot), so the host
    // enqueues as many slots as the phase has iterations left — all it needs when no trial is rejected — then reads the control block and
    // enqueues more if the phase is not over. The caller's stop flag, which g2o polls once per iteration and once per trial, is polled
    // here before every chunk and on the device after every trial, through its page-locked mirror.
    int run() {
        if (state == ST_DONE) return VIORB_OK;
        VIORB_TRY(ba_launch_pairs(D, st));
        const int npts = D.NP, ne = D.NE, n_local = D.W, TB = 256, gE = (ne + TB - 1) / TB, gP = (npts + TB - 1) / TB;
        const int gL = model == 0 ? std::max(gE, gP) : std::max(gP, 1);        // the linearisation's blocks also carry the restore (one thread per point / local key frame)
        const size_t n2 = (size_t)D.np * D.np, nl2 = (size_t)D.ld * D.ld;
        const unsigned gC = (unsigned)std::min<size_t>((n2 + TB - 1) / TB, 256), gR = (unsigned)((nl2 + TB - 1) / TB);
        (void)raise_dynamic_lds(reinterpret_cast<const void*>(k_ba_chol_solve), BA_CHOL_LDS_BYTES);
        BaSolve* self = this;
        double* c = h + BA_PIN_CTL;
        D.use_ctl = 1;
        for (int t = 0; t < BA_B_N; t++) c[t] = lba_ctl_init(t);
        hipLaunchKernelGGL(k_ba_ctl_init, dim3(1), dim3(64), 0, st, D);
        do {
            // an optimize() call: chi2 at the starting point (computeActiveErrors of the first iteration)
            const int mono_kernel = c[BA_B_MONO] != 0.0;
            VIORB_HIP_TRY(hipMemsetAsync(D.scal, 0, sizeof(double), st));
            if (model == 0) hipLaunchKernelGGL(k_ba_errors, dim3(gE), dim3(TB), 0, st, D, mono_kernel);
            else hipLaunchKernelGGL(k_ba_se3_errors, dim3(gE), dim3(TB), 0, st, D, mono_kernel);
            while (c[BA_B_GATE] == 0.0 && !terminate()) {
                const double trials = c[BA_CTL_TRIALS];
                const int n = std::max(1, (int)(c[BA_B_ITERS] - c[BA_CTL_IT]));
                for (int i = 0; i < n; i++) {
                    if (model == 0) {
                        hipLaunchKernelGGL(k_ba_f_line_clear, dim3(gL + gC), dim3(TB), 0, st, D, mono_kernel, gL, (int)gC);
                        hipLaunchKernelGGL(k_ba_f_hpp_imu_hll, dim3(2 * n_local + gP), dim3(256), 0, st, D);
                    } else {
                        hipLaunchKernelGGL(k_ba_f_lin_clear, dim3(gL + gC), dim3(TB), 0, st, D, mono_kernel, gL, (int)gC);
                        hipLaunchKernelGGL(k_ba_f_hpp, dim3(n_local), dim3(256), 0, st, D);
                    }
                    if (i == 0 && c[BA_B_FIRST] != 0.0) {
                        hipLaunchKernelGGL(k_ba_max_diag, dim3(32), dim3(256), 0, st, D);
                        hipLaunchKernelGGL(k_ba_lambda0, dim3(1), dim3(64), 0, st, D);
                    }
                    hipLaunchKernelGGL(k_ba_f_init_dinv, dim3(gR + gP), dim3(TB), 0, st, D, (int)gR);
                    hipLaunchKernelGGL(k_ba_schur, dim3(n_local * (n_local + 1) / 2), dim3(64), 0, st, D);
                    hipLaunchKernelGGL(k_ba_chol_solve, dim3(1), dim3(BA_CHOL_THREADS), BA_CHOL_LDS_BYTES, st, D);
                    hipLaunchKernelGGL(k_ba_f_backsub8_update, dim3((unsigned)std::max((8 * npts + TB - 1) / TB, 1)), dim3(TB), 0, st, D);
                    hipLaunchKernelGGL(k_ba_f_errors_decide, dim3(gE), dim3(TB), 0, st, D, mono_kernel);
                }
                VIORB_HIP_TRY(hipGetLastError());
                VIORB_HIP_TRY(hipMemcpyAsync(c, D.ctl, BA_B_N * sizeof(double), hipMemcpyDeviceToHost, st));
                VIORB_HIP_TRY(ba_wait(st, &self, 1));
                if (c[BA_B_GATE] == 0.0 && c[BA_CTL_TRIALS] == trials) { set_error("window solve: a chunk of trials took no decision"); return VIORB_ERR_HIP; }
            }
            // a trial rejected at the very end is undone before the gate, which then sees that trial's errors beside the restored estimate
            if (c[BA_B_RESTORE] != 0.0) hipLaunchKernelGGL(k_ba_restore, dim3(std::max(gP, 1)), dim3(TB), 0, st, D);
            if (terminate()) c[BA_B_GATE] = 2.0;                   // "&& !terminate()": no second optimize(), final gate on the state as it is
            const int set_level = c[BA_B_GATE] == 1.0;            // after the first optimize() the gate drops edges; after the last it writes the erase flags
            if (model == 0) hipLaunchKernelGGL(k_ba_gate, dim3(gE), dim3(TB), 0, st, D, d_erase, set_level);
            else hipLaunchKernelGGL(k_ba_se3_gate, dim3(gE), dim3(TB), 0, st, D, d_erase, set_level);
            if (set_level) hipLaunchKernelGGL(k_ba_phase, dim3(1), dim3(64), 0, st, D);      // the second optimize(): the device's block and the host's copy take the same step
        } while (!lba_phase(c));
        VIORB_HIP_TRY(hipMemcpyAsync(kfs_out, D.kf, (size_t)n_local * D.kf_stride * sizeof(double), hipMemcpyDeviceToHost, st));
        VIORB_HIP_TRY(hipMemcpyAsync(points_out, D.pt, (size_t)npts * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        VIORB_HIP_TRY(hipMemcpyAsync(erase, d_erase, ne, hipMemcpyDeviceToHost, st));
        VIORB_HIP_TRY(ba_wait(st, &self, 1));
        ba_info_from_ctl(c, info);
        state = ST_DONE;
        return VIORB_OK;
    }
};

static void ba_mirror_stop_flags(BaSolve* const* S, int n) {
    for (int i = 0; i < n; i++)
        if (S[i] && S[i]->h && S[i]->D.abort_host && S[i]->terminate())
            reinterpret_cast<volatile unsigned long long*>(S[i]->h)[BA_PIN_ABORT] = 1ull;
}
// the page-locked mirror of the caller's stop flag, mapped for the device (called by ba_prepare_* once S.h and S.stop are set)
static hipError_t ba_map_stop_flag(BaSolve& S) {
    S.D.abort_host = nullptr;
    if (!S.stop) return hipSuccess;
    reinterpret_cast<volatile unsigned long long*>(S.h)[BA_PIN_ABORT] = 0ull;
    void* dp = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dp, S.h + BA_PIN_ABORT, 0);
    if (e == hipSuccess) S.D.abort_host = reinterpret_cast<const unsigned long long*>(dp);
    return e;
}


// The gather lists of k_ba_schur, built on the device when a window is prepared (the graph is fixed over the solve): (edge of a, edge of b)
// for every pair of local key frames a >= b and every point both observe; the diagonal pairs list every local observation once. One
// 1024-thread workgroup per window on the window's stream: histogram of the pairs in LDS, exclusive scan, fill through LDS cursors (the
// order inside a pair's list is not fixed: it only permutes the terms of that block's sum). Building the lists on the host cost 0.1-0.2 ms
// per window, counting with global atomics 0.1 ms (30 k increments of 210 counters) — more than a batched solve gains from them.
#define BA_MAX_PAIRS 820                                               // 40 local key frames (the SE3 window's limit)
template <class F> __device__ __forceinline__ void ba_pairs_walk(const BaDev& D, F f) {
    for (int p = threadIdx.x; p < D.NP; p += blockDim.x) {
        const int k0 = D.pt_start[p], k1 = D.pt_start[p + 1];
        for (int i = k0; i < k1; i++) {
            const int a = D.e_kf[i];
            if (a >= D.W) continue;
            for (int j = k0; j < k1; j++) {
                const int b = D.e_kf[j];
                if (b <= a) f(a * (a + 1) / 2 + b, i, j);            // (i, j) with kf(i) >= kf(j); i == j once
            }
        }
    }
}
__device__ __forceinline__ void k_ba_pairs_build_body(const BaDev& D) {
    __shared__ int s_h[BA_MAX_PAIRS + 1];
    const int npairs = D.W * (D.W + 1) / 2, t = threadIdx.x;
    for (int q = t; q <= npairs; q += blockDim.x) s_h[q] = 0;
    __syncthreads();
    ba_pairs_walk(D, [&](int q, int, int) { atomicAdd(&s_h[q], 1); });
    __syncthreads();
    if (t < 64) {                                                      // exclusive scan; the counters become the fill cursors
        int run = 0;
        for (int base = 0; base <= npairs; base += 64) {
            const int q = base + t, c = q < npairs ? s_h[q] : 0;
            int incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (t >= d) incl += o; }
            if (q <= npairs) { D.pr_start[q] = run + incl - c; s_h[q] = run + incl - c; }
            run += __shfl(incl, 63);
        }
    }
    __syncthreads();
    ba_pairs_walk(D, [&](int q, int i, int j) { const int at = atomicAdd(&s_h[q], 1); D.pr_ent[2 * (size_t)at] = i; D.pr_ent[2 * (size_t)at + 1] = j; });
}
__global__ __launch_bounds__(1024) void k_ba_pairs_build(BaDev D) { k_ba_pairs_build_body(D); }
__global__ __launch_bounds__(1024) void k_bab_pairs_build(const BaDev* __restrict__ Dv) { k_ba_pairs_build_body(Dv[blockIdx.x]); }   // a lock-step group's windows in one launch
static int ba_launch_pairs(const BaDev& D, hipStream_t st) {
    hipLaunchKernelGGL(k_ba_pairs_build, dim3(1), dim3(1024), 0, st, D);
    VIORB_HIP_TRY(hipGetLastError());
    return VIORB_OK;
}
// upper bound of the pair lists' length: every ordered pair of a point's local observations
static size_t ba_pairs_bound(const std::vector<int>& e_kf, const std::vector<int>& pt_start, int npts, int n_local) {
    size_t tot = 0;
    for (int p = 0; p < npts; p++) { size_t k = 0; for (int i = pt_start[p]; i < pt_start[p + 1]; i++) k += e_kf[i] < n_local; tot += k * k; }
    return tot;
}

// Argument checks, host-side graph bookkeeping and the upload of one NavState window; leaves `S` ready for BaSolve::run() or a lock-step group (or already done
// when the stop flag was set on entry).
static int ba_prepare_navstate(BaSolve& S, const double* kfs, int nk, int n_local, int prev_kf, const double* preint, const double* points, int npts,
                               const int32_t* edge_idx, const double* edge_obs, int ne, const double gw[3], const double cam[16],
                               const volatile int* stop, double* kfs_out, double* points_out, uint8_t* erase, double info[6]) {
    VIORB_REQUIRE(kfs && preint && points && edge_idx && edge_obs && gw && cam && kfs_out && points_out && erase && info, "null array");
    VIORB_REQUIRE(n_local >= 1 && n_local <= 20 && nk >= n_local && npts >= 1 && ne >= 1, "1 <= n_local <= 20 key frames, at least one point and edge");
    VIORB_REQUIRE(prev_kf == -1 || (prev_kf >= n_local && prev_kf < nk), "prev_kf must index a fixed key frame or be -1");
    VIORB_TRY(require_device());
    for (int i = 0; i < 6; i++) info[i] = 0;
    for (int i = 0; i < n_local * 22; i++) kfs_out[i] = kfs[i];
    for (int i = 0; i < npts * 3; i++) points_out[i] = points[i];
    for (int k = 0; k < ne; k++) erase[k] = 0;
    auto terminate = [&]() { return stop && *stop; };
    if (terminate()) { S.state = BaSolve::ST_DONE; return VIORB_OK; }
    // ---- host-side graph bookkeeping
    std::vector<int> e_pt(ne), e_kf(ne), pt_start(npts + 1, 0);
    for (int k = 0; k < ne; k++) {
        e_pt[k] = edge_idx[2 * k]; e_kf[k] = edge_idx[2 * k + 1];
        VIORB_REQUIRE(e_pt[k] >= 0 && e_pt[k] < npts && e_kf[k] >= 0 && e_kf[k] < nk, "edge index out of range");
        VIORB_REQUIRE(k == 0 || e_pt[k] >= e_pt[k - 1], "edges must be grouped by point (ascending point index)");
        pt_start[e_pt[k] + 1]++;
    }
    for (int p = 0; p < npts; p++) pt_start[p + 1] += pt_start[p];
    std::vector<int> kf_start(n_local + 1, 0), kf_list;
    for (int k = 0; k < ne; k++) if (e_kf[k] < n_local) kf_start[e_kf[k] + 1]++;
    for (int i = 0; i < n_local; i++) kf_start[i + 1] += kf_start[i];
    kf_list.resize(kf_start[n_local]);
    { std::vector<int> pos(kf_start.begin(), kf_start.end() - 1); for (int k = 0; k < ne; k++) if (e_kf[k] < n_local) kf_list[pos[e_kf[k]]++] = k; }
    const size_t pr_bound = ba_pairs_bound(e_kf, pt_start, npts, n_local);
    std::vector<double> info_pvr((size_t)n_local * 81);
    for (int i = 0; i < n_local; i++) if (!host_inverse9(preint + (size_t)i * 142 + 60, &info_pvr[(size_t)i * 81])) { set_error("singular IMU covariance"); return VIORB_ERR_INVALID_ARG; }

    VIORB_HIP_TRY(hipSetDevice(lba_device()));
    StreamCtxLease& lease = S.lease;
    if (!lease.ready()) { set_error("could not create a HIP stream"); return VIORB_ERR_HIP; }
    BaBuf B; BaDev& D = S.D;
    D.W = n_local; D.NK = nk; D.NP = npts; D.NE = ne; D.np = 12 * n_local; D.prev_kf = prev_kf; D.acc_bias_rw2 = 5e-3 * 5e-3;
    D.pose_dim = 12; D.rows = 2; D.kf_stride = 22;
    for (int i = 0; i < 16; i++) D.cam[i] = cam[i];
    for (int i = 0; i < 3; i++) D.gw[i] = gw[i];
    int *d_ept, *d_ekf, *d_pts, *d_kfs, *d_kfl; double *d_obs, *d_pre, *d_info; uint8_t* d_erase;
    D.ld = (D.np + 15) & ~15;
    const size_t n2 = (size_t)D.np * D.np, nl2 = (size_t)D.ld * D.ld;
    bool ok = B.alloc(&D.kf, (size_t)nk * 22, kfs) && B.alloc_raw(&D.kf_bak, (size_t)nk * 22) && B.alloc(&D.pt, (size_t)npts * 3, points) && B.alloc_raw(&D.pt_bak, (size_t)npts * 3) &&
              B.alloc(&d_ept, ne, e_pt.data()) && B.alloc(&d_ekf, ne, e_kf.data()) && B.alloc(&d_obs, (size_t)ne * 3, edge_obs) && B.alloc(&D.level, ne) &&
              B.alloc_raw(&D.err, (size_t)ne * 2) && B.alloc_raw(&D.Jp, (size_t)ne * 6) && B.alloc_raw(&D.Jk, (size_t)ne * 12) && B.alloc_raw(&D.wgt, ne) && B.alloc_raw(&D.We, (size_t)ne * 18) &&
              B.alloc(&D.pr_start, (size_t)n_local * (n_local + 1) / 2 + 1) && B.alloc_raw(&D.pr_ent, 2 * pr_bound + 2) &&
              B.alloc(&d_pts, npts + 1, pt_start.data()) && B.alloc(&d_kfs, n_local + 1, kf_start.data()) && B.alloc(&d_kfl, kf_list.size(), kf_list.data()) &&
              B.alloc_raw(&D.Hll, (size_t)npts * 9) && B.alloc_raw(&D.bl, (size_t)npts * 3) && B.alloc_raw(&D.Dinv, (size_t)npts * 9) &&
              B.alloc_raw(&D.Hpp, n2) && B.alloc(&D.bp, D.np) && B.alloc(&D.S, nl2 + (size_t)16 * D.ld + (size_t)(D.ld / 16) * 256) && B.alloc(&D.bs, D.ld) && B.alloc(&D.xp, D.ld) && B.alloc_raw(&D.db, (size_t)npts * 3) && B.alloc_raw(&D.xl, (size_t)npts * 3) &&
              B.alloc(&d_pre, (size_t)n_local * 142, preint) && B.alloc(&d_info, info_pvr.size(), info_pvr.data()) &&
              B.alloc(&D.e_pvr, (size_t)n_local * 9) && B.alloc(&D.e_b, (size_t)n_local * 3) && B.alloc(&D.scal, 8) && B.alloc(&D.ctl, (size_t)BA_CTL_N) && B.alloc(&D.ticket, 1) && B.alloc(&d_erase, ne) && B.commit(lease.c);
    if (!ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    D.e_pt = d_ept; D.e_kf = d_ekf; D.e_obs = d_obs; D.pt_start = d_pts; D.kf_start = d_kfs; D.kf_list = d_kfl; D.preint = d_pre; D.info_pvr = d_info;
    S.st = lease.c->st; S.h = lease.c->pinned; S.model = 0; S.stop = stop; S.d_erase = d_erase;
    VIORB_HIP_TRY(ba_map_stop_flag(S));
    S.kfs_out = kfs_out; S.points_out = points_out; S.erase = erase; S.info = info;
    return VIORB_OK;
}

extern "C" int viorb_local_ba_set_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n) { set_error("no such HIP device: %d", device); return VIORB_ERR_INVALID_ARG; }
    g_lba_device.store(device < 0 ? -1 : device);
    return VIORB_OK;
}

extern "C" int viorb_local_ba_navstate(const double* kfs, int nk, int n_local, int prev_kf, const double* preint, const double* points, int npts,
                                       const int32_t* edge_idx, const double* edge_obs, int ne, const double gw[3], const double cam[16],
                                       const volatile int* stop, double* kfs_out, double* points_out, uint8_t* erase, double info[6]) {
    BaSolve S;
    const int rc = ba_prepare_navstate(S, kfs, nk, n_local, prev_kf, preint, points, npts, edge_idx, edge_obs, ne, gw, cam, stop, kfs_out, points_out, erase, info);
    return rc != VIORB_OK ? rc : S.run();
}

// Lock-step batch of NavState windows (kernels k_bab_*): returns the first error; every window's status through set_status.
template <class Win, class Prepare>
static int ba_run_lockstep(Win* w, int n, int max_in_flight, Prepare prepare) {
    VIORB_TRY(require_device());
    VIORB_HIP_TRY(hipSetDevice(lba_device()));
    int first_error = VIORB_OK;
    // windows advanced together (max_in_flight of the batch entry points; default 128): every solver step is one launch over the group
    const int GROUP = max_in_flight > 0 ? std::min(max_in_flight, 512) : 128, TB = 256, ROUNDS_PER_CHECK = 4, MAX_ROUNDS = 600;
    for (int g0 = 0; g0 < n; g0 += GROUP) {
        const int ng = std::min(GROUP, n - g0);
        std::vector<std::unique_ptr<BaSolve>> S(ng);
        std::vector<int> act;
        {   // argument checks, graph bookkeeping, input mirror and upload of every window: independent per window (own context, stream and
            // arena), ~0.1 ms of host time each — spread over a few host threads so that the device does not wait for them
            const int dev = lba_device();
            const int nthr = std::max(1, std::min(std::min(8, (int)std::thread::hardware_concurrency()), ng / 4));
            std::vector<std::string> errs(ng);
            auto work = [&](int t0) {
                (void)hipSetDevice(dev);
                for (int i = t0; i < ng; i += nthr) {
                    Win& q = w[g0 + i];
                    S[i] = std::make_unique<BaSolve>();
                    q.status = prepare(*S[i], q);
                    if (q.status != VIORB_OK) errs[i] = viorb_last_error();      // the error text is per thread
                }
            };
            std::vector<std::thread> pool;
            for (int t0 = 1; t0 < nthr; t0++) pool.emplace_back(work, t0);
            work(0);
            for (std::thread& th : pool) th.join();
            for (int i = 0; i < ng; i++) {
                const int rc = w[g0 + i].status;
                if (rc != VIORB_OK) { if (first_error == VIORB_OK) { first_error = rc; set_error("%s", errs[i].c_str()); } continue; }
                if (S[i]->state == BaSolve::ST_DONE) continue;           // stop flag already set: inputs copied to the outputs
                act.push_back(i);
            }
        }
        const int na = (int)act.size();
        if (na == 0) continue;
        // the group's solve; an early return (a HIP error, MAX_ROUNDS) must not leave status == VIORB_OK on windows whose outputs were never written
        auto solve_group = [&]() -> int {
        hipStream_t st = S[act[0]]->st;
        std::vector<BaDev> Dh(na); std::vector<uint8_t*> Eh(na);
        int gE = 1, gP = 1, Wmax = 1; size_t nl2 = 1, n2 = 1;
        for (int a = 0; a < na; a++) {
            BaSolve& B = *S[act[a]];
            VIORB_HIP_TRY(hipStreamSynchronize(B.st));                   // the window's inputs are uploaded
            Dh[a] = B.D; Dh[a].use_ctl = 1; Eh[a] = B.d_erase;
            gE = std::max(gE, (B.D.NE + TB - 1) / TB); gP = std::max(gP, (B.D.NP + TB - 1) / TB); Wmax = std::max(Wmax, B.D.W);
            nl2 = std::max(nl2, (size_t)B.D.ld * B.D.ld); n2 = std::max(n2, (size_t)B.D.np * B.D.np);
        }
        BaDev* Dv = nullptr; uint8_t** Ev = nullptr; int* d_done = nullptr;
        // the group's descriptor arrays: grow-only buffers of the calling thread (hipMalloc / hipFree synchronise the whole device)
        struct GroupBufs {
            void* p[3] = {nullptr, nullptr, nullptr}; int cap = 0, device = -1;
            void drop() { for (void*& q : p) { if (q) (void)hipFree(q); q = nullptr; } cap = 0; }
            ~GroupBufs() { drop(); }
        };
        static thread_local GroupBufs gb;
        if (gb.device != lba_device() || gb.cap < na) {
            gb.drop(); gb.device = lba_device();
            const int want = std::max(na, 128);
            VIORB_HIP_TRY(hipMalloc(&gb.p[0], sizeof(BaDev) * want)); VIORB_HIP_TRY(hipMalloc(&gb.p[1], sizeof(uint8_t*) * want)); VIORB_HIP_TRY(hipMalloc(&gb.p[2], sizeof(int)));
            gb.cap = want;
        }
        Dv = (BaDev*)gb.p[0]; Ev = (uint8_t**)gb.p[1]; d_done = (int*)gb.p[2];
        VIORB_HIP_TRY(hipMemcpyAsync(Dv, Dh.data(), sizeof(BaDev) * na, hipMemcpyHostToDevice, st));
        VIORB_HIP_TRY(hipMemcpyAsync(Ev, Eh.data(), sizeof(uint8_t*) * na, hipMemcpyHostToDevice, st));
        VIORB_HIP_TRY(hipMemsetAsync(d_done, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_bab_ctl_init, dim3(na), dim3(64), 0, st, Dv);
        hipLaunchKernelGGL(k_bab_pairs_build, dim3(na), dim3(1024), 0, st, Dv);            // the Schur complement's gather lists of every window
        double* pin = S[act[0]]->h;                                      // page-locked scratch of the first window's context
        int* h_done = reinterpret_cast<int*>(pin + 48);
        const unsigned gw = (unsigned)((na + 63) / 64), gR = (unsigned)((nl2 + TB - 1) / TB), gC = (unsigned)std::min<size_t>((n2 + TB - 1) / TB, 64);
        const dim3 Y1(1, na), YE(gE, na), YP(std::max(gP, 1), na);
        const int gL = std::max(gE, gP), g8 = std::max(8 * gP, 1);      // blocks of the linearisation (edges or points, by the kind of window) and of the 8-lane back-substitution
        int rounds = 0, done = 0;
        std::vector<char> aborted(na, 0);
        std::vector<BaSolve*> Sp(na);
        for (int a = 0; a < na; a++) Sp[a] = S[act[a]].get();
        while (done < na && rounds < MAX_ROUNDS) {
            for (int r = 0; r < ROUNDS_PER_CHECK; r++, rounds++) {
                // (ProfScope: HIP-event pairs around the heavy launches when viorb_profile_enable is on — bench.py --config local_ba; free otherwise)
                hipLaunchKernelGGL(k_bab_round_begin, dim3(gw), dim3(64), 0, st, Dv, na);
                { ProfScope ps("k_bab_errors_chi", st); hipLaunchKernelGGL(k_bab_errors_chi, YE, dim3(TB), 0, st, Dv); }
                hipLaunchKernelGGL(k_bab_take_chi, dim3(gw), dim3(64), 0, st, Dv, na);
                { ProfScope ps("k_bab_f_lin_clear", st); hipLaunchKernelGGL(k_bab_f_lin_clear, dim3((unsigned)gL + gC, na), dim3(TB), 0, st, Dv, gL, (int)gC); }
                { ProfScope ps("k_bab_f_hpp_imu_hll", st); hipLaunchKernelGGL(k_bab_f_hpp_imu_hll, dim3((unsigned)(2 * Wmax + gP), na), dim3(256), 0, st, Dv, Wmax); }
                hipLaunchKernelGGL(k_bab_max_diag, dim3(8, na), dim3(256), 0, st, Dv);
                hipLaunchKernelGGL(k_bab_lambda0, dim3(gw), dim3(64), 0, st, Dv, na);
                { ProfScope ps("k_bab_f_init_dinv", st); hipLaunchKernelGGL(k_bab_f_init_dinv, dim3(gR + (unsigned)gP, na), dim3(TB), 0, st, Dv, (int)gR); }
                { ProfScope ps("k_bab_schur", st);
                  hipLaunchKernelGGL(k_bab_schur, dim3((unsigned)(Wmax * (Wmax + 1) / 2) * 8u * (unsigned)((na + 7) / 8)), dim3(64), 0, st, Dv, Wmax * (Wmax + 1) / 2, na); }
                (void)raise_dynamic_lds(reinterpret_cast<const void*>(k_bab_chol_solve), BA_CHOL_LDS_BYTES);
                { ProfScope ps("k_bab_chol_solve", st); hipLaunchKernelGGL(k_bab_chol_solve, Y1, dim3(BA_CHOL_THREADS), BA_CHOL_LDS_BYTES, st, Dv); }
                { ProfScope ps("k_bab_f_backsub8_update", st); hipLaunchKernelGGL(k_bab_f_backsub8_update, dim3((unsigned)g8, na), dim3(TB), 0, st, Dv); }
                { ProfScope ps("k_bab_errors", st); hipLaunchKernelGGL(k_bab_errors, YE, dim3(TB), 0, st, Dv); }
                hipLaunchKernelGGL(k_bab_decide, dim3(gw), dim3(64), 0, st, Dv, na);
                hipLaunchKernelGGL(k_bab_restore, YP, dim3(TB), 0, st, Dv);
                hipLaunchKernelGGL(k_bab_gate, YE, dim3(TB), 0, st, Dv, Ev);
                hipLaunchKernelGGL(k_bab_phase, dim3(gw), dim3(64), 0, st, Dv, na, d_done);
            }
            VIORB_HIP_TRY(hipGetLastError());
            VIORB_HIP_TRY(hipMemcpyAsync(h_done, d_done, sizeof(int), hipMemcpyDeviceToHost, st));
            VIORB_HIP_TRY(ba_wait(st, Sp.data(), na));
            done = *h_done;
            // the callers' stop flags: g2o polls pbStopFlag once per iteration and per trial; k_bab_decide does the same through the mirrored
            // words ba_wait keeps up to date, and the host marks the window here so that the next rounds skip its kernels altogether
            for (int a = 0; a < na; a++) {
                BaSolve& B = *S[act[a]];
                if (!aborted[a] && B.terminate()) {
                    aborted[a] = 1;
                    static const double one = 1.0;                 // static storage: outlives the asynchronous copy
                    VIORB_HIP_TRY(hipMemcpyAsync(B.D.ctl + BA_B_ABORT, &one, sizeof(double), hipMemcpyHostToDevice, st));
                }
            }
        }
        if (done < na) { set_error("window solve did not finish in %d rounds", MAX_ROUNDS); return VIORB_ERR_HIP; }
        // results: packed by one kernel into a group buffer on the device, ONE copy into page-locked memory, then plain memcpy into the callers'
        // (pageable) arrays
        {
            std::vector<unsigned long long> offs(4 * (size_t)na);
            size_t total = 0, max_ne = 1;
            auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
            for (int a = 0; a < na; a++) {
                const BaDev& Da = S[act[a]]->D;
                offs[4 * a] = total; total += up((size_t)Da.W * Da.kf_stride * sizeof(double));
                offs[4 * a + 1] = total; total += up((size_t)Da.NP * 3 * sizeof(double));
                offs[4 * a + 2] = total; total += up((size_t)Da.NE);
                offs[4 * a + 3] = total; total += up(sizeof(double) * BA_B_N);
                max_ne = std::max(max_ne, (size_t)std::max(Da.NE, std::max(Da.NP * 3, Da.W * Da.kf_stride)));
            }
            // grow-only buffers of the calling thread (hipMalloc / hipHostMalloc synchronise the device and take longer than a round)
            struct Bufs {
                void* dev = nullptr; void* host = nullptr; void* doffs = nullptr; size_t bytes = 0, noffs = 0; int device = -1;
                void drop() { if (dev) (void)hipFree(dev); if (host) (void)hipHostFree(host); if (doffs) (void)hipFree(doffs); dev = host = doffs = nullptr; bytes = noffs = 0; }
                ~Bufs() { drop(); }
            };
            static thread_local Bufs bufs;
            if (bufs.device != lba_device() || bufs.bytes < total || bufs.noffs < offs.size()) {
                bufs.drop(); bufs.device = lba_device();
                const size_t want = total + total / 4, wo = offs.size() + 64;
                VIORB_HIP_TRY(hipMalloc(&bufs.dev, want)); VIORB_HIP_TRY(hipHostMalloc(&bufs.host, want)); VIORB_HIP_TRY(hipMalloc(&bufs.doffs, wo * sizeof(unsigned long long)));
                bufs.bytes = want; bufs.noffs = wo;
            }
            VIORB_HIP_TRY(hipMemcpyAsync(bufs.doffs, offs.data(), offs.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_bab_pack, dim3((unsigned)std::min<size_t>((max_ne + TB - 1) / TB, 64), na), dim3(TB), 0, st, Dv, Ev, static_cast<uint8_t*>(bufs.dev),
                               static_cast<const unsigned long long*>(bufs.doffs));
            VIORB_HIP_TRY(hipGetLastError());
            VIORB_HIP_TRY(hipMemcpyAsync(bufs.host, bufs.dev, total, hipMemcpyDeviceToHost, st));
            VIORB_HIP_TRY(hipStreamSynchronize(st));
            const uint8_t* hb = static_cast<const uint8_t*>(bufs.host);
            for (int a = 0; a < na; a++) {
                BaSolve& B = *S[act[a]];
                memcpy(B.kfs_out, hb + offs[4 * a], (size_t)B.D.W * B.D.kf_stride * sizeof(double));
                memcpy(B.points_out, hb + offs[4 * a + 1], (size_t)B.D.NP * 3 * sizeof(double));
                memcpy(B.erase, hb + offs[4 * a + 2], (size_t)B.D.NE);
                ba_info_from_ctl(reinterpret_cast<const double*>(hb + offs[4 * a + 3]), B.info);
            }
        }
        return VIORB_OK;
        };
        const int grc = solve_group();
        if (grc != VIORB_OK) {
            for (int i : act) w[g0 + i].status = grc;
            for (int j = g0 + ng; j < n; j++) w[j].status = grc;
            return grc;
        }
    }
    return first_error;
}

extern "C" int viorb_local_ba_navstate_batch(viorb_lba_window* w, int n, int max_in_flight) {
    VIORB_REQUIRE(w && n >= 0, "null windows");
    return ba_run_lockstep(w, n, max_in_flight, [](BaSolve& S, viorb_lba_window& q) {
        return ba_prepare_navstate(S, q.kfs, q.nk, q.n_local, q.prev_kf, q.preint, q.points, q.np, q.edge_idx, q.edge_obs, q.ne, q.gw, q.cam, q.stop,
                                   q.kfs_out, q.points_out, q.erase, q.info);
    });
}

static int ba_prepare_se3(BaSolve& S, const double* kfs, int nk, int n_local, const double* points, int npts, const int32_t* edge_idx,
                          const double* edge_obs, int ne, const double intr5[5], const volatile int* stop, double* kfs_out,
                          double* points_out, uint8_t* erase, double info[6]) {
    VIORB_REQUIRE(kfs && points && edge_idx && edge_obs && intr5 && kfs_out && points_out && erase && info, "null array");
    VIORB_REQUIRE(n_local >= 1 && n_local <= 40 && nk >= n_local && npts >= 1 && ne >= 1, "1 <= n_local <= 40 key frames, at least one point and edge");
    VIORB_TRY(require_device());
    for (int i = 0; i < 6; i++) info[i] = 0;
    for (int i = 0; i < n_local * 7; i++) kfs_out[i] = kfs[i];
    for (int i = 0; i < npts * 3; i++) points_out[i] = points[i];
    for (int k = 0; k < ne; k++) erase[k] = 0;
    if (stop && *stop) { S.state = BaSolve::ST_DONE; return VIORB_OK; }
    std::vector<int> e_pt(ne), e_kf(ne), pt_start(npts + 1, 0);
    for (int k = 0; k < ne; k++) {
        e_pt[k] = edge_idx[2 * k]; e_kf[k] = edge_idx[2 * k + 1];
        VIORB_REQUIRE(e_pt[k] >= 0 && e_pt[k] < npts && e_kf[k] >= 0 && e_kf[k] < nk, "edge index out of range");
        VIORB_REQUIRE(k == 0 || e_pt[k] >= e_pt[k - 1], "edges must be grouped by point (ascending point index)");
        pt_start[e_pt[k] + 1]++;
    }
    for (int p = 0; p < npts; p++) pt_start[p + 1] += pt_start[p];
    std::vector<int> kf_start(n_local + 1, 0), kf_list;
    for (int k = 0; k < ne; k++) if (e_kf[k] < n_local) kf_start[e_kf[k] + 1]++;
    for (int i = 0; i < n_local; i++) kf_start[i + 1] += kf_start[i];
    kf_list.resize(kf_start[n_local]);
    { std::vector<int> pos(kf_start.begin(), kf_start.end() - 1); for (int k = 0; k < ne; k++) if (e_kf[k] < n_local) kf_list[pos[e_kf[k]]++] = k; }
    const size_t pr_bound = ba_pairs_bound(e_kf, pt_start, npts, n_local);
    VIORB_HIP_TRY(hipSetDevice(lba_device()));
    StreamCtxLease& lease = S.lease;
    if (!lease.ready()) { set_error("could not create a HIP stream"); return VIORB_ERR_HIP; }
    BaBuf B; BaDev& D = S.D;
    D.W = n_local; D.NK = nk; D.NP = npts; D.NE = ne; D.np = 6 * n_local; D.prev_kf = -1; D.acc_bias_rw2 = 0;
    D.pose_dim = 6; D.rows = 3; D.kf_stride = 7;
    for (int i = 0; i < 16; i++) D.cam[i] = i < 5 ? intr5[i] : 0.0;
    for (int i = 0; i < 3; i++) D.gw[i] = 0;
    D.ld = (D.np + 15) & ~15;
    const size_t n2 = (size_t)D.np * D.np, nl2 = (size_t)D.ld * D.ld;
    int *d_ept, *d_ekf, *d_pts, *d_kfs, *d_kfl; double* d_obs; uint8_t* d_erase;
    D.preint = nullptr; D.info_pvr = nullptr; D.e_pvr = nullptr; D.e_b = nullptr;
    bool ok = B.alloc(&D.kf, (size_t)nk * 7, kfs) && B.alloc_raw(&D.kf_bak, (size_t)nk * 7) && B.alloc(&D.pt, (size_t)npts * 3, points) && B.alloc_raw(&D.pt_bak, (size_t)npts * 3) &&
              B.alloc(&d_ept, ne, e_pt.data()) && B.alloc(&d_ekf, ne, e_kf.data()) && B.alloc(&d_obs, (size_t)ne * 4, edge_obs) && B.alloc(&D.level, ne) &&
              B.alloc_raw(&D.err, (size_t)ne * 3) && B.alloc_raw(&D.Jp, (size_t)ne * 9) && B.alloc_raw(&D.Jk, (size_t)ne * 18) && B.alloc_raw(&D.wgt, ne) && B.alloc_raw(&D.We, (size_t)ne * 18) &&
              B.alloc(&D.pr_start, (size_t)n_local * (n_local + 1) / 2 + 1) && B.alloc_raw(&D.pr_ent, 2 * pr_bound + 2) &&
              B.alloc(&d_pts, npts + 1, pt_start.data()) && B.alloc(&d_kfs, n_local + 1, kf_start.data()) && B.alloc(&d_kfl, kf_list.size(), kf_list.data()) &&
              B.alloc_raw(&D.Hll, (size_t)npts * 9) && B.alloc_raw(&D.bl, (size_t)npts * 3) && B.alloc_raw(&D.Dinv, (size_t)npts * 9) &&
              B.alloc_raw(&D.Hpp, n2) && B.alloc(&D.bp, D.np) && B.alloc(&D.S, nl2 + (size_t)16 * D.ld + (size_t)(D.ld / 16) * 256) && B.alloc(&D.bs, D.ld) && B.alloc(&D.xp, D.ld) &&
              B.alloc_raw(&D.db, (size_t)npts * 3) && B.alloc_raw(&D.xl, (size_t)npts * 3) && B.alloc(&D.scal, 8) && B.alloc(&D.ctl, (size_t)BA_CTL_N) && B.alloc(&D.ticket, 1) && B.alloc(&d_erase, ne) && B.commit(lease.c);
    if (!ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    D.e_pt = d_ept; D.e_kf = d_ekf; D.e_obs = d_obs; D.pt_start = d_pts; D.kf_start = d_kfs; D.kf_list = d_kfl;
    S.st = lease.c->st; S.h = lease.c->pinned; S.model = 1; S.stop = stop; S.d_erase = d_erase;
    VIORB_HIP_TRY(ba_map_stop_flag(S));
    S.kfs_out = kfs_out; S.points_out = points_out; S.erase = erase; S.info = info;
    return VIORB_OK;
}

extern "C" int viorb_local_ba_se3(const double* kfs, int nk, int n_local, const double* points, int npts, const int32_t* edge_idx,
                                  const double* edge_obs, int ne, const double intr5[5], const volatile int* stop, double* kfs_out,
                                  double* points_out, uint8_t* erase, double info[6]) {
    BaSolve S;
    const int rc = ba_prepare_se3(S, kfs, nk, n_local, points, npts, edge_idx, edge_obs, ne, intr5, stop, kfs_out, points_out, erase, info);
    return rc != VIORB_OK ? rc : S.run();
}

extern "C" int viorb_local_ba_se3_batch(viorb_lba_se3_window* w, int n, int max_in_flight) {
    VIORB_REQUIRE(w && n >= 0, "null windows");
    return ba_run_lockstep(w, n, max_in_flight, [](BaSolve& S, viorb_lba_se3_window& q) {
        return ba_prepare_se3(S, q.kfs, q.nk, q.n_local, q.points, q.np, q.edge_idx, q.edge_obs, q.ne, q.intr5, q.stop, q.kfs_out, q.points_out, q.erase, q.info);
    });
}
