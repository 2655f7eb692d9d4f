// viorb_amd/csrc/sim3.hip — the Sim3 RANSAC solver on the device: Sim3Solver::iterate and everything beneath it (reference
// src/Sim3Solver.cc:37-423) for a batch of independent key-frame pairs. The arithmetic is sim3_core.h.
//   k_sim3_prepare      one lane per correspondence: the two fixed projections (FromCameraToImage) and the two truncated thresholds,
//                       packed with the points into three float4 arrays so that the inlier kernel loads coalesce
//   k_sim3_hypotheses   one lane per (pair, iteration): Horn's closed form from the three correspondences of a set (the 4 x 4 Jacobi in
//                       double registers), a reason per set
//   k_sim3_inliers      one wavefront per (pair, iteration): 64 lanes stride over the correspondences, both reprojections, count by
//                       ballot; inlier flags only on request (the returned model, or every hypothesis for the stage entry)
//   k_sim3_select       one wavefront per pair: the acceptance rule of iterate over the counts in iteration order, 64 at a time, by a
//                       running maximum and first-set-lane; writes the model of the last best update
// viorb_sim3_ransac_device launches them in this order on one stream; the stage entries launch the same kernels.
#include <math.h>
#include <vector>
#include "viorb_common.h"
#include "sim3_core.h"
#include "lm_core.h"

namespace viorb {

struct S3Work {          // the workspace arrays (s3_layout below)
    float4 *pa, *pb, *pc;           // [b][cap]: X1c p1u | X2c p1v | p2u p2v max1 max2
    float *R, *t, *s;               // [b][it][9], [b][it][3], [b][it]
    int *reason, *counts;           // [b][it]
    int *status, *done, *best, *best_it;      // [b]
};

__device__ __forceinline__ int s3_n(const viorb_sim3_inputs& I, int b) { return min(max(I.n[b], 0), I.cap); }
__device__ __forceinline__ Sim3K s3_k(const float* K, int b) { Sim3K k; k.fx = K[4 * b]; k.fy = K[4 * b + 1]; k.cx = K[4 * b + 2]; k.cy = K[4 * b + 3]; return k; }

// The iterations one call of iterate can reach: [first, min(first + per_call, max_its)). first == NULL (the stage entries): all of them.
struct S3Window { const int *first, *max_its; int per_call; };
__device__ __forceinline__ bool s3_in_window(const S3Window& w, int b, int it) {
    if (!w.first) return true;
    const int start = max(w.first[b], 0);
    return it >= start && (long long)it < (long long)start + w.per_call && it < w.max_its[b];
}

__global__ __launch_bounds__(256) void k_sim3_prepare(viorb_sim3_inputs I, S3Work W) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s3_n(I, b)) return;
    const size_t o = (size_t)b * I.cap + i;
    const float* X1 = I.X1c + o * 3; const float* X2 = I.X2c + o * 3;
    float u1, v1, u2, v2;
    sim3_to_image(s3_k(I.K1, b), X1[0], X1[1], X1[2], u1, v1);
    sim3_to_image(s3_k(I.K2, b), X2[0], X2[1], X2[2], u2, v2);
    W.pa[o] = make_float4(X1[0], X1[1], X1[2], u1);
    W.pb[o] = make_float4(X2[0], X2[1], X2[2], v1);
    W.pc[o] = make_float4(u2, v2, sim3_max_error(I.sigma2_1[o]), sim3_max_error(I.sigma2_2[o]));
}

struct S3HypArgs { viorb_sim3_inputs I; S3Work W; S3Window win; const int* sets; float *R, *t, *s; int* reason; int iters, min_inliers, fix_scale; };

__global__ __launch_bounds__(64) void k_sim3_hypotheses(S3HypArgs A) {
    const int b = blockIdx.y, it = blockIdx.x * 64 + threadIdx.x;
    if (it >= A.iters || !s3_in_window(A.win, b, it)) return;
    const size_t m = (size_t)b * A.iters + it;
    const int N = s3_n(A.I, b);
    float R[9], t[3], s = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = 0.0f;
    t[0] = t[1] = t[2] = 0.0f;
    int reason = SIM3_SET_OK;
    if (N < A.min_inliers || N < 3) reason = SIM3_SET_FEW;
    else {
        const int i0 = A.sets[m * 3], i1 = A.sets[m * 3 + 1], i2 = A.sets[m * 3 + 2];
        if (i0 < 0 || i0 >= N || i1 < 0 || i1 >= N || i2 < 0 || i2 >= N || i0 == i1 || i0 == i2 || i1 == i2) reason = SIM3_SET_BAD;
        else {
            const size_t o = (size_t)b * A.I.cap;
            const float4 a0 = A.W.pa[o + i0], a1 = A.W.pa[o + i1], a2 = A.W.pa[o + i2];
            const float4 b0 = A.W.pb[o + i0], b1 = A.W.pb[o + i1], b2 = A.W.pb[o + i2];
            const float P1[3][3] = {{a0.x, a0.y, a0.z}, {a1.x, a1.y, a1.z}, {a2.x, a2.y, a2.z}};
            const float P2[3][3] = {{b0.x, b0.y, b0.z}, {b1.x, b1.y, b1.z}, {b2.x, b2.y, b2.z}};
            reason = sim3_horn(P1, P2, A.fix_scale != 0, R, t, s);
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) A.R[m * 9 + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) A.t[m * 3 + k] = t[k];
    A.s[m] = s;
    A.reason[m] = reason;
}

// which == NULL: hypothesis blockIdx.x of every pair, counts [b][it]. which != NULL: hypothesis which[b] where status[b] is FOUND (no
// model otherwise: zero flags and a zero count), the count to n_inliers [b].
struct S3InlArgs {
    viorb_sim3_inputs I; S3Work W; S3Window win; const float *R, *t, *s; const int *which, *status; int* counts; int* n_inliers; uint8_t* flags;
    size_t flag_stride_b, flag_stride_it; int iters;
};

__global__ __launch_bounds__(64) void k_sim3_inliers(S3InlArgs A) {
    const int b = blockIdx.y, lane = threadIdx.x;
    const bool one = A.which != nullptr;
    const int it = one ? A.which[b] : (int)blockIdx.x;
    if (!one && !s3_in_window(A.win, b, it)) return;
    const bool run = !one || (it >= 0 && it < A.iters && A.status[b] == SIM3_FOUND);
    const int N = run ? s3_n(A.I, b) : 0;
    uint8_t* flags = A.flags ? A.flags + (size_t)b * A.flag_stride_b + (one ? 0 : (size_t)it * A.flag_stride_it) : nullptr;
    const size_t m = (size_t)b * A.iters + (run ? it : 0);
    Sim3Pair T = Sim3Pair();
    if (run) sim3_transforms(A.R + m * 9, A.t + m * 3, A.s[m], T);        // without a model nothing of the workspace is read
    const Sim3K k1 = s3_k(A.I.K1, b), k2 = s3_k(A.I.K2, b);
    const size_t o = (size_t)b * A.I.cap;
    int cnt = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < N) {
            const float4 a = A.W.pa[o + i], q = A.W.pb[o + i], c = A.W.pc[o + i];
            const float X1[3] = {a.x, a.y, a.z}, X2[3] = {q.x, q.y, q.z};
            float e1, e2;
            in = sim3_is_inlier(k1, k2, T, X1, X2, a.w, q.w, c.x, c.y, c.z, c.w, e1, e2);
            if (flags) flags[i] = in;
        }
        cnt += __popcll(__ballot(in));
    }
    if (flags) for (int i = N + lane; i < A.I.cap; i += 64) flags[i] = 0;
    if (lane == 0) {
        if (!one) A.counts[m] = cnt;
        else if (A.n_inliers) A.n_inliers[b] = cnt;
    }
}

struct S3SelArgs {
    const int *counts, *n, *max_its, *first, *best_in; int iters, min_inliers, per_call, cap;
    int *status, *done, *best, *best_it;        // required (the workspace's where the caller gave none)
    const float *R, *t, *s;                      // NULL: no model outputs
    float *o_R, *o_t, *o_s, *o_T;
};

__global__ __launch_bounds__(64) void k_sim3_select(S3SelArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N = min(max(A.n[b], 0), A.cap), first = A.first[b], max_its = A.max_its[b];
    int best = A.best_in[b], best_it = -1, found = -1, status = SIM3_FEW, done = first;
    if (N >= A.min_inliers) {
        const int start = max(first, 0);
        const long long lim = (long long)start + A.per_call;
        const int end = (int)min((long long)min(max_its, A.iters), lim);
        for (int base = start; base < end && found < 0; base += 64) {
            const int i = base + lane;
            const int c = i < end ? A.counts[(size_t)b * A.iters + i] : -1;
            int pm = c;                                   // inclusive running maximum over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(pm, d); if (lane >= d) pm = max(pm, o); }
            const int prev = __shfl_up(pm, 1);
            const int before = lane > 0 ? max(best, prev) : best;      // mnBestInliers when iteration i begins
            const bool upd = i < end && c >= before;
            const unsigned long long hit = __ballot(upd && c > A.min_inliers), up = __ballot(upd);
            if (hit) {
                const int f = __ffsll((long long)hit) - 1;
                found = base + f; best_it = found; best = __shfl(c, f);
            } else {
                if (up) best_it = base + 63 - __clzll((long long)up);
                best = max(best, __shfl(pm, 63));
            }
        }
        done = found >= 0 ? found + 1 : max(end, start);
        status = found >= 0 ? SIM3_FOUND : (done >= max_its ? SIM3_NO_MORE : SIM3_CONTINUE);
    }
    if (lane == 0) { A.status[b] = status; A.done[b] = done; A.best[b] = best; A.best_it[b] = best_it; }
    if (!A.R) return;
    const size_t m = (size_t)b * A.iters + max(best_it, 0);
    const bool have = best_it >= 0;
    if (lane < 9 && A.o_R) A.o_R[(size_t)b * 9 + lane] = have ? A.R[m * 9 + lane] : 0.0f;
    if (lane < 3 && A.o_t) A.o_t[(size_t)b * 3 + lane] = have ? A.t[m * 3 + lane] : 0.0f;
    if (lane == 0 && A.o_s) A.o_s[b] = have ? A.s[m] : 0.0f;
    if (lane == 0 && A.o_T) {
        float T16[16];
#pragma unroll
        for (int k = 0; k < 16; k++) T16[k] = 0.0f;
        if (have) sim3_T12(A.R + m * 9, A.t + m * 3, A.s[m], T16);
#pragma unroll
        for (int k = 0; k < 16; k++) A.o_T[(size_t)b * 16 + k] = T16[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Optimizer::OptimizeSim3 (reference src/Optimizer.cc:4589-4784): one 7-DoF VertexSim3Expmap over two projection edges per correspondence,
// g2o Levenberg with Huber, optimize(5), outlier removal, optimize(5 or 10). One workgroup of 256 per pair, structured like
// k_pose_opt_se3. The edges define no linearizeOplus, so g2o differentiates numerically (central differences, delta = 1e-9, through
// oplus on the Sim3 vertex): the 14 perturbed estimates and their inverses are uniform per problem and are computed once per
// linearisation into LDS by 14 lanes; every edge then takes 15 projections. The 7 x 7 system is factorised by one lane in LDS.
struct S3OptArgs { viorb_sim3_opt_inputs I; double th2, delta; int fix_scale; double* S_out; uint8_t* keep; int* n_in; double* info; };
struct S3OptShared {
    double H[49], L[49], b[7], x[7], y[7], red[4][36], est[8], esti[8], bak[8], ev[8], evi[8], P[14][8], Pi[14][8], sc[4];
    int flag[4];
};

__device__ bool s3_chol7(const double* H, const double* b, double lambda, double* L, double* y, double* x) {
    for (int i = 0; i < 7; i++)
        for (int j = 0; j <= i; j++) {
            double v = H[i * 7 + j] + (i == j ? lambda : 0.0);
            for (int k = 0; k < j; k++) v -= L[i * 7 + k] * L[j * 7 + k];
            if (i == j) { if (!(v > 0.0) || !isfinite(v)) return false; L[i * 7 + i] = sqrt(v); }
            else L[i * 7 + j] = v / L[j * 7 + j];
        }
    for (int i = 0; i < 7; i++) { double v = b[i]; for (int k = 0; k < i; k++) v -= L[i * 7 + k] * y[k]; y[i] = v / L[i * 7 + i]; }
    for (int i = 6; i >= 0; i--) { double v = y[i]; for (int k = i + 1; k < 7; k++) v -= L[k * 7 + i] * x[k]; x[i] = v / L[i * 7 + i]; }
    return true;
}

__global__ __launch_bounds__(256) void k_sim3_optimize(S3OptArgs A) {
    __shared__ S3OptShared S;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, cap = A.I.cap;
    const int n = min(max(A.I.n[b], 0), cap);
    const size_t o = (size_t)b * cap;
    const float *X1 = A.I.X1c + o * 3, *X2 = A.I.X2c + o * 3, *ob1 = A.I.obs1 + o * 2, *ob2 = A.I.obs2 + o * 2;
    const float *is1 = A.I.inv_sigma2_1 + o, *is2 = A.I.inv_sigma2_2 + o;
    uint8_t* keep = A.keep + o;
    const bool fix = A.fix_scale != 0;
    const double K1[4] = {(double)A.I.K1[4 * b], (double)A.I.K1[4 * b + 1], (double)A.I.K1[4 * b + 2], (double)A.I.K1[4 * b + 3]};
    const double K2[4] = {(double)A.I.K2[4 * b], (double)A.I.K2[4 * b + 1], (double)A.I.K2[4 * b + 2], (double)A.I.K2[4 * b + 3]};
    const double* S0 = A.I.S12 + (size_t)b * 8;
    int ncorr_l = 0;
    for (int i = t; i < cap; i += 256) { const uint8_t v = i < n && A.I.valid[o + i] != 0; keep[i] = v; ncorr_l += v; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) ncorr_l += __shfl_xor(ncorr_l, d);
    if (t == 0) { S.flag[1] = 0; S.flag[2] = 0; S.flag[3] = 0; }
    if (t < 8) S.est[t] = S0[t];
    __syncthreads();
    if (lane == 0) atomicAdd(&S.flag[3], ncorr_l);
    __syncthreads();
    const int ncorr = S.flag[3];
    double* inf = A.info + (size_t)b * 8;
    if (ncorr == 0) {                                   // an empty graph: nothing to optimise, nothing to count
        if (t < 8) { A.S_out[(size_t)b * 8 + t] = S0[t]; inf[t] = 0; }
        if (t == 0) A.n_in[b] = 0;
        return;
    }
    const double d_huber = (double)(float)sqrt((float)A.th2);           // const float deltaHuber = sqrt(th2) (:4638), both rounds
    const double scalar = 1 / (2 * A.delta);
    auto evaluate = [&](bool lin) -> double {
        if (lin && t < 14) { const sim3d p = sim3_perturbed(sim3_ld(S.est), t, fix); sim3_st(S.P[t], p); sim3_st(S.Pi[t], sim3_inv(p)); }
        if (t == 14) sim3_st(S.esti, sim3_inv(sim3_ld(S.est)));
        __syncthreads();
        const sim3d s12 = sim3_ld(S.est), s21 = sim3_ld(S.esti);
        double a[36];
#pragma unroll
        for (int k = 0; k < 36; k++) a[k] = 0;
        for (int i = t; i < n; i += 256) {
            if (!keep[i]) continue;
            const d3 x1 = mk3((double)X1[3 * i], (double)X1[3 * i + 1], (double)X1[3 * i + 2]), x2 = mk3((double)X2[3 * i], (double)X2[3 * i + 1], (double)X2[3 * i + 2]);
#pragma unroll
            for (int edge = 0; edge < 2; edge++) {
                const double u = edge == 0 ? (double)ob1[2 * i] : (double)ob2[2 * i], v = edge == 0 ? (double)ob1[2 * i + 1] : (double)ob2[2 * i + 1];
                const double w0 = edge == 0 ? (double)is1[i] : (double)is2[i];
                const d3 X = edge == 0 ? x2 : x1;
                const double* K = edge == 0 ? K1 : K2;
                double e[2];
                sim3_edge_error(edge == 0 ? s12 : s21, X, K, u, v, e);
                const double chi = w0 * (e[0] * e[0] + e[1] * e[1]);
                double r0, r1;
                huber(chi, d_huber, &r0, &r1);
                a[35] += r0;
                if (lin) {
                    double J[14];
#pragma unroll
                    for (int d = 0; d < 7; d++) {
                        double ep[2], em[2];
                        sim3_edge_error(sim3_ld(edge == 0 ? S.P[2 * d] : S.Pi[2 * d]), X, K, u, v, ep);
                        sim3_edge_error(sim3_ld(edge == 0 ? S.P[2 * d + 1] : S.Pi[2 * d + 1]), X, K, u, v, em);
                        J[d] = scalar * (ep[0] - em[0]); J[7 + d] = scalar * (ep[1] - em[1]);
                    }
                    const double w = r1 * w0;
                    int k = 0;
#pragma unroll
                    for (int r = 0; r < 7; r++)
#pragma unroll
                        for (int c = r; c < 7; c++) a[k++] += w * (J[r] * J[c] + J[7 + r] * J[7 + c]);
#pragma unroll
                    for (int r = 0; r < 7; r++) a[28 + r] -= w * (J[r] * e[0] + J[7 + r] * e[1]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 36; k++) {
            if (!lin && k != 35) continue;
            double v = a[k];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
            if (lane == 0) S.red[wave][k] = v;
        }
        __syncthreads();
        if (lin && t < 35) {
            const double v = S.red[0][t] + S.red[1][t] + S.red[2][t] + S.red[3][t];
            if (t < 28) {
                int kk = 0, rr = 0, cc = 0;
                for (int r = 0; r < 7; r++) for (int c = r; c < 7; c++) { if (kk == t) { rr = r; cc = c; } kk++; }
                S.H[rr * 7 + cc] = v; S.H[cc * 7 + rr] = v;
            } else S.b[t - 28] = v;
        }
        if (t == 35) S.sc[0] = S.red[0][35] + S.red[1][35] + S.red[2][35] + S.red[3][35];
        __syncthreads();
        return S.sc[0];
    };
    int nbad = 0, its_done[2] = {0, 0};
    double chi_round[2] = {0, 0};
    for (int round = 0; round < 2; round++) {
        const int max_it = round == 0 ? 5 : (nbad > 0 ? 10 : 5);
        double lambda = 0, ni = 2; int nBadLM = 0, its = 0;
        for (int it = 0; it < max_it; it++) {
            double currentChi = evaluate(true);
            const double iniChi = currentChi;
            if (it == 0) { double mx = 0; for (int i = 0; i < 7; i++) mx = fmax(fabs(S.H[i * 8]), mx); lambda = lm_lambda_init(mx); ni = 2; nBadLM = 0; }
            double rho = 0; int qmax = 0;
            do {
                if (t < 8) S.bak[t] = S.est[t];
                if (t == 0) {
                    const bool ok = s3_chol7(S.H, S.b, lambda, S.L, S.y, S.x);
                    if (!ok) for (int k = 0; k < 7; k++) S.x[k] = 0;
                    if (fix) S.x[6] = 0;                             // oplusImpl zeroes the caller's update[6] in place
                    S.flag[0] = ok ? 1 : 0;
                    sim3_st(S.est, sim3_oplus(sim3_ld(S.est), S.x, fix));
                }
                __syncthreads();
                const int ok2 = S.flag[0];
                if (t < 8) S.ev[t] = S.est[t];
                const double tempChi = lm_trial_chi2(ok2, evaluate(false));
                rho = lm_rho(currentChi, tempChi, lm_scale<7>(S.x, S.b, lambda));
                const bool rejected = !lm_accepted(rho, tempChi);
                if (!rejected) { lm_good_step(lambda, ni, lm_cube_pow(2 * rho - 1)); currentChi = tempChi; }
                else { lm_bad_step(lambda, ni); if (t < 8) S.est[t] = S.bak[t]; }
                if (t == 0) S.flag[rejected ? 2 : 1]++;
                __syncthreads();
                qmax++;
            } while (lm_retry(rho, qmax));
            its++;
            chi_round[round] = currentChi;
            if (lm_iteration_stops(rho, qmax, iniChi, currentChi, nBadLM)) break;
        }
        its_done[round] = its;
        // e->chi2() reads the error of the last computeActiveErrors, the last trial's state: stale after a rejected last trial
        if (t == 0) { sim3_st(S.evi, sim3_inv(sim3_ld(S.ev))); S.flag[3] = 0; }
        __syncthreads();
        const sim3d e12s = sim3_ld(S.ev), e21s = sim3_ld(S.evi);
        int cnt = 0;
        for (int i = t; i < n; i += 256) {
            if (!keep[i]) continue;
            double e1[2], e2[2];
            sim3_edge_error(e12s, mk3((double)X2[3 * i], (double)X2[3 * i + 1], (double)X2[3 * i + 2]), K1, (double)ob1[2 * i], (double)ob1[2 * i + 1], e1);
            sim3_edge_error(e21s, mk3((double)X1[3 * i], (double)X1[3 * i + 1], (double)X1[3 * i + 2]), K2, (double)ob2[2 * i], (double)ob2[2 * i + 1], e2);
            const bool bad = (double)is1[i] * (e1[0] * e1[0] + e1[1] * e1[1]) > A.th2 || (double)is2[i] * (e2[0] * e2[0] + e2[1] * e2[1]) > A.th2;
            if (bad) keep[i] = 0;
            cnt += round == 0 ? (int)bad : (int)!bad;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
        if (lane == 0) atomicAdd(&S.flag[3], cnt);
        __syncthreads();
        const int total = S.flag[3];
        __syncthreads();
        if (round == 0) {
            nbad = total;
            if (ncorr - nbad < 10) {                     // :4754: returns 0 with g2oS12 unchanged; the removals above stay
                if (t < 8) A.S_out[(size_t)b * 8 + t] = S0[t];
                if (t == 0) {
                    A.n_in[b] = 0;
                    inf[0] = ncorr; inf[1] = nbad; inf[2] = its_done[0]; inf[3] = 0; inf[4] = chi_round[0]; inf[5] = 0; inf[6] = S.flag[1]; inf[7] = S.flag[2];
                }
                return;
            }
        } else if (t == 0) A.n_in[b] = total;
    }
    if (t < 8) A.S_out[(size_t)b * 8 + t] = S.est[t];
    if (t == 0) {
        inf[0] = ncorr; inf[1] = nbad; inf[2] = its_done[0]; inf[3] = its_done[1]; inf[4] = chi_round[0]; inf[5] = chi_round[1]; inf[6] = S.flag[1]; inf[7] = S.flag[2];
    }
}

} // namespace viorb

using namespace viorb;

namespace {

struct S3Layout { S3Work W; size_t total; };
S3Layout s3_layout(void* base, int cap, int iters, int batch) {
    S3Layout L; WorkspaceLayout Y(base); S3Work& W = L.W;
    const size_t B = (size_t)batch, n = B * cap, m = B * iters;
    Y.take(&W.pa, n); Y.take(&W.pb, n); Y.take(&W.pc, n);
    Y.take(&W.R, m * 9); Y.take(&W.t, m * 3); Y.take(&W.s, m); Y.take(&W.reason, m); Y.take(&W.counts, m);
    Y.take(&W.status, B); Y.take(&W.done, B); Y.take(&W.best, B); Y.take(&W.best_it, B);
    L.total = Y.end();
    return L;
}

bool s3_sizes_ok(int cap, int iterations, int batch) { return cap >= 1 && iterations >= 1 && iterations <= 4096 && batch >= 1 && batch <= 65535; }

int s3_check_cfg(const viorb_sim3_config* cfg, int batch) {
    VIORB_REQUIRE(cfg && cfg->iterations >= 1 && cfg->iterations <= 4096 && cfg->iterations_per_call >= 1 && cfg->min_inliers >= 1,
                  "config: 1 <= iterations <= 4096, iterations_per_call >= 1, min_inliers >= 1");
    VIORB_REQUIRE(batch >= 1 && batch <= 65535, "1 <= batch <= 65535");
    return VIORB_OK;
}

int s3_check_common(const viorb_sim3_inputs* in, const viorb_sim3_config* cfg, int batch, void* workspace, size_t workspace_bytes) {
    VIORB_TRY(s3_check_cfg(cfg, batch));
    VIORB_REQUIRE(in && in->X1c && in->X2c && in->sigma2_1 && in->sigma2_2 && in->K1 && in->K2 && in->n && workspace, "null array");
    VIORB_REQUIRE(in->cap >= 1, "cap >= 1");
    VIORB_REQUIRE(workspace_bytes >= s3_layout(nullptr, in->cap, cfg->iterations, batch).total && ((uintptr_t)workspace & 255) == 0,
                  "workspace smaller than viorb_sim3_workspace_bytes or not 256-byte aligned");
    return VIORB_OK;
}

int launch_prepare(const viorb_sim3_inputs& I, const S3Work& W, int batch, hipStream_t st) {
    VIORB_LAUNCH(k_sim3_prepare, dim3((I.cap + 255) / 256, batch), 256, 0, st, I, W);
    return VIORB_OK;
}
int launch_hypotheses(const viorb_sim3_inputs& I, const S3Work& W, const S3Window& win, const viorb_sim3_config* cfg, const int32_t* sets, float* R, float* t,
                      float* s, int32_t* reason, int batch, hipStream_t st) {
    S3HypArgs A; A.I = I; A.W = W; A.win = win; A.sets = sets; A.R = R; A.t = t; A.s = s; A.reason = reason; A.iters = cfg->iterations;
    A.min_inliers = cfg->min_inliers; A.fix_scale = cfg->fix_scale;
    VIORB_LAUNCH(k_sim3_hypotheses, dim3((cfg->iterations + 63) / 64, batch), 64, 0, st, A);
    return VIORB_OK;
}
int launch_inliers(const viorb_sim3_inputs& I, const S3Work& W, const S3Window& win, const viorb_sim3_config* cfg, const float* R, const float* t, const float* s,
                   const int* which, const int* status, int32_t* counts, int32_t* n_inliers, uint8_t* flags, size_t stride_b, size_t stride_it,
                   int batch, hipStream_t st) {
    S3InlArgs A; A.I = I; A.W = W; A.win = win; A.R = R; A.t = t; A.s = s; A.which = which; A.status = status; A.counts = counts; A.n_inliers = n_inliers;
    A.flags = flags; A.flag_stride_b = stride_b; A.flag_stride_it = stride_it; A.iters = cfg->iterations;
    VIORB_LAUNCH(k_sim3_inliers, dim3(which ? 1 : cfg->iterations, batch), 64, 0, st, A);
    return VIORB_OK;
}

uint64_t splitmix64(uint64_t& state) {
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

bool set_ok(const int32_t* s, int n) {
    for (int j = 0; j < 3; j++) {
        if (s[j] < 0 || s[j] >= n) return false;
        for (int k = 0; k < j; k++) if (s[k] == s[j]) return false;
    }
    return true;
}
} // namespace

extern "C" {

int viorb_sim3_draw_sets(int n, int iterations, uint64_t seed, int32_t* sets) {
    VIORB_REQUIRE(sets && n >= 3 && iterations >= 1, "sets != NULL, n >= 3, iterations >= 1");
    std::vector<int32_t> avail((size_t)n);
    uint64_t state = seed;
    for (int it = 0; it < iterations; it++) {
        for (int i = 0; i < n; i++) avail[i] = i;
        int left = n;
        for (int j = 0; j < 3; j++) {
            int r = (int)((double)(splitmix64(state) >> 11) * (1.0 / 9007199254740992.0) * (double)left);
            if (r >= left) r = left - 1;
            sets[(size_t)it * 3 + j] = avail[r];
            avail[r] = avail[left - 1];
            left--;
        }
    }
    return VIORB_OK;
}

int viorb_sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations) {
    VIORB_REQUIRE(n >= 1 && min_inliers >= 1 && max_iterations >= 1 && probability > 0 && probability < 1,
                  "n >= 1, min_inliers >= 1, max_iterations >= 1, 0 < probability < 1");
    const float epsilon = (float)min_inliers / n;
    int its = max_iterations;
    if (min_inliers == n) its = 1;
    else {
        const double v = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3)));
        if (v < (double)max_iterations) its = (int)v;          // false for a NaN (n < min_inliers) and for +inf
    }
    return std::max(1, std::min(its, max_iterations));
}

size_t viorb_sim3_workspace_bytes(int cap, int iterations, int batch) {
    if (!s3_sizes_ok(cap, iterations, batch)) return 0;
    return s3_layout(nullptr, cap, iterations, batch).total;
}

int viorb_sim3_hypotheses_device(const viorb_sim3_inputs* in, const viorb_sim3_config* cfg, const int32_t* d_sets, int batch, float* d_R12,
                                 float* d_t12, float* d_s12, int32_t* d_reason, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(s3_check_common(in, cfg, batch, workspace, workspace_bytes));
    VIORB_REQUIRE(d_sets && d_R12 && d_t12 && d_s12 && d_reason, "null array");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const S3Work W = s3_layout(workspace, in->cap, cfg->iterations, batch).W;
    VIORB_TRY(launch_prepare(*in, W, batch, st));
    return launch_hypotheses(*in, W, S3Window{nullptr, nullptr, 0}, cfg, d_sets, d_R12, d_t12, d_s12, d_reason, batch, st);
}

int viorb_sim3_inliers_device(const viorb_sim3_inputs* in, const viorb_sim3_config* cfg, int batch, const float* d_R12, const float* d_t12,
                              const float* d_s12, int32_t* d_counts, uint8_t* d_flags, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(s3_check_common(in, cfg, batch, workspace, workspace_bytes));
    VIORB_REQUIRE(d_R12 && d_t12 && d_s12 && d_counts, "null array");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const S3Work W = s3_layout(workspace, in->cap, cfg->iterations, batch).W;
    VIORB_TRY(launch_prepare(*in, W, batch, st));
    return launch_inliers(*in, W, S3Window{nullptr, nullptr, 0}, cfg, d_R12, d_t12, d_s12, nullptr, nullptr, d_counts, nullptr, d_flags, (size_t)cfg->iterations * in->cap,
                          (size_t)in->cap, batch, st);
}

int viorb_sim3_select_device(const viorb_sim3_config* cfg, const int32_t* d_counts, const int32_t* d_n, const int32_t* d_max_its,
                             const int32_t* d_first_iteration, const int32_t* d_best_inliers_in, int batch, int32_t* d_status,
                             int32_t* d_iterations_done, int32_t* d_best_inliers, int32_t* d_best_iter, void* stream) {
    VIORB_TRY(s3_check_cfg(cfg, batch));
    VIORB_REQUIRE(d_counts && d_n && d_max_its && d_first_iteration && d_best_inliers_in && d_status && d_iterations_done && d_best_inliers && d_best_iter,
                  "null array");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    S3SelArgs A; A.counts = d_counts; A.n = d_n; A.max_its = d_max_its; A.first = d_first_iteration; A.best_in = d_best_inliers_in;
    A.iters = cfg->iterations; A.min_inliers = cfg->min_inliers; A.per_call = cfg->iterations_per_call; A.cap = 0x7fffffff;      // the stage entry has no capacity to clamp n[b] to
    A.status = d_status; A.done = d_iterations_done; A.best = d_best_inliers; A.best_it = d_best_iter;
    A.R = A.t = A.s = nullptr; A.o_R = A.o_t = A.o_s = A.o_T = nullptr;
    VIORB_LAUNCH(k_sim3_select, batch, 64, 0, st, A);
    return VIORB_OK;
}

int viorb_sim3_ransac_device(const viorb_sim3_inputs* in, const viorb_sim3_config* cfg, const int32_t* d_sets, const int32_t* d_max_its,
                             const int32_t* d_first_iteration, const int32_t* d_best_inliers_in, int batch, const viorb_sim3_outputs* out,
                             void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(s3_check_common(in, cfg, batch, workspace, workspace_bytes));
    VIORB_REQUIRE(d_sets && d_max_its && d_first_iteration && d_best_inliers_in && out && out->status, "null array (status is required)");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const S3Work W = s3_layout(workspace, in->cap, cfg->iterations, batch).W;
    VIORB_TRY(launch_prepare(*in, W, batch, st));
    const S3Window win = {d_first_iteration, d_max_its, cfg->iterations_per_call};       // iterations no pair can reach this call are skipped
    VIORB_TRY(launch_hypotheses(*in, W, win, cfg, d_sets, W.R, W.t, W.s, W.reason, batch, st));
    VIORB_TRY(launch_inliers(*in, W, win, cfg, W.R, W.t, W.s, nullptr, nullptr, W.counts, nullptr, nullptr, 0, 0, batch, st));
    S3SelArgs A; A.counts = W.counts; A.n = in->n; A.max_its = d_max_its; A.first = d_first_iteration; A.best_in = d_best_inliers_in;
    A.iters = cfg->iterations; A.min_inliers = cfg->min_inliers; A.per_call = cfg->iterations_per_call; A.cap = in->cap;
    A.status = out->status; A.done = out->iterations_done ? out->iterations_done : W.done; A.best = out->best_inliers ? out->best_inliers : W.best;
    A.best_it = out->best_iter ? out->best_iter : W.best_it;
    A.R = W.R; A.t = W.t; A.s = W.s; A.o_R = out->R12; A.o_t = out->t12; A.o_s = out->s12; A.o_T = out->T12;
    VIORB_LAUNCH(k_sim3_select, batch, 64, 0, st, A);
    if (!out->n_inliers && !out->inliers) return VIORB_OK;
    return launch_inliers(*in, W, win, cfg, W.R, W.t, W.s, A.best_it, A.status, nullptr, out->n_inliers, out->inliers, (size_t)in->cap, 0, batch, st);
}

int viorb_sim3_ransac(const viorb_sim3_config* cfg, const float* X1c, const float* X2c, const float* sigma2_1, const float* sigma2_2,
                      const float* K1, const float* K2, int n, const int32_t* sets, int max_its, int first_iteration, int best_inliers_in,
                      const viorb_sim3_outputs* out) {
    VIORB_TRY(s3_check_cfg(cfg, 1));
    VIORB_REQUIRE(n >= 0 && (n == 0 || (X1c && X2c && sigma2_1 && sigma2_2)) && K1 && K2 && sets && out && out->status,
                  "null array (status is required) or a negative count");
    VIORB_REQUIRE(max_its <= cfg->iterations, "max_its > iterations: no sets for the later iterations");
    if (n >= cfg->min_inliers && n >= 3)
        for (int it = 0; it < cfg->iterations; it++) VIORB_REQUIRE(set_ok(sets + (size_t)it * 3, n), "a set with an index outside 0..n-1 or a repeated index");
    VIORB_TRY(require_device());
    const int cap = std::max(n, 1);
    const size_t c = (size_t)cap, its = (size_t)cfg->iterations;
    DeviceBufs B;
    viorb_sim3_inputs I;
    I.X1c = B.up(X1c, 3 * (size_t)n, 3 * c); I.X2c = B.up(X2c, 3 * (size_t)n, 3 * c);
    I.sigma2_1 = B.up(sigma2_1, (size_t)n, c); I.sigma2_2 = B.up(sigma2_2, (size_t)n, c);
    I.K1 = B.up(K1, 4); I.K2 = B.up(K2, 4); I.n = B.up(&n, 1); I.cap = cap;
    int *ds = B.up(sets, its * 3), *dmax = B.up(&max_its, 1), *dfirst = B.up(&first_iteration, 1), *dbest = B.up(&best_inliers_in, 1);
    viorb_sim3_outputs D;
    D.status = B.zeros<int32_t>(1); D.iterations_done = B.zeros<int32_t>(1); D.best_inliers = B.zeros<int32_t>(1); D.best_iter = B.zeros<int32_t>(1);
    D.R12 = B.zeros<float>(9); D.t12 = B.zeros<float>(3); D.s12 = B.zeros<float>(1); D.T12 = B.zeros<float>(16);
    D.n_inliers = B.zeros<int32_t>(1); D.inliers = B.zeros<uint8_t>(c);
    const size_t wb = viorb_sim3_workspace_bytes(cap, cfg->iterations, 1);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_sim3_ransac_device(&I, cfg, ds, dmax, dfirst, dbest, 1, &D, dw, wb, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
#define S3_DOWN(field, count) \
    if (out->field) VIORB_HIP_TRY(hipMemcpy(out->field, D.field, sizeof(*D.field) * (size_t)(count), hipMemcpyDeviceToHost))
    S3_DOWN(status, 1); S3_DOWN(iterations_done, 1); S3_DOWN(best_inliers, 1); S3_DOWN(best_iter, 1); S3_DOWN(R12, 9); S3_DOWN(t12, 3);
    S3_DOWN(s12, 1); S3_DOWN(T12, 16); S3_DOWN(n_inliers, 1); S3_DOWN(inliers, c);
#undef S3_DOWN
    return VIORB_OK;
}

// ---- host-only test hooks: sim3_core.h compiled for the host --------------------------------------------------------------------------
int viorb_debug_sim3_horn(const float* P1, const float* P2, int fix_scale, float* R9, float* t3, float* s1) {
    float A[3][3], Bm[3][3], R[9], t[3], s = 0.0f;
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) { A[i][k] = P1[3 * i + k]; Bm[i][k] = P2[3 * i + k]; }
    const int reason = sim3_horn(A, Bm, fix_scale != 0, R, t, s);
    for (int k = 0; k < 9; k++) R9[k] = R[k];
    for (int k = 0; k < 3; k++) t3[k] = t[k];
    *s1 = s;
    return reason;
}

int viorb_debug_sim3_inlier(const float* R9, const float* t3, float s, const float* K1, const float* K2, const float* X1c3, const float* X2c3,
                            float sigma2_1, float sigma2_2, float* err2, float* max2) {
    const Sim3K k1 = {K1[0], K1[1], K1[2], K1[3]}, k2 = {K2[0], K2[1], K2[2], K2[3]};
    Sim3Pair T;
    sim3_transforms(R9, t3, s, T);
    float p1u, p1v, p2u, p2v, e1, e2;
    sim3_to_image(k1, X1c3[0], X1c3[1], X1c3[2], p1u, p1v);
    sim3_to_image(k2, X2c3[0], X2c3[1], X2c3[2], p2u, p2v);
    const float m1 = sim3_max_error(sigma2_1), m2 = sim3_max_error(sigma2_2);
    const bool in = sim3_is_inlier(k1, k2, T, X1c3, X2c3, p1u, p1v, p2u, p2v, m1, m2, e1, e2);
    if (err2) { err2[0] = e1; err2[1] = e2; }
    if (max2) { max2[0] = m1; max2[1] = m2; }
    return in ? 1 : 0;
}

int viorb_debug_sim3_select(const int32_t* counts, int n_counts, int n, int min_inliers, int max_its, int first_iteration, int best_inliers_in,
                            int iterations_per_call, int32_t* out4) {
    VIORB_REQUIRE(counts && out4 && n_counts >= 0 && iterations_per_call >= 1, "null array, n_counts < 0 or iterations_per_call < 1");
    const Sim3Select r = sim3_select(counts, n_counts, n, min_inliers, max_its, first_iteration, best_inliers_in, iterations_per_call);
    out4[0] = r.status; out4[1] = r.iterations_done; out4[2] = r.best_inliers; out4[3] = r.best_iter;
    return VIORB_OK;
}

int viorb_optimize_sim3_device(const viorb_sim3_opt_inputs* in, float th2, int fix_scale, int batch, double* d_S12_out, uint8_t* d_keep,
                               int32_t* d_n_in, double* d_info, void* stream) {
    VIORB_REQUIRE(in && in->S12 && in->X1c && in->X2c && in->obs1 && in->obs2 && in->inv_sigma2_1 && in->inv_sigma2_2 && in->valid && in->K1 && in->K2 &&
                  in->n && d_S12_out && d_keep && d_n_in && d_info, "null array");
    VIORB_REQUIRE(in->cap >= 1 && batch >= 1 && batch <= 65535 && th2 > 0, "cap >= 1, 1 <= batch <= 65535, th2 > 0");
    VIORB_TRY(require_device());
    S3OptArgs A; A.I = *in; A.th2 = (double)th2; A.delta = 1e-9; A.fix_scale = fix_scale; A.S_out = d_S12_out; A.keep = d_keep; A.n_in = d_n_in; A.info = d_info;
    VIORB_LAUNCH(k_sim3_optimize, batch, 256, 0, (hipStream_t)stream, A);
    return VIORB_OK;
}

int viorb_optimize_sim3(const double* S12, float th2, int fix_scale, const float* X1c, const float* X2c, const float* obs1, const float* obs2,
                        const float* inv_sigma2_1, const float* inv_sigma2_2, const uint8_t* valid, const float* K1, const float* K2, int n,
                        double* S12_out, uint8_t* keep, int32_t* n_in, double* info8) {
    VIORB_REQUIRE(S12 && K1 && K2 && S12_out && n_in && info8 && n >= 0 && (n == 0 || (X1c && X2c && obs1 && obs2 && inv_sigma2_1 && inv_sigma2_2 && valid && keep)) &&
                  th2 > 0, "null array, a negative count or th2 <= 0");
    VIORB_TRY(require_device());
    const size_t c = (size_t)std::max(n, 1), m = (size_t)n;
    DeviceBufs B;
    viorb_sim3_opt_inputs I;
    I.S12 = B.up(S12, 8); I.X1c = B.up(X1c, 3 * m, 3 * c); I.X2c = B.up(X2c, 3 * m, 3 * c); I.obs1 = B.up(obs1, 2 * m, 2 * c); I.obs2 = B.up(obs2, 2 * m, 2 * c);
    I.inv_sigma2_1 = B.up(inv_sigma2_1, m, c); I.inv_sigma2_2 = B.up(inv_sigma2_2, m, c); I.valid = B.up(valid, m, c); I.K1 = B.up(K1, 4); I.K2 = B.up(K2, 4);
    I.n = B.up(&n, 1); I.cap = (int)c;
    double *dS = B.zeros<double>(8), *dinfo = B.zeros<double>(8); uint8_t* dk = B.zeros<uint8_t>(c); int32_t* dn = B.zeros<int32_t>(1);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_optimize_sim3_device(&I, th2, fix_scale, 1, dS, dk, dn, dinfo, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_HIP_TRY(hipMemcpy(S12_out, dS, 64, hipMemcpyDeviceToHost)); VIORB_HIP_TRY(hipMemcpy(info8, dinfo, 64, hipMemcpyDeviceToHost));
    VIORB_HIP_TRY(hipMemcpy(n_in, dn, 4, hipMemcpyDeviceToHost));
    if (n) VIORB_HIP_TRY(hipMemcpy(keep, dk, m, hipMemcpyDeviceToHost));
    return VIORB_OK;
}

int viorb_debug_sim3_exp(const double* u7, const double* est8, double* exp8, double* prod8) {
    VIORB_REQUIRE(u7 && est8 && exp8 && prod8, "null array");
    const sim3d e = sim3_exp(u7);
    sim3_st(exp8, e); sim3_st(prod8, sim3_mul(e, sim3_ld(est8)));
    return VIORB_OK;
}

int viorb_debug_sim3_edges(const double* S8, const double* X1c3, const double* X2c3, const double* obs1_2, const double* obs2_2, const double* K1,
                           const double* K2, int fix_scale, double* e4, double* J28) {
    VIORB_REQUIRE(S8 && X1c3 && X2c3 && obs1_2 && obs2_2 && K1 && K2 && e4 && J28, "null array");
    const sim3d est = sim3_ld(S8);
    sim3_edge_error(est, ld3(X2c3), K1, obs1_2[0], obs1_2[1], e4);
    sim3_edge_error(sim3_inv(est), ld3(X1c3), K2, obs2_2[0], obs2_2[1], e4 + 2);
    const double scalar = 1 / (2 * 1e-9);
    for (int d = 0; d < 7; d++) {
        const sim3d p = sim3_perturbed(est, 2 * d, fix_scale != 0), m = sim3_perturbed(est, 2 * d + 1, fix_scale != 0);
        double ep[2], em[2];
        sim3_edge_error(p, ld3(X2c3), K1, obs1_2[0], obs1_2[1], ep); sim3_edge_error(m, ld3(X2c3), K1, obs1_2[0], obs1_2[1], em);
        J28[d] = scalar * (ep[0] - em[0]); J28[7 + d] = scalar * (ep[1] - em[1]);
        sim3_edge_error(sim3_inv(p), ld3(X1c3), K2, obs2_2[0], obs2_2[1], ep); sim3_edge_error(sim3_inv(m), ld3(X1c3), K2, obs2_2[0], obs2_2[1], em);
        J28[14 + d] = scalar * (ep[0] - em[0]); J28[21 + d] = scalar * (ep[1] - em[1]);
    }
    return VIORB_OK;
}

} // extern "C"
