// viorb_amd/csrc/two_view.hip — the two-view initialiser on the device: Initializer::Initialize and everything beneath it (reference
// src/Initializer.cc:44-929) for a batch of independent streams. The arithmetic is two_view_core.h.
//   k_tv_prepare      per (stream, role): Normalize of frame 1 / frame 2 over ALL its key points (sums in double), and the ordered
//                     compaction of vMatches12 into the match list (u1 v1 u2 v2 as one float4 per match, so that scoring loads coalesce)
//   k_tv_hypotheses   one wavefront per (stream, iteration, model): nine lanes hold the nine columns of A in double registers and run
//                     the one-sided Jacobi by exchanging columns with shuffles; rank-2 step (F), de-normalisation, H12 = H21^-1
//   k_tv_score        one wavefront per (stream, iteration, model): 64 lanes stride over the match list and reduce the score; inlier
//                     flags only on request (the two winners, or every hypothesis for the stage entry)
//   k_tv_select       one wavefront per stream: first-maximum argmax of both searches, RH, the model
//   k_tv_decompose    one wavefront per stream: H -> 8 or E -> 4 motions (3 x 3 Jacobi SVD in double), the inlier count
//   k_tv_check_rt     one workgroup per (stream, motion): triangulate and vet every inlier (mapping_core.h's 4 x 4 Jacobi), count by
//                     ballot, the min(50, n - 1)-th smallest parallax cosine by a radix select on the float bits (histogram in LDS)
//   k_tv_accept       one workgroup per stream: the accept rule, then the winner's points and flags scattered to key-point order
// viorb_two_view_init_device launches them in this order on one stream; the stage entries launch the same kernels.
#include <algorithm>
#include <vector>
#include "viorb_common.h"
#include "two_view_core.h"

namespace viorb {

struct TvWork {          // the workspace arrays (TvLayout below)
    float* nrm;          // [b][2][4]
    int* nm;             // [b]
    float4* pm;          // [b][cap]
    int* mi1;            // [b][cap]
    float *H21i, *H12i, *F21i;      // [b][it][9]
    float* scores;       // [b][it][2]
    int* reason;         // [b]
    int* model;          // [b]
    float* M;            // [b][9]
    int* best_it;        // [b][2]
    uint8_t *inl_h, *inl_f;         // [b][cap]
    float *hyp_R, *hyp_t;           // [b][8][9], [b][8][3]
    int *nh, *n_inl;     // [b]
    uint8_t* rt_code;    // [b][8][cap]
    float* rt_P;         // [b][8][cap][3]
    uint32_t* rt_key;    // [b][8][cap]
    int* hyp_ng;         // [b][8]
    float* hyp_par;      // [b][8]
};

struct TvIn { const float *xy1, *xy2; const int *n1, *n2, *matches12; int cap; };

__device__ __forceinline__ double tv_block_sum(double v, double* s, int t) {
    s[t] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (t < k) s[t] += s[t + k]; __syncthreads(); }
    const double r = s[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void k_tv_prepare(TvIn I, TvWork W) {
    __shared__ double s_red[256];
    __shared__ int s_scan[256];
    const int b = blockIdx.y, role = blockIdx.x, t = threadIdx.x;
    const size_t o = (size_t)b * I.cap;
    if (role < 2) {
        const float* xy = (role == 0 ? I.xy1 : I.xy2) + o * 2;
        const int n = min(max((role == 0 ? I.n1 : I.n2)[b], 0), I.cap);
        float* nrm = W.nrm + ((size_t)b * 2 + role) * 4;
        if (n == 0) { if (t < 4) nrm[t] = 0.0f; return; }
        double sx = 0, sy = 0;
        for (int i = t; i < n; i += 256) { sx += (double)xy[2 * i]; sy += (double)xy[2 * i + 1]; }
        sx = tv_block_sum(sx, s_red, t); sy = tv_block_sum(sy, s_red, t);
        float m[4];
        tv_norm_finish_mean(sx, sy, n, m);
        double dx = 0, dy = 0;
        for (int i = t; i < n; i += 256) { dx += (double)fabsf(xy[2 * i] - m[0]); dy += (double)fabsf(xy[2 * i + 1] - m[1]); }
        dx = tv_block_sum(dx, s_red, t); dy = tv_block_sum(dy, s_red, t);
        tv_norm_finish_dev(dx, dy, n, m);
        if (t == 0) { nrm[0] = m[0]; nrm[1] = m[1]; nrm[2] = m[2]; nrm[3] = m[3]; }
        return;
    }
    // the match list (:51-63), in increasing i1
    const int n1 = min(max(I.n1[b], 0), I.cap), n2 = min(max(I.n2[b], 0), I.cap);
    const int chunk = (I.cap + 255) / 256, i_lo = min(t * chunk, n1), i_hi = min(i_lo + chunk, n1);
    int cnt = 0;
    for (int i = i_lo; i < i_hi; i++) { const int m = I.matches12[o + i]; cnt += m >= 0 && m < n2; }
    s_scan[t] = cnt;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const int v = t >= s ? s_scan[t - s] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    const int total = s_scan[255];
    int pos = s_scan[t] - cnt;
    for (int i = i_lo; i < i_hi; i++) {
        const int m = I.matches12[o + i];
        if (m >= 0 && m < n2) {
            W.pm[o + pos] = make_float4(I.xy1[(o + i) * 2], I.xy1[(o + i) * 2 + 1], I.xy2[(o + m) * 2], I.xy2[(o + m) * 2 + 1]);
            W.mi1[o + pos] = i;
            pos++;
        }
    }
    if (t == 0) { W.nm[b] = total; W.reason[b] = total < 8 ? TV_REASON_FEW_MATCHES : TV_REASON_OK; }
}

// The nine-lane Jacobi: lane c < 9 owns column c. Returns vt.row(8) (the row of the smallest column norm) in every lane.
template <int M> __device__ __forceinline__ void tv_null9_wave(TvCol<M>& mine, int lane, float (&x)[9]) {
    const bool col = lane < 9;
    tv_col_init(mine, lane);
    for (int sweep = 0; sweep < TV_MAX_SWEEPS; sweep++) {
        bool changed = false;
        for (int r = 0; r < 9; r++) {
            const int q = col ? tv_partner(lane, r) : -1;
            const int src = q >= 0 ? q : lane;
            TvCol<M> other;
#pragma unroll
            for (int k = 0; k < M; k++) other.a[k] = __shfl(mine.a[k], src);
#pragma unroll
            for (int k = 0; k < 9; k++) other.v[k] = __shfl(mine.v[k], src);
            other.w = __shfl(mine.w, src);
            if (q >= 0) {
                const bool lower = lane < q;
                const double p = tv_col_dot(mine, other);
                double c = 1, s = 0;
                if (tv_rot_cs(lower ? mine.w : other.w, lower ? other.w : mine.w, p, c, s)) { tv_col_rotate(mine, other, c, s, lower); changed = true; }
            }
        }
        if (!__any(changed)) break;
    }
    int best = 0;
    double wb = __shfl(mine.w, 0);
#pragma unroll
    for (int c = 1; c < 9; c++) { const double wc = __shfl(mine.w, c); if (wc < wb) { wb = wc; best = c; } }
#pragma unroll
    for (int k = 0; k < 9; k++) x[k] = (float)__shfl(mine.v[k], best);
}

struct HypArgs { TvWork W; const int* sets; float *H21i, *H12i, *F21i; int iters, cap; };

__global__ __launch_bounds__(64) void k_tv_hypotheses(HypArgs A) {
    const int it = blockIdx.x, model = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const size_t om = ((size_t)b * A.iters + it) * 9;
    const int N = A.W.nm[b];
    const int idx = lane < 8 ? A.sets[((size_t)b * A.iters + it) * 8 + lane] : 0;
    bool bad = lane < 8 && (idx < 0 || idx >= N);
#pragma unroll
    for (int j = 0; j < 7; j++) { const int o = __shfl(idx, j); bad |= lane < 8 && j < lane && o == idx; }
    const bool few = N < 8;
    if (few || __any(bad)) {
        if (!few && lane == 0) A.W.reason[b] = TV_REASON_BAD_SET;       // every writer stores the same value
        if (lane < 9) { if (model == 0) { A.H21i[om + lane] = 0.0f; A.H12i[om + lane] = 0.0f; } else A.F21i[om + lane] = 0.0f; }
        return;
    }
    const float* nrm1 = A.W.nrm + (size_t)b * 8;
    const float* nrm2 = nrm1 + 4;
    float un1 = 0, vn1 = 0, un2 = 0, vn2 = 0;
    if (lane < 8) {
        const float4 p = A.W.pm[(size_t)b * A.cap + idx];
        tv_norm_point(nrm1, p.x, p.y, un1, vn1); tv_norm_point(nrm2, p.z, p.w, un2, vn2);
    }
    float x[9];
    if (model == 0) {
        TvCol<16> mine;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            float e0, e1;
            tv_entry_h(lane < 9 ? lane : 0, __shfl(un1, i), __shfl(vn1, i), __shfl(un2, i), __shfl(vn2, i), e0, e1);
            mine.a[2 * i] = (double)e0; mine.a[2 * i + 1] = (double)e1;
        }
        tv_null9_wave(mine, lane, x);
        float H21[9], H12[9];
        tv_h_denorm(x, nrm1, nrm2, H21, H12);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) { A.H21i[om + k] = H21[k]; A.H12i[om + k] = H12[k]; }
        }
    } else {
        TvCol<8> mine;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            mine.a[i] = (double)tv_entry_f(lane < 9 ? lane : 0, __shfl(un1, i), __shfl(vn1, i), __shfl(un2, i), __shfl(vn2, i));
        }
        tv_null9_wave(mine, lane, x);
        float Fn[9], F21[9];
        tv_f_rank2(x, Fn);
        tv_f_denorm(Fn, nrm1, nrm2, F21);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) A.F21i[om + k] = F21[k];
        }
    }
}

// which == NULL: hypothesis blockIdx.x of every stream, scores [b][it][2]. which != NULL: hypothesis which[b][model] (< 0: none).
struct ScoreArgs {
    TvWork W; const float *H21i, *H12i, *F21i; const int* which; float* scores; uint8_t *flags0, *flags1; size_t flag_stride_b, flag_stride_it;
    int iters, cap; float inv_sigma2;
};

__global__ __launch_bounds__(64) void k_tv_score(ScoreArgs A) {
    const int model = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int it = A.which ? A.which[b * 2 + model] : (int)blockIdx.x;
    const int N = A.W.reason[b] == TV_REASON_OK ? A.W.nm[b] : 0;
    uint8_t* flags = model == 0 ? A.flags0 : A.flags1;
    if (flags) flags += (size_t)b * A.flag_stride_b + (A.which ? 0 : (size_t)it * A.flag_stride_it);
    float M21[9], M12[9];
    const size_t om = ((size_t)b * A.iters + max(it, 0)) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) { M21[k] = model == 0 ? A.H21i[om + k] : A.F21i[om + k]; M12[k] = model == 0 ? A.H12i[om + k] : 0.0f; }
    const int n = it >= 0 ? N : 0;
    const float4* pm = A.W.pm + (size_t)b * A.cap;
    float sum = 0.0f;
    for (int i = lane; i < n; i += 64) {
        const float4 p = pm[i];
        float chi2[2]; bool in;
        const float s = model == 0 ? tv_score_h(M21, M12, p.x, p.y, p.z, p.w, A.inv_sigma2, chi2, in) : tv_score_f(M21, p.x, p.y, p.z, p.w, A.inv_sigma2, chi2, in);
        sum += s;
        if (flags) flags[i] = in;
    }
    if (flags) for (int i = n + lane; i < A.cap; i += 64) flags[i] = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s);
    if (A.scores && lane == 0 && !A.which) A.scores[((size_t)b * A.iters + it) * 2 + model] = sum;
}

struct SelectArgs { TvWork W; const float *H21i, *F21i, *scores; int iters; int* o_best_it; float *o_scores, *o_H21, *o_F21; };

__global__ __launch_bounds__(64) void k_tv_select(SelectArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float S[2]; int B[2];
#pragma unroll
    for (int model = 0; model < 2; model++) {
        float bs = 0.0f; int bi = -1;                                      // strictly greater than the best so far, from 0 (:165, 216)
        for (int it = lane; it < A.iters; it += 64) { const float s = A.scores[((size_t)b * A.iters + it) * 2 + model]; if (s > bs) { bs = s; bi = it; } }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const float os = __shfl_xor(bs, s); const int oi = __shfl_xor(bi, s);
            if (oi >= 0 && (os > bs || bi < 0 || (os == bs && oi < bi))) { bs = os; bi = oi; }
        }
        S[model] = bs; B[model] = bi;
    }
    const bool ok = A.W.reason[b] == TV_REASON_OK;
    if (!ok) { S[0] = S[1] = 0.0f; B[0] = B[1] = -1; }
    const float RH = S[0] / (S[0] + S[1]);
    int model = (double)RH > 0.40 ? TV_FROM_H : TV_FROM_F;
    if (ok && (model == TV_FROM_H ? B[0] : B[1]) < 0) { if (lane == 0) A.W.reason[b] = TV_REASON_NO_MODEL; model = TV_FAILED; }
    if (!ok) model = TV_FAILED;
    if (lane < 9) {
        const float h = B[0] >= 0 ? A.H21i[((size_t)b * A.iters + B[0]) * 9 + lane] : 0.0f;
        const float f = B[1] >= 0 ? A.F21i[((size_t)b * A.iters + B[1]) * 9 + lane] : 0.0f;
        if (A.o_H21) A.o_H21[(size_t)b * 9 + lane] = h;
        if (A.o_F21) A.o_F21[(size_t)b * 9 + lane] = f;
        A.W.M[(size_t)b * 9 + lane] = model == TV_FROM_H ? h : (model == TV_FROM_F ? f : 0.0f);
    }
    if (lane < 2) {
        A.W.best_it[b * 2 + lane] = B[lane];
        if (A.o_best_it) A.o_best_it[b * 2 + lane] = B[lane];
        if (A.o_scores) A.o_scores[b * 2 + lane] = S[lane];
    }
    if (lane == 0) A.W.model[b] = model;
}

struct RecArgs {
    TvWork W; TvK k; const int* model; const float* M; const uint8_t *inl_h, *inl_f; int cap; float th2, min_parallax; int min_tri;
    viorb_two_view_outputs out;
};

__global__ __launch_bounds__(64) void k_tv_decompose(RecArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int model = A.model[b];
    const bool run = (model == TV_FROM_H || model == TV_FROM_F) && A.W.reason[b] == TV_REASON_OK;
    const int N = A.W.nm[b];
    const uint8_t* inl = (model == TV_FROM_H ? A.inl_h : A.inl_f) + (size_t)b * A.cap;
    int cnt = 0;
    if (run) for (int base = 0; base < N; base += 64) { const int i = base + lane; cnt += __popcll(__ballot(i < N && inl[i] != 0)); }
    if (lane != 0) return;
    A.W.n_inl[b] = cnt;
    float R[8][9], t[8][3], d3[3];
    int nh = 0;
    if (!run) { if (A.W.reason[b] == TV_REASON_OK) A.W.reason[b] = TV_REASON_NO_MODEL; }
    else {
        if (model == TV_FROM_H) { nh = tv_decompose_h(A.M + (size_t)b * 9, A.k, R, t, d3) ? 8 : 0; if (!nh) A.W.reason[b] = TV_REASON_H_DEGENERATE; }
        else { tv_decompose_f(A.M + (size_t)b * 9, A.k, R, t); nh = 4; }
    }
    A.W.nh[b] = nh;
    float* oR = A.W.hyp_R + (size_t)b * 72; float* ot = A.W.hyp_t + (size_t)b * 24;
#pragma unroll
    for (int h = 0; h < 8; h++) {
#pragma unroll
        for (int i = 0; i < 9; i++) oR[h * 9 + i] = h < nh ? R[h][i] : 0.0f;
#pragma unroll
        for (int i = 0; i < 3; i++) ot[h * 3 + i] = h < nh ? t[h][i] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_tv_check_rt(RecArgs A) {
    __shared__ int s_hist[256];
    __shared__ int s_cnt[4];
    __shared__ uint32_t s_prefix;
    __shared__ int s_k;
    const int h = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const size_t bh = (size_t)b * 8 + h;
    if (h >= A.W.nh[b]) { if (t == 0) { A.W.hyp_ng[bh] = 0; A.W.hyp_par[bh] = 0.0f; } return; }
    const int N = A.W.nm[b];
    const uint8_t* inl = (A.model[b] == TV_FROM_H ? A.inl_h : A.inl_f) + (size_t)b * A.cap;
    const float4* pm = A.W.pm + (size_t)b * A.cap;
    uint8_t* code = A.W.rt_code + bh * A.cap; float* P = A.W.rt_P + bh * A.cap * 3; uint32_t* key = A.W.rt_key + bh * A.cap;
    TvPose pose;
    tv_pose(A.k, A.W.hyp_R + bh * 9, A.W.hyp_t + bh * 3, pose);
    int cnt = 0;
    for (int base = 0; base < N; base += 256) {
        const int i = base + t;
        int c = TV_RT_NONE;
        if (i < N) {
            float X[3] = {0.0f, 0.0f, 0.0f}, q6[6];
            q6[0] = 0.0f;
            if (inl[i]) { const float4 p = pm[i]; c = tv_check_rt_match(A.k, pose, p.x, p.y, p.z, p.w, A.th2, X, q6); }
            code[i] = (uint8_t)c; key[i] = tv_float_key(q6[0]);
            P[3 * i] = X[0]; P[3 * i + 1] = X[1]; P[3 * i + 2] = X[2];
        }
        cnt += __popcll(__ballot(c != TV_RT_NONE));
    }
    if ((t & 63) == 0) s_cnt[t >> 6] = cnt;
    __syncthreads();
    const int ng = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (ng == 0) { if (t == 0) { A.W.hyp_ng[bh] = 0; A.W.hyp_par[bh] = 0.0f; } return; }
    // the min(50, ng - 1)-th smallest key: four 8-bit digits from the top
    if (t == 0) { s_prefix = 0; s_k = min(50, ng - 1); }
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        s_hist[t] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (int i = t; i < N; i += 256) if (code[i] && (key[i] & mask) == prefix) atomicAdd(&s_hist[(key[i] >> shift) & 255], 1);
        __syncthreads();
        if (t == 0) {
            int k = s_k, d = 0;
            while (d < 255 && k >= s_hist[d]) { k -= s_hist[d]; d++; }
            s_k = k; s_prefix = prefix | ((uint32_t)d << shift);
        }
        __syncthreads();
    }
    if (t == 0) { A.W.hyp_ng[bh] = ng; A.W.hyp_par[bh] = tv_parallax_deg(tv_key_float(s_prefix)); }
}

__global__ __launch_bounds__(256) void k_tv_accept(RecArgs A) {
    __shared__ int s_win, s_status;
    const int b = blockIdx.x, t = threadIdx.x;
    const int model = A.model[b], nh = A.W.nh[b], N = A.W.nm[b];
    const viorb_two_view_outputs& O = A.out;
    if (t == 0) {
        int reason = A.W.reason[b], win = -1;
        if (reason == TV_REASON_OK) {
            const int* ng = A.W.hyp_ng + (size_t)b * 8; const float* par = A.W.hyp_par + (size_t)b * 8;
            win = model == TV_FROM_H ? tv_accept_h(ng, par, A.W.n_inl[b], A.min_parallax, A.min_tri, reason)
                                     : tv_accept_f(ng, par, A.W.n_inl[b], A.min_parallax, A.min_tri, reason);
        }
        s_win = win; s_status = win >= 0 ? model : TV_FAILED;
        O.status[b] = s_status; O.reason[b] = reason;
        if (O.n_matches) O.n_matches[b] = N;
        if (O.n_hyp) O.n_hyp[b] = nh;
    }
    __syncthreads();
    const int win = s_win;
    if (t < 8) {
        if (O.hyp_n_good) O.hyp_n_good[(size_t)b * 8 + t] = t < nh ? A.W.hyp_ng[(size_t)b * 8 + t] : 0;
        if (O.hyp_parallax) O.hyp_parallax[(size_t)b * 8 + t] = t < nh ? A.W.hyp_par[(size_t)b * 8 + t] : 0.0f;
    }
    if (t < 72 && O.hyp_R) O.hyp_R[(size_t)b * 72 + t] = A.W.hyp_R[(size_t)b * 72 + t];
    if (t < 24 && O.hyp_t) O.hyp_t[(size_t)b * 24 + t] = A.W.hyp_t[(size_t)b * 24 + t];
    if (t < 9 && O.R21) O.R21[(size_t)b * 9 + t] = win >= 0 ? A.W.hyp_R[((size_t)b * 8 + win) * 9 + t] : 0.0f;
    if (t < 3 && O.t21) O.t21[(size_t)b * 3 + t] = win >= 0 ? A.W.hyp_t[((size_t)b * 8 + win) * 3 + t] : 0.0f;
    const size_t o = (size_t)b * A.cap;
    for (int i = t; i < A.cap; i += 256) {
        if (O.P3D) { O.P3D[(o + i) * 3] = 0.0f; O.P3D[(o + i) * 3 + 1] = 0.0f; O.P3D[(o + i) * 3 + 2] = 0.0f; }
        if (O.triangulated) O.triangulated[o + i] = 0;
    }
    __syncthreads();
    if (win < 0) return;
    const size_t bw = ((size_t)b * 8 + win) * A.cap;
    for (int i = t; i < N; i += 256) {
        const int c = A.W.rt_code[bw + i];
        if (c == TV_RT_NONE) continue;
        const int i1 = A.W.mi1[o + i];                                  // distinct per match: no two threads write the same key point
        if (O.P3D) { O.P3D[(o + i1) * 3] = A.W.rt_P[(bw + i) * 3]; O.P3D[(o + i1) * 3 + 1] = A.W.rt_P[(bw + i) * 3 + 1]; O.P3D[(o + i1) * 3 + 2] = A.W.rt_P[(bw + i) * 3 + 2]; }
        if (O.triangulated) O.triangulated[o + i1] = c == TV_RT_TRIANGULATED;
    }
}

} // namespace viorb

using namespace viorb;

namespace {

struct TvLayout { TvWork W; size_t total; };
TvLayout tv_layout(void* base, int cap, int iters, int batch) {
    TvLayout L; WorkspaceLayout Y(base); TvWork& W = L.W;
    const size_t B = (size_t)batch, n = B * cap, m = B * iters;
    Y.take(&W.nrm, B * 8); Y.take(&W.nm, B); Y.take(&W.pm, n); Y.take(&W.mi1, n);
    Y.take(&W.H21i, m * 9); Y.take(&W.H12i, m * 9); Y.take(&W.F21i, m * 9); Y.take(&W.scores, m * 2);
    Y.take(&W.reason, B); Y.take(&W.model, B); Y.take(&W.M, B * 9); Y.take(&W.best_it, B * 2);
    Y.take(&W.inl_h, n); Y.take(&W.inl_f, n); Y.take(&W.hyp_R, B * 72); Y.take(&W.hyp_t, B * 24); Y.take(&W.nh, B); Y.take(&W.n_inl, B);
    Y.take(&W.rt_code, n * 8); Y.take(&W.rt_P, n * 24); Y.take(&W.rt_key, n * 8); Y.take(&W.hyp_ng, B * 8); Y.take(&W.hyp_par, B * 8);
    L.total = Y.end();
    return L;
}

int tv_check_common(const viorb_two_view_config* cfg, const float* xy1, const int32_t* n1, const float* xy2, const int32_t* n2, int cap,
                    const int32_t* matches12, int batch, void* workspace, size_t workspace_bytes) {
    VIORB_REQUIRE(cfg && cfg->iterations >= 1 && cfg->iterations <= 4096 && cfg->sigma > 0 && cfg->fx != 0 && cfg->fy != 0,
                  "config: 1 <= iterations <= 4096, sigma > 0, fx, fy != 0");
    VIORB_REQUIRE(xy1 && n1 && xy2 && n2 && matches12 && workspace, "null array");
    VIORB_REQUIRE(cap >= 1 && batch >= 1 && batch <= 65535, "cap >= 1, 1 <= batch <= 65535");
    VIORB_REQUIRE(workspace_bytes >= tv_layout(nullptr, cap, cfg->iterations, batch).total && ((uintptr_t)workspace & 255) == 0,
                  "workspace smaller than viorb_two_view_workspace_bytes or not 256-byte aligned");
    return VIORB_OK;
}

TvIn tv_in(const float* xy1, const int32_t* n1, const float* xy2, const int32_t* n2, int cap, const int32_t* matches12) {
    TvIn I; I.xy1 = xy1; I.xy2 = xy2; I.n1 = n1; I.n2 = n2; I.matches12 = matches12; I.cap = cap;
    return I;
}

int launch_prepare(const TvIn& I, const TvWork& W, int batch, hipStream_t st) {
    VIORB_LAUNCH(k_tv_prepare, dim3(3, batch), 256, 0, st, I, W);
    return VIORB_OK;
}
int launch_hypotheses(const TvWork& W, const int32_t* sets, float* H21i, float* H12i, float* F21i, int iters, int cap, int batch, hipStream_t st) {
    HypArgs A; A.W = W; A.sets = sets; A.H21i = H21i; A.H12i = H12i; A.F21i = F21i; A.iters = iters; A.cap = cap;
    VIORB_LAUNCH(k_tv_hypotheses, dim3(iters, 2, batch), 64, 0, st, A);
    return VIORB_OK;
}
int launch_score(const TvWork& W, const viorb_two_view_config* cfg, const float* H21i, const float* H12i, const float* F21i, const int* which,
                 float* scores, uint8_t* flags0, uint8_t* flags1, size_t stride_b, size_t stride_it, int cap, int batch, hipStream_t st) {
    ScoreArgs A; A.W = W; A.H21i = H21i; A.H12i = H12i; A.F21i = F21i; A.which = which; A.scores = scores; A.flags0 = flags0; A.flags1 = flags1;
    A.flag_stride_b = stride_b; A.flag_stride_it = stride_it; A.iters = cfg->iterations; A.cap = cap; A.inv_sigma2 = tv_inv_sigma2(cfg->sigma);
    VIORB_LAUNCH(k_tv_score, dim3(which ? 1 : cfg->iterations, 2, batch), 64, 0, st, A);
    return VIORB_OK;
}
int launch_reconstruct(const TvWork& W, const viorb_two_view_config* cfg, const int* model, const float* M, const uint8_t* inl_h, const uint8_t* inl_f,
                       const viorb_two_view_outputs* out, int cap, int batch, hipStream_t st) {
    RecArgs A; A.W = W; A.k.fx = cfg->fx; A.k.fy = cfg->fy; A.k.cx = cfg->cx; A.k.cy = cfg->cy; A.model = model; A.M = M; A.inl_h = inl_h; A.inl_f = inl_f;
    A.cap = cap; A.th2 = tv_th2(cfg->sigma); A.min_parallax = cfg->min_parallax_deg; A.min_tri = cfg->min_triangulated; A.out = *out;
    VIORB_LAUNCH(k_tv_decompose, batch, 64, 0, st, A);
    VIORB_LAUNCH(k_tv_check_rt, dim3(8, batch), 256, 0, st, A);
    VIORB_LAUNCH(k_tv_accept, batch, 256, 0, st, A);
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
    for (int j = 0; j < 8; j++) {
        if (s[j] < 0 || s[j] >= n) return false;
        for (int k = 0; k < j; k++) if (s[k] == s[j]) return false;
    }
    return true;
}
} // namespace

extern "C" {

int viorb_two_view_draw_sets(int n_matches, int iterations, uint64_t seed, int32_t* sets) {
    VIORB_REQUIRE(sets && n_matches >= 8 && iterations >= 1, "sets != NULL, n_matches >= 8, iterations >= 1");
    std::vector<int32_t> avail((size_t)n_matches);
    uint64_t state = seed;
    for (int it = 0; it < iterations; it++) {
        for (int i = 0; i < n_matches; i++) avail[i] = i;
        int left = n_matches;
        for (int j = 0; j < 8; j++) {
            int r = (int)((double)(splitmix64(state) >> 11) * (1.0 / 9007199254740992.0) * (double)left);
            if (r >= left) r = left - 1;
            sets[(size_t)it * 8 + j] = avail[r];
            avail[r] = avail[left - 1];
            left--;
        }
    }
    return VIORB_OK;
}

size_t viorb_two_view_workspace_bytes(int cap, int iterations, int batch) {
    if (cap < 1 || iterations < 1 || batch < 1) return 0;
    return tv_layout(nullptr, cap, iterations, batch).total;
}

int viorb_two_view_hypotheses_device(const viorb_two_view_config* cfg, const float* d_xy1, const int32_t* d_n1, const float* d_xy2,
                                     const int32_t* d_n2, int cap, const int32_t* d_matches12, const int32_t* d_sets, int batch,
                                     float* d_H21i, float* d_H12i, float* d_F21i, int32_t* d_reason, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    VIORB_TRY(tv_check_common(cfg, d_xy1, d_n1, d_xy2, d_n2, cap, d_matches12, batch, workspace, workspace_bytes));
    VIORB_REQUIRE(d_sets && d_H21i && d_H12i && d_F21i && d_reason, "null array");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const TvWork W = tv_layout(workspace, cap, cfg->iterations, batch).W;
    VIORB_TRY(launch_prepare(tv_in(d_xy1, d_n1, d_xy2, d_n2, cap, d_matches12), W, batch, st));
    VIORB_TRY(launch_hypotheses(W, d_sets, d_H21i, d_H12i, d_F21i, cfg->iterations, cap, batch, st));
    VIORB_HIP_TRY(hipMemcpyAsync(d_reason, W.reason, sizeof(int) * (size_t)batch, hipMemcpyDeviceToDevice, st));
    return VIORB_OK;
}

int viorb_two_view_score_device(const viorb_two_view_config* cfg, const float* d_xy1, const int32_t* d_n1, const float* d_xy2,
                                const int32_t* d_n2, int cap, const int32_t* d_matches12, int batch, const float* d_H21i,
                                const float* d_H12i, const float* d_F21i, float* d_scores, uint8_t* d_flags, void* workspace,
                                size_t workspace_bytes, void* stream) {
    VIORB_TRY(tv_check_common(cfg, d_xy1, d_n1, d_xy2, d_n2, cap, d_matches12, batch, workspace, workspace_bytes));
    VIORB_REQUIRE(d_H21i && d_H12i && d_F21i && d_scores, "null array");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const TvWork W = tv_layout(workspace, cap, cfg->iterations, batch).W;
    VIORB_TRY(launch_prepare(tv_in(d_xy1, d_n1, d_xy2, d_n2, cap, d_matches12), W, batch, st));
    return launch_score(W, cfg, d_H21i, d_H12i, d_F21i, nullptr, d_scores, d_flags, d_flags ? d_flags + cap : nullptr,
                        (size_t)cfg->iterations * 2 * cap, (size_t)2 * cap, cap, batch, st);
}

int viorb_two_view_reconstruct_device(const viorb_two_view_config* cfg, const float* d_xy1, const int32_t* d_n1, const float* d_xy2,
                                      const int32_t* d_n2, int cap, const int32_t* d_matches12, int batch, const int32_t* d_model,
                                      const float* d_M, const uint8_t* d_inliers, const viorb_two_view_outputs* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    VIORB_TRY(tv_check_common(cfg, d_xy1, d_n1, d_xy2, d_n2, cap, d_matches12, batch, workspace, workspace_bytes));
    VIORB_REQUIRE(d_model && d_M && d_inliers && out && out->status && out->reason, "null array (status and reason are required)");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const TvWork W = tv_layout(workspace, cap, cfg->iterations, batch).W;
    VIORB_TRY(launch_prepare(tv_in(d_xy1, d_n1, d_xy2, d_n2, cap, d_matches12), W, batch, st));
    return launch_reconstruct(W, cfg, d_model, d_M, d_inliers, d_inliers, out, cap, batch, st);
}

int viorb_two_view_init_device(const viorb_two_view_config* cfg, const float* d_xy1, const int32_t* d_n1, const float* d_xy2,
                               const int32_t* d_n2, int cap, const int32_t* d_matches12, const int32_t* d_sets, int batch,
                               const viorb_two_view_outputs* out, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(tv_check_common(cfg, d_xy1, d_n1, d_xy2, d_n2, cap, d_matches12, batch, workspace, workspace_bytes));
    VIORB_REQUIRE(d_sets && out && out->status && out->reason, "null array (status and reason are required)");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const TvWork W = tv_layout(workspace, cap, cfg->iterations, batch).W;
    VIORB_TRY(launch_prepare(tv_in(d_xy1, d_n1, d_xy2, d_n2, cap, d_matches12), W, batch, st));
    VIORB_TRY(launch_hypotheses(W, d_sets, W.H21i, W.H12i, W.F21i, cfg->iterations, cap, batch, st));
    VIORB_TRY(launch_score(W, cfg, W.H21i, W.H12i, W.F21i, nullptr, W.scores, nullptr, nullptr, 0, 0, cap, batch, st));
    SelectArgs S; S.W = W; S.H21i = W.H21i; S.F21i = W.F21i; S.scores = W.scores; S.iters = cfg->iterations;
    S.o_best_it = out->best_iter; S.o_scores = out->scores; S.o_H21 = out->H21; S.o_F21 = out->F21;
    VIORB_LAUNCH(k_tv_select, batch, 64, 0, st, S);
    uint8_t* ih = out->inliers_h ? out->inliers_h : W.inl_h; uint8_t* jf = out->inliers_f ? out->inliers_f : W.inl_f;
    VIORB_TRY(launch_score(W, cfg, W.H21i, W.H12i, W.F21i, W.best_it, nullptr, ih, jf, (size_t)cap, 0, cap, batch, st));
    return launch_reconstruct(W, cfg, W.model, W.M, ih, jf, out, cap, batch, st);
}

int viorb_two_view_init(const viorb_two_view_config* cfg, const float* xy1, int n1, const float* xy2, int n2, const int32_t* matches12,
                        const int32_t* sets, const viorb_two_view_outputs* out) {
    VIORB_REQUIRE(cfg && cfg->iterations >= 1 && cfg->iterations <= 4096 && cfg->sigma > 0 && cfg->fx != 0 && cfg->fy != 0,
                  "config: 1 <= iterations <= 4096, sigma > 0, fx, fy != 0");
    VIORB_REQUIRE(n1 >= 0 && n2 >= 0 && (n1 == 0 || (xy1 && matches12)) && (n2 == 0 || xy2) && sets && out && out->status && out->reason,
                  "null array (status and reason are required) or a negative count");
    int N = 0;
    for (int i = 0; i < n1; i++) { VIORB_REQUIRE(matches12[i] < n2, "matches12[i1] >= n2"); N += matches12[i] >= 0; }
    if (N >= 8) for (int it = 0; it < cfg->iterations; it++) VIORB_REQUIRE(set_ok(sets + (size_t)it * 8, N), "a set with an index outside 0..N-1 or a repeated index");
    VIORB_TRY(require_device());
    const int cap = std::max(std::max(n1, n2), 1);
    const size_t c = (size_t)cap, its = (size_t)cfg->iterations;
    DeviceBufs B;
    float *dx1 = B.up(xy1, 2 * (size_t)n1, 2 * c), *dx2 = B.up(xy2, 2 * (size_t)n2, 2 * c);
    int *dn1 = B.up(&n1, 1), *dn2 = B.up(&n2, 1), *dm = B.up(matches12, (size_t)n1, c), *ds = B.up(sets, its * 8);
    viorb_two_view_outputs D;
    D.status = B.zeros<int32_t>(1); D.reason = B.zeros<int32_t>(1); D.n_matches = B.zeros<int32_t>(1); D.scores = B.zeros<float>(2);
    D.best_iter = B.zeros<int32_t>(2); D.H21 = B.zeros<float>(9); D.F21 = B.zeros<float>(9); D.inliers_h = B.zeros<uint8_t>(c);
    D.inliers_f = B.zeros<uint8_t>(c); D.R21 = B.zeros<float>(9); D.t21 = B.zeros<float>(3); D.P3D = B.zeros<float>(3 * c);
    D.triangulated = B.zeros<uint8_t>(c); D.n_hyp = B.zeros<int32_t>(1); D.hyp_n_good = B.zeros<int32_t>(8); D.hyp_parallax = B.zeros<float>(8);
    D.hyp_R = B.zeros<float>(72); D.hyp_t = B.zeros<float>(24);
    const size_t wb = viorb_two_view_workspace_bytes(cap, cfg->iterations, 1);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_two_view_init_device(cfg, dx1, dn1, dx2, dn2, cap, dm, ds, 1, &D, dw, wb, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
#define TV_DOWN(field, count) \
    if (out->field) VIORB_HIP_TRY(hipMemcpy(out->field, D.field, sizeof(*D.field) * (size_t)(count), hipMemcpyDeviceToHost))
    TV_DOWN(status, 1); TV_DOWN(reason, 1); TV_DOWN(n_matches, 1); TV_DOWN(scores, 2); TV_DOWN(best_iter, 2); TV_DOWN(H21, 9); TV_DOWN(F21, 9);
    TV_DOWN(inliers_h, c); TV_DOWN(inliers_f, c); TV_DOWN(R21, 9); TV_DOWN(t21, 3); TV_DOWN(P3D, 3 * c); TV_DOWN(triangulated, c);
    TV_DOWN(n_hyp, 1); TV_DOWN(hyp_n_good, 8); TV_DOWN(hyp_parallax, 8); TV_DOWN(hyp_R, 72); TV_DOWN(hyp_t, 24);
#undef TV_DOWN
    return VIORB_OK;
}

// ---- host-only test hooks: two_view_core.h compiled for the host ------------------------------------------------------------------
int viorb_debug_two_view_hypothesis(int model, const float* pn1, const float* pn2, float* M9, float* pre9) {
    float x[9];
    if (model == TV_FROM_H) {
        float A[16][9];
        for (int i = 0; i < 8; i++) tv_rows_h(pn1[2 * i], pn1[2 * i + 1], pn2[2 * i], pn2[2 * i + 1], A[2 * i], A[2 * i + 1]);
        tv_null9_host<16>(A, x);
        for (int k = 0; k < 9; k++) M9[k] = x[k];
    } else if (model == TV_FROM_F) {
        float A[8][9];
        for (int i = 0; i < 8; i++) tv_row_f(pn1[2 * i], pn1[2 * i + 1], pn2[2 * i], pn2[2 * i + 1], A[i]);
        tv_null9_host<8>(A, x);
        tv_f_rank2(x, M9);
    } else return VIORB_ERR_INVALID_ARG;
    if (pre9) for (int k = 0; k < 9; k++) pre9[k] = x[k];
    return VIORB_OK;
}

int viorb_debug_two_view_denormalise(int model, const float* Mn9, const float* nrm1_4, const float* nrm2_4, float* M21, float* M12) {
    if (model == TV_FROM_H) tv_h_denorm(Mn9, nrm1_4, nrm2_4, M21, M12);
    else if (model == TV_FROM_F) tv_f_denorm(Mn9, nrm1_4, nrm2_4, M21);
    else return VIORB_ERR_INVALID_ARG;
    return VIORB_OK;
}

int viorb_debug_two_view_normalise(const float* xy, int n, float* nrm4) {
    if (n < 1) return VIORB_ERR_INVALID_ARG;
    double sx = 0, sy = 0, dx = 0, dy = 0;
    for (int i = 0; i < n; i++) { sx += (double)xy[2 * i]; sy += (double)xy[2 * i + 1]; }
    tv_norm_finish_mean(sx, sy, n, nrm4);
    for (int i = 0; i < n; i++) { dx += (double)fabsf(xy[2 * i] - nrm4[0]); dy += (double)fabsf(xy[2 * i + 1] - nrm4[1]); }
    tv_norm_finish_dev(dx, dy, n, nrm4);
    return VIORB_OK;
}

int viorb_debug_two_view_chi2(int model, const float* M21, const float* M12, const float* uv4, float sigma, float* chi2_2, float* score) {
    float chi2[2]; bool in = false;
    const float is2 = tv_inv_sigma2(sigma);
    const float s = model == TV_FROM_H ? tv_score_h(M21, M12, uv4[0], uv4[1], uv4[2], uv4[3], is2, chi2, in)
                                       : tv_score_f(M21, uv4[0], uv4[1], uv4[2], uv4[3], is2, chi2, in);
    chi2_2[0] = chi2[0]; chi2_2[1] = chi2[1];
    if (score) *score = s;
    return in ? 1 : 0;
}

int viorb_debug_two_view_decompose(int model, const float* M21, const float* K4, float* R, float* t, float* d3) {
    TvK k; k.fx = K4[0]; k.fy = K4[1]; k.cx = K4[2]; k.cy = K4[3];
    float Rh[8][9], th[8][3], d[3] = {0.0f, 0.0f, 0.0f};
    int n;
    if (model == TV_FROM_H) n = tv_decompose_h(M21, k, Rh, th, d) ? 8 : 0;
    else { tv_decompose_f(M21, k, Rh, th); n = 4; }
    for (int h = 0; h < 8; h++) { for (int i = 0; i < 9; i++) R[h * 9 + i] = Rh[h][i]; for (int i = 0; i < 3; i++) t[h * 3 + i] = th[h][i]; }
    if (d3) { d3[0] = d[0]; d3[1] = d[1]; d3[2] = d[2]; }
    return n;
}

int viorb_debug_two_view_check_rt(const float* K4, const float* R9, const float* t3, const float* uv4, float sigma, float* X3, float* q6) {
    TvK k; k.fx = K4[0]; k.fy = K4[1]; k.cx = K4[2]; k.cy = K4[3];
    TvPose p;
    tv_pose(k, R9, t3, p);
    float X[3], q[6];
    const int c = tv_check_rt_match(k, p, uv4[0], uv4[1], uv4[2], uv4[3], tv_th2(sigma), X, q);
    for (int i = 0; i < 3; i++) X3[i] = X[i];
    if (q6) for (int i = 0; i < 6; i++) q6[i] = q[i];
    return c;
}

float viorb_debug_two_view_parallax(const float* cos_parallax, int n) {
    if (n <= 0) return 0.0f;
    int k = std::min(50, n - 1);
    uint32_t prefix = 0;
    for (int pass = 0; pass < 4; pass++) {                      // k_tv_check_rt's select
        const int shift = 24 - 8 * pass;
        const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        int hist[256] = {0};
        for (int i = 0; i < n; i++) { const uint32_t key = tv_float_key(cos_parallax[i]); if ((key & mask) == prefix) hist[(key >> shift) & 255]++; }
        int d = 0;
        while (d < 255 && k >= hist[d]) { k -= hist[d]; d++; }
        prefix |= (uint32_t)d << shift;
    }
    return tv_parallax_deg(tv_key_float(prefix));
}

int viorb_debug_two_view_accept(int model, const int32_t* n_good, const float* parallax, int n_inliers, float min_parallax_deg,
                                int min_triangulated, int32_t* reason) {
    int r = TV_REASON_OK;
    const int w = model == TV_FROM_H ? tv_accept_h(n_good, parallax, n_inliers, min_parallax_deg, min_triangulated, r)
                                     : tv_accept_f(n_good, parallax, n_inliers, min_parallax_deg, min_triangulated, r);
    if (reason) *reason = r;
    return w;
}

} // extern "C"
