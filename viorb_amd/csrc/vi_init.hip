// viorb_amd/csrc/vi_init.hip — visual-inertial initialisation (LocalMapping::TryInitVIO, reference src/LocalMapping.cc:191-786) for a
// ragged batch of independent streams. Arithmetic shared with the host hooks: vi_init_core.h, vio_core.h.
//   k_preint_intervals    KeyFrame::ComputePreInt / KeyFrameInit::ComputePreInt for every (stream, interval): one wavefront per interval,
//                         four per workgroup, no workgroup barrier. Every lane carries the 3 x 3 state recursion (preint_step); lanes
//                         0..44 own the distinct entries of the symmetric 9 x 9 covariance and form A S A^T + N from the sparse rows
//                         of A = [[I, dt I, A06], [0, I, A36], [0, 0, A66]] (at most five entries a row) out of the wave's LDS slice.
//                         Samples reach the wave nine at a time through one coalesced 8-byte load per lane.
//   k_vi_gyro_bias        Optimizer::OptimizeInitialGyroBias: one wavefront per stream, lanes stride over the edges, butterfly sum.
//   k_vi_solve            steps 2 and 3: rows generated on the fly from three key frames, Gram matrices summed across the wave,
//                         Jacobi eigen-solve in registers (4 x 4, then 6 x 6), Rwi, gw.
//   k_vi_apply            NavStates (P, R, V, biases) of all key frames and the rescaled float poses: one wavefront per stream, lanes
//                         stride over the key frames; the two velocities that depend on a predecessor recompute it (depth <= 2).
//   k_scale_map_points    MapPoint::UpdateScale, element-wise, 16-byte accesses where the row allows them.
// No floating-point atomics anywhere: the same call gives the same bytes.
#include <algorithm>
#include <vector>
#include "viorb_common.h"
#include "vi_init_core.h"

namespace viorb {

#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define PI_WAVES 4
#define PI_CHUNK 9                                            // samples staged per refill: 63 doubles + the stamp that follows them
#define PI_WAVE_DOUBLES (142 + 45 + 27 + 64)

struct PreintArgs {
    const int32_t* n_kf; const double* kf_time; const int32_t* imu_start; const double* imu; long long total_imu;
    const double* bg; const double* ba; int bg_stride, ba_stride;
    double gyr_cov, acc_cov; int clamp, max_kf, batch;
    const int32_t* only_ok;                                   // not NULL: streams whose status is not VIORB_OK are left untouched
    double* preint;
};

// one IMUPreintegrator::update of the covariance for the lane's entry (r, c), r <= c. AR[9][5]: sparse rows of A (columns r, r + 3
// or r again with a zero weight, 6, 7, 8); NB[9][3]: rows 0..5 = Ca, rows 6..8 = Bg. The sums run over the non-zero terms of
// A cov A^T in the order the dense product visits them, so an entry equals the dense result bit for bit given the same input.
__device__ __forceinline__ double cov_entry(const double* S, const double* AR, const double* NB, int r, int c, double gyr_cov, double acc_cov) {
    const int cr[5] = {r, r < 3 ? r + 3 : r, 6, 7, 8}, cc[5] = {c, c < 3 ? c + 3 : c, 6, 7, 8};
    double acc = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        double t = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) t += AR[5 * r + i] * S[9 * cr[i] + cc[j]];
        acc += t * AR[5 * c + j];
    }
    double nn = 0;
    const bool gy = r >= 6 && c >= 6, ac = r < 6 && c < 6;
    if (gy || ac) {
        const double sig = gy ? gyr_cov : acc_cov;
#pragma unroll
        for (int k = 0; k < 3; k++) nn += NB[3 * r + k] * sig * NB[3 * c + k];
    }
    return acc + nn;
}

__device__ __forceinline__ void cov_publish(double* AR, double* NB, const preint_cov_blocks& C) {
    const double a06[9] = {C.A06.a00, C.A06.a01, C.A06.a02, C.A06.a10, C.A06.a11, C.A06.a12, C.A06.a20, C.A06.a21, C.A06.a22};
    const double a36[9] = {C.A36.a00, C.A36.a01, C.A36.a02, C.A36.a10, C.A36.a11, C.A36.a12, C.A36.a20, C.A36.a21, C.A36.a22};
    const double a66[9] = {C.A66.a00, C.A66.a01, C.A66.a02, C.A66.a10, C.A66.a11, C.A66.a12, C.A66.a20, C.A66.a21, C.A66.a22};
    const double ca0[9] = {C.Ca0.a00, C.Ca0.a01, C.Ca0.a02, C.Ca0.a10, C.Ca0.a11, C.Ca0.a12, C.Ca0.a20, C.Ca0.a21, C.Ca0.a22};
    const double ca3[9] = {C.Ca3.a00, C.Ca3.a01, C.Ca3.a02, C.Ca3.a10, C.Ca3.a11, C.Ca3.a12, C.Ca3.a20, C.Ca3.a21, C.Ca3.a22};
    const double bg[9] = {C.Bg.a00, C.Bg.a01, C.Bg.a02, C.Bg.a10, C.Bg.a11, C.Bg.a12, C.Bg.a20, C.Bg.a21, C.Bg.a22};
#pragma unroll
    for (int r = 0; r < 3; r++) {
        AR[5 * r] = 1.0; AR[5 * r + 1] = C.dt;
        AR[5 * (r + 3)] = 1.0; AR[5 * (r + 3) + 1] = 0.0;
        AR[5 * (r + 6)] = 0.0; AR[5 * (r + 6) + 1] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            AR[5 * r + 2 + k] = a06[3 * r + k]; AR[5 * (r + 3) + 2 + k] = a36[3 * r + k]; AR[5 * (r + 6) + 2 + k] = a66[3 * r + k];
            NB[3 * r + k] = ca0[3 * r + k]; NB[3 * (r + 3) + k] = ca3[3 * r + k]; NB[3 * (r + 6) + k] = bg[3 * r + k];
        }
    }
}

__global__ __launch_bounds__(64 * PI_WAVES) void k_preint_intervals(PreintArgs A) {
    __shared__ double s_all[PI_WAVES * PI_WAVE_DOUBLES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long wid = (long long)blockIdx.x * PI_WAVES + wv;
    if (wid >= (long long)A.batch * A.max_kf) return;
    const int b = (int)(wid / A.max_kf), i = (int)(wid % A.max_kf);
    if (A.only_ok && A.only_ok[b] != VIORB_OK) return;
    double* row = s_all + wv * PI_WAVE_DOUBLES;                // the output row: small part [0, 60), covariance [60, 141), dt
    double* S = row + 60; double* AR = row + 142; double* NB = AR + 45; double* stage = NB + 27;
    double* out = A.preint + ((size_t)b * A.max_kf + i) * 142;
    for (int k = lane; k < 142; k += 64) row[k] = (k == 6 || k == 10 || k == 14) ? 1.0 : 0.0;   // the reset pre-integrator
    WAVE_SYNC();
    int n = 0; long long s0 = 0;
    const int nk = min(A.n_kf[b], A.max_kf);
    if (i >= 1 && i < nk) {
        s0 = A.imu_start[(size_t)b * (A.max_kf + 1) + i];
        const long long s1 = A.imu_start[(size_t)b * (A.max_kf + 1) + i + 1];
        if (s0 >= 0 && s1 > s0 && s1 <= A.total_imu && s1 - s0 < (1ll << 30)) n = (int)(s1 - s0);       // anything else: the interval stays reset
    }
    if (n > 0) {
        const double t_prev = A.kf_time[(size_t)b * A.max_kf + i - 1], t_cur = A.kf_time[(size_t)b * A.max_kf + i];
        const d3 bg = A.bg ? ld3(A.bg + (size_t)b * A.bg_stride) : mk3(0, 0, 0), ba = A.ba ? ld3(A.ba + (size_t)b * A.ba_stride) : mk3(0, 0, 0);
        const double* smp = A.imu + (size_t)s0 * 7;
        // the lane's covariance entry: r <= c, packed row by row
        int r = 0, c = lane;
#pragma unroll
        for (int k = 0; k < 8; k++) if (c >= 9 - r) { c -= 9 - r; r++; }
        c += r;
        const bool owner = lane < 45;
        preint_small M;
        M.dP = mk3(0, 0, 0); M.dV = mk3(0, 0, 0); M.dR = eye3();
        M.JPg = zero3(); M.JPa = zero3(); M.JVg = zero3(); M.JVa = zero3(); M.JRg = zero3(); M.dt = 0;
        for (int base = 0; base < n; base += PI_CHUNK) {
            const int m = min(PI_CHUNK, n - base);
            WAVE_SYNC();                                     // the previous chunk has been consumed
            if (lane < 7 * m) stage[lane] = smp[(size_t)base * 7 + lane];
            else if (lane == 63) stage[63] = (base + m < n) ? smp[(size_t)(base + m) * 7 + 6] : t_cur;
            WAVE_SYNC();
            for (int k = 0; k < m; k++) {
                const double* s = stage + 7 * k;
                const d3 om = ld3(s) - bg, ac = ld3(s + 3) - ba;
                const double t_next = (k == m - 1) ? stage[63] : s[13];
                // the first sample also covers [t_prev, its stamp]
                for (int pass = (base + k == 0 ? 0 : 1); pass < 2; pass++) {
                    double d = pass == 0 ? s[6] - t_prev : t_next - s[6];
                    if (A.clamp) d = d > 0. ? d : 0.;
                    const preint_cov_blocks C = preint_step(M, om, ac, d);
                    if (lane == 0) cov_publish(AR, NB, C);
                    WAVE_SYNC();
                    const double v = owner ? cov_entry(S, AR, NB, r, c, A.gyr_cov, A.acc_cov) : 0.0;
                    WAVE_SYNC();
                    if (owner) { S[9 * r + c] = v; S[9 * c + r] = v; }        // visible after the next step's first WAVE_SYNC
                }
            }
        }
        if (lane == 0) {
            st3(row, M.dP); st3(row + 3, M.dV); stm(row + 6, M.dR); stm(row + 15, M.JPg); stm(row + 24, M.JPa);
            stm(row + 33, M.JVg); stm(row + 42, M.JVa); stm(row + 51, M.JRg); row[141] = M.dt;
        }
        WAVE_SYNC();
    }
    for (int k = lane; k < 142; k += 64) out[k] = row[k];
}

struct ViArgs {
    vi_extr X; double G;
    const int32_t* n_est; const float* twc12; const double* preint; int max_kf, min_n;
    double* bg; int bg_stride; double* est; int32_t* status;
};

template <int K> __device__ __forceinline__ void wave_sum(double (&a)[K]) {
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) a[k] += __shfl_xor(a[k], d);
}

__global__ __launch_bounds__(64) void k_vi_gyro_bias(ViArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N = A.n_est[b];
    double* bg = A.bg + (size_t)b * A.bg_stride;
    if (N < A.min_n || N > A.max_kf) {
        if (lane < 3) bg[lane] = 0.0;
        if (lane == 0) A.status[b] = VIORB_VI_INVALID;
        return;
    }
    const float* T = A.twc12 + (size_t)b * A.max_kf * 12;
    const double* P = A.preint + (size_t)b * A.max_kf * 142;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0;
    for (int i = 1 + lane; i < N; i += 64) {
        d3 e; m33 J, W; double hg[12];
        vi_gyro_edge(T + (size_t)(i - 1) * 12, T + (size_t)i * 12, A.X.Rcb, P + (size_t)i * 142, &e, &J, &W);
        vi_gyro_normal(e, J, W, hg);
#pragma unroll
        for (int k = 0; k < 12; k++) acc[k] += hg[k];
    }
    wave_sum(acc);
    d3 r;
    const bool ok = vi_gyro_solve(acc, &r);
    if (lane == 0) { st3(bg, r); A.status[b] = ok ? VIORB_OK : VIORB_VI_DEGENERATE; }
}

__global__ __launch_bounds__(64) void k_vi_solve(ViArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double* E = A.est + (size_t)b * VI_EST_DOUBLES;
    int st = A.status[b];
    const int N = A.n_est[b];
    const float* T = A.twc12 + (size_t)b * A.max_kf * 12;
    const double* P = A.preint + (size_t)b * A.max_kf * 142;
    if (st == VIORB_OK) {
        int bad = 0;
        for (int i = 1 + lane; i < N; i += 64) bad |= !(P[(size_t)i * 142 + 141] > 0.0);       // an empty interval stays reset: dt = 0
        if (__any(bad)) st = VIORB_VI_INVALID;
    }
    double x4[4], w4[4], y6[6], w6[6];
    m33 Rwi = eye3(), Rwi2 = eye3();
    if (st == VIORB_OK) {
        double acc[14];
#pragma unroll
        for (int k = 0; k < 14; k++) acc[k] = 0;
        for (int i = lane; i < N - 2; i += 64) {
            double rows[15];
            const vi_triplet t = vi_triplet_common(T + (size_t)i * 12, T + (size_t)(i + 1) * 12, T + (size_t)(i + 2) * 12, A.X, P + (size_t)(i + 1) * 142, P + (size_t)(i + 2) * 142);
            vi_rows_ab(t, rows);
            vi_gram_add<4>(rows, acc);
        }
        wave_sum(acc);
        if (vi_gram_solve<4>(acc, x4, w4)) st = VIORB_VI_DEGENERATE;
        else if (!vi_rwi_from_gravity(mk3(x4[1], x4[2], x4[3]), &Rwi)) st = VIORB_VI_DEGENERATE;
    }
    if (st == VIORB_OK) {
        double acc[27];
#pragma unroll
        for (int k = 0; k < 27; k++) acc[k] = 0;
        for (int i = lane; i < N - 2; i += 64) {
            double rows[21];
            const double *p2 = P + (size_t)(i + 1) * 142, *p3 = P + (size_t)(i + 2) * 142;
            const vi_triplet t = vi_triplet_common(T + (size_t)i * 12, T + (size_t)(i + 1) * 12, T + (size_t)(i + 2) * 12, A.X, p2, p3);
            vi_rows_cd(t, p2, p3, Rwi, A.G, rows);
            vi_gram_add<6>(rows, acc);
        }
        wave_sum(acc);
        if (vi_gram_solve<6>(acc, y6, w6)) st = VIORB_VI_DEGENERATE;
        else Rwi2 = mul(Rwi, qmat(so3_exp(mk3(y6[1], y6[2], 0.0))));
    }
    if (lane != 0) return;
    A.status[b] = st;
    if (st != VIORB_OK) {
        for (int k = 0; k < VI_EST_DOUBLES; k++) E[k] = 0.0;
        return;
    }
    E[VI_SSTAR] = x4[0]; E[VI_GWSTAR] = x4[1]; E[VI_GWSTAR + 1] = x4[2]; E[VI_GWSTAR + 2] = x4[3];
    E[VI_S] = y6[0]; E[VI_DTHETA] = y6[1]; E[VI_DTHETA + 1] = y6[2]; E[VI_BA] = y6[3]; E[VI_BA + 1] = y6[4]; E[VI_BA + 2] = y6[5];
    stm(E + VI_RWI, Rwi); stm(E + VI_RWI2, Rwi2);
    st3(E + VI_GW, mulv(Rwi2, mk3(0, 0, A.G)));
#pragma unroll
    for (int k = 0; k < 4; k++) E[VI_W4 + k] = w4[k];
#pragma unroll
    for (int k = 0; k < 6; k++) E[VI_W6 + k] = w6[k];
    for (int k = VI_W6 + 6; k < VI_EST_DOUBLES; k++) E[k] = 0.0;
}

struct ApplyArgs {
    vi_extr X;
    const int32_t* n_est; const int32_t* n_kf; const float* twc12; const float* pose12; const double* est; const int32_t* status;
    const double* preint_v; const double* preint_final; int max_kf;
    double* navstate; float* pose12_scaled;
};

__global__ __launch_bounds__(64) void k_vi_apply(ApplyArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (A.status[b] != VIORB_OK) return;                      // untouched
    const int N = A.n_est[b], K = max(N, min(A.n_kf[b], A.max_kf));
    const double* E = A.est + (size_t)b * VI_EST_DOUBLES;
    const double s = E[VI_S];
    const d3 bg = ld3(E + VI_BG), ba = ld3(E + VI_BA), gw = ld3(E + VI_GW);
    const float* T = A.twc12 + (size_t)b * A.max_kf * 12;
    const double *Pv = A.preint_v + (size_t)b * A.max_kf * 142, *Pf = A.preint_final + (size_t)b * A.max_kf * 142;
    const float sf = (float)s;
    for (int i = lane; i < K; i += 64) {
        double* ns = A.navstate + ((size_t)b * A.max_kf + i) * 22;
        pvr o;
        vi_kf_pose(T + 12 * i, A.X, s, &o.P, &o.q);
        o.V = vi_kf_velocity(i, N, K, T, A.X, s, Pv, Pf, ba, gw);
        st_pvr(ns, o);
        st3(ns + 10, bg); st3(ns + 13, ba);
#pragma unroll
        for (int k = 16; k < 22; k++) ns[k] = 0.0;
        const float* pi = A.pose12 + ((size_t)b * A.max_kf + i) * 12;
        float* po = A.pose12_scaled + ((size_t)b * A.max_kf + i) * 12;
#pragma unroll
        for (int k = 0; k < 9; k++) po[k] = pi[k];
#pragma unroll
        for (int k = 9; k < 12; k++) po[k] = pi[k] * sf;
    }
}

// x[j] *= s for j < n, float4 over the 16-byte aligned middle of the row
__device__ __forceinline__ void scale_row(float* x, long long n, float s, long long tid, long long nthreads) {
    long long head = (long long)((16 - ((uintptr_t)x & 15)) & 15) / 4;
    if (((uintptr_t)x & 3) != 0 || head > n) head = n;      // a pointer off the float grid or a short row: all head, no float4 access
    const long long n4 = (n - head) / 4;
    float4* v = (float4*)(x + head);
    for (long long j = tid; j < n4; j += nthreads) { float4 t = v[j]; t.x *= s; t.y *= s; t.z *= s; t.w *= s; v[j] = t; }
    for (long long j = tid; j < head; j += nthreads) x[j] *= s;
    for (long long j = head + 4 * n4 + tid; j < n; j += nthreads) x[j] *= s;
}
__global__ __launch_bounds__(256) void k_scale_map_points(float* points, float* min_dist, float* max_dist, const double* est, const int32_t* status, int np) {
    const int b = blockIdx.y;
    if (status[b] != VIORB_OK) return;
    const float s = (float)est[(size_t)b * VI_EST_DOUBLES + VI_S];
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nt = (long long)gridDim.x * blockDim.x;
    scale_row(points + (size_t)b * np * 3, 3ll * np, s, tid, nt);
    if (min_dist) scale_row(min_dist + (size_t)b * np, np, s, tid, nt);
    if (max_dist) scale_row(max_dist + (size_t)b * np, np, s, tid, nt);
}

} // namespace viorb

using namespace viorb;

namespace {
double gyr_or_default(double v) { return v > 0 ? v : 2.0e-3 * 2.0e-3 * 200; }           // reference src/IMU/imudata.cpp:36-37
double acc_or_default(double v) { return v > 0 ? v : 8.0e-3 * 8.0e-3 * 200; }

int launch_preint(const int32_t* n_kf, const double* kf_time, const int32_t* imu_start, const double* imu, long long total_imu, const double* bg,
                  int bg_stride, const double* ba, int ba_stride, double gyr, double acc, int flags, int max_kf, int batch, double* preint, hipStream_t st,
                  const int32_t* only_ok = nullptr) {
    PreintArgs A;
    A.only_ok = only_ok;
    A.n_kf = n_kf; A.kf_time = kf_time; A.imu_start = imu_start; A.imu = imu; A.total_imu = total_imu; A.bg = bg; A.ba = ba; A.bg_stride = bg_stride;
    A.ba_stride = ba_stride; A.gyr_cov = gyr_or_default(gyr); A.acc_cov = acc_or_default(acc); A.clamp = (flags & VIORB_PREINT_NO_CLAMP) ? 0 : 1;
    A.max_kf = max_kf; A.batch = batch; A.preint = preint;
    const long long waves = (long long)batch * max_kf;
    VIORB_LAUNCH(k_preint_intervals, (unsigned)((waves + PI_WAVES - 1) / PI_WAVES), 64 * PI_WAVES, 0, st, A);
    return VIORB_OK;
}
ViArgs vi_args(const viorb_vi_init_config* cfg, const int32_t* n_est, const float* twc12, const double* preint, int max_kf, int min_n, double* bg,
               int bg_stride, double* est, int32_t* status) {
    ViArgs A;
    A.X = vi_extrinsics(cfg->Tbc); A.G = cfg->g; A.n_est = n_est; A.twc12 = twc12; A.preint = preint; A.max_kf = max_kf; A.min_n = min_n;
    A.bg = bg; A.bg_stride = bg_stride; A.est = est; A.status = status;
    return A;
}
bool shape_ok(int max_kf, int batch) { return max_kf >= 1 && max_kf <= 4096 && batch >= 1 && batch <= (1 << 20); }
} // namespace

extern "C" {

int viorb_preintegrate_intervals_device(const int32_t* n_kf, const double* kf_time, const int32_t* imu_start, const double* imu, int64_t total_imu,
                                        const double* bg, const double* ba, double gyr_meas_cov, double acc_meas_cov, int flags, int max_kf,
                                        int batch, double* preint, void* stream) {
    VIORB_REQUIRE(n_kf && kf_time && imu_start && preint && (imu || total_imu == 0), "null array");
    VIORB_REQUIRE(shape_ok(max_kf, batch) && total_imu >= 0, "1 <= max_kf <= 4096, 1 <= batch <= 2^20, total_imu >= 0");
    VIORB_REQUIRE((flags & ~VIORB_PREINT_NO_CLAMP) == 0, "unknown flag");
    VIORB_TRY(require_device());
    return launch_preint(n_kf, kf_time, imu_start, imu, total_imu, bg, 3, ba, 3, gyr_meas_cov, acc_meas_cov, flags, max_kf, batch, preint, (hipStream_t)stream);
}

int viorb_preintegrate_intervals(int n_kf, const double* kf_time, const int32_t* imu_start, const double* imu, const double bg[3], const double ba[3],
                                 double gyr_meas_cov, double acc_meas_cov, int flags, double* preint) {
    VIORB_REQUIRE(n_kf >= 1 && n_kf <= 4096 && kf_time && imu_start && preint, "1 <= n_kf <= 4096, arrays not null");
    const int32_t total = imu_start[n_kf];
    VIORB_REQUIRE(total >= 0 && (imu || total == 0), "imu_start[n_kf] = number of samples");
    VIORB_TRY(require_device());
    DeviceBufs B;
    int32_t* dn = B.up(&n_kf, 1, 1); double* dt = B.up(kf_time, n_kf, n_kf); int32_t* ds = B.up(imu_start, (size_t)n_kf + 1);
    double* di = B.up(imu, (size_t)total * 7); double* dbg = bg ? B.up(bg, 3, 3) : nullptr; double* dba = ba ? B.up(ba, 3, 3) : nullptr;
    double* dp = B.zeros<double>((size_t)n_kf * 142);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_preintegrate_intervals_device(dn, dt, ds, di, total, dbg, dba, gyr_meas_cov, acc_meas_cov, flags, n_kf, 1, dp, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_HIP_TRY(hipMemcpy(preint, dp, sizeof(double) * 142 * n_kf, hipMemcpyDeviceToHost));
    return VIORB_OK;
}

int viorb_optimize_initial_gyro_bias_device(const viorb_vi_init_config* cfg, const int32_t* n_est, const float* twc12, const double* preint_in,
                                            int max_kf, int batch, double* bg, int32_t* status, void* stream) {
    VIORB_REQUIRE(cfg && n_est && twc12 && preint_in && bg && status, "null argument");
    VIORB_REQUIRE(shape_ok(max_kf, batch), "1 <= max_kf <= 4096, 1 <= batch <= 2^20");
    VIORB_TRY(require_device());
    VIORB_LAUNCH(k_vi_gyro_bias, batch, 64, 0, (hipStream_t)stream, vi_args(cfg, n_est, twc12, preint_in, max_kf, 2, bg, 3, nullptr, status));
    return VIORB_OK;
}

int viorb_optimize_initial_gyro_bias(const viorb_vi_init_config* cfg, int n, const float* twc12, const double* preint_in, double bg[3], int32_t* status) {
    VIORB_REQUIRE(cfg && twc12 && preint_in && bg && status && n >= 1 && n <= 4096, "null argument or n outside 1..4096");
    VIORB_TRY(require_device());
    DeviceBufs B;
    int32_t* dn = B.up(&n, 1, 1); float* dT = B.up(twc12, (size_t)n * 12); double* dP = B.up(preint_in, (size_t)n * 142);
    double* db = B.zeros<double>(3); int32_t* ds = B.zeros<int32_t>(1);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_optimize_initial_gyro_bias_device(cfg, dn, dT, dP, n, 1, db, ds, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_HIP_TRY(hipMemcpy(bg, db, sizeof(double) * 3, hipMemcpyDeviceToHost));
    VIORB_HIP_TRY(hipMemcpy(status, ds, sizeof(int32_t), hipMemcpyDeviceToHost));
    return VIORB_OK;
}

int viorb_vi_init_device(const viorb_vi_init_config* cfg, const int32_t* n_est, const double* kf_time, const int32_t* imu_start, const double* imu,
                         int64_t total_imu, const float* twc12, const double* preint_in, int max_kf, int batch, double* est, int32_t* status,
                         double* preint_bg, void* stream) {
    VIORB_REQUIRE(cfg && n_est && kf_time && imu_start && twc12 && preint_in && est && status && (imu || total_imu == 0), "null argument");
    VIORB_REQUIRE(preint_bg, "preint_bg: the re-integration is an output and the call's only work array");
    VIORB_REQUIRE(shape_ok(max_kf, batch) && total_imu >= 0, "1 <= max_kf <= 4096, 1 <= batch <= 2^20, total_imu >= 0");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    // step 1: bg into est[b][0..2], INVALID for n_est < 4
    VIORB_LAUNCH(k_vi_gyro_bias, batch, 64, 0, st, vi_args(cfg, n_est, twc12, preint_in, max_kf, 4, est, VI_EST_DOUBLES, est, status));
    // KeyFrameInit::ComputePreInt with the new gyro bias: no accelerometer bias, dt clamped (src/LocalMapping.cc:58-94, 285-292)
    const int rc = launch_preint(n_est, kf_time, imu_start, imu, total_imu, est, VI_EST_DOUBLES, nullptr, 0, cfg->gyr_meas_cov, cfg->acc_meas_cov, 0, max_kf,
                                 batch, preint_bg, st);
    if (rc != VIORB_OK) return rc;
    VIORB_LAUNCH(k_vi_solve, batch, 64, 0, st, vi_args(cfg, n_est, twc12, preint_bg, max_kf, 4, est, VI_EST_DOUBLES, est, status));
    return VIORB_OK;
}

int viorb_vi_init(const viorb_vi_init_config* cfg, int n_est, const double* kf_time, const int32_t* imu_start, const double* imu, const float* twc12,
                  const double* preint_in, double est[48], int32_t* status, double* preint_bg) {
    VIORB_REQUIRE(cfg && kf_time && imu_start && twc12 && preint_in && est && status && n_est >= 1 && n_est <= 4096, "null argument or n_est outside 1..4096");
    const int32_t total = imu_start[n_est];
    VIORB_REQUIRE(total >= 0 && (imu || total == 0), "imu_start[n_est] = number of samples");
    VIORB_TRY(require_device());
    DeviceBufs B;
    int32_t* dn = B.up(&n_est, 1, 1); double* dt = B.up(kf_time, n_est); int32_t* ds = B.up(imu_start, (size_t)n_est + 1);
    double* di = B.up(imu, (size_t)total * 7); float* dT = B.up(twc12, (size_t)n_est * 12); double* dP = B.up(preint_in, (size_t)n_est * 142);
    double* de = B.zeros<double>(VI_EST_DOUBLES); int32_t* dst = B.zeros<int32_t>(1);
    double* dq = B.zeros<double>((size_t)n_est * 142);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_vi_init_device(cfg, dn, dt, ds, di, total, dT, dP, n_est, 1, de, dst, dq, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_HIP_TRY(hipMemcpy(est, de, sizeof(double) * VI_EST_DOUBLES, hipMemcpyDeviceToHost));
    VIORB_HIP_TRY(hipMemcpy(status, dst, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (preint_bg) VIORB_HIP_TRY(hipMemcpy(preint_bg, dq, sizeof(double) * 142 * n_est, hipMemcpyDeviceToHost));
    return VIORB_OK;
}

int viorb_vi_init_apply_device(const viorb_vi_init_config* cfg, const int32_t* n_est, const int32_t* n_kf, const double* kf_time, const int32_t* imu_start,
                               const double* imu, int64_t total_imu, const float* twc12, const float* pose12, const double* est, const int32_t* status,
                               const double* preint_v, int max_kf, int batch, double* navstate, float* pose12_scaled, double* preint, void* stream) {
    VIORB_REQUIRE(cfg && n_est && n_kf && kf_time && imu_start && twc12 && pose12 && est && status && preint_v && navstate && pose12_scaled && preint &&
                  (imu || total_imu == 0), "null argument");
    VIORB_REQUIRE(preint != preint_v, "preint (out) must not be the array the velocities are read from");
    VIORB_REQUIRE(shape_ok(max_kf, batch) && total_imu >= 0, "1 <= max_kf <= 4096, 1 <= batch <= 2^20, total_imu >= 0");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    // KeyFrame::ComputePreInt with the new biases, no clamp (src/LocalMapping.cc:683-688, 729-735), for the streams that are OK
    const int rc = launch_preint(n_kf, kf_time, imu_start, imu, total_imu, est + VI_BG, VI_EST_DOUBLES, est + VI_BA, VI_EST_DOUBLES, cfg->gyr_meas_cov,
                                 cfg->acc_meas_cov, VIORB_PREINT_NO_CLAMP, max_kf, batch, preint, st, status);
    if (rc != VIORB_OK) return rc;
    ApplyArgs A;
    A.X = vi_extrinsics(cfg->Tbc); A.n_est = n_est; A.n_kf = n_kf; A.twc12 = twc12; A.pose12 = pose12; A.est = est; A.status = status; A.preint_v = preint_v;
    A.preint_final = preint; A.max_kf = max_kf; A.navstate = navstate; A.pose12_scaled = pose12_scaled;
    VIORB_LAUNCH(k_vi_apply, batch, 64, 0, st, A);
    return VIORB_OK;
}

int viorb_vi_init_apply(const viorb_vi_init_config* cfg, int n_est, int n_kf, const double* kf_time, const int32_t* imu_start, const double* imu,
                        const float* twc12, const float* pose12, const double est[48], const double* preint_v, double* navstate, float* pose12_scaled,
                        double* preint) {
    VIORB_REQUIRE(cfg && kf_time && imu_start && twc12 && pose12 && est && preint_v && navstate && pose12_scaled && preint, "null argument");
    VIORB_REQUIRE(n_est >= 4 && n_kf >= n_est && n_kf <= 4096, "4 <= n_est <= n_kf <= 4096");
    const int32_t total = imu_start[n_kf];
    VIORB_REQUIRE(total >= 0 && (imu || total == 0), "imu_start[n_kf] = number of samples");
    VIORB_TRY(require_device());
    DeviceBufs B;
    const int32_t ok = VIORB_OK;
    int32_t *dne = B.up(&n_est, 1, 1), *dnk = B.up(&n_kf, 1, 1), *dst = B.up(&ok, 1, 1), *ds = B.up(imu_start, (size_t)n_kf + 1);
    double *dt = B.up(kf_time, n_kf), *di = B.up(imu, (size_t)total * 7), *de = B.up(est, VI_EST_DOUBLES), *dv = B.up(preint_v, (size_t)n_kf * 142);
    float *dT = B.up(twc12, (size_t)n_kf * 12), *dp = B.up(pose12, (size_t)n_kf * 12), *dq = B.zeros<float>((size_t)n_kf * 12);
    double *dn = B.zeros<double>((size_t)n_kf * 22), *dr = B.zeros<double>((size_t)n_kf * 142);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_vi_init_apply_device(cfg, dne, dnk, dt, ds, di, total, dT, dp, de, dst, dv, n_kf, 1, dn, dq, dr, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_HIP_TRY(hipMemcpy(navstate, dn, sizeof(double) * 22 * n_kf, hipMemcpyDeviceToHost));
    VIORB_HIP_TRY(hipMemcpy(pose12_scaled, dq, sizeof(float) * 12 * n_kf, hipMemcpyDeviceToHost));
    VIORB_HIP_TRY(hipMemcpy(preint, dr, sizeof(double) * 142 * n_kf, hipMemcpyDeviceToHost));
    return VIORB_OK;
}

int viorb_scale_map_points_device(float* points, float* min_dist, float* max_dist, const double* est, const int32_t* status, int np, int batch, void* stream) {
    VIORB_REQUIRE(points && est && status, "null argument");
    VIORB_REQUIRE(np >= 0 && batch >= 1 && batch <= 65535, "np >= 0, 1 <= batch <= 65535");
    VIORB_TRY(require_device());
    if (np == 0) return VIORB_OK;
    const int blocks = std::max(1, std::min(64, (3 * np / 4 + 255) / 256));
    VIORB_LAUNCH(k_scale_map_points, dim3(blocks, batch), 256, 0, (hipStream_t)stream, points, min_dist, max_dist, est, status, np);
    return VIORB_OK;
}

// ---- host-only hooks: vi_init_core.h compiled for the host -----------------------------------------------------------------------
void viorb_debug_vi_init_gyro_edge(const double* Tbc16, const float* twc_i12, const float* twc_j12, const double* preint142, double* e3, double* J9,
                                   double* Hg12) {
    const vi_extr X = vi_extrinsics(Tbc16);
    d3 e; m33 J, W;
    vi_gyro_edge(twc_i12, twc_j12, X.Rcb, preint142, &e, &J, &W);
    st3(e3, e); stm(J9, J);
    if (Hg12) vi_gyro_normal(e, J, W, Hg12);
}
int viorb_debug_vi_init_gyro_solve(const double* Hg12, double* bg3) {
    d3 r;
    const bool ok = vi_gyro_solve(Hg12, &r);
    st3(bg3, r);
    return ok ? VIORB_OK : VIORB_VI_DEGENERATE;
}
void viorb_debug_vi_init_rows(const double* Tbc16, const float* twc36, const double* preint2, const double* preint3, const double* Rwi9, double g,
                              double* rows_ab15, double* rows_cd21) {
    const vi_extr X = vi_extrinsics(Tbc16);
    const vi_triplet t = vi_triplet_common(twc36, twc36 + 12, twc36 + 24, X, preint2, preint3);
    vi_rows_ab(t, rows_ab15);
    vi_rows_cd(t, preint2, preint3, ldm(Rwi9), g, rows_cd21);
}
int viorb_debug_vi_init_solve(const double* M, const double* v, int m, int n, double* x, double* w) {
    if (!M || !v || !x || !w || m < 1 || (n != 4 && n != 6)) return VIORB_ERR_INVALID_ARG;
    double acc[27] = {0};
    for (int r0 = 0; r0 < m; r0 += 3) {                      // three rows at a time, as a key-frame triplet delivers them
        double rows[21] = {0};
        for (int r = r0; r < std::min(m, r0 + 3); r++) {
            for (int c = 0; c < n; c++) rows[(n + 1) * (r - r0) + c] = M[(size_t)r * n + c];
            rows[(n + 1) * (r - r0) + n] = v[r];
        }
        if (n == 4) vi_gram_add<4>(rows, acc); else vi_gram_add<6>(rows, acc);
    }
    const int bad = n == 4 ? vi_gram_solve<4>(acc, x, w) : vi_gram_solve<6>(acc, x, w);
    return bad ? VIORB_VI_DEGENERATE : VIORB_OK;
}
void viorb_debug_vi_init_navstate(const double* Tbc16, int i, int n_est, int n_kf, const float* twc12, const double* est48, const double* preint_v,
                                  const double* preint_final, double* ns22) {
    const vi_extr X = vi_extrinsics(Tbc16);
    const d3 bg = ld3(est48 + VI_BG), ba = ld3(est48 + VI_BA), gw = ld3(est48 + VI_GW);
    pvr o;
    vi_kf_pose(twc12 + 12 * i, X, est48[VI_S], &o.P, &o.q);
    o.V = vi_kf_velocity(i, n_est, n_kf, twc12, X, est48[VI_S], preint_v, preint_final, ba, gw);
    st_pvr(ns22, o); st3(ns22 + 10, bg); st3(ns22 + 13, ba);
    for (int k = 16; k < 22; k++) ns22[k] = 0.0;
}
int viorb_debug_vi_init_rwi(const double* gwstar3, double* Rwi9) {
    m33 R;
    if (!vi_rwi_from_gravity(ld3(gwstar3), &R)) return VIORB_VI_DEGENERATE;
    stm(Rwi9, R);
    return VIORB_OK;
}

} // extern "C"
