// ---------------------------------------------------------------------------------------------
// k_pose_opt_vi_mp<P, WPP>: Optimizer::PoseOptimization(Frame*, KeyFrame* | Frame*, IMUPreintegrator, gw, bComputeMarg) (reference
// src/Optimizer.cc:323-1112) with P problems per workgroup, WPP wavefronts per problem, advanced in LOCK STEP one evaluation ("tick") at a
// time. Unknowns x = [cur PVR(9) | cur bias(3) | last PVR(9) | last bias(3)] (n = 24, Frame / Frame overload with its prior edge) or
// [cur PVR(9) | cur bias(3)] (n = 12, Frame / KeyFrame overload: the key frame is fixed). Rounds 1-3 ran one 256-thread workgroup per
// problem (k_pose_opt_vi, removed in round 4); the arithmetic per value is that kernel's (same helpers, same operation order inside a
// wavefront), what changed is who executes it:
//   * the scalar phases of an evaluation — the IMU factor (three pieces), the prior factor, NavState::IncSmallPVR and the bias update —
//     were one LANE of one wavefront per problem: ~3 k wave-instructions per evaluation at 1/64 lane efficiency (tools/ubench/valu_rate:
//     a wave64 instruction costs its 4 SIMD cycles however many lanes are on). Here wavefront w runs piece w for ALL problems of the
//     workgroup, one problem per lane: the same instruction stream serves P problems;
//   * a problem's reprojection edges are dealt to its WPP wavefronts (chunks of 64, two per trip), so a problem pays WPP transpose-
//     reductions per frame instead of four, and the normal-equation assembly / Cholesky / LM decision run on the problem's own wavefronts;
//   * g2o's nested loops (4 rounds x <= 10 iterations x <= 10 trials, Optimizer.cc:600-690, optimization_algorithm_levenberg.cpp:61-189)
//     are flattened into ticks: a tick is [solve + update unless it is the first evaluation of a round] -> evaluate + linearise ->
//     Levenberg decision -> [re-classification of the edges when the round ended]. Every problem of the workgroup executes every barrier
//     of a tick; a finished problem idles. The LM state of a problem is decided by its first wavefront and published through LDS.
// Instantiations: <1, 4> is the round-3 mapping (one problem per 256-thread workgroup); <2, 2> and <4, 2> share the scalar phases between
// two / four problems with two wavefronts each; <4, 1> is one wavefront per problem.
// ---------------------------------------------------------------------------------------------
template <int WPP> struct PoseMpProblem {
    double Hb[2][24 * 24], bb[2][24], x[24];               // two normal-equation buffers: current system / speculative next
    // IMU / prior factor Jacobians and Omega*J; the packed lower triangle of L (300 doubles) of the Cholesky solve lives in OJ1 | OJ2 (333,
    // dead between the assembly and the next evaluation; J1 / J2 keep their static zero pattern), the 24 x 24 work matrix of the final
    // marginalisation spans all four (666 >= 576). The order of the four arrays matters.
    double J1[9 * 21], J2[12 * 12], OJ1[9 * 21], OJ2[12 * 12];
    double e1[12], e2[12], q[32];
    double oe1[12], oe2[12], dump[64];                     // Omega e of the two dense factors; where results outside a product are stored (matrix-core assembly)
    double info_pvr[81], info_prior[144];
    double red[WPP][2][28];                                 // per wave, per frame: 21 G + 6 g + chi
    double est[2][10], bias[2][3], bak[2][10], bakb[2][3], base_ba[2][3];
    double ev[2][10];                                       // P V q of the last evaluation (g2o's stored edge errors belong to this state)
    double sc[16];                                          // 0 chi total, 3 bias weight, 4-6 bias error, 7 last chi, 8 bias rho, 9 / 10 robust chi2 of the IMU / prior factor
    double pre[64], gw[3], dbg[3], cpv[6], corrT[4], pri[13];
    double GT[2][36], b6[2][6];
    double lm[4];                                           // lambda, ni, currentChi, iniChi (published by the deciding wavefront)
    int lmi[12];                                            // 0 variant, 1 it, 2 qmax, 3 nBadLM, 4 cur, 5 hb_last, 6 mode, 9 end_round, 10 the round's last trial was rejected
    int flag[4];                                            // 0 solve ok, 1 LM iterations, 2 bad-edge counter
};
template <int P, int WPP> struct PoseMpShared {
    PoseMpProblem<WPP> p[P];
    double T6[36];
    uint32_t tab[2][324][2];                                // assembly tables of the two variants (n = 12, n = 24)
    int alive[P];
};

// Cholesky solve of (H + lambda I) x = b as wave_solve_reg, with L kept as a PACKED lower triangle (Lp[r (r + 1) / 2 + c], 300 doubles for
// N = 24) for the back substitution.
template <int N>
__device__ bool wave_solve_reg_packed(const double* __restrict__ H, const double* __restrict__ bvec, double lambda,
                                      double* __restrict__ Lp, double* __restrict__ x, int lane) {
    const int li = lane < N ? lane : N - 1;
    double a[N], myinv = 0.0;                               // 1 / L[j][j] stays with lane j (an array of N of them per lane was 2 N registers at the kernel's register peak)
#pragma unroll
    for (int c = 0; c < N; c++) a[c] = H[li * N + c];
    double rhs = bvec[li];
    LDS_READS_DONE();
#pragma unroll
    for (int c = 0; c < N; c++) a[c] += ((c == li) ? lambda : 0.0);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const double d = readlane_d(a[j], j);
        double row[N];
#pragma unroll
        for (int k = j + 1; k < N; k++) row[k] = readlane_d(a[k], j);
        ok = ok && (d > 0.0) && isfinite(d);
        const double inv = rsqrt_nr(d);
        myinv = lane == j ? inv : myinv;
        const double lij = a[j] * inv;
        a[j] = lij;
        const double yj = readlane_d(rhs, j) * inv;
        if (lane == j) rhs = yj; else if (lane > j) rhs = fma(-lij, yj, rhs);
        const double m = lij * inv;
#pragma unroll
        for (int k = j + 1; k < N; k++) a[k] = fma(-m, row[k], a[k]);
    }
    const int rbase = li * (li + 1) / 2;
#pragma unroll
    for (int c = 0; c < N; c++) if (c <= li && lane < N) Lp[rbase + c] = a[c];
    WAVE_LDS_SYNC();
    double col[N];
#pragma unroll
    for (int j = 0; j < N; j++) col[j] = Lp[j * (j + 1) / 2 + (li <= j ? li : 0)];      // L[j][i], only used by lanes i < j
    LDS_READS_DONE();
    double acc = rhs;
#pragma unroll
    for (int j = N - 1; j >= 0; j--) {
        const double xj = readlane_d(acc, j) * readlane_d(myinv, j);
        if (lane == j) acc = xj; else if (lane < j) acc = fma(-col[j], xj, acc);
    }
    if (lane < N) x[lane] = acc;
    return ok;
}


// Sum of 32 per-lane values over the 64 lanes of a wavefront by transpose-reduction (16 + 8 + 4 + 2 + 1 exchanges leave lane l with the wave
// total of value (l >> 1) & 31, one more exchange pairs the two copies), without LDS: the two widest levels by v_permlane32_swap /
// v_permlane16_swap (gfx950: a swap of the upper half of one register with the lower half of another IS the exchange step, no select), the
// four narrow levels by DPP moves inside a row (row_ror:8, row_half_mirror, quad_perm). __shfl_xor goes through ds_bpermute: six dependent
// LDS round trips, 2.2 k cycles per reduction where the instructions need 0.9 k (-DVIORB_POSE_TIMING).
__device__ __forceinline__ double dpp_mov_d(double v, const int ctrl_sel) {
    union { double d; int i[2]; } a, r; a.d = v;
    switch (ctrl_sel) {      // compile-time constant after inlining
        case 8: r.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], 0x128, 0xf, 0xf, false); r.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], 0x128, 0xf, 0xf, false); break;   // row_ror:8 = lane ^ 8
        case 4: r.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], 0x141, 0xf, 0xf, false); r.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], 0x141, 0xf, 0xf, false); break;   // row_half_mirror = lane ^ 7
        case 2: r.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], 0x4e, 0xf, 0xf, false); r.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], 0x4e, 0xf, 0xf, false); break;     // quad_perm [2,3,0,1] = lane ^ 2
        default: r.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], 0xb1, 0xf, 0xf, false); r.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], 0xb1, 0xf, 0xf, false); break;    // quad_perm [1,0,3,2] = lane ^ 1
    }
    return r.d;
}
template <int WIDE32> __device__ __forceinline__ double swap_add_d(double a, double b) {
    // after the swap a = [a.lo | b.lo], b = [a.hi | b.hi] (halves of 32 lanes, or odd / even rows of 16): a + b is the exchange step
    typedef unsigned uint2v __attribute__((ext_vector_type(2)));
    union { double d; unsigned i[2]; } x, y; x.d = a; y.d = b;
    uint2v r0, r1;
    if (WIDE32) { r0 = __builtin_amdgcn_permlane32_swap(x.i[0], y.i[0], false, false); r1 = __builtin_amdgcn_permlane32_swap(x.i[1], y.i[1], false, false); }
    else { r0 = __builtin_amdgcn_permlane16_swap(x.i[0], y.i[0], false, false); r1 = __builtin_amdgcn_permlane16_swap(x.i[1], y.i[1], false, false); }
    x.i[0] = r0[0]; y.i[0] = r0[1]; x.i[1] = r1[0]; y.i[1] = r1[1];
    return x.d + y.d;
}
__device__ __forceinline__ double wave_transpose_reduce32(double (&v)[32], int lane) {
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = swap_add_d<1>(v[i], v[16 + i]);
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = swap_add_d<0>(v[i], v[8 + i]);
    {
        const bool up = (lane & 8) != 0;
#pragma unroll
        for (int i = 0; i < 4; i++) { const double keep = up ? v[4 + i] : v[i], send = up ? v[i] : v[4 + i]; v[i] = keep + dpp_mov_d(send, 8); }
    }
    {
        const bool up = (lane & 4) != 0;
#pragma unroll
        for (int i = 0; i < 2; i++) { const double keep = up ? v[2 + i] : v[i], send = up ? v[i] : v[2 + i]; v[i] = keep + dpp_mov_d(send, 4); }
    }
    {
        const bool up = (lane & 2) != 0;
        const double keep = up ? v[1] : v[0], send = up ? v[0] : v[1];
        v[0] = keep + dpp_mov_d(send, 2);
    }
    return v[0] + dpp_mov_d(v[0], 1);
}

#ifdef VIORB_POSE_TIMING
#define MPT_DECL unsigned long long mpt_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, mpt_t0 = __builtin_amdgcn_s_memtime(); const unsigned long long mpt_begin = mpt_t0; int mpt_ticks = 0
#define MPT_LAP(k) do { const unsigned long long mpt_now = __builtin_amdgcn_s_memtime(); mpt_acc[k] += mpt_now - mpt_t0; mpt_t0 = mpt_now; } while (0)
#else
#define MPT_DECL
#define MPT_LAP(k)
#endif
#ifndef POSE_ASM_MFMA
#define POSE_ASM_MFMA 1            // Omega J of the dense factors on the matrix cores (0: the work-item form)
#endif
#ifndef POSE_EDGE_ILP
#define POSE_EDGE_ILP 1            // edges per lane and trip of the edge loop. 2 = two interleaved chains: 245 registers instead of 215, i.e. two resident solver wavefronts leave a SIMD 16 registers instead of 80 and the extraction stream stalls for the whole solve (resize 455 us instead of 75): 179.0 k against 182.7 k frames/s
#endif
#ifndef POSE_MIN_WAVES
#define POSE_MIN_WAVES 2          // wavefronts per SIMD the register allocation leaves room for (2: <= 256 registers per lane)
#endif
#ifdef POSE_NUM_VGPR
#define POSE_VGPR_ATTR __attribute__((amdgpu_num_vgpr(POSE_NUM_VGPR)))
#else
#define POSE_VGPR_ATTR
#endif
template <int P, int WPP>
__global__ __launch_bounds__(64 * P * WPP, POSE_MIN_WAVES) POSE_VGPR_ATTR void k_pose_opt_vi_mp(PoseOptArgs A, int batch) {
    constexpr int PT = 64 * WPP, NW = P * WPP, NT = 64 * NW;
#ifndef POSE_WAVE_PRIO
#define POSE_WAVE_PRIO 3
#endif
    // Issue priority: a solve is a chain of latency-bound phases on four wavefronts per CU, and the step waits for it (the tracking chain is
    // the step's period) while the extraction stream's hundreds of throughput-bound wavefronts share the SIMDs; a ready instruction of this
    // kernel goes first, which costs the other stream a fraction of a percent of its issue slots.
    __builtin_amdgcn_s_setprio(POSE_WAVE_PRIO);
    MPT_DECL;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_pose_mp[];
    PoseMpShared<P, WPP>& SH = *reinterpret_cast<PoseMpShared<P, WPP>*>(s_pose_mp);
    const int t = threadIdx.x, lane = t & 63, cap = A.cap;
    // the wavefront index as a SCALAR: everything derived from it (the problem, its pointers, counts and LDS block) then lives in SGPRs, as
    // blockIdx-derived values would; taken from threadIdx alone the compiler keeps all of it in vector registers (+40 VGPRs, spills)
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), p = wave / WPP, pw = wave % WPP, pt = pw * 64 + lane;
    const int b_raw = blockIdx.x * P + p;
    const bool exists = b_raw < batch;
    const int b = exists ? b_raw : batch - 1;
    PoseMpProblem<WPP>& S = SH.p[p];
    const int variant = A.variant_arr ? (A.variant_arr[b] ? 1 : 0) : A.variant, n = variant ? 24 : 12;
    const bool skipped = A.skip && A.skip[b];
    const int ncur_all = min(A.n_cur[b], cap);
    const int ncur = skipped ? 0 : ncur_all, nlast = variant ? min(A.n_last[b], cap) : 0;
    const double* obs_c = A.obs_cur + (size_t)b * cap * 6;
    const double* obs_l = A.obs_last ? A.obs_last + (size_t)b * cap * 6 : nullptr;
    uint8_t* out_c = A.outlier_cur + (size_t)b * cap;
    uint8_t* out_l = A.outlier_last ? A.outlier_last + (size_t)b * cap : nullptr;
    const double* curns = A.cur_ns + (size_t)b * 22;
    const double* lastns = A.last_ns + (size_t)b * 22;
    const double* pre = A.preint + (size_t)b * 142;
    const double* priorns = variant ? A.prior_ns + (size_t)b * 22 : nullptr;
    const cam_t K = ld_cam(A.cam);
    const double d_mono = (double)(float)sqrt(5.991), d_pvr = (double)(float)sqrt(21.666), d_bias = (double)(float)sqrt(16.812),
                 d_prior = (double)(float)sqrt(30.5779);
    const double bias_info = 1.0 / A.acc_bias_rw2 / pre[141];
    struct obs_t { d3 X; double u, v, is2; };
    auto load_obs = [&](const double* ob, int i) {
        const double2* q = reinterpret_cast<const double2*>(ob) + 3 * i;
        const double2 q0 = q[0], q1 = q[1], q2 = q[2];
        obs_t o; o.X = mk3(q0.x, q0.y, q1.x); o.u = q1.y; o.v = q2.x; o.is2 = q2.y;
        return o;
    };
    // ---- setup (every barrier is executed by every thread of the workgroup)
    if (exists) {
        for (int i = pt; i < ncur_all; i += PT) out_c[i] = 0;
        for (int i = pt; i < nlast; i += PT) out_l[i] = 0;
    }
    {   // information of the IMU factor: cov^-1 + diag(1e2,1,1e2) (x) I3, Gauss-Jordan without pivoting (SPD), per problem
        double* a = S.Hb[0]; double* inv = S.Hb[0] + 96;
        for (int i = pt; i < 81; i += PT) { a[i] = pre[60 + i]; inv[i] = (i / 9 == i % 9) ? 1.0 : 0.0; }
        __syncthreads();
        constexpr int NI = (162 + PT - 1) / PT;
        for (int col = 0; col < 9; col++) {
            const double piv = a[col * 9 + col];
            __syncthreads();
            for (int i = pt; i < 18; i += PT) { if (i < 9) a[col * 9 + i] /= piv; else inv[col * 9 + i - 9] /= piv; }
            __syncthreads();
            double f[NI];
#pragma unroll
            for (int k = 0; k < NI; k++) { const int i = pt + k * PT, el = i % 81, r = el / 9; f[k] = i < 162 ? a[r * 9 + col] : 0.0; }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < NI; k++) {
                const int i = pt + k * PT, which = i / 81, el = i % 81, r = el / 9, c = el % 9;
                double* M = which ? inv : a;
                if (i < 162 && r != col) M[r * 9 + c] -= f[k] * M[col * 9 + c];
            }
            __syncthreads();
        }
        for (int i = pt; i < 81; i += PT) {
            const int r = i / 9, c = i % 9;
            S.info_pvr[i] = inv[i] + ((r == c) ? ((r < 3 || r >= 6) ? 1e2 : 1.0) : 0.0);
        }
    }
    if (variant) {
        const double* mc = A.marg_cov_inv + (size_t)b * 144;
        for (int i = pt; i < 144; i += PT) {
            const int r = i / 12, c = i % 12;
            S.info_prior[i] = mc[i] + ((r == c && r < 9) ? ((r < 3 || r >= 6) ? 1e2 : 1.0) : 0.0);
        }
    }
    for (int i = pt; i < 189; i += PT) S.J1[i] = 0;                  // the factors' Jacobians keep a static zero pattern
    for (int i = pt; i < 144; i += PT) S.J2[i] = 0;
    for (int i = pt; i < 64; i += PT) { if (i < 61) S.pre[i] = i < 60 ? pre[i] : pre[141]; else { S.gw[i - 61] = A.gw[i - 61]; S.dbg[i - 61] = lastns[16 + i - 61]; } }
    if (pt == 0) {
        for (int k = 0; k < 3; k++) { S.base_ba[0][k] = curns[13 + k]; S.base_ba[1][k] = lastns[13 + k]; }
        S.flag[1] = 0; S.lmi[0] = variant;
    }
    // Assembly tables of both variants, once per workgroup: work item q < n (n + 1) / 2 is the lower-triangle entry (R, C) of H, the next n items
    // are b[R]. Word 0: R | C << 5 | isb << 10 | reduction index << 11 (31 = no reprojection term) | frame of R << 16 | IMU-factor column of R << 17 |
    // IMU-factor column of C << 22 (31 = none) | bias-factor sign << 27 (0 none, 1 +, 2 -) | bias component << 29; word 1: prior-factor column of
    // R | of C << 4 (15 = none) | index of R in its frame's (dP, dPhi) block << 8 | of C << 11.
    for (int vv = 0; vv < 2; vv++) {
        const int nn = vv ? 24 : 12, ntri = nn * (nn + 1) / 2;
        for (int q = t; q < ntri + nn; q += NT) {
            const bool isb = q >= ntri;
            int R, Cc;
            if (isb) { R = q - ntri; Cc = 0; }
            else {
                R = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
                while (R * (R + 1) / 2 > q) R--;
                while ((R + 1) * (R + 2) / 2 <= q) R++;
                Cc = q - R * (R + 1) / 2;
            }
            auto six = [](int x) { const int r = x % 12; return r < 3 ? r : (r >= 6 && r < 9 ? r - 3 : -1); };
            auto imu_col = [](int x) { return x < 9 ? 9 + x : (x >= 12 && x < 21 ? x - 12 : (x >= 21 ? 18 + x - 21 : 31)); };
            auto bias_of = [](int x) { return (x >= 9 && x < 12) ? x - 9 : (x >= 21 ? x - 21 : -1); };
            const int sideR = R / 12, r6 = six(R);
            int redk = 31;
            if (isb) { if (r6 >= 0) redk = 21 + r6; }
            else {
                const int c6 = six(Cc);
                if (sideR == Cc / 12 && r6 >= 0 && c6 >= 0) { const int lo6 = min(r6, c6), hi6 = max(r6, c6); redk = lo6 * 6 - lo6 * (lo6 - 1) / 2 + (hi6 - lo6); }
            }
            const int mR = imu_col(R), mC = isb ? 31 : imu_col(Cc);
            const int bR = bias_of(R);
            int bsign = 0;
            if (bR >= 0) {
                if (isb) bsign = R < 12 ? 2 : 1;
                else if (bias_of(Cc) == bR) bsign = ((Cc < 12) == (R < 12)) ? 1 : 2;
            }
            const int pR = (vv && R >= 12) ? R - 12 : 15, pC = (!isb && vv && Cc >= 12) ? Cc - 12 : 15;
            SH.tab[vv][q][0] = (uint32_t)R | ((uint32_t)Cc << 5) | ((uint32_t)isb << 10) | ((uint32_t)redk << 11) | ((uint32_t)sideR << 16) | ((uint32_t)mR << 17) |
                               ((uint32_t)mC << 22) | ((uint32_t)bsign << 27) | ((uint32_t)(bR < 0 ? 0 : bR) << 29);
            const int c6t = isb ? 0 : six(Cc);
            SH.tab[vv][q][1] = (uint32_t)pR | ((uint32_t)pC << 4) | ((uint32_t)(r6 < 0 ? 0 : r6) << 8) | ((uint32_t)(c6t < 0 ? 0 : c6t) << 11);
        }
    }
    if (t == NT - 1) {                                                    // T = [Rcb, -hat(Rcb Pbc) Rcb; 0, Rcb]
        const m33 HR = mul(hat3(K.RcbPbc), K.Rcb);
        const double Rm[9] = {K.Rcb.a00, K.Rcb.a01, K.Rcb.a02, K.Rcb.a10, K.Rcb.a11, K.Rcb.a12, K.Rcb.a20, K.Rcb.a21, K.Rcb.a22};
        const double Hm[9] = {HR.a00, HR.a01, HR.a02, HR.a10, HR.a11, HR.a12, HR.a20, HR.a21, HR.a22};
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                SH.T6[r * 6 + c] = Rm[r * 3 + c]; SH.T6[r * 6 + 3 + c] = -Hm[r * 3 + c];
                SH.T6[(r + 3) * 6 + c] = 0; SH.T6[(r + 3) * 6 + 3 + c] = Rm[r * 3 + c];
            }
    }
    __syncthreads();
    if (pt == 0) imu_constants(S.pre, S.dbg, S.cpv, S.corrT);
    else if (pt == PT - 1 && variant) {
        prior_constants(priorns, S.pri);
        for (int r = 0; r < 3; r++) { S.J2[(3 + r) * 12 + 3 + r] = -1; S.J2[(9 + r) * 12 + 9 + r] = -1; }
    }
    // ---- Levenberg state of this thread's problem (uniform over the problem's threads; re-read from LDS after every decision)
    // (lambda, ni, the two chi2 and the iteration counters live in S.lm / S.lmi and are loaded by the deciding wavefront only: as loop-carried
    // variables of every thread they were 12 registers held through the edge loop, the kernel's register peak)
    int cur = 0, mode = 0;                                              // (the round number lives in S.lmi[7], the inlier count's complement in S.lmi[8])
    bool done = !exists || ncur < 3;                                   // "if(nInitialCorrespondences<3) return 0"
    const int n_edges_total = ncur + nlast + (variant ? 3 : 2);
    if (exists && ncur < 3 && pt == 0) {
        double* o = A.out_ns + (size_t)b * 22; for (int k = 0; k < 22; k++) o[k] = curns[k];
        if (A.out_last_ns) { double* ol = A.out_last_ns + (size_t)b * 22; for (int k = 0; k < 22; k++) ol[k] = lastns[k]; }
        double* inf = A.info + (size_t)b * 4; inf[0] = 0; inf[1] = 0; inf[2] = 0; inf[3] = 0;
    }
    const bool never_ran = done;
    if (pt == 0) {
        SH.alive[p] = done ? 0 : 1;
        // reset the estimates to the frames' NavStates (Optimizer.cc:614-617 / :984-985)
        sh_put(S.est[0], ld_pvr(curns)); sh_put(S.est[1], ld_pvr(lastns));
        for (int k = 0; k < 3; k++) { S.bias[0][k] = curns[19 + k]; S.bias[1][k] = lastns[19 + k]; }
        S.lmi[6] = 0;                                                   // mode of the coming tick, read by the shared update phase
        S.lmi[7] = 0; S.lmi[8] = 0;
        S.lm[0] = 0; S.lm[1] = 2; S.lm[2] = 0; S.lm[3] = 0; S.lmi[1] = 0; S.lmi[2] = 0; S.lmi[3] = 0; S.lmi[4] = 0; S.lmi[5] = 0; S.lmi[9] = 0;
    }
    __syncthreads();
    const uint32_t (*tab)[2] = SH.tab[variant];
    MPT_LAP(9);                                                          // setup
#ifdef VIORB_POSE_TIMING
    const unsigned long long mpt_setup = mpt_acc[9];
#endif

    for (;;) {
        bool any = false;
#pragma unroll
        for (int q = 0; q < P; q++) any = any || SH.alive[q] != 0;
        if (!any) break;
        const bool act = !done;
        double* Hc = S.Hb[cur]; double* bc = S.bb[cur];
        double* Hm = mode ? S.Hb[cur ^ 1] : Hc; double* bv = mode ? S.bb[cur ^ 1] : bc;      // this tick's linearisation goes here
        // ---- (1) trial: back up the state, solve (H + lambda I) x = b on the problem's first wavefront
        if (act && mode) {
            if (pt < 20) S.bak[pt / 10][pt % 10] = S.est[pt / 10][pt % 10]; else if (pt < 26) S.bakb[(pt - 20) / 3][(pt - 20) % 3] = S.bias[(pt - 20) / 3][(pt - 20) % 3];
            if (pw == 0) {
                const double lambda = S.lm[0];
                const bool ok = variant ? wave_solve_reg_packed<24>(Hc, bc, lambda, S.OJ1, S.x, lane) : wave_solve_reg_packed<12>(Hc, bc, lambda, S.OJ1, S.x, lane);
                if (!ok && lane < n) S.x[lane] = 0;
                if (lane == 0) S.flag[0] = ok ? 1 : 0;
            }
        }
        __syncthreads();
        MPT_LAP(0);
        // ---- (2) NavState::IncSmallPVR + bias increment: wavefront = piece (rotation of cur / last, position-velocity-bias of cur / last),
        // lane = problem
        if (lane < P) {
            PoseMpProblem<WPP>& Q = SH.p[lane];
            const bool upd = SH.alive[lane] && Q.lmi[6];
            const int qvar = Q.lmi[0];
#pragma unroll
            for (int piece = 0; piece < 4; piece++) {
                if (wave != piece % NW) continue;
                const int side = piece & 1;
                if (!upd || (side && !qvar)) continue;
                double u[12], old[10];
                lds_get(Q.x + 12 * side, u); lds_get(Q.bak[side], old);
                LDS_READS_DONE();
                const quat q0 = mkq(old[6], old[7], old[8], old[9]);
                if (piece < 2) {
                    const quat r = so3_mul_f(q0, so3_exp_f(mk3(u[6], u[7], u[8])));
                    Q.est[side][6] = r.x; Q.est[side][7] = r.y; Q.est[side][8] = r.z; Q.est[side][9] = r.w;
                } else {
                    st3(Q.est[side], ld3(old) + mulv(qmat(q0), mk3(u[0], u[1], u[2])));
                    st3(Q.est[side] + 3, ld3(old + 3) + mk3(u[3], u[4], u[5]));
                    const d3 bo = ld3(Q.bias[side]);
                    st3(Q.bias[side], bo + mk3(u[9], u[10], u[11]));
                }
            }
        }
        __syncthreads();
        MPT_LAP(1);
        const int ok2 = S.flag[0];
        // ---- (3) evaluate + linearise at the current estimate into (Hm, bv)
        {
            const int nch0 = (ncur + 63) >> 6, nch1 = (nlast + 63) >> 6;
            const int cnt0 = nch0 > pw ? (nch0 - pw + WPP - 1) / WPP : 0, cnt1 = nch1 > pw ? (nch1 - pw + WPP - 1) / WPP : 0;
            constexpr int EI = POSE_EDGE_ILP;                                   // edges per lane and trip of the edge loop
            const int np0 = (cnt0 + EI - 1) / EI, npairs = act ? np0 + (cnt1 + EI - 1) / EI : 0;
            auto fetch_pair = [&](int q, obs_t (&o)[EI], int (&f)[EI], int (&ix)[EI]) {
                const int sd = q >= np0 && q < npairs, pq = q >= npairs ? 0 : (sd ? q - np0 : q);
                const double* ob = sd ? obs_l : obs_c; const uint8_t* ol = sd ? out_l : out_c; const int ne = sd ? nlast : ncur;
                const int last = max(ne - 1, 0);
#pragma unroll
                for (int e = 0; e < EI; e++) {
                    const int i = (pw + WPP * (EI * pq + e)) * 64 + lane, c = min(i, last);
                    f[e] = ol[c]; o[e] = load_obs(ob, c);
                    ix[e] = c;                                          // (a lane past the end holds edge `last` again: it stores that edge's own chi2 once more)
                    if (i >= ne || q >= npairs) f[e] = 1;
                }
            };
            obs_t oc[EI]; int fc[EI], ic[EI];
            fetch_pair(0, oc, fc, ic);
            int qpos = 0;
            if (act && pt < 20) S.ev[pt / 10][pt % 10] = S.est[pt / 10][pt % 10];
            // dense factors: wavefront = piece, lane = problem
            if (lane < P && SH.alive[lane]) {
                PoseMpProblem<WPP>& Q = SH.p[lane];
                const int qvar = Q.lmi[0];
#pragma unroll
                for (int piece = 0; piece < 4; piece++) {
                    if (wave != piece % NW) continue;
                    if (piece == 0) imu_piece_pv(Q.est[1], Q.est[0], Q.cpv, Q.bias[1], Q.pre, Q.gw, Q.e1, Q.J1);
                    else if (piece == 1) { if (qvar) prior_piece(Q.est[1], ld3(Q.base_ba[1]) + ld3(Q.bias[1]), Q.pri, Q.e2, Q.J2); }
                    else if (piece == 2) imu_piece_rot(Q.est[1], Q.est[0], Q.corrT, Q.e1, Q.J1);
                    else imu_piece_blocks(Q.est[1], Q.est[0], Q.pre, Q.J1);
                }
            }
            MPT_LAP(2);
            for (int side = 0; side < (act ? (variant ? 2 : 1) : 0); side++) {
                const pvr s = sh_pvr(S.est[side]);
                const m33 Rcw = mul(K.Rcb, tr(qmat(s.q)));
                double a[28];
#pragma unroll
                for (int k = 0; k < 28; k++) a[k] = 0;
                const double dsq_mono = d_mono * d_mono;
                const bool kernel_on = S.lmi[7] < 3;                     // the robust kernel is off in the last round (Optimizer.cc:618-620: its[3] without it)
                float* chi_side = A.chi_store + ((size_t)b * 2 + side) * cap;
                auto accumulate2 = [&](const obs_t (&o)[EI], const int (&flag)[EI], const int (&ix)[EI]) {
                    double pcx[EI], pcy[EI], pcz[EI], iz[EI], xz[EI], yz[EI], ea0[EI], ea1[EI], chi0[EI], ra0[EI], ra1[EI];
#pragma unroll
                    for (int e = 0; e < EI; e++) {
                        const d3 dd = o[e].X - s.P;
                        pcx[e] = fma(Rcw.a02, dd.z, fma(Rcw.a01, dd.y, fma(Rcw.a00, dd.x, -K.RcbPbc.x)));
                        pcy[e] = fma(Rcw.a12, dd.z, fma(Rcw.a11, dd.y, fma(Rcw.a10, dd.x, -K.RcbPbc.y)));
                        pcz[e] = fma(Rcw.a22, dd.z, fma(Rcw.a21, dd.y, fma(Rcw.a20, dd.x, -K.RcbPbc.z)));
                    }
#pragma unroll
                    for (int e = 0; e < EI; e++) {
                        iz[e] = __builtin_amdgcn_rcp(pcz[e]);
                        iz[e] = fma(fma(-pcz[e], iz[e], 1.0), iz[e], iz[e]);
                        iz[e] = fma(fma(-pcz[e], iz[e], 1.0), iz[e], iz[e]);
                    }
#pragma unroll
                    for (int e = 0; e < EI; e++) {
                        xz[e] = pcx[e] * iz[e]; yz[e] = pcy[e] * iz[e];
                        ea0[e] = o[e].u - fma(xz[e], K.fx, K.cx); ea1[e] = o[e].v - fma(yz[e], K.fy, K.cy);
                        chi0[e] = o[e].is2 * fma(ea0[e], ea0[e], ea1[e] * ea1[e]);
                        ra0[e] = chi0[e]; ra1[e] = 1.0;
                    }
                    // the edge's stored error (g2o keeps every active edge's error of the last computeActiveErrors; the round's classification reads it)
#pragma unroll
                    for (int e = 0; e < EI; e++) chi_side[ix[e]] = (float)chi0[e];
                    bool hb[EI], anyh = false;
#pragma unroll
                    for (int e = 0; e < EI; e++) { hb[e] = kernel_on && chi0[e] > dsq_mono; anyh = anyh || hb[e]; }
                    if (__builtin_amdgcn_ballot_w64(anyh) != 0) {
#pragma unroll
                        for (int e = 0; e < EI; e++) {
                            const double rs = rsqrt_nr(fmax(chi0[e], 1e-300));
                            const bool hub = hb[e];
                            ra0[e] = hub ? fma(2.0 * d_mono, chi0[e] * rs, -dsq_mono) : chi0[e]; ra1[e] = hub ? d_mono * rs : 1.0;
                        }
                    }
#pragma unroll
                    for (int e = 0; e < EI; e++) a[27] += flag[e] ? 0.0 : ra0[e];
#pragma unroll
                    for (int e = 0; e < EI; e++) {
                        const double w0 = flag[e] ? 0.0 : ra1[e] * o[e].is2;
                        const double Aa = K.fx * iz[e], Bb = K.fy * iz[e], fxp = K.fx * xz[e], fyq = K.fy * yz[e];
                        const double r0[6] = {Aa, 0.0, -(Aa * xz[e]), -(fxp * yz[e]), fma(fxp, xz[e], K.fx), -(K.fx * yz[e])};
                        const double r1[6] = {0.0, Bb, -(Bb * yz[e]), -fma(fyq, yz[e], K.fy), fyq * xz[e], K.fy * xz[e]};
                        double w0r[6], w1r[6];
#pragma unroll
                        for (int r = 0; r < 6; r++) { w0r[r] = w0 * r0[r]; w1r[r] = w0 * r1[r]; }
                        int k = 0;
#pragma unroll
                        for (int r = 0; r < 6; r++)
#pragma unroll
                            for (int c = r; c < 6; c++, k++) {
                                if (r != 1 && c != 1) a[k] = fma(w0r[r], r0[c], a[k]);
                                if (r != 0 && c != 0) a[k] = fma(w1r[r], r1[c], a[k]);
                            }
#pragma unroll
                        for (int r = 0; r < 6; r++) {
                            if (r != 1) a[21 + r] = fma(-w0r[r], ea0[e], a[21 + r]);
                            if (r != 0) a[21 + r] = fma(-w1r[r], ea1[e], a[21 + r]);
                        }
                    }
                };
                const int qend = side ? npairs : min(np0, npairs);
                while (qpos < qend) {
                    obs_t on[EI]; int fn[EI], in[EI];
                    fetch_pair(qpos + 1, on, fn, in);
                    accumulate2(oc, fc, ic);
                    #pragma unroll
                    for (int e = 0; e < EI; e++) { oc[e] = on[e]; fc[e] = fn[e]; ic[e] = in[e]; }
                    qpos++;
                }
                MPT_LAP(3);
                {   // transpose-reduce 32 padded values over the 64 lanes
                    double v[32];
#pragma unroll
                    for (int k = 0; k < 28; k++) v[k] = a[k];
#pragma unroll
                    for (int k = 28; k < 32; k++) v[k] = 0;
                    const double tot = wave_transpose_reduce32(v, lane);
                    const int idx = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
                    if ((lane & 1) == 0 && idx < 28) S.red[pw][side][idx] = tot;
                }
                MPT_LAP(4);
            }
            __syncthreads();
            MPT_LAP(5);
#if POSE_ASM_MFMA
            // ---- assembly, step 1 on the matrix cores: [Omega1 J1 | Omega1 e1] (9 x 22) and, frame / frame problems, [Omega2 J2 | Omega2 e2]
            // (12 x 13) as nine v_mfma_f64_16x16x4 on the problem's first wavefront (operands A[i][k]: lane 16 k + i, B[k][j]: lane 16 k + j; result
            // row = lane / 16 + 4 reg, column = lane % 16; every load unconditional at a clamped address, every store unconditional with the
            // results outside the product sent to S.dump), the quadratic forms e^T (Omega e) term by term from the extra column; meanwhile another
            // wavefront of the problem takes G T, T^T g and the bias factor's weight. As work items (333 entries of Omega J, a dot product of 9 or
            // 12 LDS operand pairs each, three trips) this step was 6.7 k of a tick's 54 k cycles; it is 2.3 k. The sums associate differently
            // from the item form (same algebra as g2o's Omega A; parity tests: 1e-5, every discrete result equal). Step 2 stays in the item form:
            // on gfx950 the FP64 matrix rate equals the vector rate, and J^T (Omega J) in the state's coordinates as 24 more matrix instructions
            // on one wavefront (measured) took as long as the 324 work items on two.
            typedef double v4d_t __attribute__((ext_vector_type(4)));
            // (the lane index through an opaque move: everything derived from it below — tile coordinates, LDS addresses — is
            // otherwise loop-invariant, gets hoisted out of the tick loop and spilled: 55 scratch reloads per tick, 25 k cycles)
            int lane_v = lane;
            asm volatile("" : "+v"(lane_v));
            const int l16 = lane_v & 15, lk = lane_v >> 4;
            constexpr int GW_ = WPP > 1 ? 1 : 0;                          // the wavefront of the problem that prepares the reprojection blocks
            if (act && pw == GW_) {
                // G T (6 x 6 per frame) and T^T g
                for (int i = lane; i < 84; i += 64) {
                    const int side = i >= 42, j = i - 42 * side;
                    if (side && !variant) continue;
                    double gv[6][WPP], tv[6];
                    if (j < 36) {
                        const int r = j / 6, c = j % 6;
#pragma unroll
                        for (int k = 0; k < 6; k++) {
                            const int lo = min(r, k), hi = max(r, k), gi = lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
#pragma unroll
                            for (int w = 0; w < WPP; w++) gv[k][w] = S.red[w][side][gi];
                            tv[k] = SH.T6[k * 6 + c];
                        }
                        LDS_READS_DONE();
                        double v = 0;
#pragma unroll
                        for (int k = 0; k < 6; k++) {
                            double g = 0;
#pragma unroll
                            for (int w = 0; w < WPP; w++) g += gv[k][w];
                            v = fma(g, tv[k], v);
                        }
                        S.GT[side][j] = v;
                    } else {
                        const int c = j - 36;
#pragma unroll
                        for (int k = 0; k < 6; k++) {
#pragma unroll
                            for (int w = 0; w < WPP; w++) gv[k][w] = S.red[w][side][21 + k];
                            tv[k] = SH.T6[k * 6 + c];
                        }
                        LDS_READS_DONE();
                        double v = 0;
#pragma unroll
                        for (int k = 0; k < 6; k++) {
                            double g = 0;
#pragma unroll
                            for (int w = 0; w < WPP; w++) g += gv[k][w];
                            v = fma(tv[k], g, v);
                        }
                        S.b6[side][c] = v;
                    }
                }
                if (lane == 63) {                                          // the bias random-walk factor: weight, error, robust chi2
                    const d3 eb = (ld3(S.base_ba[0]) + ld3(S.bias[0])) - (ld3(S.base_ba[1]) + ld3(S.bias[1]));
                    double r0, r1; huber(bias_info * dot3(eb, eb), d_bias, &r0, &r1);
                    S.sc[3] = r1 * bias_info; S.sc[4] = eb.x; S.sc[5] = eb.y; S.sc[6] = eb.z; S.sc[8] = r0;
                }
            }
            if (act && pw == 0) {
                // ---- A: Omega [J | e]. Every load and store is unconditional: an operand outside the product reads a clamped address and is
                // replaced by zero, a result outside it goes to this lane's slot of S.dump (a predicated store is a branch per element)
#pragma unroll
                for (int jt = 0; jt < 2; jt++) {
                    v4d_t acc = {0, 0, 0, 0};
                    const int j = 16 * jt + l16;
                    const double* pa = S.info_pvr + min(l16, 8) * 9;
                    const double* pb = j == 21 ? S.e1 : S.J1 + min(j, 20);
                    const int sb = j == 21 ? 1 : 21;
                    double av[3], bw[3];
#pragma unroll
                    for (int kc = 0; kc < 3; kc++) { const int kk = min(4 * kc + lk, 8); av[kc] = pa[kk]; bw[kc] = pb[kk * sb]; }
                    LDS_READS_DONE();
#pragma unroll
                    for (int kc = 0; kc < 3; kc++) {
                        const bool kok = 4 * kc + lk < 9;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((l16 < 9 && kok) ? av[kc] : 0.0, (j < 22 && kok) ? bw[kc] : 0.0, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const int row = lk + 4 * r;
                        double* dst = (row < 9 && j < 21) ? S.OJ1 + row * 21 + j : ((row < 9 && j == 21) ? S.oe1 + row : S.dump + lane_v);
                        *dst = acc[r];
                    }
                }
                if (variant) {
                    v4d_t acc = {0, 0, 0, 0};
                    const double* pa = S.info_prior + min(l16, 11) * 12 + lk;
                    const double* pb = l16 == 12 ? S.e2 + lk : S.J2 + min(l16, 11) + lk * 12;
                    const int sb = l16 == 12 ? 4 : 48;
                    double av[3], bw[3];
#pragma unroll
                    for (int kc = 0; kc < 3; kc++) { av[kc] = pa[4 * kc]; bw[kc] = pb[kc * sb]; }
                    LDS_READS_DONE();
#pragma unroll
                    for (int kc = 0; kc < 3; kc++)
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(l16 < 12 ? av[kc] : 0.0, l16 < 13 ? bw[kc] : 0.0, acc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const int row = lk + 4 * r;
                        double* dst = l16 < 12 ? S.OJ2 + row * 12 + l16 : (l16 == 12 ? S.oe2 + row : S.dump + lane_v);
                        *dst = acc[r];
                    }
                }
                WAVE_LDS_SYNC();
                // quadratic forms e^T Omega e term by term (summed in index order below, as before), Huber weights
                if (lane < 9) S.q[lane] = S.e1[lane] * S.oe1[lane];
                else if (lane >= 16 && lane < 28 && variant) S.q[12 + lane - 16] = S.e2[lane - 16] * S.oe2[lane - 16];
                WAVE_LDS_SYNC();
            }
            __syncthreads();
            MPT_LAP(6);
#else
            // ---- assembly, step 1: quadratic forms of the dense factors, Omega * J of both, the bias factor's weight, G T and T^T g
            if (act) {
                for (int i = pt; i < 22; i += PT) {
                    if (i < 9) {
                        double iv[9], ev[9]; lds_get(S.info_pvr + i * 9, iv); lds_get(S.e1, ev); const double et = S.e1[i]; LDS_READS_DONE();
                        double sq = 0;
#pragma unroll
                        for (int c = 0; c < 9; c++) sq = fma(iv[c], ev[c], sq);
                        S.q[i] = et * sq;
                    } else if (i < 21) {
                        if (variant) {
                            const int r = i - 9; double iv[12], ev[12]; lds_get(S.info_prior + r * 12, iv); lds_get(S.e2, ev); const double et = S.e2[r]; LDS_READS_DONE();
                            double sq = 0;
#pragma unroll
                            for (int c = 0; c < 12; c++) sq = fma(iv[c], ev[c], sq);
                            S.q[12 + r] = et * sq;
                        }
                    } else {
                        const d3 eb = (ld3(S.base_ba[0]) + ld3(S.bias[0])) - (ld3(S.base_ba[1]) + ld3(S.bias[1]));
                        double r0, r1; huber(bias_info * dot3(eb, eb), d_bias, &r0, &r1);
                        S.sc[3] = r1 * bias_info; S.sc[4] = eb.x; S.sc[5] = eb.y; S.sc[6] = eb.z; S.sc[8] = r0;
                    }
                }
                for (int i = pt; i < 189 + (variant ? 144 : 0); i += PT) {
                    const bool f1 = i < 189; const int ii = f1 ? i : i - 189, nc = f1 ? 21 : 12, r = ii / nc, c = ii - r * nc, nk = f1 ? 9 : 12;
                    const double* ip = f1 ? S.info_pvr + r * 9 : S.info_prior + r * 12; const double* jp = (f1 ? S.J1 : S.J2) + c;
                    double iv[12], jvv[12];
#pragma unroll
                    for (int kk = 0; kk < 12; kk++) { const int k2 = kk < nk ? kk : 0; iv[kk] = ip[k2]; jvv[kk] = jp[k2 * nc]; }
                    LDS_READS_DONE();
                    double sq = 0;
#pragma unroll
                    for (int kk = 0; kk < 12; kk++) sq = kk < nk ? fma(iv[kk], jvv[kk], sq) : sq;
                    (f1 ? S.OJ1 : S.OJ2)[ii] = sq;
                }
                // reprojection blocks back in (dP, dPhi) coordinates, from the far end of the problem's threads
                for (int i = PT - 1 - pt; i < 84; i += PT) {
                    const int side = i >= 42, j = i - 42 * side;
                    if (side && !variant) continue;
                    double gv[6][WPP], tv[6];
                    if (j < 36) {
                        const int r = j / 6, c = j % 6;
#pragma unroll
                        for (int k = 0; k < 6; k++) {
                            const int lo = min(r, k), hi = max(r, k), gi = lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
#pragma unroll
                            for (int w = 0; w < WPP; w++) gv[k][w] = S.red[w][side][gi];
                            tv[k] = SH.T6[k * 6 + c];
                        }
                        LDS_READS_DONE();
                        double v = 0;
#pragma unroll
                        for (int k = 0; k < 6; k++) {
                            double g = 0;
#pragma unroll
                            for (int w = 0; w < WPP; w++) g += gv[k][w];
                            v = fma(g, tv[k], v);
                        }
                        S.GT[side][j] = v;
                    } else {
                        const int c = j - 36;
#pragma unroll
                        for (int k = 0; k < 6; k++) {
#pragma unroll
                            for (int w = 0; w < WPP; w++) gv[k][w] = S.red[w][side][21 + k];
                            tv[k] = SH.T6[k * 6 + c];
                        }
                        LDS_READS_DONE();
                        double v = 0;
#pragma unroll
                        for (int k = 0; k < 6; k++) {
                            double g = 0;
#pragma unroll
                            for (int w = 0; w < WPP; w++) g += gv[k][w];
                            v = fma(tv[k], g, v);
                        }
                        S.b6[side][c] = v;
                    }
                }
            }
            __syncthreads();
            MPT_LAP(6);
#endif
            // ---- assembly, step 2: Huber weights of the dense factors, total robust chi2, complete H / b entries from all their sources
            if (act) {
                double w1, w2 = 0, rob1, rob2 = 0;
                {
                    double qv[24];
                    lds_get(S.q, qv);
                    LDS_READS_DONE();
                    double chi = 0;
#pragma unroll
                    for (int i = 0; i < 9; i++) chi += qv[i];
                    huber(chi, d_pvr, &rob1, &w1);
                    if (variant) {
                        double chi2 = 0;
#pragma unroll
                        for (int i = 0; i < 12; i++) chi2 += qv[12 + i];
                        huber(chi2, d_prior, &rob2, &w2);
                    }
                }
                if (pt == 0) {
                    double tot = 0;
                    for (int w = 0; w < WPP; w++) { tot += S.red[w][0][27]; if (variant) tot += S.red[w][1][27]; }
                    tot += rob1; tot += S.sc[8];
                    if (variant) tot += rob2;
                    S.sc[0] = tot;
                }
                const double wb = S.sc[3];
                const int nitems = n * (n + 1) / 2 + n;
                for (int q = pt; q < nitems; q += PT) {
                    const uint32_t d0 = tab[q][0], d1 = tab[q][1];
                    const int R = d0 & 31, Cc = (d0 >> 5) & 31, redk = (d0 >> 11) & 31, sideR = (d0 >> 16) & 1, mR = (d0 >> 17) & 31, mC = (d0 >> 22) & 31;
                    const int bsign = (d0 >> 27) & 3, bR = d0 >> 29, pR = d1 & 15, pC = (d1 >> 4) & 15;
                    const bool isb = (d0 >> 10) & 1;
                    double v = 0, s1 = 0, s2 = 0, scb;
                    {
                        const int r6 = (d1 >> 8) & 7, c6 = (d1 >> 11) & 7;
                        const int mRc = mR == 31 ? 0 : mR, mCc = mC == 31 ? 0 : mC, pRc = pR == 15 ? 0 : pR, pCc = pC == 15 ? 0 : pC;
                        const double* a1 = (isb ? S.OJ1 : S.J1) + mRc; const double* b1 = isb ? S.e1 : S.OJ1 + mCc; const int sb1 = isb ? 1 : 21;
                        const double* a2 = (isb ? S.OJ2 : S.J2) + pRc; const double* b2 = isb ? S.e2 : S.OJ2 + pCc; const int sb2 = isb ? 1 : 12;
                        double A1[9], B1[9], A2[12], B2[12], Tt[6], Gt[6];
                        lds_get(a1, A1, 21); lds_get(b1, B1, sb1); lds_get(a2, A2, 12); lds_get(b2, B2, sb2);
                        lds_get(SH.T6 + r6, Tt, 6); lds_get(S.GT[sideR] + c6, Gt, 6);
                        const double bb6 = S.b6[sideR][r6]; scb = S.sc[4 + bR];
                        LDS_READS_DONE();
                        double sr = 0;
#pragma unroll
                        for (int k = 0; k < 6; k++) sr = fma(Tt[k], Gt[k], sr);
                        if (isb) sr = bb6;
                        v = redk != 31 ? sr : 0.0;
#pragma unroll
                        for (int kk = 0; kk < 9; kk++) s1 = fma(A1[kk], B1[kk], s1);
#pragma unroll
                        for (int kk = 0; kk < 12; kk++) s2 = fma(A2[kk], B2[kk], s2);
                    }
                    const bool has1 = mR != 31 && (isb || mC != 31), has2 = pR != 15 && (isb || pC != 15);
                    if (isb) {
                        if (has1) v -= w1 * s1;
                        if (has2) v -= w2 * s2;
                        if (bsign) v += (bsign == 2 ? -wb : wb) * scb;
                        bv[R] = v;
                    } else {
                        if (has1) v += w1 * s1;
                        if (has2) v += w2 * s2;
                        if (bsign) v += bsign == 1 ? wb : -wb;
                        Hm[R * n + Cc] = v; Hm[Cc * n + R] = v;
                    }
                }
            }
            __syncthreads();
            MPT_LAP(7);
        }
        // ---- (4) Levenberg decision on the problem's first wavefront (g2o optimization_algorithm_levenberg.cpp:61-189), published through LDS
        if (act && pw == 0) {
            const double chi = S.sc[0];
            int end_round = 0;
            double lambda = S.lm[0], ni = S.lm[1], currentChi = S.lm[2], iniChi = S.lm[3];
            int it = S.lmi[1], qmax = S.lmi[2], nBadLM = S.lmi[3], hb_last = S.lmi[5];
            if (!mode) {                                                  // first evaluation of a round: computeActiveErrors + buildSystem of iteration 0
                currentChi = chi; hb_last = cur; iniChi = chi;
                double mx = 0; for (int i = 0; i < n; i++) mx = fmax(fabs(Hc[i * n + i]), mx);
                lambda = lm_lambda_init(mx); ni = 2; nBadLM = 0; qmax = 0; mode = 1;
            } else {
                const double tempChi = lm_trial_chi2(ok2, chi);
                double scale = 0;                                        // computeScale(): sum_j x_j (lambda x_j + b_j), in order
                {
                    double xs[24], bs[24];
#pragma unroll
                    for (int j = 0; j < 24; j++) { xs[j] = S.x[j < n ? j : 0]; bs[j] = bc[j < n ? j : 0]; }
                    LDS_READS_DONE();
#pragma unroll
                    for (int j = 0; j < 24; j++) if (j < n) scale += xs[j] * (lambda * xs[j] + bs[j]);
                }
                const double rho = lm_rho(currentChi, tempChi, scale);
                const bool accepted = lm_accepted(rho, tempChi);
                if (accepted) { lm_good_step(lambda, ni, lm_cube_mul(2 * rho - 1)); currentChi = tempChi; }
                else {
                    lm_bad_step(lambda, ni);
                    if (lane < 20) S.est[lane / 10][lane % 10] = S.bak[lane / 10][lane % 10]; else if (lane < 26) S.bias[(lane - 20) / 3][(lane - 20) % 3] = S.bakb[(lane - 20) / 3][(lane - 20) % 3];
                }
                qmax++;
                if (!lm_retry(rho, qmax)) {                              // the iteration is over
                    if (accepted) cur ^= 1;                               // the speculative buffer is the next iteration's system
                    if (lane == 0) { S.flag[1]++; S.sc[7] = currentChi; }
                    const bool brk = lm_iteration_stops(rho, qmax, iniChi, currentChi, nBadLM);
                    it++;
                    if (brk || it == 10) { end_round = 1; if (lane == 0) S.lmi[10] = accepted ? 0 : 1; }
                    else { hb_last = cur; iniChi = currentChi; qmax = 0; }
                }
            }
            if (lane == 0) {
                S.lm[0] = lambda; S.lm[1] = ni; S.lm[2] = currentChi; S.lm[3] = iniChi;
                S.lmi[1] = it; S.lmi[2] = qmax; S.lmi[3] = nBadLM; S.lmi[4] = cur; S.lmi[5] = hb_last; S.lmi[6] = mode; S.lmi[9] = end_round;
                S.flag[2] = 0;
            }
        }
        __syncthreads();
        int end_round = 0;
        if (act) {
            cur = S.lmi[4]; mode = S.lmi[6]; end_round = S.lmi[9];
        }
        MPT_LAP(8);
        // ---- (5) end of a round: re-classify every mono edge by its chi2 at the new estimate (Optimizer.cc:622-688). Entered only on a tick that
        // ends a round of some problem of the workgroup (uniform over the workgroup: the flags were published before the barrier above) — its two
        // barriers are 1 k cycles, and four ticks of twenty end a round
        bool any_end = false;
#pragma unroll
        for (int q = 0; q < P; q++) any_end = any_end || (SH.alive[q] != 0 && SH.p[q].lmi[9] != 0);
        if (any_end) {
            int bad_local = 0;
            if (act && end_round) {
                // Optimizer.cc:622-688: an edge flagged as outlier is re-evaluated at the new estimate ("if(mvbOutlier[idx]) e->computeError()"), an
                // inlier is classified by its STORED error — the error of the last computeActiveErrors, i.e. of the last trial state, which is not
                // the estimate when that trial was rejected (optimization_algorithm_levenberg.cpp:143-147 restores the vertices only)
                const bool stale = S.lmi[10] != 0;
                for (int side = 0; side < (variant ? 2 : 1); side++) {
                    const pvr s = sh_pvr(S.est[side]);
                    const m33 RT = tr(qmat(s.q));
                    const double* ob = side ? obs_l : obs_c; uint8_t* ol = side ? out_l : out_c; const int ne = side ? nlast : ncur;
                    // Every edge's chi2 at the last evaluation is in the solver's scratch (written by the edge loop, flagged edges included): an inlier
                    // is classified by it (g2o's stored error), an edge flagged as outlier too unless the round's last trial was rejected — the estimate
                    // is then not the state of that evaluation and the flagged edge is evaluated again (rare). Four edges per trip, loads together.
                    // (Re-evaluating every edge at the estimate, one edge and one dependent global round trip per trip, was 25 k cycles per round.)
                    const float* chi_rd = A.chi_store + ((size_t)b * 2 + side) * cap;
                    for (int i0 = pt; i0 < ne; i0 += 4 * PT) {
                        float cst[4]; int fl[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) { const int i = min(i0 + u * PT, ne - 1); cst[u] = chi_rd[i]; fl[u] = ol[i]; }
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const int i = i0 + u * PT;
                            float chi2 = cst[u];
                            if (stale && fl[u] && i < ne) {
                                const obs_t o = load_obs(ob, i);
                                double e[2];
                                proj_edge(K, RT, s.P, o.X, o.u, o.v, false, e, nullptr, nullptr);
                                chi2 = (float)(o.is2 * (e[0] * e[0] + e[1] * e[1]));
                            }
                            const int bad = chi2 > 5.991f;
                            if (i < ne) { ol[i] = (uint8_t)bad; if (side == 0) bad_local += bad; }
                        }
                    }
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) bad_local += __shfl_xor(bad_local, d);
                if (lane == 0) atomicAdd(&S.flag[2], bad_local);
                if (pt == 0) S.lmi[7] = S.lmi[7] + 1;                      // rounds completed
            }
            __syncthreads();
            if (act && end_round) {
                const int round = S.lmi[7];
                if (pt == 0) S.lmi[8] = S.flag[2];                        // outliers of the current frame after this round
                if (round == 4 || n_edges_total < 10) done = true;
                else {
                    mode = 0; cur = 0;
                    if (pt == 0) {
                        S.lmi[1] = 0; S.lmi[4] = 0;                             // it, cur
                        sh_put(S.est[0], ld_pvr(curns)); sh_put(S.est[1], ld_pvr(lastns));
                        for (int k = 0; k < 3; k++) { S.bias[0][k] = curns[19 + k]; S.bias[1][k] = lastns[19 + k]; }
                        S.lmi[6] = 0;
                    }
                }
                if (pt == 0 && done) SH.alive[p] = 0;
            }
            __syncthreads();
        }
        MPT_LAP(9);
#ifdef VIORB_POSE_TIMING
        mpt_ticks++;
#endif
    }
#ifdef VIORB_POSE_TIMING
    if (blockIdx.x == 0 && lane == 0)
        printf("pose_mp wave=%d ticks=%d total=%llu solve=%llu update=%llu dense=%llu edges=%llu reduce=%llu wait=%llu asm1=%llu asm2=%llu decide=%llu classify+setup=%llu (setup %llu)\n", wave, mpt_ticks,
               __builtin_amdgcn_s_memtime() - mpt_begin, mpt_acc[0], mpt_acc[1], mpt_acc[2], mpt_acc[3], mpt_acc[4], mpt_acc[5], mpt_acc[6], mpt_acc[7], mpt_acc[8], mpt_acc[9], mpt_setup);
#endif
    // ---- outputs
    if (exists && !never_ran && pt == 0) {
        double* o = A.out_ns + (size_t)b * 22;
        for (int k = 0; k < 10; k++) o[k] = S.est[0][k];
        for (int k = 10; k < 19; k++) o[k] = curns[k];
        for (int k = 0; k < 3; k++) o[19 + k] = S.bias[0][k];
        if (A.out_last_ns) {
            double* ol = A.out_last_ns + (size_t)b * 22;
            for (int k = 0; k < 10; k++) ol[k] = variant ? S.est[1][k] : lastns[k];
            for (int k = 10; k < 19; k++) ol[k] = lastns[k];
            for (int k = 0; k < 3; k++) ol[19 + k] = variant ? S.bias[1][k] : lastns[19 + k];
        }
        double* inf = A.info + (size_t)b * 4;
        inf[0] = ncur - S.lmi[8]; inf[1] = S.sc[7]; inf[2] = S.flag[1]; inf[3] = 0;
    }
    if (A.compute_marg) {
        // mMargCovInv from the last linearised H: Schur complement of the last-frame block (see k_pose_opt_vi)
        const bool mine = exists && !never_ran;
        double* mo = A.marg_out + (size_t)b * 144;
        double* Lm = S.J1;                                               // 576 doubles over J1 | OJ1 | J2 | OJ2 (all dead now)
        if (mine && variant)
            for (int i = pt; i < 576; i += PT) {
                const int r = i / 24, c = i % 24;
                Lm[i] = S.Hb[S.lmi[5]][((r + 12) % 24) * 24 + (c + 12) % 24];     // [last | cur] ordering
            }
        __syncthreads();
        if (mine && variant && pw == 0) wave_cholesky(Lm, 24, 12, lane);
        __syncthreads();
        if (mine)
            for (int i = pt; i < 144; i += PT) {
                const int r = i / 12, c = i % 12;
                // variant 0: H = diag(H_pp (9x9), H_bb (3x3)) exactly (no factor couples cur PVR and cur bias when the KF is fixed)
                if (variant) mo[i] = (c <= r) ? Lm[(12 + r) * 24 + 12 + c] : Lm[(12 + c) * 24 + 12 + r];
                else mo[i] = ((r < 9) == (c < 9)) ? S.Hb[S.lmi[5]][r * 12 + c] : 0.0;
            }
    }
}
