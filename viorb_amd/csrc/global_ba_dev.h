// viorb_amd/csrc/global_ba_dev.h — what the two global bundle adjustments share on the device side: the work arrays of one solve
// (GbaDev), the host functions of global_ba.hip that both call (graph bookkeeping, the blocked Cholesky chain, the Levenberg loop) and
// the table of launches a solve plugs into that loop (GbaOps). global_ba.hip is the NavState solve (12 coordinates per free key frame,
// IMU factors), global_ba_se3.hip the vision-only one (6 coordinates, monocular and stereo edges). The kernels named here live in
// global_ba.hip; the other translation unit reaches them through these host functions only. The Schur complement, the back-substitution
// and the point blocks differ between the two only in the block order and the residual rows: one template body each, below.
// essential_graph.hip is a third client of the loop and the Cholesky chain: a Sim3 pose graph (7 coordinates, kf_w = 8) with np = ne = 0
// here, whose edges live in arrays of its own behind GbaDev::ext.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "viorb_common.h"
#include "global_ba_core.h"

namespace viorb {

enum { GBA_S_CHI = 0, GBA_S_SCALE, GBA_S_FAIL, GBA_S_MAXDIAG, GBA_S_N = 8 };
enum { GBA_ST_INVALID = 0, GBA_ST_NFREE, GBA_ST_N = 4 };
// bits of status[GBA_ST_INVALID]
enum { GBA_BAD_PREV = 1, GBA_BAD_EDGE = 2, GBA_BAD_COV = 4, GBA_BAD_SIGMA = 8, GBA_BAD_BF = 16,
       GBA_BAD_EG_EDGE = 32, GBA_BAD_EG_POSE = 64, GBA_BAD_EG_GAUGE = 128, GBA_BAD_EG_REF = 256 };     // the essential-graph solve's (essential_graph.hip)

struct GbaDev {
    int nk, np, ne, nfree, n, ld, robust;
    int blk, kf_w, obs_w, rows;         // coordinates per free key frame (12 / 6), doubles per key-frame row (22 / 7), per edge_obs row (3 / 4;
                                        // the last one is invSigma2), error rows per edge (2 / 3)
    double *kf, *kf_bak;                // [nk][kf_w]
    double *pt, *pt_bak;                // [np][3]
    const int32_t* prev;                // [nk] (NavState solve)
    const uint8_t* fixed;               // [nk]
    const int32_t* e_idx;               // [ne][2] (point, key frame)
    const double *e_obs, *preint;       // [ne][obs_w], [nk][142] (NavState solve)
    int *fidx, *pt_start, *kf_start, *kf_cur, *kf_tmp, *kf_list;   // rank among the free key frames or -1; CSR by point; CSR by key frame
    double* info_pvr;                   // [nk][81] (NavState solve)
    double *err, *Jp, *Jk, *wgt, *We;   // [ne][rows], [ne][3 rows], [ne][6 rows], [ne], [ne][18] = wgt Jk^T Jp
    double *Hll, *bl, *Dinv, *db, *xl;  // [np][9], [np][3], [np][9], [np][3], [np][3]
    double *Hd, *Ho, *bp;               // diagonal blocks [nk][blk blk] by free rank, block (key frame i, prev[i]) [nk][144] (NavState solve), [blk nk]
    double *S, *rhs, *xp;               // [ld][ld] lower triangle, [ld], [ld]
    double* scal;                       // GBA_S_*
    int* status;                        // GBA_ST_*
    uint8_t* included;                  // [np]
    double cam[16], gw[3];              // NavState solve: cam[16], gw; SE3 solve: cam[0..4] = fx fy cx cy bf
    const void* ext;                    // host pointer to a solve's own arrays (essential graph: its EgDev); no kernel reads it
};

// ---- kernel bodies both solves instantiate with their block order BLK (12 / 6) and residual rows ROWS (2 / 3); the __global__
// wrappers k_gba_* / k_gse3_* keep the names the profile tools report
// one thread per point: Hll, bl in edge order
template <int ROWS> __device__ __forceinline__ void gba_hll_body(const GbaDev& D) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.np) return;
    double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    for (int k = D.pt_start[p]; k < D.pt_start[p + 1]; k++) {
        const double* Jp = D.Jp + 3 * ROWS * (size_t)k;
        const double w = D.wgt[k];
        double e[ROWS];
        for (int r = 0; r < ROWS; r++) e[r] = D.err[ROWS * k + r];
        ba_point_add<ROWS>(H, b, w, Jp, e);
    }
    ba_point_store(D.Hll + (size_t)p * 9, D.bl + (size_t)p * 3, H, b);
    D.included[p] = D.pt_start[p + 1] > D.pt_start[p];            // a point without an edge is not a vertex (src/Optimizer.cc:234-242, :3685-3693)
}
// Schur complement of the point block (block_solver.hpp:381-432): one wavefront per point walks the ordered pairs (a, b) of its
// observers; the pair with rank(a) > rank(b) owns block (a, b) of the lower triangle, a pair on one key frame the lower triangle of its
// diagonal block. S_ab -= W_a Dinv W_b^T, bs_a -= W_a Dinv bl (W = wgt Jk^T Jp, 6 x 3), FP64 hardware atomics.
template <int BLK> __device__ __forceinline__ void gba_schur_body(const GbaDev& D) {
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
            double* row = D.S + (size_t)(BLK * fa + loc6(BLK, r)) * ld + BLK * fb;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                if (fa == fb && c > r) continue;
                unsafeAtomicAdd(&row[loc6(BLK, c)], -(BD[3 * r] * Wb[3 * c] + BD[3 * r + 1] * Wb[3 * c + 1] + BD[3 * r + 2] * Wb[3 * c + 2]));
            }
            if (a == b) unsafeAtomicAdd(&D.rhs[BLK * fa + loc6(BLK, r)], -(Wa[3 * r] * db[0] + Wa[3 * r + 1] * db[1] + Wa[3 * r + 2] * db[2]));
        }
    }
}
// point increments xl = Dinv (bl - sum W^T xp): every edge's product is summed first and subtracted once
template <int BLK> __device__ __forceinline__ void gba_backsub_body(const GbaDev& D) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.np) return;
    if (D.scal[GBA_S_FAIL] != 0.0) return;
    double cl[3] = {D.bl[3 * (size_t)p], D.bl[3 * (size_t)p + 1], D.bl[3 * (size_t)p + 2]};
    for (int k = D.pt_start[p]; k < D.pt_start[p + 1]; k++) {
        const int r = D.fidx[D.e_idx[2 * k + 1]];
        if (r < 0) continue;
        const double* W = D.We + 18 * (size_t)k; const double* x = D.xp + BLK * (size_t)r;
        for (int c = 0; c < 3; c++) { double s = 0; for (int a = 0; a < 6; a++) s += W[3 * a + c] * x[loc6(BLK, a)]; cl[c] -= s; }
    }
    const double* Di = D.Dinv + (size_t)p * 9;
    for (int a = 0; a < 3; a++) D.xl[3 * (size_t)p + a] = Di[3 * a] * cl[0] + Di[3 * a + 1] * cl[1] + Di[3 * a + 2] * cl[2];
}

// The host form's lease of a stream context. An error path may leave work queued on the stream: nothing of it may still run when the
// next borrower takes the context, so the stream is drained before the context goes back. The arena grows to exactly what is asked for.
struct GbaArena : StreamCtxLease {
    ~GbaArena() { if (c) (void)hipStreamSynchronize(c->st); }
    bool reserve(size_t bytes) {
        if (c->bytes >= bytes) return true;
        if (c->arena) (void)hipFree(c->arena);
        c->arena = nullptr; c->bytes = 0;
        if (hipMalloc(&c->arena, bytes) != hipSuccess) return false;
        c->bytes = bytes;
        return true;
    }
};

inline unsigned gba_blocks(size_t n, unsigned per) { return (unsigned)std::max<size_t>(1, (n + per - 1) / per); }

// The launches a solve supplies to gba_run. setup: free ranks (fidx, status[GBA_ST_NFREE]) and the solve's own argument checks;
// errors: err[] and the robust chi2 into scal[GBA_S_CHI]; linearise: Jacobians, Hll / bl, Hd / bp; reduce: Dinv, S = Hpp + lambda I,
// the right-hand side and the Schur complement; step: point increments, the retraction of every vertex and scal[GBA_S_SCALE].
// lambda_init: setUserLambdaInit; zero = g2o's own rule, lm_lambda_init of the largest diagonal entry.
struct GbaOps {
    int max_free;
    int (*setup)(const GbaDev&, hipStream_t);
    int (*errors)(const GbaDev&, hipStream_t);
    int (*linearise)(const GbaDev&, hipStream_t);
    int (*reduce)(const GbaDev&, double lambda, hipStream_t);
    int (*step)(const GbaDev&, double lambda, hipStream_t);
    double lambda_init;
};

// Lays the work arrays out in a workspace by D.nk / np / ne / blk / kf_w / rows; S (the only array whose size depends on the number of
// free key frames) comes last. Returns the bytes in all; nfree < 0: only the head (everything but S) is laid out and returned.
// *clear_bytes: the leading bytes gba_run clears.
size_t gba_layout(GbaDev& D, void* base, int nfree, size_t* clear_bytes);
// the factorisation chain + both substitutions; S and rhs hold the system, xp receives the solution
int gba_factor_solve(const GbaDev& D, hipStream_t st, bool solve);
// Dinv = (Hll + lambda I)^-1 and db = Dinv bl of every point
int gba_point_inverses(const GbaDev& D, double lambda, hipStream_t st);
// point_included without a solve (a stop flag raised before the call): a point with an edge is a vertex
int gba_mark_included(const GbaDev& D, hipStream_t st);
// The solve proper on device-resident inputs. `pinned`: 16 page-locked doubles. kf / pt (the working states) are kfs_out / points_out.
int gba_run(const viorb_gba_config* cfg, GbaDev& D, const GbaOps& ops, void* workspace, size_t workspace_bytes, const volatile int* stop,
            double* pinned, double info[6], hipStream_t st);
int gba_check_config(const viorb_gba_config* cfg, int nk, int np, int ne);
// accept (1) / reject (0) of every trial of the calling thread's last solve, for viorb_debug_gba_last_trials
std::vector<uint8_t>& gba_trials();

} // namespace viorb
