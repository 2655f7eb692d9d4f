// viorb_amd/csrc/global_ba_dev.h — what the two global bundle adjustments share on the device side: the work arrays of one solve
// (GbaDev), the host functions of global_ba.hip that both call (graph bookkeeping, the blocked Cholesky chain, the Levenberg loop) and
// the table of launches a solve plugs into that loop (GbaOps). global_ba.hip is the NavState solve (12 coordinates per free key frame,
// IMU factors), global_ba_se3.hip the vision-only one (6 coordinates, monocular and stereo edges). The kernels named here live in
// global_ba.hip; the other translation unit reaches them through these host functions only.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "viorb_common.h"
#include "global_ba_core.h"

namespace viorb {

enum { GBA_S_CHI = 0, GBA_S_SCALE, GBA_S_FAIL, GBA_S_MAXDIAG, GBA_S_N = 8 };
enum { GBA_ST_INVALID = 0, GBA_ST_NFREE, GBA_ST_N = 4 };
// bits of status[GBA_ST_INVALID]
enum { GBA_BAD_PREV = 1, GBA_BAD_EDGE = 2, GBA_BAD_COV = 4, GBA_BAD_SIGMA = 8, GBA_BAD_BF = 16 };

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
};

__device__ __forceinline__ double gba_block_sum(double v, double* s_red) {      // 256 threads; result valid in thread 0
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
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
struct GbaOps {
    int max_free;
    int (*setup)(const GbaDev&, hipStream_t);
    int (*errors)(const GbaDev&, hipStream_t);
    int (*linearise)(const GbaDev&, hipStream_t);
    int (*reduce)(const GbaDev&, double lambda, hipStream_t);
    int (*step)(const GbaDev&, double lambda, hipStream_t);
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
