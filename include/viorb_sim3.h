/* include/viorb_sim3.h — the Sim3 RANSAC solver of the C ABI: reference src/Sim3Solver.cc:37-423 (the arithmetic of
 * LoopClosing::ComputeSim3, src/LoopClosing.cc:255-375, up to the call of SearchBySim3, which is viorb_search_by_sim3_device of
 * viorb_sim3_match.h and reads R12 / t12 / s12 of viorb_sim3_outputs where they lie). Included by viorb.h; include viorb.h, not this
 * file. The ctypes mirror is viorb_amd/capi.py: SIGNATURES_SIM3.
 *
 * Conventions (those of viorb_two_view.h): a batch of independent key-frame pairs, arrays [batch][cap] with per-pair counts
 * n[b] <= cap; 3 x 3 matrices are row-major float[9]. The caller passes the flat snapshot that Sim3Solver's constructor (:37-112)
 * builds from the map graph: correspondence i of a pair is the i-th one that survives the isBad / GetIndexInKeyFrame filtering, which
 * stays with the caller (viorb_amd/shim/Sim3Solver_shim.h). The library has no CPU fallback: every entry that launches returns
 * VIORB_ERR_NO_DEVICE without a device. Every entry checks its arguments before any GPU call. */
#ifndef VIORB_SIM3_H
#define VIORB_SIM3_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* The correspondences of `batch` pairs; device pointers for the _device entries.
 *   X1c, X2c [batch][cap][3]: mvX3Dc1 / mvX3Dc2, the matched points in the frame of their own camera (Rcw * Xw + tcw, :95-98);
 *   sigma2_1, sigma2_2 [batch][cap]: mvLevelSigma2[octave] of the two key points; the inlier thresholds are
 *   (float)(size_t)(9.210 * sigma2): mvnMaxError1/2 are vectors of size_t (include/Sim3Solver.h:78-79), so 9.21 sigma2 is truncated to
 *   an integer before the float comparison of :356;
 *   K1, K2 [batch][4] = fx fy cx cy; n [batch] = N, the number of correspondences (values outside 0..cap are clamped into it). */
typedef struct viorb_sim3_inputs {
    const float* X1c; const float* X2c; const float* sigma2_1; const float* sigma2_2; const float* K1; const float* K2; const int32_t* n;
    int32_t cap;
} viorb_sim3_inputs;

/* status of a pair after one call of the acceptance rule */
#define VIORB_SIM3_FOUND     0   /* iterate returned a model (bNoMore stays false, even at the last iteration) */
#define VIORB_SIM3_CONTINUE  1   /* iterations_per_call iterations ran without a model; mnIterations < mRansacMaxIts */
#define VIORB_SIM3_NO_MORE   2   /* mnIterations >= mRansacMaxIts without a model (bNoMore) */
#define VIORB_SIM3_FEW       3   /* N < min_inliers (:146-150): bNoMore, nothing is indexed */
/* why a set gave no hypothesis (0 for a set that did) */
#define VIORB_SIM3_SET_OK            0
#define VIORB_SIM3_SET_FEW           1   /* N < min_inliers or N < 3 */
#define VIORB_SIM3_SET_BAD           2   /* device entries only: an index outside 0..N-1 or a repeated index */
#define VIORB_SIM3_SET_ZERO_ROTATION 3   /* the quaternion's imaginary part is zero: the reference divides 0 / 0 (:280), its matrices are NaN
                                            and every comparison of :356 fails; here the matrices are zero and the count is 0 */

/* The RANSAC parameters and the carried state. iterations = the number of sets given per pair (1..4096); min_inliers = mRansacMinInliers
 * (20 in LoopClosing; >= 1); iterations_per_call = the argument of iterate (5 in LoopClosing; >= 1). */
typedef struct viorb_sim3_config {
    int32_t iterations; int32_t min_inliers; int32_t fix_scale; int32_t iterations_per_call;
} viorb_sim3_config;

/* Per-pair outputs; device pointers for viorb_sim3_ransac_device, host pointers for viorb_sim3_ransac. Any pointer may be NULL (that
 * output is not written) except status.
 *   status [batch] VIORB_SIM3_*; iterations_done [batch] = mnIterations after the call; best_inliers [batch] = mnBestInliers after the
 *   call; best_iter [batch] = the last iteration of this call that updated the best (-1: none did);
 *   R12 [batch][9], t12 [batch][3], s12 [batch], T12 [batch][16] = [s R | t; 0 0 0 1] of iteration best_iter (zero when best_iter < 0):
 *   on FOUND the returned model, otherwise mBestRotation / mBestTranslation / mBestScale as far as this call changed them;
 *   n_inliers [batch] and inliers [batch][cap] (mvbInliersi over the N correspondences, zero from N on): the returned model's on FOUND,
 *   zero otherwise, as iterate leaves nInliers and vbInliers. */
typedef struct viorb_sim3_outputs {
    int32_t* status; int32_t* iterations_done; int32_t* best_inliers; int32_t* best_iter; float* R12; float* t12; float* s12; float* T12;
    int32_t* n_inliers; uint8_t* inliers;
} viorb_sim3_outputs;

/* The RANSAC sets of :163-177 as an input (the reference draws them from a process-wide generator): sets [iterations][3], three draws
 * without replacement per set by the scheme and the splitmix64 generator that viorb_two_view_draw_sets documents. Host only.
 * VIORB_ERR_INVALID_ARG for n < 3 or iterations < 1. */
int viorb_sim3_draw_sets(int n, int iterations, uint64_t seed, int32_t* sets);
/* SetRansacParameters (:114-138): mRansacMaxIts = max(1, min(nIterations, max_iterations)) with the float epsilon = min_inliers / N and
 * nIterations = 1 for min_inliers == N, else ceil(log(1 - probability) / log(1 - epsilon^3)) in double. Host only, so that no device
 * log / pow decides an integer. Returns the value (>= 1), or VIORB_ERR_INVALID_ARG (< 0) for n < 1, min_inliers < 1, max_iterations < 1
 * or a probability outside (0, 1). For n < min_inliers the formula's log has a negative argument; the reference's conversion of a NaN
 * to int is undefined and iterate never reads the result (:146): the value returned is max_iterations. */
int viorb_sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations);
/* Device scratch of every _device entry below for these sizes (256-byte aligned device memory; its contents on entry are ignored); 0 for
 * sizes outside the limits. */
size_t viorb_sim3_workspace_bytes(int cap, int iterations, int batch);

/* The stages; viorb_sim3_ransac_device runs exactly these kernels in this order.
 * Common errors: VIORB_ERR_INVALID_ARG for a null array, cap < 1, batch outside 1..65535, iterations outside 1..4096, a workspace that is
 * too small or misaligned. All kernels go to `stream`; nothing is synchronised.
 *
 * Hypotheses (ComputeSim3 :226-337): d_sets [batch][iterations][3]; d_R12 [batch][iterations][9], d_t12 [..][3], d_s12 [..] and
 * d_reason [batch][iterations] = VIORB_SIM3_SET_* per set (zero matrices for a set that is not OK). */
int viorb_sim3_hypotheses_device(const viorb_sim3_inputs* in, const viorb_sim3_config* cfg, const int32_t* d_sets, int batch, float* d_R12,
                                 float* d_t12, float* d_s12, int32_t* d_reason, void* workspace, size_t workspace_bytes, void* stream);
/* Inlier counts (CheckInliers / Project :340-403, T21 as :332-336 write it) of given (R, t, s): d_counts [batch][iterations];
 * d_flags NULL or [batch][iterations][cap] (zero from N on). A zero model counts 0. */
int viorb_sim3_inliers_device(const viorb_sim3_inputs* in, const viorb_sim3_config* cfg, int batch, const float* d_R12, const float* d_t12,
                              const float* d_s12, int32_t* d_counts, uint8_t* d_flags, void* workspace, size_t workspace_bytes, void* stream);
/* The acceptance rule of iterate (:140-207) over given counts [batch][iterations], replayed literally from the carried state
 * d_first_iteration [batch] (mnIterations) and d_best_inliers_in [batch] (mnBestInliers) for at most cfg->iterations_per_call
 * iterations: the best count is updated on >=; the call returns FOUND at the first iteration whose count is both >= the running best
 * and > min_inliers; otherwise NO_MORE when d_max_its[b] (mRansacMaxIts) is reached, else CONTINUE; FEW when n[b] < min_inliers.
 * Iterations from cfg->iterations on have no set: a pair with d_max_its[b] > cfg->iterations stops there with CONTINUE.
 * d_n [batch]; outputs [batch] each, d_best_iter as in viorb_sim3_outputs. No workspace. */
int viorb_sim3_select_device(const viorb_sim3_config* cfg, const int32_t* d_counts, const int32_t* d_n, const int32_t* d_max_its,
                             const int32_t* d_first_iteration, const int32_t* d_best_inliers_in, int batch, int32_t* d_status,
                             int32_t* d_iterations_done, int32_t* d_best_inliers, int32_t* d_best_iter, void* stream);

/* Sim3Solver::iterate for `batch` pairs: hypotheses -> counts -> select -> the flags of the returned model. */
int viorb_sim3_ransac_device(const viorb_sim3_inputs* in, const viorb_sim3_config* cfg, const int32_t* d_sets, const int32_t* d_max_its,
                             const int32_t* d_first_iteration, const int32_t* d_best_inliers_in, int batch, const viorb_sim3_outputs* out,
                             void* workspace, size_t workspace_bytes, void* stream);
/* One pair from host buffers (re-entrant; allocates, runs, synchronises, copies back): X1c, X2c [n][3], sigma2_1/2 [n], K1, K2 [4],
 * sets [cfg->iterations][3]; the output arrays are sized with cap = max(n, 1). Here a set with an index outside 0..n-1 or a repeated
 * index is VIORB_ERR_INVALID_ARG (for n >= min_inliers and n >= 3), as is max_its > cfg->iterations. */
int viorb_sim3_ransac(const viorb_sim3_config* cfg, const float* X1c, const float* X2c, const float* sigma2_1, const float* sigma2_2,
                      const float* K1, const float* K2, int n, const int32_t* sets, int max_its, int first_iteration, int best_inliers_in,
                      const viorb_sim3_outputs* out);

/* ---- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:4589-4784) for `batch` key-frame pairs -------------------------------------
 * The flat snapshot of :4642-4721; device pointers for the _device entry.
 *   S12 [batch][8] double = r(x y z w) t s of g2oS12; X1c, X2c [batch][cap][3] float, widened as Converter::toVector3d does;
 *   obs1, obs2 [batch][cap][2]: the undistorted key points; inv_sigma2_1/2 [batch][cap] = mvInvLevelSigma2[octave];
 *   valid [batch][cap]: the correspondence exists and passes :4655-4657; K1, K2 [batch][4]; n [batch] entries are read (clamped to 0..cap). */
typedef struct viorb_sim3_opt_inputs {
    const double* S12; const float* X1c; const float* X2c; const float* obs1; const float* obs2; const float* inv_sigma2_1;
    const float* inv_sigma2_2; const uint8_t* valid; const float* K1; const float* K2; const int32_t* n; int32_t cap;
} viorb_sim3_opt_inputs;
/* g2o Levenberg (lambda = 1e-5 max diag at iteration 0 of each optimize() call) with Huber delta (double)(float)sqrt(th2) in both rounds:
 * optimize(5), the removal of every correspondence with a chi2 above th2 (10 in LoopClosing), optimize(10 if any was removed, else 5).
 * The Jacobians are g2o's numeric ones (central differences, delta 1e-9, through oplus); e->chi2() reads the error of the last trial.
 * d_S12_out [batch][8]; d_keep [batch][cap] = 0 where the reference sets vpMatches1[idx] = NULL in either round (and where valid is 0);
 * d_n_in [batch] = the return value; d_info [batch][8] = nCorrespondences, nBad, the iterations of both rounds, the robust chi2 after
 * both rounds, the accepted and the rejected LM trials. With nCorrespondences - nBad < 10 (:4754) n_in is 0 and S12_out = S12, the
 * first round's removals stay in keep; a pair without a valid correspondence returns at once with a zero info.
 * VIORB_ERR_INVALID_ARG: a null array, cap < 1, batch outside 1..65535, th2 <= 0. Nothing is synchronised. */
int viorb_optimize_sim3_device(const viorb_sim3_opt_inputs* in, float th2, int fix_scale, int batch, double* d_S12_out, uint8_t* d_keep,
                               int32_t* d_n_in, double* d_info, void* stream);
/* One pair from host buffers (re-entrant; allocates, runs, synchronises, copies back); arrays of n entries. */
int viorb_optimize_sim3(const double* S12, float th2, int fix_scale, const float* X1c, const float* X2c, const float* obs1, const float* obs2,
                        const float* inv_sigma2_1, const float* inv_sigma2_2, const uint8_t* valid, const float* K1, const float* K2, int n,
                        double* S12_out, uint8_t* keep, int32_t* n_in, double* info8);

/* Test hooks (no device): sim3_core.h compiled for the host.
 * One Horn hypothesis from three pairs P1, P2 [3][3] (point i of camera 1 / camera 2): returns VIORB_SIM3_SET_OK or _ZERO_ROTATION. */
int viorb_debug_sim3_horn(const float* P1, const float* P2, int fix_scale, float* R9, float* t3, float* s1);
/* One correspondence of CheckInliers under (R, t, s): err2 = err1 err2, max2 = the two truncated thresholds; returns 1 for an inlier. */
int viorb_debug_sim3_inlier(const float* R9, const float* t3, float s, const float* K1, const float* K2, const float* X1c3, const float* X2c3,
                            float sigma2_1, float sigma2_2, float* err2, float* max2);
/* The acceptance rule over n_counts counts from a carried state: out4 = status iterations_done best_inliers best_iter. */
int viorb_debug_sim3_select(const int32_t* counts, int n_counts, int n, int min_inliers, int max_its, int first_iteration, int best_inliers_in,
                            int iterations_per_call, int32_t* out4);

/* The Sim3 exponential of a 7-vector (omega, upsilon, sigma; sim3.h:70-142) as r(x y z w) t s, and exp(u) * estimate. */
int viorb_debug_sim3_exp(const double* u7, const double* est8, double* exp8, double* prod8);
/* Both edges of one correspondence under the estimate S8: e4 = the errors of EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ, J28 = their
 * 2 x 7 numeric Jacobians (row-major, one after the other) as g2o forms them; column 6 is exactly zero with fix_scale. */
int viorb_debug_sim3_edges(const double* S8, const double* X1c3, const double* X2c3, const double* obs1_2, const double* obs2_2, const double* K1,
                           const double* K2, int fix_scale, double* e4, double* J28);

#endif /* VIORB_SIM3_H */
