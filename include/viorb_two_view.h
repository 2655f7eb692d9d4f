/* include/viorb_two_view.h — the two-view (monocular) initialiser of the C ABI: reference src/Initializer.cc:44-929. Included by viorb.h;
 * include viorb.h, not this file. The ctypes mirror is viorb_amd/capi.py: SIGNATURES_TWO_VIEW.
 *
 * Conventions (those of viorb_create_new_map_points(_device)): a batch of independent streams, arrays [batch][cap] with per-stream
 * counts n1[b], n2[b] <= cap; key points are undistorted float xy pairs (Frame::mvKeysUn[i].pt); matches12[b][i1] = index in frame 2
 * or < 0 (vMatches12). The match list of a stream is the (i1, matches12[i1]) pairs with matches12[i1] >= 0 in increasing i1 (:51-63);
 * N is its length, and "compacted index" below means an index into it. 3 x 3 matrices are row-major float[9]. The library has no CPU
 * fallback: every entry that launches returns VIORB_ERR_NO_DEVICE without a device. */
#ifndef VIORB_TWO_VIEW_H
#define VIORB_TWO_VIEW_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* Initializer(ReferenceFrame, sigma, iterations) (:32-42), the 1.0 / 50 of the ReconstructH / ReconstructF calls (:116-118) and mK. */
typedef struct viorb_two_view_config {
    float sigma;               /* 1.0 */
    int32_t iterations;        /* 200; 1..4096 */
    float min_parallax_deg;    /* 1.0 */
    int32_t min_triangulated;  /* 50 */
    float fx, fy, cx, cy;
} viorb_two_view_config;

#define VIORB_TWO_VIEW_FAILED 0
#define VIORB_TWO_VIEW_FROM_H 1
#define VIORB_TWO_VIEW_FROM_F 2
/* why a stream failed (0 for a stream that did not) */
#define VIORB_TWO_VIEW_REASON_OK            0
#define VIORB_TWO_VIEW_REASON_FEW_MATCHES   1   /* N < 8: no set is ever indexed */
#define VIORB_TWO_VIEW_REASON_BAD_SET       2   /* device entries only: a set with an index outside 0..N-1 or a repeated index */
#define VIORB_TWO_VIEW_REASON_NO_MODEL      3   /* no hypothesis of the chosen model scored above 0 (undefined behaviour in the reference, :165, 216) */
#define VIORB_TWO_VIEW_REASON_H_DEGENERATE  4   /* d1/d2 < 1.00001 || d2/d3 < 1.00001 (:597) */
#define VIORB_TWO_VIEW_REASON_NO_WINNER     5   /* secondBestGood >= 0.75 bestGood (:721); nsimilar > 1 (:517) */
#define VIORB_TWO_VIEW_REASON_FEW_GOOD      6   /* bestGood <= minTriangulated or <= 0.9 N_inliers (:721); maxGood < nMinGood (:517) */
#define VIORB_TWO_VIEW_REASON_PARALLAX      7   /* bestParallax < minParallax (:721); parallax <= minParallax (:525) */
#define VIORB_TWO_VIEW_MAX_HYPOTHESES 8

/* Per-stream outputs; device pointers for the _device entries, host pointers for viorb_two_view_init. Any pointer may be NULL (that
 * output is not written) except status and reason.
 *   status [batch] VIORB_TWO_VIEW_*; reason [batch]; n_matches [batch] = N; scores [batch][2] = SH SF; best_iter [batch][2] = the winning
 *   iteration of the H and of the F search (-1: none scored above 0); H21, F21 [batch][9] of those winners; inliers_h, inliers_f
 *   [batch][cap]: their vbMatchesInliers over the compacted list (zero from N on);
 *   R21 [batch][9], t21 [batch][3], P3D [batch][cap][3] and triangulated [batch][cap], indexed by i1 (vP3D, vbTriangulated): all zero for
 *   a failed stream; the point of a key point without a surviving match is (0, 0, 0);
 *   n_hyp [batch] = 8 (H), 4 (F) or 0 motion hypotheses; hyp_n_good [batch][8], hyp_parallax [batch][8], hyp_R [batch][8][9],
 *   hyp_t [batch][8][3]: CheckRT's nGood and parallax per hypothesis in the reference's order (zero from n_hyp on). */
typedef struct viorb_two_view_outputs {
    int32_t* status; int32_t* reason; int32_t* n_matches; float* scores; int32_t* best_iter; float* H21; float* F21;
    uint8_t* inliers_h; uint8_t* inliers_f; float* R21; float* t21; float* P3D; uint8_t* triangulated;
    int32_t* n_hyp; int32_t* hyp_n_good; float* hyp_parallax; float* hyp_R; float* hyp_t;
} viorb_two_view_outputs;

/* The RANSAC sets of :78-97 as an input (the reference draws them from a process-wide rand()): sets [iterations][8], indices into the
 * compacted list. Per set: a uniform index into the shrinking list of available indices, the last entry moved into the hole, eight
 * draws without replacement. Generator: splitmix64 (state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31) started from `seed`; the index is floor((z >> 11) * 2^-53 * available).
 * Host only. VIORB_ERR_INVALID_ARG for n_matches < 8 or iterations < 1. */
int viorb_two_view_draw_sets(int n_matches, int iterations, uint64_t seed, int32_t* sets);

/* Device scratch of every _device entry below for these sizes (256-byte aligned device memory; its contents on entry are ignored). */
size_t viorb_two_view_workspace_bytes(int cap, int iterations, int batch);

/* Initializer::Initialize (:44-121) for `batch` streams: Normalize over all key points of each frame (:749-795), cfg->iterations
 * homography and fundamental hypotheses from the same sets (FindHomography :124-172, FindFundamental :175-223, ComputeH21 / ComputeF21
 * :226-303), their scores (CheckHomography / CheckFundamental :305-468), the first-maximum winners, RH = SH / (SH + SF) > 0.40 (:112-118),
 * ReconstructH (:572-732) or ReconstructF / DecomposeE (:470-570, 909-929) with CheckRT / Triangulate (:734-747, 798-907).
 * d_sets [batch][iterations][8]. A stream with N < 8 fails with REASON_FEW_MATCHES, one with a bad set with REASON_BAD_SET.
 * VIORB_ERR_INVALID_ARG: a null array, cap < 1, batch outside 1..65535, iterations outside 1..4096, sigma <= 0, fx or fy == 0, a
 * workspace that is too small or misaligned. All kernels go to `stream`; nothing is synchronised. */
int viorb_two_view_init_device(const viorb_two_view_config* cfg, const float* d_xy1, const int32_t* d_n1, const float* d_xy2,
                               const int32_t* d_n2, int cap, const int32_t* d_matches12, const int32_t* d_sets, int batch,
                               const viorb_two_view_outputs* out, void* workspace, size_t workspace_bytes, void* stream);
/* One stream from host buffers (re-entrant; allocates, runs, synchronises, copies back). The output arrays are sized with
 * cap = max(n1, n2, 1). Here a set with an index outside 0..N-1 or a repeated index is VIORB_ERR_INVALID_ARG, as is matches12[i1] >= n2. */
int viorb_two_view_init(const viorb_two_view_config* cfg, const float* xy1, int n1, const float* xy2, int n2, const int32_t* matches12,
                        const int32_t* sets, const viorb_two_view_outputs* out);

/* The stages of the above on their own; viorb_two_view_init_device runs exactly these kernels in this order.
 * Hypotheses (:148-161, 199-212): H21i, H12i, F21i [batch][iterations][9] per set; reason [batch] = OK, FEW_MATCHES or BAD_SET (the
 * matrices of a bad set, and all of a stream with too few matches, are zero). */
int viorb_two_view_hypotheses_device(const viorb_two_view_config* cfg, const float* d_xy1, const int32_t* d_n1, const float* d_xy2,
                                     const int32_t* d_n2, int cap, const int32_t* d_matches12, const int32_t* d_sets, int batch,
                                     float* d_H21i, float* d_H12i, float* d_F21i, int32_t* d_reason, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* Scores (:305-468) of given matrices: d_scores [batch][iterations][2] (H, F); d_flags NULL or [batch][iterations][2][cap], the inlier
 * flags over the compacted list. */
int viorb_two_view_score_device(const viorb_two_view_config* cfg, const float* d_xy1, const int32_t* d_n1, const float* d_xy2,
                                const int32_t* d_n2, int cap, const int32_t* d_matches12, int batch, const float* d_H21i,
                                const float* d_H12i, const float* d_F21i, float* d_scores, uint8_t* d_flags, void* workspace,
                                size_t workspace_bytes, void* stream);
/* Reconstruction (:470-732, 798-929) from a given model: d_model [batch] = VIORB_TWO_VIEW_FROM_H / _FROM_F (anything else: the stream
 * is skipped and fails with REASON_NO_MODEL), d_M [batch][9] = H21 or F21, d_inliers [batch][cap] over the compacted list. Writes
 * status, reason, n_matches, R21, t21, P3D, triangulated, n_hyp and hyp_* of `out`. */
int viorb_two_view_reconstruct_device(const viorb_two_view_config* cfg, const float* d_xy1, const int32_t* d_n1, const float* d_xy2,
                                      const int32_t* d_n2, int cap, const int32_t* d_matches12, int batch, const int32_t* d_model,
                                      const float* d_M, const uint8_t* d_inliers, const viorb_two_view_outputs* out, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* Test hooks (no device): two_view_core.h compiled for the host.
 * One hypothesis from eight pairs of normalised points pn1, pn2 [8][2]: model FROM_H -> Hn = vt.row(8) of the 16 x 9 A (:226-266),
 * FROM_F -> Fn after the rank-2 step (:268-303); pre9 (may be NULL) = vt.row(8) itself. */
int viorb_debug_two_view_hypothesis(int model, const float* pn1, const float* pn2, float* M9, float* pre9);
/* De-normalisation (:160-161, 212) with nrm4 = meanX meanY sX sY of each frame: FROM_H -> M21 = H21i, M12 = H12i; FROM_F -> M21 = F21i. */
int viorb_debug_two_view_denormalise(int model, const float* Mn9, const float* nrm1_4, const float* nrm2_4, float* M21, float* M12);
/* Normalize (:749-795) of n key points: nrm4 = meanX meanY sX sY. */
int viorb_debug_two_view_normalise(const float* xy, int n, float* nrm4);
/* One match's two chi-squares (:352-374 with M12 = H12; :428-454, M12 unused); returns 1 for an inlier; *score = its contribution. */
int viorb_debug_two_view_chi2(int model, const float* M21, const float* M12, const float* uv4, float sigma, float* chi2_2, float* score);
/* One decomposition: FROM_H -> the eight (R, t) of :584-686 (returns 8, or 0 when the singular-value gate refuses; d3 = d1 d2 d3),
 * FROM_F -> the four of :479-486, 909-929 (returns 4). R [8][9], t [8][3]. */
int viorb_debug_two_view_decompose(int model, const float* M21, const float* K4, float* R, float* t, float* d3);
/* One match of CheckRT (:830-893) with th2 = 4 sigma^2: returns 0 (not counted), 1 (counted) or 2 (counted and vbGood); X3 = the
 * point, q6 = cosParallax z1 z2 squareError1 squareError2 dist2. */
int viorb_debug_two_view_check_rt(const float* K4, const float* R9, const float* t3, const float* uv4, float sigma, float* X3, float* q6);
/* sort + vCosParallax[min(50, size - 1)] + acos (:896-904) by the kernels' radix select on the float bits; 0 for n == 0. */
float viorb_debug_two_view_parallax(const float* cos_parallax, int n);
/* The accept rules (:499-569, 689-731): returns the winning hypothesis or -1, *reason = VIORB_TWO_VIEW_REASON_*. */
int viorb_debug_two_view_accept(int model, const int32_t* n_good, const float* parallax, int n_inliers, float min_parallax_deg,
                                int min_triangulated, int32_t* reason);

#endif /* VIORB_TWO_VIEW_H */
