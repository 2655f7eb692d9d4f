/* include/viorb_relocalization.h — what Tracking::Relocalization (reference src/Tracking.cc:2127-2291) does after PnPsolver::iterate has
 * returned a hypothesis: the projection matcher ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:1473-1600, Frame::GetFeaturesInArea src/Frame.cc:507-560) and the refine cascade of :2209-2273 (solve, coarse search,
 * solve, narrow search, solve). Included by viorb.h; include viorb.h, not this file. The ctypes mirror is viorb_amd/capi.py:
 * SIGNATURES_RELOCALIZATION. The pieces before the hypothesis are viorb_kfdb_query* (DetectRelocalizationCandidates), viorb_search_by_bow*
 * (SearchByBoW(KF, F)) and, on the host, the reference's PnPsolver, which hands over Tcw and vbInliers.
 *
 * Conventions (those of viorb_sim3_match.h): arrays are [batch][cap] with per-item counts clamped into 0..cap; a pose is pose12 = Rcw(9)
 * tcw(3), float; a map point is pts_f[p][8] = Pw(3) normal(3) mfMinDistance mfMaxDistance plus pts_desc[p][32]; the camera is a
 * viorb_mapping_camera (fx fy cx cy, nlevels, scale_factors) plus bounds4 = mnMinX mnMaxX mnMinY mnMaxY. The lost frames are a
 * viorb_s3m_keyframes of n_frames frames (mvKeysUn, mDescriptors, N, the CSR grid of viorb_frontend_grid_device or
 * viorb_keyframe_grid_device), each of capacity fcap = frames->cap; hyp_frame [batch] names the frame of each hypothesis, so that the
 * candidates of one lost frame share one copy of it (NULL: hypothesis b uses frame b, n_frames >= batch; an index outside 0..n_frames-1
 * is a frame without features). The candidate key frame of hypothesis b is [kcap] arrays indexed by its feature i (the order of
 * pKF->GetMapPointMatches()), kf_count [batch] of them in use.
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null array, kcap < 1, fcap < 1, batch outside 1..65535,
 * n_frames < 1 (or < batch without hyp_frame), th <= 0, orb_dist outside 0..255, nlevels outside 1..16, empty bounds, a workspace that is
 * too small or not 256-byte aligned. VIORB_ERR_CAPACITY: fcap above VIORB_S3M_MAX_FEATURES. kcap has no limit beyond memory. Nothing is
 * ever truncated. Nothing in a _device entry synchronises. There is no CPU fallback: without a device the launching entries return
 * VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_RELOCALIZATION_H
#define VIORB_RELOCALIZATION_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* reason[i] of the matcher: the VIORB_S3M_* codes of viorb_sim3_match.h (NOT_CANDIDATE: no map point, bad, in sAlreadyFound, or i >=
 * kf_count; OUT_OF_IMAGE: :1508-1511; OUT_OF_RANGE: :1521; NO_FEATURE_IN_WINDOW: :1531; ABOVE_THRESHOLD: bestDist > ORBdist, no free
 * feature included; MATCHED), and one more. This function has no z < 0 gate and no viewing-angle gate, so BEHIND and VIEW_ANGLE (and
 * NOT_MUTUAL) never occur. */
#define VIORB_S3M_ROTATION              9   /* matched in the loop (:1556-1559), then removed by the rotation histogram (:1586-1596) */

/* Device scratch of viorb_search_by_projection_reloc_device for frames of fcap features, kcap key-frame features and `batch` hypotheses
 * (256-byte aligned device memory; its contents on entry are ignored). 0 for sizes outside the limits. */
size_t viorb_relocalization_workspace_bytes(int fcap, int kcap, int batch);

/* ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) for `batch` hypotheses. pose12 [batch][12] =
 * CurrentFrame.mTcw. Key-frame side [batch][kcap]: kf_angle = pKF->mvKeysUn[i].angle; kf_valid: vpMPs[i] exists and !isBad(); kf_found:
 * vpMPs[i] is in sAlreadyFound; pts_f [..][8], pts_desc [..][32]: the map point of feature i; kf_count [batch]. Frame side: feat_taken
 * [batch][fcap]: CurrentFrame.mvpMapPoints[i2] != NULL on entry. check_orientation = mbCheckOrientation.
 * best_idx [batch][kcap]: the frame feature the point of key-frame feature i keeps after the histogram, or -1; nmatches [batch]: the
 * return value; reason [batch][kcap] or NULL.
 * The result equals the reference's loop in the order of i exactly: point i takes the first minimum, in Frame::GetFeaturesInArea visiting
 * order with the level limits nPredictedLevel - 1 .. nPredictedLevel + 1 applied before the distance test, among the features that are
 * neither taken on entry nor taken by a point before i, if its distance is <= orb_dist; a feature stays claimed during the loop even if
 * the histogram removes its match afterwards. A point behind the camera whose projection lands inside the bounds is searched and can
 * match; the bounds test is `u < min || u > max`, which a coordinate on a bound and a NaN coordinate pass (z = 0 with x = y = 0: the
 * window of such a point is empty). */
int viorb_search_by_projection_reloc_device(const viorb_s3m_keyframes* frames, int n_frames, const int32_t* hyp_frame, const float* pose12,
                                            const float* kf_angle, const uint8_t* kf_valid, const uint8_t* kf_found, const float* pts_f,
                                            const uint8_t* pts_desc, const int32_t* kf_count, int kcap, const uint8_t* feat_taken,
                                            const viorb_mapping_camera* cam, const float bounds4[4], float th, int orb_dist, int check_orientation,
                                            int batch, int32_t* best_idx, int32_t* nmatches, int32_t* reason, void* workspace,
                                            size_t workspace_bytes, void* stream);
/* One hypothesis from host buffers (re-entrant; allocates, builds the grid, runs, synchronises, copies back): frame arrays of n entries,
 * key-frame arrays of npts entries. */
int viorb_search_by_projection_reloc(const viorb_keypoint* kps, const uint8_t* desc, int n, const float pose12[12], const float* kf_angle,
                                     const uint8_t* kf_valid, const uint8_t* kf_found, const float* pts_f, const uint8_t* pts_desc, int npts,
                                     const uint8_t* feat_taken, const viorb_mapping_camera* cam, const float bounds4[4], float th, int orb_dist,
                                     int check_orientation, int32_t* best_idx, int32_t* nmatches, int32_t* reason);

/* ---- the refine cascade (src/Tracking.cc:2209-2273) --------------------------------------------------------------------------------- */

/* stage[b]: the statement at which hypothesis b left the cascade */
#define VIORB_RELOC_FEW_INLIERS         1   /* :2228 nGood < min_good after the first solve: `continue`, nothing nulled */
#define VIORB_RELOC_ACCEPTED_FIRST      2   /* :2236 nGood >= accept after the first solve */
#define VIORB_RELOC_COARSE_SHORT        3   /* :2240 nadditional + nGood < accept after the coarse search */
#define VIORB_RELOC_SECOND_WEAK         4   /* :2246 nGood <= narrow_above after the second solve */
#define VIORB_RELOC_ACCEPTED_SECOND     5   /* :2246 nGood >= accept after the second solve */
#define VIORB_RELOC_NARROW_SHORT        6   /* :2255 nGood + nadditional < accept after the narrow search */
#define VIORB_RELOC_THIRD_REJECTED      7   /* :2269 nGood < accept after the third solve */
#define VIORB_RELOC_ACCEPTED_THIRD      8   /* :2269 nGood >= accept after the third solve */

/* The constants of :2228-2269. viorb_reloc_config_default sets the reference's: min_good 10, accept 50, narrow_above 30 (the narrow search
 * runs for narrow_above < nGood < accept), th_coarse 10 with orb_dist_coarse 100, th_narrow 3 with orb_dist_narrow 64, check_orientation 1
 * (matcher2 is ORBmatcher(0.9, true)). */
typedef struct viorb_reloc_config {
    int32_t min_good, accept, narrow_above;
    float th_coarse; int32_t orb_dist_coarse;
    float th_narrow; int32_t orb_dist_narrow;
    int32_t check_orientation;
} viorb_reloc_config;
int viorb_reloc_config_default(viorb_reloc_config* cfg);

/* Inputs of the cascade (device pointers): the matcher's (without kf_found and feat_taken, which the cascade derives), plus uright
 * [n_frames][fcap] = the frames' mvuRight (NULL: monocular, every edge is a mono edge), bow_match [batch][fcap]: the key-frame feature
 * whose map point frame feature j received from SearchByBoW (vvpMapPointMatches[i][j]), or -1; inlier [batch][fcap] = vbInliers.
 * Precondition: the frame's map points are identified by key-frame feature index, because every point the cascade touches belongs to the
 * candidate; a key frame holds a map point at most once (a pointer that repeats in GetMapPointMatches() would need two indices). */
typedef struct viorb_reloc_inputs {
    const viorb_s3m_keyframes* frames; int32_t n_frames; const int32_t* hyp_frame; const float* uright;
    const float* pose12; const float* kf_angle; const uint8_t* kf_valid; const float* pts_f; const uint8_t* pts_desc; const int32_t* kf_count;
    int32_t kcap;
    const int32_t* bow_match; const uint8_t* inlier;
} viorb_reloc_inputs;

/* Outputs per hypothesis (device pointers, none NULL): accepted [batch] (:2269), n_good [batch]: nGood at the exit, stage [batch], counts
 * [batch][8] = nGood1 nadditional1 nGood2 nadditional2 nGood3 0 0 0 (-1: the step did not run), out_pose12 [batch][12]: the pose after
 * the last solve that ran (mCurrentFrame.mTcw), chi2 [batch]: the final robust chi2 of that solve, frame_match [batch][fcap] and outlier
 * [batch][fcap]: mvpMapPoints (as key-frame feature indices, -1 = NULL) and mvbOutlier exactly as the reference leaves them at that exit
 * (mvbOutlier is false everywhere on entry, as the Frame constructor leaves it). */
typedef struct viorb_reloc_outputs {
    int32_t* accepted; int32_t* n_good; int32_t* stage; int32_t* counts; float* out_pose12; double* chi2; int32_t* frame_match; uint8_t* outlier;
} viorb_reloc_outputs;

/* Device scratch of viorb_relocalization_refine_device (its contents on entry are ignored); hcap is the capacity of the front-end handle
 * (viorb_frontend_capacity). */
size_t viorb_relocalization_refine_workspace_bytes(int fcap, int kcap, int hcap, int batch);

/* Steps (a) to (g) of :2209-2273 for `batch` hypotheses in lock step on one stream, with no host round trip: the per-hypothesis stage and
 * activity live in device memory, and a hypothesis that has left the cascade enters the remaining searches with no key-frame points and
 * the remaining solves with zero observations (the solver returns at once for fewer than three). The solves are
 * viorb_frontend_pose_opt_se3_device of handle h (its intrinsics; batch <= its max_batch, fcap <= its cap), bf = mbf. invSigma2 of an
 * observation is 1 / scale_factors[octave]^2 rounded to float as ORBextractor builds mvInvLevelSigma2.
 * The caller takes the first accepted hypothesis in candidate order: that equals the reference's sequential loop with its `break`
 * (:2186-2273), because each hypothesis rewrites the whole frame state (:2209 the pose, :2215-2224 every map point; mvbOutlier is written
 * before it is read for every feature that holds a point). */
int viorb_relocalization_refine_device(viorb_frontend* h, const viorb_reloc_inputs* in, const viorb_reloc_config* cfg,
                                       const viorb_mapping_camera* cam, const float bounds4[4], double bf, int batch,
                                       const viorb_reloc_outputs* out, void* workspace, size_t workspace_bytes, void* stream);

/* One hypothesis from host buffers (re-entrant; creates a front-end handle for the camera, allocates, builds the grid, runs, synchronises,
 * copies back): frame arrays of n entries (uright may be NULL), key-frame arrays of npts entries; every output is a caller's array
 * (counts [8], out_pose12 [12], frame_match [n], outlier [n]) or scalar. The call site of the shim (viorb_amd/shim). */
int viorb_relocalization_refine(const viorb_keypoint* kps, const uint8_t* desc, const float* uright, int n, const float pose12[12],
                                const float* kf_angle, const uint8_t* kf_valid, const float* pts_f, const uint8_t* pts_desc, int npts,
                                const int32_t* bow_match, const uint8_t* inlier, const viorb_reloc_config* cfg, const viorb_mapping_camera* cam,
                                const float bounds4[4], double bf, int32_t* accepted, int32_t* n_good, int32_t* stage, int32_t* counts,
                                float* out_pose12, double* chi2, int32_t* frame_match, uint8_t* outlier);

/* Shapes of the built kernels, for tests that probe their edges: out3 = points per workgroup of the gate kernel, the wavefront size, the
 * candidates a point's list holds before the claim rescans its window. */
int viorb_relocalization_shape(int32_t* out3);

/* Test hooks (no device): reloc_core.h compiled for the host.
 * One point through the gates: pt8 = pts_f of the point. out4 = u v dist3D radius; out6 = level, the cell rectangle x0 x1 y0 y1, reason
 * (VIORB_S3M_MATCHED: the point reaches the window scan). */
int viorb_debug_reloc_project(const float* pose12, const float* pt8, const viorb_mapping_camera* cam, const float bounds4[4], float th, float* out4,
                              int32_t* out6);
/* The claim loop plus the rotation histogram over given candidate lists (cand [npts][lcap] = distance << 16 | feature in visiting order,
 * cand_n [npts] <= lcap, taken_in [nfeat]); angle_kf [npts], angle_f [nfeat]. best_idx [npts], removed [npts] (the histogram took the match
 * away), *nmatches. */
int viorb_debug_reloc_match(const uint32_t* cand, const int32_t* cand_n, int npts, int lcap, const uint8_t* taken_in, int nfeat, int orb_dist,
                            int check_orientation, const float* angle_kf, const float* angle_f, int32_t* best_idx, uint8_t* removed,
                            int32_t* nmatches);
/* The decision after each step: step 1 = first solve, 2 = coarse search, 3 = second solve, 4 = narrow search, 5 = third solve; n_good
 * and n_additional as at that statement. Returns 0 when the cascade goes on, else the VIORB_RELOC_* exit. */
int viorb_debug_reloc_decide(const viorb_reloc_config* cfg, int step, int n_good, int n_additional);

#endif /* VIORB_RELOCALIZATION_H */
