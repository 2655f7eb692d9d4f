/* include/viorb_search_init.h — the monocular matcher of Tracking::MonocularInitialization and the scene depth of
 * CreateInitialMapMonocular: reference src/ORBmatcher.cc:405-520 (ORBmatcher::SearchForInitialization), src/Frame.cc:507-560
 * (Frame::GetFeaturesInArea), src/KeyFrame.cc:970-1000 (KeyFrame::ComputeSceneMedianDepth). Its matches12 / xy1 / xy2 are the inputs of
 * viorb_two_view_init_device (viorb_two_view.h). Included by viorb.h; include viorb.h, not this file. The ctypes mirror is
 * viorb_amd/capi.py: SIGNATURES_SEARCH_INIT.
 *
 * Conventions (those of viorb_sim3_match.h): a batch of independent streams, arrays [batch][cap] with per-stream counts clamped into
 * 0..cap; key points are viorb_keypoint (mvKeysUn); descriptors are 32 bytes; frame 2 is a viorb_s3m_keyframes whose cap equals `cap`
 * and whose grid is the CSR of viorb_keyframe_grid_device (Frame::AssignFeaturesToGrid is the key frame's arithmetic); bounds4 = mnMinX
 * mnMaxX mnMinY mnMaxY; a pose is pose12 = Rcw(9) tcw(3).
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null array, cap < 1, a frame-2 cap other than cap, batch
 * outside 1..65535, window_size <= 0, nnratio <= 0, empty bounds, q < 1, a workspace that is too small or not 256-byte aligned.
 * VIORB_ERR_CAPACITY: cap above VIORB_S3M_MAX_FEATURES (16-bit feature indices in the candidate lists; the ordered phase keeps one LDS
 * word per feature). Nothing is ever truncated. Nothing in a _device entry synchronises. There is no CPU fallback: without a device the
 * launching entries return VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_SEARCH_INIT_H
#define VIORB_SEARCH_INIT_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* reason[i]: how point i of frame 1 ends */
#define VIORB_SI_MATCHED               0   /* matches12[i] >= 0 */
#define VIORB_SI_NOT_CANDIDATE         1   /* i >= n1 or octave > 0 (:422) */
#define VIORB_SI_NO_FEATURE_IN_WINDOW  2   /* vIndices2.empty() (:427) */
#define VIORB_SI_ABOVE_THRESHOLD       3   /* bestDist > TH_LOW (50), every candidate skipped by :444 included (:459) */
#define VIORB_SI_RATIO                 4   /* !(bestDist < (float)bestDist2 * nnratio) (:461) */
#define VIORB_SI_DISPLACED             5   /* accepted, then a later point took its feature (:463-467) */
#define VIORB_SI_ROTATION              6   /* accepted, then removed by the rotation histogram (:497-510) */

/* Optional outputs (device pointers for the _device entry, host pointers for the host entry; NULL: not written).
 *   matches21, matched_distance [batch][cap]: vnMatches21 and vMatchedDistance as the main loop leaves them (the rotation step does not
 *   clear them); -1 / INT_MAX for an untouched feature and from n2 on. rot_hist [batch][30]: rotHist[i].size(), displaced entries
 *   included (zero when check_orientation is 0). reason [batch][cap]: VIORB_SI_*. xy1, xy2 [batch][cap][2]: mvKeysUn[i].pt of frame 1
 *   and frame 2 (zero from the count on), the layout viorb_two_view_init_device reads. sweeps [batch]: the sweeps the ordered phase took. */
typedef struct viorb_search_init_outputs {
    int32_t* matches21; int32_t* matched_distance; int32_t* rot_hist; int32_t* reason; float* xy1; float* xy2; int32_t* sweeps;
} viorb_search_init_outputs;

/* Device scratch of viorb_search_for_initialization_device (256-byte aligned device memory; its contents on entry are ignored). 0 for
 * sizes outside the limits. */
size_t viorb_search_init_workspace_bytes(int cap, int batch);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:405-520) for `batch` streams,
 * equal to the reference's i1-ascending loop bit for bit. kps1 / desc1 [batch][cap], n1 [batch]: frame 1; kf2: frame 2 and its grid;
 * prev_matched [batch][cap][2]: vbPrevMatched, read as the window centres and overwritten for the points that end matched (:515-517);
 * window_size is converted to float as GetFeaturesInArea's `r` is; nnratio = mfNNratio; check_orientation = mbCheckOrientation.
 * matches12 [batch][cap]: the index in frame 2 or -1 (-1 from n1 on); nmatches [batch]. out may be NULL. */
int viorb_search_for_initialization_device(const viorb_keypoint* kps1, const uint8_t* desc1, const int32_t* n1, const viorb_s3m_keyframes* kf2,
                                           float* prev_matched, int cap, int batch, const float bounds4[4], int window_size, float nnratio,
                                           int check_orientation, int32_t* matches12, int32_t* nmatches,
                                           const viorb_search_init_outputs* out, void* workspace, size_t workspace_bytes, void* stream);
/* One stream from host buffers (re-entrant; allocates, builds the grid of frame 2, runs, synchronises, copies back): kps1 / desc1 /
 * prev_matched / matches12 / reason / xy1 of n1 entries, kps2 / desc2 / matches21 / matched_distance / xy2 of n2 entries. */
int viorb_search_for_initialization(const viorb_keypoint* kps1, const uint8_t* desc1, int n1, const viorb_keypoint* kps2, const uint8_t* desc2,
                                    int n2, float* prev_matched, const float bounds4[4], int window_size, float nnratio, int check_orientation,
                                    int32_t* matches12, int32_t* nmatches, const viorb_search_init_outputs* out);

/* Shapes of the built kernels, for tests that probe their edges: out4 = points per workgroup of the candidate pass (one wavefront each),
 * the wavefront size, the candidates a point's list holds before the ordered phase rescans its window, threads of the ordered phase. */
int viorb_search_init_shape(int32_t* out4);

/* KeyFrame::ComputeSceneMedianDepth(q) (src/KeyFrame.cc:970-1000) for `batch` key frames: pose12 [batch][12]; points [batch][cap][3] =
 * GetWorldPos of feature i's map point; has_point [batch][cap]; count [batch] = N. median [batch]: the (n - 1) / q-th smallest of the
 * depths (float)(r20 x + r21 y + r22 z + tz), summed in double in that order, exactly; n_depths [batch] = n. A key frame without a point
 * gives median -1 and n_depths 0 (the reference indexes out of range). */
int viorb_scene_median_depth_device(const float* pose12, const float* points, const uint8_t* has_point, const int32_t* count, int cap, int batch,
                                    int q, float* median, int32_t* n_depths, void* stream);
/* One key frame from host buffers: points [n][3], has_point [n]. */
int viorb_scene_median_depth(const float pose12[12], const float* points, const uint8_t* has_point, int n, int q, float* median, int32_t* n_depths);

/* Test hooks (no device): search_init_core.h compiled for the host.
 * The ordered phase over given candidate lists: cand [npts][lcap] = distance << 16 | feature in visiting order, cand_n [npts] (<= lcap).
 * state [npts] = distance << 16 | feature of an accepted point or 0xffffffff, why [npts] = VIORB_SI_MATCHED / _ABOVE_THRESHOLD / _RATIO,
 * and matches12 [npts], matches21 / matched_distance [nfeat] as the main loop leaves them; *nmatches before the rotation step. Returns
 * the number of sweeps (>= 1) or an error (< 0). */
int viorb_debug_search_init_ordered(const uint32_t* cand, const int32_t* cand_n, int npts, int lcap, int nfeat, float nnratio, uint32_t* state,
                                    int32_t* why, int32_t* matches12, int32_t* matches21, int32_t* matched_distance, int32_t* nmatches);
/* One window through GetFeaturesInArea(x, y, r, level1, level1) over a host grid (cell_start [64*48+1], cell_idx) of kps2 [n2]:
 * rect4 = nMinCellX nMaxCellX nMinCellY nMaxCellY (as far as the early returns computed them), out_idx [n2] the features in visiting
 * order. Returns their number, or an error (< 0). */
int viorb_debug_search_init_window(const viorb_keypoint* kps2, int n2, const int32_t* cell_start, const int32_t* cell_idx, const float bounds4[4],
                                   float x, float y, float r, int level1, int32_t* rect4, int32_t* out_idx);
/* The depth of one point (:992). */
float viorb_debug_scene_depth(const float* pose12, const float* point3);

#endif /* VIORB_SEARCH_INIT_H */
