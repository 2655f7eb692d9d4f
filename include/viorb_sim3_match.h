/* include/viorb_sim3_match.h — the three projection matchers of loop closing that take a similarity instead of a pose, and the key-frame
 * grid they search: reference src/ORBmatcher.cc:290-403 (SearchByProjection(KeyFrame*, Scw, ...)), :977-1100 (Fuse(KeyFrame*, Scw, ...)),
 * :1102-1326 (SearchBySim3), src/KeyFrame.cc:906-945 (GetFeaturesInArea). With viorb_sim3.h they are the arithmetic of
 * LoopClosing::ComputeSim3 (src/LoopClosing.cc:255-441) and of LoopClosing::SearchAndFuse (:616-642). Included by viorb.h; include
 * viorb.h, not this file. The ctypes mirror is viorb_amd/capi.py: SIGNATURES_SIM3_MATCH.
 *
 * Conventions (those of viorb_sim3.h and of viorb_frontend_fuse_device): arrays are [batch][cap] with per-item counts clamped into
 * 0..cap; 3 x 3 matrices are row-major float[9]; a pose is pose12 = Rcw(9) tcw(3); a similarity Scw is float[12], the top three rows of
 * the 4 x 4; a map point is pts_f[p][8] = Pw(3) normal(3) mfMinDistance mfMaxDistance plus pts_desc[p][32] = GetDescriptor(); the camera
 * is a viorb_mapping_camera (fx fy cx cy, nlevels, scale_factors; the logarithm of scale_factors[1] is taken on the host as viorb_fuse
 * takes it) plus bounds4 = mnMinX mnMaxX mnMinY mnMaxY; the grid is the CSR cell_start[64*48+1] / cell_idx[cap] in storage order
 * ix*48 + iy. What stays with the caller: the map writes (Replace, AddObservation, AddMapPoint; viorb_amd/shim), the mnLoopPointForKF
 * de-duplication that builds mvpLoopMapPoints (the covisibility graph that follows them is viorb_update_connections, viorb_covisibility.h).
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null array, cap < 1 (pcap < 1), batch outside 1..65535,
 * th <= 0, nlevels outside 1..16, empty bounds, a workspace that is too small or not 256-byte aligned. VIORB_ERR_CAPACITY: cap above
 * VIORB_S3M_MAX_FEATURES (16-bit feature indices in the candidate lists; the grid sort and the ordered phase keep one LDS word per
 * feature). Nothing is ever truncated. Nothing in a _device entry synchronises. There is no CPU fallback: without a device the launching
 * entries return VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_SIM3_MATCH_H
#define VIORB_SIM3_MATCH_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

#define VIORB_S3M_MAX_FEATURES 16384

/* reason[i]: which statement of the reference ended point i (one per `continue`) */
#define VIORB_S3M_MATCHED               0   /* best_idx / match >= 0 */
#define VIORB_S3M_NOT_CANDIDATE         1   /* no map point, bad, already matched / found (:317, :1005, :1152-1156, :1232-1236), or i >= count */
#define VIORB_S3M_BEHIND                2   /* z < 0 (:327, :1015, :1163, :1243) */
#define VIORB_S3M_OUT_OF_IMAGE          3   /* !IsInImage(u, v) (:339, :1027, :1174, :1254); z == 0 ends here */
#define VIORB_S3M_OUT_OF_RANGE          4   /* dist outside [0.8 mfMinDistance, 1.2 mfMaxDistance] (:348, :1036, :1182, :1262) */
#define VIORB_S3M_VIEW_ANGLE            5   /* PO . Pn < 0.5 dist (:354, :1042); the two Scw functions only */
#define VIORB_S3M_NO_FEATURE_IN_WINDOW  6   /* vIndices.empty() (:364, :1053, :1193, :1273) */
#define VIORB_S3M_ABOVE_THRESHOLD       7   /* bestDist > TH_LOW (50; the Scw functions) / TH_HIGH (100; SearchBySim3), no free or level-compatible feature included */
#define VIORB_S3M_NOT_MUTUAL            8   /* SearchBySim3: a one-way match the other direction does not return (:1314-1322) */

/* `batch` key frames (device pointers): kps / desc [batch][cap] (mvKeysUn, mDescriptors), count [batch] = N, the grid of
 * viorb_keyframe_grid_device. */
typedef struct viorb_s3m_keyframes {
    const viorb_keypoint* kps; const uint8_t* desc; const int32_t* count; const int32_t* cell_start; const int32_t* cell_idx; int32_t cap;
} viorb_s3m_keyframes;

/* One side of SearchBySim3 (device pointers): pose12 [batch][12] = GetRotation / GetTranslation; has_point [batch][cap]: feature i has a
 * map point and it is not bad; pts_f [batch][cap][8], pts_desc [batch][cap][32]: the map point of feature i; already [batch][cap] =
 * vbAlreadyMatched1 / 2 (:1129-1142), which the caller derives from vpMatches12 and GetIndexInKeyFrame. */
typedef struct viorb_s3m_side {
    viorb_s3m_keyframes kf; const float* pose12; const uint8_t* has_point; const float* pts_f; const uint8_t* pts_desc; const uint8_t* already;
} viorb_s3m_side;

/* Device scratch of every _device entry below (256-byte aligned device memory; its contents on entry are ignored) for key frames of `cap`
 * features, `pcap` points per list and `batch` items; for SearchBySim3 cap is the larger of the two sides' and pcap is ignored. 0 for
 * sizes outside the limits. */
size_t viorb_sim3_match_workspace_bytes(int cap, int pcap, int batch);

/* KeyFrame::mGrid (a copy of Frame::mGrid; Frame::AssignFeaturesToGrid, src/Frame.cc:410-425) without a front-end handle: the CSR that
 * viorb_frontend_grid_device builds, by the same kernel. kps [batch][cap], count [batch]; cell_start [batch][64*48+1], cell_idx
 * [batch][cap] (entries from cell_start[..][64*48] on are not written). */
int viorb_keyframe_grid_device(const viorb_keypoint* kps, const int32_t* count, int cap, int batch, const float bounds4[4], int32_t* cell_start,
                               int32_t* cell_idx, void* stream);
/* One key frame from host buffers: kps [n], cell_start [64*48+1], cell_idx [max(n, 1)]. */
int viorb_keyframe_grid(const viorb_keypoint* kps, int n, const float bounds4[4], int32_t* cell_start, int32_t* cell_idx);

/* ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1102-1326) for `batch` key-frame pairs. R12 [batch][9], t12 [batch][3], s12 [batch]: the
 * arrays viorb_sim3_outputs holds, so that the RANSAC's model feeds this call without leaving the device. th is 7.5 in LoopClosing.
 * match12 [batch][cap1]: idx2 where the two one-way searches agree (:1307-1323), else -1 (the caller merges with the matches it had);
 * nfound [batch]. Optional (NULL: not written): match1 [batch][cap1], match2 [batch][cap2] = vnMatch1 / vnMatch2; reason1 [batch][cap1],
 * reason2 [batch][cap2] = VIORB_S3M_* per feature. The descriptor gate is TH_HIGH (100). */
int viorb_search_by_sim3_device(const viorb_s3m_side* side1, const viorb_s3m_side* side2, const float* R12, const float* t12, const float* s12,
                                const viorb_mapping_camera* cam, const float bounds4[4], float th, int batch, int32_t* match12, int32_t* nfound,
                                int32_t* match1, int32_t* match2, int32_t* reason1, int32_t* reason2, void* workspace, size_t workspace_bytes,
                                void* stream);
/* One pair from host buffers (re-entrant; allocates, builds both grids, runs, synchronises, copies back): arrays of n1 / n2 entries. */
int viorb_search_by_sim3(const viorb_keypoint* kps1, const uint8_t* desc1, int n1, const float pose12_1[12], const uint8_t* has_point1,
                         const float* pts_f1, const uint8_t* pts_desc1, const uint8_t* already1, const viorb_keypoint* kps2, const uint8_t* desc2,
                         int n2, const float pose12_2[12], const uint8_t* has_point2, const float* pts_f2, const uint8_t* pts_desc2,
                         const uint8_t* already2, const float R12[9], const float t12[3], float s12, const viorb_mapping_camera* cam,
                         const float bounds4[4], float th, int32_t* match12, int32_t* nfound, int32_t* match1, int32_t* match2, int32_t* reason1,
                         int32_t* reason2);

/* ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:290-403) for `batch` key frames, each with
 * its own point list: Scw [batch][12]; pts_f [batch][pcap][8], pts_desc [batch][pcap][32], pts_count [batch]; pts_valid [batch][pcap]:
 * not bad and not in spAlreadyFound; feat_taken [batch][cap]: vpMatched[idx] != NULL on entry. best_idx [batch][pcap]: the feature point
 * p takes, or -1; nmatches [batch]; reason [batch][pcap] or NULL.
 * The function is ordered (:375 skips a feature an earlier point of the same call has taken, :396 takes it), and the result equals the
 * reference's point-order loop exactly: point p takes the first minimum, in GetFeaturesInArea visiting order, among the features that
 * are neither taken on entry nor taken by a point before p, if its distance is <= TH_LOW (50). */
int viorb_search_by_projection_sim3_device(const viorb_s3m_keyframes* kf, const float* Scw, const float* pts_f, const uint8_t* pts_desc,
                                           const uint8_t* pts_valid, const int32_t* pts_count, int pcap, const uint8_t* feat_taken,
                                           const viorb_mapping_camera* cam, const float bounds4[4], float th, int batch, int32_t* best_idx,
                                           int32_t* nmatches, int32_t* reason, void* workspace, size_t workspace_bytes, void* stream);
/* One key frame from host buffers: arrays of n features and npts points. */
int viorb_search_by_projection_sim3(const viorb_keypoint* kps, const uint8_t* desc, int n, const float Scw[12], const float* pts_f,
                                    const uint8_t* pts_desc, const uint8_t* pts_valid, int npts, const uint8_t* feat_taken,
                                    const viorb_mapping_camera* cam, const float bounds4[4], float th, int32_t* best_idx, int32_t* nmatches,
                                    int32_t* reason);

/* ORBmatcher::Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:977-1100) for `batch` key frames over ONE shared
 * point list, as LoopClosing::SearchAndFuse (src/LoopClosing.cc:616-642) runs it over mvpLoopMapPoints: pts_f [pcap][8] and pts_desc
 * [pcap][32] are given once, npts <= pcap of them are read; pts_valid [batch][pcap]: not bad and not already in key frame b; Scw
 * [batch][12]. best_idx [batch][pcap]: the feature, when the distance is <= TH_LOW, or -1; nfused [batch]; reason [batch][pcap] or NULL.
 * The replace / add block of :1081-1096 is the caller's. No chi-square gate and no uright, unlike viorb_frontend_fuse_device. */
int viorb_fuse_sim3_device(const viorb_s3m_keyframes* kf, const float* Scw, const float* pts_f, const uint8_t* pts_desc, const uint8_t* pts_valid,
                           int npts, int pcap, const viorb_mapping_camera* cam, const float bounds4[4], float th, int batch, int32_t* best_idx,
                           int32_t* nfused, int32_t* reason, void* workspace, size_t workspace_bytes, void* stream);
/* One key frame from host buffers. */
int viorb_fuse_sim3(const viorb_keypoint* kps, const uint8_t* desc, int n, const float Scw[12], const float* pts_f, const uint8_t* pts_desc,
                    const uint8_t* pts_valid, int npts, const viorb_mapping_camera* cam, const float bounds4[4], float th, int32_t* best_idx,
                    int32_t* nfused, int32_t* reason);

/* Shapes of the built kernels, for tests that probe their edges: out3 = points per workgroup of the projection kernels, the wavefront
 * size, the candidates a point's list holds before the ordered phase rescans its window. */
int viorb_sim3_match_shape(int32_t* out3);

/* Test hooks (no device): sim3_match_core.h compiled for the host.
 * Scw [12] decomposed (:298-303): out16 = scw, Rcw(9), tcw(3), Ow(3). */
int viorb_debug_sim3_decompose(const float* Scw12, float* out16);
/* The transforms of SearchBySim3 (:1119-1121): out21 = sR12(9), sR21(9), t21(3). */
int viorb_debug_sim3_pair(const float* R12, const float* t12, float s12, float* out21);
/* One point through every gate of one function: which = 0 SearchBySim3 (T12 = the pose12 of the point's own key frame, sR9 / t3 = the
 * transform into the other camera, from viorb_debug_sim3_pair), 1 SearchByProjection or 2 Fuse (T12 = Scw; sR9, t3 unused). pt8 =
 * pts_f of the point. out4 = u v dist3D radius; out6 = level, the cell rectangle x0 x1 y0 y1, reason (VIORB_S3M_MATCHED: the point
 * reaches the window scan). */
int viorb_debug_sim3_project(int which, const float* T12, const float* sR9, const float* t3, const float* pt8, const viorb_mapping_camera* cam,
                             const float bounds4[4], float th, float* out4, int32_t* out6);
/* The ordered phase of SearchByProjection(KF, Scw) over given candidate lists: cand [npts][lcap] = distance << 16 | feature in visiting
 * order, cand_n [npts] (<= lcap), taken_in [nfeat] the entry bitmap. best_idx [npts], *nmatches; returns the number of sweeps (>= 1) or
 * an error (< 0). */
int viorb_debug_claim_in_order(const uint32_t* cand, const int32_t* cand_n, int npts, int lcap, const uint8_t* taken_in, int nfeat, int32_t* best_idx,
                               int32_t* nmatches);

#endif /* VIORB_SIM3_MATCH_H */
