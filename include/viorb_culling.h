/* include/viorb_culling.h — the two culling routines of LocalMapping::Run: reference src/LocalMapping.cc:1665-1824
 * (LocalMapping::KeyFrameCulling, with what KeyFrame::SetBadFlag, src/KeyFrame.cc:744-882, and MapPoint::EraseObservation /
 * SetBadFlag, src/MapPoint.cc:118-175, change between two candidates) and :1198-1233 (LocalMapping::MapPointCulling). Included by
 * viorb.h; include viorb.h, not this file. The ctypes mirror is viorb_amd/capi.py: SIGNATURES_CULLING.
 *
 * Key-frame culling works on a snapshot of the map around mpCurrentKeyFrame, for `batch` independent streams, and returns which
 * candidates the reference's ordered loop culls and the state that loop leaves; the caller then runs the reference's own
 * KeyFrame::SetBadFlag on them (spanning tree, connections, database). Every output equals the reference's loop exactly: the
 * decisions are integer, with three double compares and one float compare.
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null struct or array (kp_depth may be NULL when
 * monocular), batch outside 1..65535, a negative total, cap < 1, a workspace that is too small or not 256-byte aligned. What lies in
 * device memory is checked on the device, per stream: see `status`. Nothing in a _device entry allocates or synchronises, and its
 * inputs are const. There is no CPU fallback: without a device the launching entries return VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_CULLING_H
#define VIORB_CULLING_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* cand_reason[j]: how candidate j leaves the loop */
#define VIORB_KFC_FIRST_KF        0   /* mnId == 0 (:1697) */
#define VIORB_KFC_TIME_GAP        1   /* prev and next exist, !GetVINSInited(), fabs(t[next] - t[prev]) > 0.5 (:1709-1713) */
#define VIORB_KFC_BEFORE_CURRENT  2   /* GetNextKeyFrame() == mpCurrentKeyFrame (:1746) */
#define VIORB_KFC_RECENT          3   /* mTimeStamp >= mpCurrentKeyFrame->mTimeStamp - 0.2 (:1749) */
#define VIORB_KFC_KEPT            4   /* counted; !(nRedundantObservations > 0.9 * nMPs) */
#define VIORB_KFC_CULLED          5   /* SetBadFlag() went through */
#define VIORB_KFC_DEFERRED        6   /* SetBadFlag() with mbNotErase: mbToBeErased, nothing else changes (KeyFrame.cc:765-769) */

/* code[i] of map-point culling: the branches of :1214-1231 in their order */
#define VIORB_MPC_KEEP              0   /* lit++ */
#define VIORB_MPC_DROP_BAD          1   /* isBad(): leaves the list */
#define VIORB_MPC_CULL_FOUND_RATIO  2   /* GetFoundRatio() < 0.25f: SetBadFlag(), leaves the list */
#define VIORB_MPC_CULL_FEW_OBS      3   /* two key frames old with Observations() <= cnThObs: SetBadFlag(), leaves the list */
#define VIORB_MPC_RETIRE            4   /* three key frames old: leaves the list */

#define VIORB_CULL_KF_FIRST      1   /* kf_flags bit 0: mnId == 0 */
#define VIORB_CULL_KF_NOT_ERASE  2   /* kf_flags bit 1: mbNotErase */

/* The snapshot: flat CSR arrays of `batch` streams. The *_start arrays hold global offsets; slots and point indices are local to their
 * stream. Device pointers for the _device entry, host pointers for the host entry. n_kf .. n_obs are the lengths of the arrays.
 *   Key frames (kf_start [batch+1]; at most 65535 per stream): kf_flags VIORB_CULL_KF_*, kf_time = mTimeStamp, kf_prev / kf_next = the
 *   slot of GetPrevKeyFrame() / GetNextKeyFrame() or -1. The prev and next of every candidate must be slots of the snapshot.
 *   Per stream: cur_kf = the slot of mpCurrentKeyFrame, vins_inited = GetVINSInited(), th_depth = mThDepth.
 *   Candidates (cand_start [batch+1]): cand_kf = the slots of GetVectorCovisibleKeyFrames() in that order, none twice. Keypoints of
 *   candidate j (kp_start [n_cand+1]): kp_point = the point of mvpMapPoints[i] or -1, kp_octave = mvKeysUn[i].octave, kp_depth =
 *   mvDepth[i] (not read when monocular).
 *   Points (pt_start [batch+1]): pt_nobs = Observations() as given (|pt_nobs| < 2^30), pt_bad = isBad(). Observations of point p
 *   (obs_start [n_pt+1]), one word each: bits 0-15 the slot of the observing key frame, bits 16-23 the octave of its keypoint, bit 24
 *   set when its mvuRight >= 0. A point's observations name distinct key frames. */
typedef struct viorb_cull_map {
    int32_t batch, n_kf, n_cand, n_kp, n_pt, n_obs;
    const int32_t* kf_start; const uint8_t* kf_flags; const double* kf_time; const int32_t* kf_prev; const int32_t* kf_next;
    const int32_t* cur_kf; const uint8_t* vins_inited; const float* th_depth;
    const int32_t* cand_start; const int32_t* cand_kf; const int32_t* kp_start; const int32_t* kp_point; const uint8_t* kp_octave; const float* kp_depth;
    const int32_t* pt_start; const int32_t* pt_nobs; const uint8_t* pt_bad; const int32_t* obs_start; const uint32_t* obs;
} viorb_cull_map;

/* The result; every array is optional (NULL: not written) and laid out as the snapshot's.
 *   Per candidate [n_cand]: cand_reason VIORB_KFC_*; cand_redundant / cand_mps = nRedundantObservations / nMPs (zero when a skip test
 *   fired); cand_recounted = 1 when the ordered phase counted the candidate itself, which it does for every candidate that no skip test
 *   removed (0 for a skipped one). culled_order: the first n_culled[b] entries of the stream's range are the ordinals (within the stream) of the
 *   culled candidates in cull order, the rest -1.
 *   Per stream [batch]: n_culled; status = VIORB_OK, or VIORB_ERR_INVALID_ARG for a stream that the validating kernel refused: an offset
 *   (of this or an earlier stream) that is negative, descending or beyond its total, a slot or point index outside its stream, cur_kf or
 *   a candidate's prev / next out of range, a candidate listed twice, more than 65535 key frames or none, |pt_nobs| >= 2^30. Nothing is
 *   read through a refused index; a refused stream has n_culled 0 and none of its other outputs is written.
 *   Per key frame [n_kf]: kf_bad (culled), kf_to_be_erased (mbToBeErased), kf_prev_out / kf_next_out (the links the loop leaves),
 *   kf_repreint = 1 for a key frame that was the `next` of a culled one whose prev also existed: it needs AppendIMUDataToFront of the
 *   culled key frame, in culled_order, and ComputePreInt (viorb_preintegrate_intervals).
 *   pt_nobs_out / pt_bad_out [n_pt]: nObs and isBad() afterwards; obs_alive [n_obs]: 1 while the observation is still in mObservations. */
typedef struct viorb_cull_result {
    int32_t* cand_reason; int32_t* cand_redundant; int32_t* cand_mps; int32_t* cand_recounted; int32_t* culled_order;
    int32_t* n_culled; int32_t* status;
    uint8_t* kf_bad; uint8_t* kf_to_be_erased; int32_t* kf_prev_out; int32_t* kf_next_out; uint8_t* kf_repreint;
    int32_t* pt_nobs_out; uint8_t* pt_bad_out; uint8_t* obs_alive;
} viorb_cull_result;

/* Device scratch of viorb_key_frame_culling_device (256-byte aligned device memory; its contents on entry are ignored) for a snapshot of
 * these totals. 0 for sizes outside the limits. */
size_t viorb_key_frame_culling_workspace_bytes(int batch, int n_kf, int n_cand, int n_pt, int n_obs);

/* LocalMapping::KeyFrameCulling (:1694-1821) for every stream of the snapshot; monocular = mbMonocular. It enqueues two kernels on
 * `stream` and returns. */
int viorb_key_frame_culling_device(const viorb_cull_map* map, int monocular, const viorb_cull_result* result, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* The same from host buffers (re-entrant; allocates, runs, synchronises, copies back). */
int viorb_key_frame_culling(const viorb_cull_map* map, int monocular, const viorb_cull_result* result);

/* Shapes of the built kernels, for tests that probe their edges: out4 = threads of the ordered phase, keypoints per workgroup and pass of
 * the count (one lane per keypoint; the count runs inside the ordered phase, so this equals the first), the wavefront size, the
 * observation chunk lanes share (0: a lane walks its point's list alone). */
int viorb_key_frame_culling_shape(int32_t* out4);

/* LocalMapping::MapPointCulling (:1198-1233) over mlpRecentAddedMapPoints as arrays [batch][cap] with count [batch] entries each: bad =
 * isBad(), found / visible = mnFound / mnVisible (0 .. 2^24 - 1), first_kf_id = mnFirstKFid, nobs = Observations(); cur_kf_id [batch] =
 * mpCurrentKeyFrame->mnId. code [batch][cap]: VIORB_MPC_*, -1 from the count on. The caller applies SetBadFlag and the list erase. */
int viorb_map_point_culling_device(const uint8_t* bad, const int32_t* found, const int32_t* visible, const int32_t* first_kf_id, const int32_t* nobs,
                                   const int32_t* count, const int32_t* cur_kf_id, int cap, int batch, int monocular, int32_t* code, void* stream);
/* One list of n points from host buffers. */
int viorb_map_point_culling(const uint8_t* bad, const int32_t* found, const int32_t* visible, const int32_t* first_kf_id, const int32_t* nobs, int n,
                            int cur_kf_id, int monocular, int32_t* code);

/* Test hooks (no device). viorb_debug_key_frame_culling_host: culling_core.h compiled for the host, the same phases on one thread over
 * host buffers. viorb_debug_map_point_code: one point of map-point culling. */
int viorb_debug_key_frame_culling_host(const viorb_cull_map* map, int monocular, const viorb_cull_result* result);
int viorb_debug_map_point_code(int bad, int found, int visible, int first_kf_id, int nobs, int cur_kf_id, int monocular);

#endif /* VIORB_CULLING_H */
