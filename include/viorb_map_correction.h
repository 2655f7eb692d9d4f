/* include/viorb_map_correction.h — the map correction of loop closing: the propagation of LoopClosing::CorrectLoop (reference
 * src/LoopClosing.cc:460-542) over the current key frame's covisibles, with KeyFrame::SetPose (src/KeyFrame.cc:361-375) and
 * MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:337-378) of what it moves. Included by viorb.h; include viorb.h, not this file. The
 * ctypes mirror is viorb_amd/capi.py: SIGNATURES_MAP_CORRECTION.
 *
 * One stream is one loop closure. The call builds CorrectedSim3 / NonCorrectedSim3 from mg2oScw and the poses of the current key frame
 * and its covisibles (the members), corrects every map point the members hold, once, by the member the reference's loop reaches it
 * from first, recomputes the normal and the scale range of each corrected point as they stand at that moment of the loop, and sets the
 * members' poses with the scale divided out. Its outputs are shaped for the stages that follow: member_kf is target_kf of
 * viorb_update_connections_device (:541), Scw_f12 the Scw rows of viorb_fuse_sim3_device, Scw_out / Smeas_out and pt_corrected_ref_out
 * what viorb_optimize_essential_graph_device reads. Every float and double output has the bits the reference's statements give
 * (DESIGN.md §2 "Map correction" lists them); pointer order enters through std::map<KeyFrame*, g2o::Sim3> and std::map<KeyFrame*, size_t>
 * and is passed in as the permutation kf_by_key.
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null struct, camera or array, batch outside 1..65535,
 * a negative total, nlevels outside 1..16, a workspace that is too small or not 256-byte aligned. What lies in device memory is checked on
 * the device, per stream: see `status`. Nothing in a _device entry allocates or synchronises, and its inputs are const. There is no CPU
 * fallback: without a device the launching entries return VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_MAP_CORRECTION_H
#define VIORB_MAP_CORRECTION_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* The snapshot: flat CSR arrays of `batch` streams, with the offset and index rules of viorb_local_map_snapshot (the *_start arrays hold
 * global offsets; slots and point indices are local to their stream), whose kf_start, kf_by_key, kp_start, kp_point, pt_start, pt_bad,
 * obs_start and obs pass unchanged. Device pointers for the _device entries, host pointers for the host entries. n_kf .. n_conn are the
 * lengths of the arrays.
 *   Key frames (kf_start [batch+1]; 1 .. 65535 per stream): kf_by_key [n_kf] = the stream's slots in ascending std::less<KeyFrame*>
 *   order; pose12 [n_kf][12] = GetPose() as Rcw(9) tcw(3).
 *   Keypoints (kp_start [n_kf+1]): kp_point = the point of mvpMapPoints[i] or -1; only the members' ranges of kp_point are read.
 *   Points (pt_start [batch+1]): pt_bad = isBad(); pts_f [n_pt][8] = mWorldPos3 mNormalVector3 mfMinDistance mfMaxDistance; pt_ref = the
 *   slot of mpRefKF (read where the point is good, observed and held by a member); pt_corrected_by = mnCorrectedByKF as int32. The
 *   observations of point p (obs_start [n_pt+1]), one word each, in any order: bits 0-15 the slot of the observing key frame, bits 16-23
 *   the octave of its keypoint, higher bits ignored.
 *   Per stream [batch]: cur_kf = the slot of mpCurrentKF, cur_id = mpCurrentKF->mnId, Scw8 [batch][8] = mg2oScw as r(x y z w) t s,
 *   and (conn_start [batch+1], conn_kf) = GetVectorCovisibleKeyFrames() of the current key frame in that order: distinct slots, never
 *   the current key frame, which the routine appends itself (:462). The list may be empty. One workgroup per stream walks the members'
 *   keypoints one member after the other and ranks the members by a count over the list (quadratic in the list): meant for the few
 *   hundred covisibles a key frame has; a list of tens of thousands is accepted and correct but takes that workgroup seconds. */
typedef struct viorb_correct_loop_map {
    int32_t batch, n_kf, n_kp, n_pt, n_obs, n_conn;
    const int32_t* kf_start; const int32_t* kf_by_key; const int32_t* kp_start; const int32_t* kp_point;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* obs_start; const uint32_t* obs;
    const float* pose12; const float* pts_f; const int32_t* pt_ref; const int32_t* pt_corrected_by;
    const int32_t* cur_kf; const int32_t* cur_id; const double* Scw8; const int32_t* conn_start; const int32_t* conn_kf;
} viorb_correct_loop_map;

/* The result; every array is required and has a fixed size, so there is no capacity status.
 *   status [batch]: VIORB_OK, or VIORB_ERR_INVALID_ARG for a stream the validating kernel refused: an offset (of this or an earlier
 *   stream) that is negative, descending or beyond its total; a slot or point index outside its stream; kf_by_key that is not a
 *   permutation; cur_kf or a conn_kf out of range, conn_kf naming a slot twice or the current key frame; a pose or Scw8 that is not
 *   finite, a scale <= 0; a good, observed point in a member whose pt_ref is out of range or not among its observers; more than 65535 key
 *   frames. Nothing is read through a refused index, a refused stream writes nothing but its status, and the other streams are not
 *   affected.
 *   Members, stream b's at rows conn_start[b] + b .. conn_start[b + 1] + b of arrays of n_conn + batch rows: n_member [batch] (the list and
 *   the current key frame); member_kf = the members in ascending key, the iteration order of CorrectedSim3 and so the call order of
 *   UpdateConnections (:541) and of SearchAndFuse; Scw_f12 [..][12] = Converter::toCvMat(CorrectedSim3[member]) as float, the top three
 *   rows of [s * R | t]: a similarity as viorb_sim3_match.h reads it.
 *   Key frames [n_kf]: Scw_out / Smeas_out [..][8] = the CorrectedSim3 / NonCorrectedSim3 entry of a member, (Quaterniond(Rcw), tcw, 1) in
 *   both for any other key frame; pose12_out [..][12] = the pose SetPose receives (:536, R | t / s as float), Ow_out [..][3] = the camera
 *   centre SetPose derives from it; the input pose and its centre for a key frame that is not a member.
 *   Points [n_pt]: pts_f_out [..][8] (a point nobody corrects is copied; a corrected point without observations keeps its normal and
 *   range), pt_corrected_by_out = mnCorrectedByKF, pt_corrected_ref_out = the slot of mnCorrectedReference where this call set it, else
 *   -1, pt_touched (u8) = 1 where the point was corrected: the members a caller has to write back. */
typedef struct viorb_correct_loop_result {
    int32_t* status; int32_t* n_member; int32_t* member_kf; float* Scw_f12; double* Scw_out; double* Smeas_out; float* pose12_out; float* Ow_out;
    float* pts_f_out; int32_t* pt_corrected_by_out; int32_t* pt_corrected_ref_out; uint8_t* pt_touched;
} viorb_correct_loop_result;

/* Device scratch of viorb_correct_loop_device (256-byte aligned device memory; its contents on entry are ignored) for a snapshot of
 * these totals. 0 for sizes outside the limits. */
size_t viorb_correct_loop_workspace_bytes(int batch, int n_kf, int n_pt, int n_obs);

/* The propagation for every stream. cam (a host pointer): nlevels and scale_factors are read, as viorb_map_points_update reads them. It
 * enqueues two kernels on `stream` and returns. The caller runs viorb_update_connections_device over member_kf afterwards. */
int viorb_correct_loop_device(const viorb_correct_loop_map* map, const viorb_mapping_camera* cam, const viorb_correct_loop_result* result,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The same from host buffers (re-entrant; allocates, runs, synchronises, copies back). */
int viorb_correct_loop(const viorb_correct_loop_map* map, const viorb_mapping_camera* cam, const viorb_correct_loop_result* result);

/* Shapes of the built kernels, for tests that probe their edges: out4 = threads of the key-frame phase (the stride of its loops over
 * key frames, list entries and a member's keypoints), threads of the point phase, the wavefront size (points per pass of a wavefront and
 * the stride of the loop over a point's observers), the largest key-frame count of a stream whose key positions live in LDS during the
 * point phase (above it: in the workspace). */
int viorb_correct_loop_shape(int32_t* out4);

/* Test hook (no device): map_correct_core.h compiled for the host, the same phases on one thread over host buffers. */
int viorb_debug_correct_loop_host(const viorb_correct_loop_map* map, const viorb_mapping_camera* cam, const viorb_correct_loop_result* result);

/* ---- The map update after a global bundle adjustment: reference src/LoopClosing.cc:712-803 (LoopClosing::RunGlobalBundleAdjustment) and,
 * line for line, src/LocalMapping.cc:824-916 (LocalMapping::TryInitVIO). viorb_global_ba_navstate / viorb_global_ba_se3 with
 * nLoopKF != 0 end in mTcwGBA / mNavStateGBA / mPosGBA; this applies them. One stream is one map.
 *   The walk (:713-766) starts at mvpKeyFrameOrigins and follows GetChilds(). A child outside the adjustment (kf_in_gba == 0) gets
 *   mTcwGBA = (Tcw_child * Twc_parent) * mTcwGBA_parent in float, the flag, and mNavStateGBA = its NavState with P, R, V replaced from
 *   toCvMatInverse(Tbc * mTcwGBA) (R through Sophus::SO3(Matrix3d), V2 = Rwb * Rw1^T * V1 in double). Every reached key frame then takes
 *   mTcwBefGBA = its pose, mNavStateBefGBA = its NavState, its NavState = mNavStateGBA and the pose of UpdatePoseFromNS(Tbc). The result
 *   does not depend on the order of the walk. A root that is not in the adjustment uses the TcwGBA12 / nsGBA22 it was given, as the
 *   reference does. Every good point (:771-802) moves to mPosGBA, or through its reference key frame's old and new pose when that key
 *   frame carries the flag after the walk, or stays.
 * Inputs, with the offset rules above: kf_start [batch+1]; the children of key frame k (child_start [n_kf+1]) in child_kf, as
 * viorb_local_map_snapshot has them; origin_start [batch+1], origin_kf = mvpKeyFrameOrigins; per key frame kf_in_gba (u8:
 * mnBAGlobalForKF == nLoopKF), pose12, TcwGBA12 (float), ns22, nsGBA22 (the 22-double NavState of viorb.h; the stored quaternion is
 * used as it is); per point (pt_start [batch+1]) pt_bad, pt_in_gba (u8), Pw [n_pt][3], PosGBA [n_pt][3], pt_ref = the slot of
 * mpRefKF (read where the point is good and not in the adjustment); per call Tbc12 = the top rows of ConfigParam::GetMatTbc() as
 * Rbc(9) tbc(3), a host pointer. */
typedef struct viorb_apply_gba_map {
    int32_t batch, n_kf, n_child, n_origin, n_pt;
    const int32_t* kf_start; const int32_t* child_start; const int32_t* child_kf; const int32_t* origin_start; const int32_t* origin_kf;
    const uint8_t* kf_in_gba; const float* pose12; const float* TcwGBA12; const double* ns22; const double* nsGBA22;
    const int32_t* pt_start; const uint8_t* pt_bad; const uint8_t* pt_in_gba; const float* Pw; const float* PosGBA; const int32_t* pt_ref;
} viorb_apply_gba_map;

#define VIORB_AGBA_PT_BAD            0   /* isBad(): skipped, the position is copied */
#define VIORB_AGBA_PT_POS_GBA        1   /* the position became mPosGBA (:781) */
#define VIORB_AGBA_PT_BY_REF         2   /* moved through the reference key frame (:792-801) */
#define VIORB_AGBA_PT_UNTOUCHED      3   /* the reference key frame does not carry the flag (:788) */
#define VIORB_AGBA_PT_REF_UNREACHED  4   /* the reference key frame carries the flag but the walk did not reach it: left untouched. The one
                                            departure: the reference reads an mTcwBefGBA that was never set */

/* The result; every array is required. Key frames [n_kf]: pose12_out, ns22_out (the input for a key frame the walk did not reach),
 * TcwBef_out / nsBef_out (the input pose and NavState: mTcwBefGBA / mNavStateBefGBA where reached), TcwGBA_out / nsGBA_out (the input
 * where the walk did not derive them), kf_in_gba_out (u8), kf_reached (u8). Points [n_pt]: Pw_out [..][3], pt_code (u8,
 * VIORB_AGBA_PT_*). status [batch]: VIORB_OK or VIORB_ERR_INVALID_ARG for a stream the validating kernel refused: the offset and index
 * rules of the snapshots; a slot that is a child twice, an origin that is a child or is listed twice, a cycle in the child lists; a pose
 * or NavState that is not finite (the GBA ones of a key frame in the adjustment), a point that is not finite, a pt_ref out of range
 * where it is read; more than 65535 key frames. A refused stream writes nothing but its status. */
typedef struct viorb_apply_gba_result {
    int32_t* status; float* pose12_out; double* ns22_out; float* TcwBef_out; double* nsBef_out; float* TcwGBA_out; double* nsGBA_out;
    uint8_t* kf_in_gba_out; uint8_t* kf_reached; float* Pw_out; uint8_t* pt_code;
} viorb_apply_gba_result;

/* Device scratch (256-byte aligned; its contents on entry are ignored). 0 for sizes outside the limits. */
size_t viorb_apply_global_ba_workspace_bytes(int batch, int n_kf);
/* Enqueues two kernels on `stream` and returns. A key frame walks up to its nearest ancestor inside the adjustment and back down:
 * quadratic in the length of a run of key frames outside it, which is a few key frames in the reference's maps. */
int viorb_apply_global_ba_device(const viorb_apply_gba_map* map, const float* Tbc12, const viorb_apply_gba_result* result,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* The same from host buffers (re-entrant; allocates, runs, synchronises, copies back). */
int viorb_apply_global_ba(const viorb_apply_gba_map* map, const float* Tbc12, const viorb_apply_gba_result* result);
/* out4 = threads of the key-frame phase, threads of the point phase, the wavefront size, the most workgroups of a stream's points. */
int viorb_apply_global_ba_shape(int32_t* out4);
/* Test hook (no device): the same phases on one thread over host buffers. */
int viorb_debug_apply_global_ba_host(const viorb_apply_gba_map* map, const float* Tbc12, const viorb_apply_gba_result* result);

#endif /* VIORB_MAP_CORRECTION_H */
