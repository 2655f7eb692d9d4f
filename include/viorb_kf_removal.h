/* include/viorb_kf_removal.h — a key frame leaves the map: KeyFrame::SetBadFlag and KeyFrame::SetErase (reference src/KeyFrame.cc:728-882)
 * with EraseConnection (:890-904), UpdateBestCovisibles (:429-448), GetWeight (:492-500), ChangeParent (:684-689) and
 * MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:118-175), for an ordered list of operations per stream. Included by viorb.h;
 * include viorb.h, not this file. The ctypes mirror is viorb_amd/capi.py: SIGNATURES_KF_REMOVAL.
 *
 * The call works on a snapshot of the map, for `batch` independent streams: the operations of a stream run one after the other, in call
 * order, each reading what the earlier ones left, and the state they leave comes back per key frame, per point and per operation. It
 * takes what viorb_key_frame_culling decided (culled_order, the deferred candidates) and leaves what viorb_update_connections,
 * viorb_update_local_map (covis10 = the first ten of ord_kf_out, kf_parent), viorb_apply_global_ba and the essential graph (kf_parent)
 * and viorb_correct_loop (pt_ref) read. Every discrete output equals the reference's statements exactly; mTcp matches bit for bit.
 * Pointer order enters through std::map<KeyFrame*, ...>, std::set<KeyFrame*> and the sort of pair<int, KeyFrame*>, and is passed in as the
 * permutation kf_by_key; a key frame's key is its position in it.
 *
 * Two rules.
 *   Children are not an input. mspChildrens of a good key frame X is the set of good (not bad) key frames whose kf_parent is X, iterated
 *   in key order: the invariant the reference keeps (AddChild / EraseChild / ChangeParent), and the convention of viorb_covis_result.
 *   Precondition: a key frame holds a map point at most once (kp_point names a point once per key frame), and a point's observations
 *   name a key frame once. The snapshot carries no keypoint index per observation: EraseMapPointMatch finds the entry by the point.
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null struct or array (the optional result arrays
 * excepted), batch outside 1..65535, a negative total, ccap < 1, a workspace that is too small or not 256-byte aligned. What lies in
 * device memory is checked on the device, per stream: see `status`. Nothing in a _device entry allocates or synchronises, and its inputs
 * are const. There is no CPU fallback: without a device the launching entries return VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_KF_REMOVAL_H
#define VIORB_KF_REMOVAL_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

#define VIORB_KFR_KF_ID0            1   /* kf_flags bit 0: mnId == 0 */
#define VIORB_KFR_KF_BAD            2   /* kf_flags bit 1: mbBad */
#define VIORB_KFR_KF_NOT_ERASE      4   /* kf_flags bit 2: mbNotErase */
#define VIORB_KFR_KF_TO_BE_ERASED   8   /* kf_flags bit 3: mbToBeErased */
#define VIORB_KFR_KF_LOOP_EDGES    16   /* kf_flags bit 4: !mspLoopEdges.empty() */

#define VIORB_KFR_SET_BAD_FLAG      0   /* op_kind: KeyFrame::SetBadFlag() */
#define VIORB_KFR_SET_ERASE         1   /* op_kind: KeyFrame::SetErase() */

#define VIORB_KFR_REMOVED           0   /* op_reason: the key frame went bad in this operation */
#define VIORB_KFR_ALREADY_BAD       1   /* :747-759; the caller erases it from the map and the database again, as the reference does */
#define VIORB_KFR_FIRST_KF          2   /* :763 */
#define VIORB_KFR_DEFERRED          3   /* :765-769: mbNotErase, mbToBeErased is set */
#define VIORB_KFR_RELEASED          4   /* a SetErase whose key frame had no mbToBeErased: SetBadFlag did not run */

#define VIORB_KFR_MAP_CHANGED       1   /* kf_touched bit 0, as VIORB_COVIS_MAP_CHANGED */
#define VIORB_KFR_ORD_REBUILT       2   /* kf_touched bit 1, as VIORB_COVIS_ORD_REBUILT */
#define VIORB_KFR_PARENT_CHANGED    4   /* kf_touched bit 2: ChangeParent ran on the key frame */

/* The snapshot: flat CSR arrays of `batch` streams with the offset and index rules of viorb_covis_map, whose kf_start, kf_by_key,
 * kf_parent, kp_start, kp_point, pt_start, pt_bad, obs_start, obs, conn_* and ord_* pass unchanged. Device pointers for the _device
 * entry, host pointers for the host entries. n_kf .. n_op are the lengths of the arrays.
 *   Key frames: kf_flags = VIORB_KFR_KF_*; kf_prev / kf_next = the slots of mpPrevKeyFrame / mpNextKeyFrame or -1; kf_pose12 [n_kf][12] =
 *   Tcw, Rcw row-major then tcw (as viorb_correct_loop_map's). Only the poses of the operations' key frames and of their parents are read.
 *   Keypoints: the ranges of kp_point of the operations' key frames are read as point indices; the others are only compared.
 *   Points: pt_nobs = nObs (|nObs| < 2^29); pt_ref = the slot of mpRefKF or -1; in an observation word bits 0-15 are the slot and bit 24
 *   is mvuRight >= 0 (the words of viorb_cull_map).
 *   Operations (op_start [batch+1], op_kf, op_kind u8 = VIORB_KFR_SET_*): in call order. A slot may be listed more than once; a stream
 *   may have none. */
typedef struct viorb_kfr_map {
    int32_t batch, n_kf, n_kp, n_pt, n_obs, n_conn, n_ord, n_op;
    const int32_t* kf_start; const int32_t* kf_by_key; const uint8_t* kf_flags; const int32_t* kf_parent; const int32_t* kf_prev; const int32_t* kf_next; const float* kf_pose12;
    const int32_t* kp_start; const int32_t* kp_point;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* pt_nobs; const int32_t* pt_ref; const int32_t* obs_start; const uint32_t* obs;
    const int32_t* conn_start; const int32_t* conn_kf; const int32_t* conn_w;
    const int32_t* ord_start; const int32_t* ord_kf; const int32_t* ord_w;
    const int32_t* op_start; const int32_t* op_kf; const uint8_t* op_kind;
} viorb_kfr_map;

/* The result. The first seven arrays are required: the rows are the working state, in the [n_kf][ccap] layout of viorb_covis_result
 * (conn in ascending key order, -1 from the count on), so that they can be fed straight back into viorb_update_connections_device.
 * Rows only shrink: there is no overflow status, and an input row longer than ccap is refused.
 *   What an operation does, in order (each reads what the earlier ones left):
 *   1. SetErase: without loop edges mbNotErase is cleared; SetBadFlag runs only if mbToBeErased is set (else VIORB_KFR_RELEASED).
 *      mbToBeErased is never cleared, as in the reference.
 *   2. The guards in the reference's order: already bad, mnId == 0, mbNotErase (which sets mbToBeErased).
 *   3. EraseConnection: for every key frame in X's own map, in key order: if its map holds X, the entry is erased and its ordered list
 *      is rebuilt from its whole map (descending weight, ties by descending key). A key frame that names X but is absent from X's own map
 *      is not visited: its stale entry stays.
 *   4. EraseObservation for every non-null mvpMapPoints[i] of X: if the point lists X, nObs drops by 1 (by 2 where bit 24 of the word is
 *      set) and the observation goes; an mpRefKF that was X becomes the remaining observer with the lowest key; nObs <= 2 makes the point
 *      bad: mObservations is cleared, nObs stays, and the point's entries at the remaining observers are nulled. isBad() of the point is
 *      not asked, as in the reference.
 *   5. X's own map and ordered list are cleared.
 *   6. The spanning tree, :786-841 literally: the candidates start as {parent of X}; each round searches the children in key order and
 *      the positions of a child's ordered list in order; a hit's weight is GetWeight from the child's map, 0 where the map does not hold
 *      the key frame the list names; the strict w > max keeps the first maximum; the winner takes that parent, joins the candidates and
 *      leaves the children; when a round finds nothing the rest take X's parent.
 *   7. mTcp = Tcw * Twc(parent), Twc as KeyFrame::SetPose builds it, four float products per entry summed left to right. X is bad.
 *   8. The links, :849-875: prev and next are joined, X's own are cleared, kf_repreint is set on next when both existed.
 *   status [batch]: VIORB_OK, or VIORB_ERR_INVALID_ARG for a stream the validating kernel refused: everything viorb_update_connections
 *   refuses (with the operations as its targets); kf_prev, kf_next or pt_ref outside -1 .. the stream's key frames - 1; |pt_nobs| >= 2^29;
 *   an op_kind above 1; an operation's key frame that is neither the first (mnId == 0) nor bad and has no parent (the reference
 *   dereferences mpParent); a chain of kf_parent that leads from an operation's key frame back to it; a non-finite kf_pose12 of an
 *   operation's key frame or of its parent. Nothing is read through a refused index, a refused stream writes nothing but its status,
 *   and the other streams are not affected.
 *   Optional (NULL: not written).
 *   Per key frame [n_kf]: kf_parent_out; kf_flags_out (u8, VIORB_KFR_KF_*); kf_prev_out / kf_next_out; kf_repreint (u8), with the meaning
 *   it has in viorb_cull_result: AppendIMUDataToFront of the removed key frames in operation order, then viorb_preintegrate_intervals;
 *   kf_Tcp_out [n_kf][12] (the layout of kf_pose12), written only for the key frames removed in this call; kf_touched (u8, VIORB_KFR_*).
 *   Per point [n_pt]: pt_nobs_out, pt_bad_out (u8), pt_ref_out: -1 where the erase emptied mObservations (the reference dereferences
 *   begin() == end() there, and the point goes bad in the same call). obs_alive [n_obs] (u8): the observation is still in mObservations.
 *   kp_point_out [n_kp] follows EraseMapPointMatch: the entry of key frame k for point p becomes -1 exactly when p went bad in this call
 *   while k's observation of it was still in mObservations. A removed key frame keeps its own entries, as in the reference.
 *   Per operation [n_op]: op_reason (VIORB_KFR_*) and, 0 unless VIORB_KFR_REMOVED: op_children = the children re-parented, op_fallback = how
 *   many of them went to the original parent by :837-841, op_rebuilt = the neighbours whose list was rebuilt, op_points_bad = the calls of
 *   MapPoint::SetBadFlag. */
typedef struct viorb_kfr_result {
    int32_t* conn_kf_out; int32_t* conn_w_out; int32_t* conn_n_out; int32_t* ord_kf_out; int32_t* ord_w_out; int32_t* ord_n_out; int32_t* status;
    int32_t* kf_parent_out; uint8_t* kf_flags_out; int32_t* kf_prev_out; int32_t* kf_next_out; uint8_t* kf_repreint; float* kf_Tcp_out; uint8_t* kf_touched;
    int32_t* pt_nobs_out; uint8_t* pt_bad_out; uint8_t* obs_alive; int32_t* pt_ref_out; int32_t* kp_point_out;
    int32_t* op_reason; int32_t* op_children; int32_t* op_fallback; int32_t* op_rebuilt; int32_t* op_points_bad;
} viorb_kfr_result;

/* Device scratch of viorb_remove_key_frames_device (256-byte aligned device memory; its contents on entry are ignored) for a snapshot
 * of these totals. 0 for sizes outside the limits. */
size_t viorb_remove_key_frames_workspace_bytes(int batch, int n_kf, int n_pt, int n_op);

/* The operations of every stream, those of a stream in call order. ccap: the row length of the result's rows. It enqueues two kernels
 * on `stream` and returns. */
int viorb_remove_key_frames_device(const viorb_kfr_map* map, const viorb_kfr_result* result, int ccap, void* workspace, size_t workspace_bytes, void* stream);
/* The same from host buffers (re-entrant; allocates, runs, synchronises, copies back). */
int viorb_remove_key_frames(const viorb_kfr_map* map, const viorb_kfr_result* result, int ccap);

/* Shapes of the built kernels, for tests that probe their edges: out4 = threads of the ordered phase (the stride of its loops over
 * keypoints and key frames), the wavefront size (the stride of the loops over a row), the largest key-frame count of a stream whose
 * candidate marks live in LDS (above it: in the workspace), the number of wavefronts that share the neighbours and the children. */
int viorb_remove_key_frames_shape(int32_t* out4);

/* Test hook (no device): kf_removal_core.h compiled for the host, the same phases on one thread over host buffers. */
int viorb_debug_remove_key_frames_host(const viorb_kfr_map* map, const viorb_kfr_result* result, int ccap);

#endif /* VIORB_KF_REMOVAL_H */
