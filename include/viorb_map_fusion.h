/* include/viorb_map_fusion.h — the results of the fuse searches applied to the map: the replace / add block of ORBmatcher::Fuse(KeyFrame*,
 * vpMapPoints) (reference src/ORBmatcher.cc:842-972 without the search, :951-971), that of ORBmatcher::Fuse(KeyFrame*, Scw, vpPoints, th,
 * vpReplacePoint) (:1000-1097, :1081-1096) with the Replace loop of LoopClosing::SearchAndFuse (src/LoopClosing.cc:632-640), and
 * MapPoint::Replace / AddObservation (src/MapPoint.cc:184-222, :105-116) with KeyFrame::AddMapPoint, ReplaceMapPointMatch and
 * EraseMapPointMatch. Included by viorb.h; include viorb.h, not this file. The ctypes mirror is viorb_amd/capi.py: SIGNATURES_MAP_FUSION.
 *
 * The call works on a snapshot of the map, for `batch` independent streams. A stream is an ordered list of calls, each one invocation
 * of ORBmatcher::Fuse whose search has already run (viorb_frontend_fuse_device, viorb_fuse_sim3_device: best_idx per listed point);
 * the calls of a stream run one after the other and each reads what the earlier ones left. It stands between those searches and
 * viorb_map_points_update_device / viorb_update_connections_device in both chains. Every output equals the
 * reference's statements exactly; everything is integer arithmetic. Pointer order enters through std::map<KeyFrame*, size_t> and is
 * passed in as the permutation kf_by_key; a key frame's key is its position in it.
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null struct or array (the optional result arrays
 * excepted), batch outside 1..65535, a negative total, a workspace that is too small or not 256-byte aligned. What lies in device
 * memory is checked on the device, per stream: see `status`. Nothing in a _device entry allocates or synchronises, and its inputs are
 * const. There is no CPU fallback: without a device the launching entries return VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_MAP_FUSION_H
#define VIORB_MAP_FUSION_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

#define VIORB_FUSE_POSE               0   /* call_kind: Fuse(pKF, vpMapPoints), the replace / add block runs inside the loop */
#define VIORB_FUSE_SIM3               1   /* call_kind: Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) + the Replace loop of SearchAndFuse */

#define VIORB_FUSE_OVERFLOW           1   /* status: the stream's region of the output observation arrays is too short; see need */

#define VIORB_FUSE_ADDED              0   /* op_reason: AddObservation + AddMapPoint */
#define VIORB_FUSE_REPLACED_KF_POINT  1   /* the key frame's point q was replaced by the candidate: q->Replace(p) (SIM3: after the loop) */
#define VIORB_FUSE_REPLACED_CANDIDATE 2   /* POSE, Observations(q) > Observations(p): p->Replace(q) */
#define VIORB_FUSE_COUNTED_ONLY       3   /* the key frame's point is bad: nFused++ and nothing else */
#define VIORB_FUSE_SKIP_BAD           4   /* pMP->isBad() */
#define VIORB_FUSE_SKIP_IN_KF         5   /* POSE: pMP->IsInKeyFrame(pKF); SIM3: spAlreadyFound.count(pMP) */
#define VIORB_FUSE_NONE               6   /* the search found no feature (op_feat < 0) */
#define VIORB_FUSE_NULL_POINT         7   /* list_point == -1 */

/* The snapshot: flat arrays of `batch` streams with the offset and index rules of viorb_covis_map (kf_start, pt_start, call_start and
 * obs_out_start [batch + 1] cut arrays into streams and hold global offsets, as the nested kp_start, obs_start and call_op do; slots,
 * point indices and feature indices are stream-local). Device pointers for the _device entry, host pointers for the host entries.
 * n_kf .. n_obs_out are the lengths of the arrays.
 *   Key frames: kf_by_key as in viorb_covis_map; kf_bad (u8) = isBad(), used only to leave observers out of the dirty lists.
 *   Keypoints: kp_point = mvpMapPoints (-1 = NULL); kp_octave (u8) = mvKeysUn[i].octave; kp_stereo (u8) = mvuRight[i] >= 0.
 *   Points: pt_bad (u8), pt_nobs = nObs, pt_found / pt_visible = mnFound / mnVisible.
 *   Observations: obs_start / obs are the words of viorb_cull_map (only the slot is read); obs_feat [n_obs] = mObservations[pKF], the
 *   feature index. With it there is no "a key frame holds a point once" precondition: ReplaceMapPointMatch(idx) and
 *   EraseMapPointMatch(idx) act on the recorded index, whatever kp_point holds there.
 *   Calls (call_start [batch + 1]): call_kf = the slot of pKF, call_kind (u8) = VIORB_FUSE_*, call_list = the offset of the call's point
 *   list in list_point, call_n = its length, call_feat = the offset of the call's best_idx row in op_feat; call_op [n_call + 1] = the
 *   running sum of call_n over all calls of the batch (call_op[c + 1] - call_op[c] == call_n[c]): the offset of the call's entries in
 *   the per-entry outputs. It is an input because a stream cannot form it without reading through the other streams' call_n.
 *   list_point [n_list]: a point, or -1 for a NULL pointer; a point may appear more than once. op_feat [n_feat]: a feature of the
 *   call's key frame, or -1. Lists and rows may be shared between calls: LoopClosing::SearchAndFuse is K calls with call_list = 0 and
 *   call_feat = c * pcap, so best_idx [K][pcap] of viorb_fuse_sim3_device is passed as it is.
 *   obs_out_start [batch + 1]: the stream's region of obs_out / obs_feat_out. */
typedef struct viorb_fuse_map {
    int32_t batch, n_kf, n_kp, n_pt, n_obs, n_call, n_list, n_feat, n_op, n_obs_out;
    const int32_t* kf_start; const int32_t* kf_by_key; const uint8_t* kf_bad;
    const int32_t* kp_start; const int32_t* kp_point; const uint8_t* kp_octave; const uint8_t* kp_stereo;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* pt_nobs; const int32_t* pt_found; const int32_t* pt_visible;
    const int32_t* obs_start; const uint32_t* obs; const int32_t* obs_feat;
    const int32_t* call_start; const int32_t* call_kf; const uint8_t* call_kind; const int32_t* call_list; const int32_t* call_n; const int32_t* call_feat;
    const int32_t* call_op;
    const int32_t* list_point; const int32_t* op_feat; const int32_t* obs_out_start;
} viorb_fuse_map;

/* The result. What a call does, entry i of its list in order, with p = list_point[call_list + i] and f = op_feat[call_feat + i]; every
 * guard reads the state as the earlier entries and calls left it:
 *   VIORB_FUSE_POSE. p == -1: NULL_POINT. p bad: SKIP_BAD. p's observations name the call's key frame: SKIP_IN_KF. f < 0: NONE. Otherwise
 *   q = kp_point[kf][f] as it stands and nFused++ (:970). q >= 0 and not bad: Observations(q) > Observations(p) ? p->Replace(q)
 *   (REPLACED_CANDIDATE) : q->Replace(p) (REPLACED_KF_POINT; a tie goes here, and q == p, which an inconsistent map allows, returns at once
 *   inside Replace). q >= 0 and bad: COUNTED_ONLY. q < 0: p->AddObservation(kf, f), kp_point[kf][f] = p (ADDED).
 *   VIORB_FUSE_SIM3. spAlreadyFound = the non-null, non-bad points of the key frame when the call starts. p == -1: NULL_POINT (the
 *   reference dereferences it). p bad: SKIP_BAD. p in spAlreadyFound: SKIP_IN_KF. f < 0: NONE. Otherwise q as above and nFused++. A live q
 *   is recorded as vpReplacePoint[i] (REPLACED_KF_POINT); a bad q: COUNTED_ONLY; q < 0: AddObservation, which returns early when p's
 *   observations already name the key frame, then kp_point[kf][f] = p (ADDED). After the loop, for i in order,
 *   vpReplacePoint[i]->Replace(list[i]), whether or not either point has gone bad since.
 *   a->Replace(s), literally: a == s returns. a's observations are taken and cleared, a becomes bad (nObs stays), mpReplaced = s. For
 *   every former observer (kf, idx): where s's observations do not name kf, kp_point[kf][idx] = s and s gains (kf, idx) with nObs += 2 for
 *   a stereo keypoint, else 1; otherwise kp_point[kf][idx] = -1. mnFound and mnVisible of a are added to s's, wrapping in 32 bits. s is
 *   descriptor-dirty (ComputeDistinctiveDescriptors).
 * Required: status [batch]; kp_point_out [n_kp]; pt_bad_out (u8), pt_nobs_out [n_pt]; the new observations as a CSR: obs_start_out
 * [n_pt + 1], obs_out (the words rebuilt from kp_octave / kp_stereo of (kf, idx)) and obs_feat_out [n_obs_out], per point in ascending key
 * order (the iteration order of std::map<KeyFrame*, size_t>). A stream's entries are packed from obs_out_start[b] on and stay inside
 * its region; need[b], when given, is how many there are. The stream writes obs_start_out of its own points, and the shared boundary
 * element behind its last point when no accepted stream follows it directly; tight regions (need of an earlier run, or batch == 1)
 * make obs_start_out the obs_start of viorb_covis_map as it is.
 *   status: VIORB_OK; VIORB_FUSE_OVERFLOW when the region is shorter than need[b]: the observation arrays and the dirty lists of the
 *   stream are not written (its dirty lists are empty), everything else is. A region as long as the stream's input observations plus
 *   its list entries with a non-negative op_feat cannot overflow. VIORB_ERR_INVALID_ARG for a stream the validating kernel refused:
 *   kf_start, pt_start, call_start, obs_out_start, kp_start, obs_start or call_op not ascending inside their totals; more than 65535 key
 *   frames; kf_by_key not a permutation; a kp_point outside -1 .. points - 1; an observation's slot outside the key frames; an obs_feat
 *   or op_feat outside its key frame's keypoints (op_feat may be -1); a list_point outside -1 .. points - 1; a call_kf, call_kind,
 *   call_list, call_n or call_feat outside its arrays, or a call_n that disagrees with call_op; an observation list that names a key
 *   frame twice. Nothing is read through a refused index, a refused stream writes nothing but its status, and the other streams are
 *   not affected.
 * Optional (NULL: not written): need [batch]; pt_found_out, pt_visible_out, pt_replaced_out (mpReplaced as set in this call, else -1)
 * [n_pt]; pt_dirty (u8) [n_pt]: ComputeDistinctiveDescriptors ran on the point; obs_touched (u8) [n_obs]: the input observation moved
 * to another point or died. The dirty lists, one CSR for the whole batch in the form viorb_map_points_update_device takes:
 * dirty_obs_start [n_pt + 1], dirty_obs_kf (global key-frame indices) and dirty_obs_feat [n_obs_out], packed over the accepted streams
 * from 0 on; a clean or bad point has an empty list (:258), observers with kf_bad are left out (:273-274). All three or none.
 * Per list entry [n_op], at call_op[c] + i: op_reason (VIORB_FUSE_*), op_other = q or -1. Per call [n_call]: call_nfused. */
typedef struct viorb_fuse_result {
    int32_t* status; int32_t* kp_point_out; uint8_t* pt_bad_out; int32_t* pt_nobs_out; int32_t* obs_start_out; uint32_t* obs_out; int32_t* obs_feat_out;
    int32_t* need; int32_t* pt_found_out; int32_t* pt_visible_out; int32_t* pt_replaced_out; uint8_t* pt_dirty; uint8_t* obs_touched;
    int32_t* dirty_obs_start; int32_t* dirty_obs_kf; int32_t* dirty_obs_feat;
    int32_t* op_reason; int32_t* op_other; int32_t* call_nfused;
} viorb_fuse_result;

/* Device scratch of viorb_apply_fuse_device (256-byte aligned device memory; its contents on entry are ignored) for a snapshot of
 * these totals. 0 for sizes outside the limits. */
size_t viorb_apply_fuse_workspace_bytes(int batch, int n_kf, int n_pt, int n_obs, int n_op);

/* The calls of every stream, those of a stream in order. It enqueues three kernels on `stream` and returns. */
int viorb_apply_fuse_device(const viorb_fuse_map* map, const viorb_fuse_result* result, void* workspace, size_t workspace_bytes, void* stream);
/* The same from host buffers (re-entrant; allocates, runs, synchronises, copies back). */
int viorb_apply_fuse(const viorb_fuse_map* map, const viorb_fuse_result* result);

/* Shapes of the built kernels, for tests that probe their edges: out4 = threads of the validating and the emitting kernel (the stride
 * of their loops), threads of the ordered phase (one wavefront: the stride of its loops over a point's observers, a call's entries and
 * a key frame's keypoints), the largest key-frame count of a stream whose state lives in LDS (0: none does), 0. */
int viorb_apply_fuse_shape(int32_t* out4);

/* viorb_map_points_update_device over the dirty lists leaves new descriptors for the points with a list and zeros for the others:
 * pts_desc[p] = new_desc[p] (rows of 32 bytes, 4-byte aligned) where pt_dirty[p] and, when dirty_obs_start is not NULL, the point's
 * dirty list is not empty (ComputeDistinctiveDescriptors returns early for a bad point or one without good observers and keeps
 * mDescriptor). It only enqueues. */
int viorb_fuse_merge_descriptors_device(const uint8_t* pt_dirty, const int32_t* dirty_obs_start, const uint8_t* new_desc, uint8_t* pts_desc, int n_pt, void* stream);

/* Test hook (no device): map_fusion_core.h compiled for the host, the same phases on one thread over host buffers. */
int viorb_debug_apply_fuse_host(const viorb_fuse_map* map, const viorb_fuse_result* result);

#endif /* VIORB_MAP_FUSION_H */
