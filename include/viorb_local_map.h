/* include/viorb_local_map.h — Tracking::UpdateLocalMap: reference src/Tracking.cc:1960-2125 (UpdateLocalKeyFrames :1996-2125,
 * UpdateLocalPoints :1970-1993), the step of Tracking::TrackLocalMap between the first pose solve and SearchLocalPoints, and the packing
 * of its result into the arrays viorb_frontend_search_local_points(_stereo)_device reads. Included by viorb.h; include viorb.h, not
 * this file. The ctypes mirror is viorb_amd/capi.py: SIGNATURES_LOCAL_MAP.
 *
 * The call works on a snapshot of the map around the current frame, for `batch` independent streams, and returns mvpLocalKeyFrames,
 * mpReferenceKF, mvpLocalMapPoints and the frame's mvpMapPoints with the bad points cleared. Every output equals the reference's loops
 * exactly: the routine is integer throughout. Pointer order enters in one place only, the walk of std::map<KeyFrame*, int>
 * keyframeCounter, and is passed in as the permutation kf_by_key. GetBestCovisibilityKeyFrames(10) is the input table covis10:
 * the first ten of ord_kf_out of viorb_update_connections (viorb_covisibility.h), which is KeyFrame::UpdateConnections. The index semantics of the neighbour loop are followed: what a
 * reallocation of mvpLocalKeyFrames under its live iterators would do is not reproduced.
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null struct or array, batch outside 1..65535, a
 * negative total, cap / lcap / pcap < 1, a workspace that is too small or not 256-byte aligned. What lies in device memory is checked on
 * the device, per stream: see `status`. Nothing in a _device entry allocates or synchronises, and its inputs are const. There is no CPU
 * fallback: without a device the launching entries return VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_LOCAL_MAP_H
#define VIORB_LOCAL_MAP_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* status[b] beside VIORB_OK and VIORB_ERR_INVALID_ARG */
#define VIORB_ULM_NO_VOTES   1   /* keyframeCounter.empty() (:2018): the key-frame list and the reference key frame are the previous frame's */
#define VIORB_ULM_OVERFLOW   2   /* more than lcap local key frames or more than pcap local points: n_lkf / n_lpt hold the needed sizes */

/* The snapshot: flat CSR arrays of `batch` streams. The *_start arrays hold global offsets; slots and point indices are local to their
 * stream. Device pointers for the _device entries, host pointers for the host entries. n_kf .. n_obs are the lengths of the arrays.
 *   Key frames (kf_start [batch+1]; at most 65535 per stream, none is allowed): kf_bad = isBad(); kf_parent / kf_prev / kf_next = the
 *   slot of GetParent() / GetPrevKeyFrame() / GetNextKeyFrame() or -1; covis10 [n_kf][10] = GetBestCovisibilityKeyFrames(10) in that
 *   order, padded with -1; the children of key frame k (child_start [n_kf+1]) in child_kf, in the iteration order of GetChilds();
 *   kf_by_key [n_kf] = the stream's slots in ascending std::less<KeyFrame*> order, a permutation of 0 .. nk-1.
 *   Keypoints of every key frame (kp_start [n_kf+1]): kp_point = the point of GetMapPointMatches()[i] or -1.
 *   Points (pt_start [batch+1]): pt_bad = isBad(). Observations of point p (obs_start [n_pt+1]), one word each: bits 0-15 the slot of
 *   the observing key frame, higher bits ignored, so the obs array of a viorb_cull_map can be passed as it is.
 *   The frame, per stream: frame_point [batch][cap] = the point of mCurrentFrame.mvpMapPoints[i] or -1 for i < frame_count[b] = N.
 *   From the previous frame, per stream: prev_lkf [batch][lcap] with prev_n_lkf[b] entries = mvpLocalKeyFrames as it stands (distinct
 *   slots), prev_ref_kf[b] = the slot of mpReferenceKF or -1. */
typedef struct viorb_local_map_snapshot {
    int32_t batch, n_kf, n_child, n_kp, n_pt, n_obs;
    const int32_t* kf_start; const uint8_t* kf_bad; const int32_t* kf_parent; const int32_t* kf_prev; const int32_t* kf_next;
    const int32_t* covis10; const int32_t* child_start; const int32_t* child_kf; const int32_t* kf_by_key;
    const int32_t* kp_start; const int32_t* kp_point;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* obs_start; const uint32_t* obs;
    const int32_t* frame_point; const int32_t* frame_count;
    const int32_t* prev_lkf; const int32_t* prev_n_lkf; const int32_t* prev_ref_kf;
} viorb_local_map_snapshot;

/* The result; every array is optional (NULL: not written).
 *   Per stream: lkf [batch][lcap] = mvpLocalKeyFrames as slots, -1 from n_lkf[b] on; n_voted[b] = the size of the list when the
 *   neighbour loop starts (:2047), 0 with VIORB_ULM_NO_VOTES; ref_kf[b] = the slot of mpReferenceKF (pKFmax, or prev_ref_kf where the
 *   reference leaves it alone); lpt [batch][pcap] = mvpLocalMapPoints as point indices, -1 from n_lpt[b] on.
 *   status[b]: VIORB_OK; VIORB_ULM_NO_VOTES (lkf = prev_lkf, ref_kf = prev_ref_kf; the points are still rebuilt from that list, as
 *   UpdateLocalPoints runs whatever UpdateLocalKeyFrames did); VIORB_ULM_OVERFLOW (n_lkf > lcap or n_lpt > pcap: both counts are the
 *   needed sizes, the arrays hold the first lcap / pcap entries and are not to be used); VIORB_ERR_INVALID_ARG for a stream the
 *   validating kernel refused: an offset (of this or an earlier stream) that is negative, descending or beyond its total, a slot or point
 *   index outside its stream, kf_by_key not a permutation, frame_count outside 0..cap, prev_n_lkf outside 0..min(lcap, key frames), a
 *   slot twice in prev_lkf, more than 65535 key frames. Nothing is read through a refused index, a refused stream writes nothing but its
 *   status, and the other streams are not affected.
 *   frame_point_out [batch][cap]: frame_point with the bad points set to -1 (:2013), -1 from frame_count[b] on.
 *   kf_votes [n_kf]: keyframeCounter (0: not in the map). Votes for a bad key frame are counted; the list skips it (:2032). */
typedef struct viorb_local_map_result {
    int32_t* lkf; int32_t* n_lkf; int32_t* n_voted; int32_t* ref_kf; int32_t* lpt; int32_t* n_lpt; int32_t* status;
    int32_t* frame_point_out; int32_t* kf_votes;
} viorb_local_map_result;

/* Device scratch of viorb_update_local_map_device (256-byte aligned device memory; its contents on entry are ignored) for a snapshot of
 * these totals. 0 for sizes outside the limits. */
size_t viorb_update_local_map_workspace_bytes(int batch, int n_kf, int n_pt);

/* Tracking::UpdateLocalMap (:1966-1967) for every stream of the snapshot. cap / lcap / pcap: the row lengths of frame_point, of lkf and
 * prev_lkf, of lpt. It enqueues four kernels on `stream` and returns. */
int viorb_update_local_map_device(const viorb_local_map_snapshot* map, const viorb_local_map_result* result, int cap, int lcap, int pcap,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* The same from host buffers (re-entrant; allocates, runs, synchronises, copies back). */
int viorb_update_local_map(const viorb_local_map_snapshot* map, const viorb_local_map_result* result, int cap, int lcap, int pcap);

/* Shapes of the built kernels, for tests that probe their edges: out4 = threads of the key-frame phase (the stride of its loops over
 * frame keypoints, key positions and list entries), entries per pass of the point compaction, the wavefront size (the stride of the
 * child scan), the largest key-frame count of a stream whose votes and list marks live in LDS (above it: in the workspace). */
int viorb_update_local_map_shape(int32_t* out4);

/* Packs the local points of a result into the [batch][pcap] layout viorb_frontend_search_local_points(_stereo)_device reads, from the
 * map's point store map_pts_f [n_pt][8] (Pw3 normal3 mfMinDistance mfMaxDistance), map_pts_desc [n_pt][32], pt_nobs [n_pt] =
 * Observations(), all indexed as the snapshot's points and 16-byte aligned. Reads map->batch, n_pt, pt_start, frame_count and
 * result->lpt, n_lpt, status, frame_point_out (all four required). pts_count[b] = n_lpt[b] for a stream with VIORB_OK or
 * VIORB_ULM_NO_VOTES, else 0. For j < pts_count[b]: pts_f / pts_desc = the rows of point lpt[b][j]; pts_flags = bit 0 (every local point
 * was !isBad() when listed), bit 1 where a keypoint of frame_point_out holds the point (mnLastFrameSeen == mCurrentFrame.mnId after the
 * first loop of Tracking::SearchLocalPoints, :1907-1923), bit 2 where pt_nobs > 0. Everything from the count on is zero. IncreaseVisible
 * and the other MapPoint counters stay with the caller. Workspace: viorb_local_points_gather_workspace_bytes(n_pt), 256-byte aligned;
 * its contents on entry are ignored. */
size_t viorb_local_points_gather_workspace_bytes(int n_pt);
int viorb_local_points_gather_device(const viorb_local_map_snapshot* map, const viorb_local_map_result* result, int cap, int pcap,
                                     const float* map_pts_f, const uint8_t* map_pts_desc, const int32_t* pt_nobs, float* pts_f, uint8_t* pts_desc,
                                     int32_t* pts_count, uint8_t* pts_flags, void* workspace, size_t workspace_bytes, void* stream);

/* Test hook (no device): local_map_core.h compiled for the host, the same phases on one thread over host buffers. */
int viorb_debug_update_local_map_host(const viorb_local_map_snapshot* map, const viorb_local_map_result* result, int cap, int lcap, int pcap);

#endif /* VIORB_LOCAL_MAP_H */
