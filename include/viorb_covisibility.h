/* include/viorb_covisibility.h — the covisibility graph: KeyFrame::UpdateConnections (reference src/KeyFrame.cc:580-670) with
 * AddConnection / UpdateBestCovisibles (:414-448) and AddChild (:672-676), for an ordered list of target key frames per stream, and the
 * LoopConnections loop of LoopClosing::CorrectLoop (src/LoopClosing.cc:572-590). Included by viorb.h; include viorb.h, not this file. The
 * ctypes mirror is viorb_amd/capi.py: SIGNATURES_COVISIBILITY.
 *
 * The call works on a snapshot of the map around the targets, for `batch` independent streams: the targets run one after the other, in
 * call order, every call changing what the next one reads, and the state they leave comes back per key frame. It produces what
 * viorb_update_local_map (covis10 = the first ten of ord_kf_out), viorb_key_frame_culling (cand_kf = ord_kf_out) and the essential
 * graph (loop_conn) consume. Every output equals the reference's loops exactly: the routine is integer throughout. Pointer order enters
 * through std::map<KeyFrame*, ...> and the sort of pair<int, KeyFrame*>, and is passed in as the permutation kf_by_key; a key frame's
 * key is its position in it.
 *
 * Every entry checks its arguments before any GPU call. VIORB_ERR_INVALID_ARG: a null struct or array (the optional result arrays
 * excepted), batch outside 1..65535, a negative total, ccap < 1, a workspace that is too small or not 256-byte aligned. What lies in
 * device memory is checked on the device, per stream: see `status`. Nothing in a _device entry allocates or synchronises, and its inputs
 * are const. There is no CPU fallback: without a device the launching entries return VIORB_ERR_NO_DEVICE. */
#ifndef VIORB_COVISIBILITY_H
#define VIORB_COVISIBILITY_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* status[b] beside VIORB_OK and VIORB_ERR_INVALID_ARG */
#define VIORB_COVIS_OVERFLOW   1   /* a row of mConnectedKeyFrameWeights would exceed ccap: need[b] holds the length it needs */

#define VIORB_COVIS_KF_ID0     1   /* kf_flags bit 0: mnId == 0 */
#define VIORB_COVIS_KF_FIRST   2   /* kf_flags bit 1: mbFirstConnection */
#define VIORB_COVIS_MAP_CHANGED   1   /* kf_touched bit 0: mConnectedKeyFrameWeights changed */
#define VIORB_COVIS_ORD_REBUILT   2   /* kf_touched bit 1: mvpOrderedConnectedKeyFrames / mvOrderedWeights were rebuilt or replaced */

/* The snapshot: flat CSR arrays of `batch` streams, with the offset and index rules of viorb_local_map_snapshot (the *_start arrays hold
 * global offsets; slots and point indices are local to their stream), whose kf_by_key, kp_start, kp_point, pt_start, pt_bad, obs_start
 * and obs pass unchanged. Device pointers for the _device entries, host pointers for the host entries. n_kf .. n_target are the lengths
 * of the arrays.
 *   Key frames (kf_start [batch+1]; at most 65535 per stream, none is allowed): kf_by_key [n_kf] = the stream's slots in ascending
 *   std::less<KeyFrame*> order; kf_flags = VIORB_COVIS_KF_*; kf_parent = the slot of mpParent or -1.
 *   Keypoints (kp_start [n_kf+1]): kp_point = the point of mvpMapPoints[i] or -1; only the targets' ranges of kp_point are read.
 *   Points (pt_start [batch+1]): pt_bad = isBad(); the observations of point p (obs_start [n_pt+1]), one word each: bits 0-15 the slot of
 *   the observing key frame, higher bits ignored.
 *   conn (conn_start [n_kf+1], conn_kf, conn_w): mConnectedKeyFrameWeights of every key frame in the map's iteration order: ascending
 *   key, distinct slots, never the key frame itself.
 *   ord (ord_start [n_kf+1], ord_kf, ord_w): mvpOrderedConnectedKeyFrames / mvOrderedWeights as they stand: distinct slots, otherwise not
 *   interpreted. They need not agree with conn: the reference's own lists do not (a key frame that was a target holds a thresholded
 *   list until a later AddConnection rebuilds it from its whole map).
 *   Targets (target_start [batch+1], target_kf): the key frames whose UpdateConnections runs, in call order. A slot may be listed more
 *   than once; a stream may have none. */
typedef struct viorb_covis_map {
    int32_t batch, n_kf, n_kp, n_pt, n_obs, n_conn, n_ord, n_target;
    const int32_t* kf_start; const int32_t* kf_by_key; const uint8_t* kf_flags; const int32_t* kf_parent;
    const int32_t* kp_start; const int32_t* kp_point;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* obs_start; const uint32_t* obs;
    const int32_t* conn_start; const int32_t* conn_kf; const int32_t* conn_w;
    const int32_t* ord_start; const int32_t* ord_kf; const int32_t* ord_w;
    const int32_t* target_start; const int32_t* target_kf;
} viorb_covis_map;

/* The result. The first seven arrays are required: the rows are the working state of the ordered loop.
 *   Per key frame, the state the loop leaves: conn_kf_out / conn_w_out [n_kf][ccap] with conn_n_out [n_kf] entries in ascending key
 *   order, ord_kf_out / ord_w_out [n_kf][ccap] with ord_n_out [n_kf] entries, -1 from the count on. An untouched key frame's rows are
 *   its input.
 *   status [batch]: VIORB_OK; VIORB_COVIS_OVERFLOW: a row of conn would exceed ccap. The rows are taken in this order: for every target
 *   in call order, first its own map (the counter), then the maps of the key frames it adds itself to, in key order; need[b] is the length
 *   of the first one that does not fit, the stream stops there and its other outputs are not to be used. ccap >= the stream's key frames
 *   - 1 can never overflow, since a map never holds its own key frame. VIORB_ERR_INVALID_ARG for a stream the validating kernel refused:
 *   an offset (of this or an earlier stream) that is negative, descending or beyond its total; a slot or point index outside its stream;
 *   kf_by_key that is not a permutation; a conn row that is out of key order, names a slot twice or names its own key frame; an ord row
 *   that names a slot twice; an input row longer than ccap; more than 65535 key frames. Nothing is read through a refused index, a
 *   refused stream writes nothing but its status, and the other streams are not affected.
 *   Optional (NULL: not written). need [batch]: 0 unless the stream overflowed. Per key frame: kf_parent_out, kf_flags_out (u8: bit 1
 *   cleared by the first connection), kf_touched (u8, VIORB_COVIS_MAP_CHANGED | VIORB_COVIS_ORD_REBUILT: the members a caller has to
 *   write back). There is no child output: mpParent->AddChild(this) is due where a call set the parent (t_parent >= 0), which for
 *   a map as the reference keeps it (no parent before the first connection) is exactly where kf_parent_out != kf_parent.
 *   Per target [n_target]: t_observers = KFcounter.size(), 0 is the early return (:614); t_max_kf / t_max_w = pKFmax / nmax, -1 and 0
 *   without observers; t_added = vPairs.size(); t_parent = the parent this call set or -1; loop_conn [n_target][ccap] with n_loop_conn
 *   entries in ascending key order, -1 from the count on = LoopConnections[target] (LoopClosing.cc:581-589): the keys of its map after
 *   the call, without the members of its ordered list just before the call and, when erase_targets != 0, without any target of the
 *   stream. */
typedef struct viorb_covis_result {
    int32_t* conn_kf_out; int32_t* conn_w_out; int32_t* conn_n_out; int32_t* ord_kf_out; int32_t* ord_w_out; int32_t* ord_n_out; int32_t* status;
    int32_t* need; int32_t* kf_parent_out; uint8_t* kf_flags_out; uint8_t* kf_touched;
    int32_t* t_observers; int32_t* t_max_kf; int32_t* t_max_w; int32_t* t_added; int32_t* t_parent; int32_t* loop_conn; int32_t* n_loop_conn;
} viorb_covis_result;

/* Device scratch of viorb_update_connections_device (256-byte aligned device memory; its contents on entry are ignored) for a snapshot
 * of these totals and this row length. 0 for sizes outside the limits. */
size_t viorb_update_connections_workspace_bytes(int batch, int n_kf, int n_target, int ccap);

/* UpdateConnections for every target of every stream, the targets of a stream in call order. ccap: the row length of the result's
 * rows. erase_targets: see loop_conn. It enqueues three kernels on `stream` and returns. */
int viorb_update_connections_device(const viorb_covis_map* map, const viorb_covis_result* result, int ccap, int erase_targets,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* The same from host buffers (re-entrant; allocates, runs, synchronises, copies back). */
int viorb_update_connections(const viorb_covis_map* map, const viorb_covis_result* result, int ccap, int erase_targets);

/* Shapes of the built kernels, for tests that probe their edges: out4 = threads of the vote and of the ordered phase (the stride of their
 * loops over keypoints, key positions and row entries), the wavefront size (the stride of AddConnection's loops over a row), the
 * largest key-frame count of a stream whose counters and marks live in LDS (above it: in the workspace), the threshold th (15). */
int viorb_update_connections_shape(int32_t* out4);

/* Test hook (no device): covis_core.h compiled for the host, the same phases on one thread over host buffers. */
int viorb_debug_update_connections_host(const viorb_covis_map* map, const viorb_covis_result* result, int ccap, int erase_targets);

#endif /* VIORB_COVISIBILITY_H */
