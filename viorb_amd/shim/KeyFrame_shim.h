// viorb_amd/shim/KeyFrame_shim.h — reference-side glue for the covisibility graph (include/viorb_covisibility.h) and, at the end of the
// file, for key-frame removal (include/viorb_kf_removal.h): function templates over
// the reference's KeyFrame / MapPoint. Like the other shims this header includes none of the reference's headers; it is compiled inside
// the reference tree, after them (INTEGRATION.md shows the one-line bodies at the call sites).
//   KeyFrame::UpdateConnections()                      reference src/KeyFrame.cc:580-670, called from src/LocalMapping.cc:1187, :1566,
//                                                      src/Tracking.cc:1414-1415, src/LoopClosing.cc:458, :541
//       void KeyFrame::UpdateConnections() { viorb_shim::update_connections<MapPoint>(this); }
//   the LoopConnections loop of LoopClosing::CorrectLoop   reference src/LoopClosing.cc:572-590
//       map<KeyFrame*, set<KeyFrame*> > LoopConnections;
//       viorb_shim::update_connections_loop<MapPoint>(mvpCurrentConnectedKFs, LoopConnections);
// The templates read mnId, mbFirstConnection, GetMapPointMatches, MapPoint::isBad and MapPoint::GetObservations, and read and write
// mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights, mpParent, mbFirstConnection (under mMutexConnections, as the
// reference does) and call AddChild. These members are protected in the reference, and other key frames' are written too, so KeyFrame.h
// names the accessor below a friend:
//       namespace viorb_shim { struct CovisAccess; }        // before class KeyFrame
//       friend struct viorb_shim::CovisAccess;              // inside it
#ifndef VIORB_KEYFRAME_SHIM_H
#define VIORB_KEYFRAME_SHIM_H

#include <mutex>
#include "viorb_tracking_shim.h"       // check, SlotTable

namespace viorb_shim {

struct CovisAccess {
    template <class K> static std::map<K*, int>& weights(K* k) { return k->mConnectedKeyFrameWeights; }
    template <class K> static std::vector<K*>& ordered(K* k) { return k->mvpOrderedConnectedKeyFrames; }
    template <class K> static std::vector<int>& ordered_weights(K* k) { return k->mvOrderedWeights; }
    template <class K> static bool& first_connection(K* k) { return k->mbFirstConnection; }
    template <class K> static K*& parent(K* k) { return k->mpParent; }
    template <class K> static std::mutex& mutex(K* k) { return k->mMutexConnections; }
};

// UpdateConnections for the key frames of `group`, in order, in one call of the library. The snapshot holds the targets, the observers of
// the targets' points (the only key frames a call can change) with their maps and ordered lists, and, as slots without rows, the key
// frames those maps name; observations are passed for the targets' good points only. Pointer order enters through kf_by_key, sorted with
// std::less<KeyFrame*>. Written back, for the key frames the library reports as touched: mConnectedKeyFrameWeights, the two ordered
// vectors; for a target whose first connection this was: mpParent, mpParent->AddChild, mbFirstConnection. loop (may be null) receives
// LoopConnections[target] of LoopClosing.cc:581-589 for every target. A failure throws.
template <class MapPointT, class KeyFrameT>
inline void update_connections_group(const std::vector<KeyFrameT*>& group, std::map<KeyFrameT*, std::set<KeyFrameT*> >* loop) {
    typedef CovisAccess A;
    if (group.empty()) return;
    SlotTable<KeyFrameT> kf_slot; const std::vector<KeyFrameT*>& kfs = kf_slot.items;
    SlotTable<MapPointT> pt_slot; const std::vector<MapPointT*>& pts = pt_slot.items;
    std::vector<int32_t> target_kf;
    for (size_t t = 0; t < group.size(); t++) target_kf.push_back(kf_slot.add(group[t]));
    const size_t n_targets = kfs.size();                             // distinct targets: slots below
    std::vector<int32_t> kp_start(1, 0), kp_point, obs_start(1, 0);
    std::vector<uint32_t> obs;
    std::vector<uint8_t> pt_bad;
    for (size_t k = 0; k < n_targets; k++) {
        const std::vector<MapPointT*> vpMP = kfs[k]->GetMapPointMatches();
        for (size_t i = 0; i < vpMP.size(); i++) {
            MapPointT* pMP = vpMP[i];
            if (!pMP) { kp_point.push_back(-1); continue; }
            const size_t before = pts.size();
            kp_point.push_back(pt_slot.add(pMP));
            if (pts.size() == before) continue;
            pt_bad.push_back(pMP->isBad() ? 1 : 0);
            if (!pt_bad.back()) {
                const std::map<KeyFrameT*, size_t> observations = pMP->GetObservations();
                for (typename std::map<KeyFrameT*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) obs.push_back((uint32_t)kf_slot.add(it->first));
            }
            obs_start.push_back((int32_t)obs.size());
        }
        kp_start.push_back((int32_t)kp_point.size());
    }
    const size_t n_rows = kfs.size();                                // targets and observers: slots below bring their rows
    std::vector<std::vector<std::pair<KeyFrameT*, int> > > conn(n_rows), ord(n_rows);
    for (size_t k = 0; k < n_rows; k++) {
        std::unique_lock<std::mutex> lock(A::mutex(kfs[k]));
        const std::map<KeyFrameT*, int>& w = A::weights(kfs[k]);
        conn[k].assign(w.begin(), w.end());                          // the map's own order is key order
        for (size_t i = 0; i < A::ordered(kfs[k]).size(); i++) ord[k].push_back(std::make_pair(A::ordered(kfs[k])[i], A::ordered_weights(kfs[k])[i]));
    }
    std::vector<int32_t> conn_start(1, 0), conn_kf, conn_w, ord_start(1, 0), ord_kf, ord_w;
    for (size_t k = 0; k < n_rows; k++) {
        for (size_t i = 0; i < conn[k].size(); i++) { conn_kf.push_back(kf_slot.add(conn[k][i].first)); conn_w.push_back(conn[k][i].second); }
        conn_start.push_back((int32_t)conn_kf.size());
        for (size_t i = 0; i < ord[k].size(); i++) { ord_kf.push_back(kf_slot.add(ord[k][i].first)); ord_w.push_back(ord[k][i].second); }
        ord_start.push_back((int32_t)ord_kf.size());
    }
    const size_t nk = kfs.size(), np = pts.size();
    if (nk > 65535) throw std::runtime_error("UpdateConnections: more than 65535 key frames in the snapshot");
    kp_start.resize(nk + 1, (int32_t)kp_point.size()); conn_start.resize(nk + 1, (int32_t)conn_kf.size()); ord_start.resize(nk + 1, (int32_t)ord_kf.size());
    std::vector<uint8_t> kf_flags(nk, 0);
    for (size_t k = 0; k < n_rows; k++) kf_flags[k] = (uint8_t)((kfs[k]->mnId == 0 ? VIORB_COVIS_KF_ID0 : 0) | (A::first_connection(kfs[k]) ? VIORB_COVIS_KF_FIRST : 0));
    std::vector<int32_t> kf_parent(nk, -1);                          // passed through only: the parent is written back from t_parent
    std::vector<std::pair<KeyFrameT*, int32_t> > by_ptr;
    for (size_t k = 0; k < nk; k++) by_ptr.push_back(std::make_pair(kfs[k], (int32_t)k));
    struct Less { bool operator()(const std::pair<KeyFrameT*, int32_t>& a, const std::pair<KeyFrameT*, int32_t>& b) const { return std::less<KeyFrameT*>()(a.first, b.first); } };
    std::sort(by_ptr.begin(), by_ptr.end(), Less());
    std::vector<int32_t> kf_by_key(nk, 0);
    for (size_t j = 0; j < nk; j++) kf_by_key[j] = by_ptr[j].second;
    // every array at least one element long: the library refuses a null pointer whatever the count
    viorb_covis_map m;
    m.batch = 1; m.n_kf = (int32_t)nk; m.n_kp = (int32_t)kp_point.size(); m.n_pt = (int32_t)np; m.n_obs = (int32_t)obs.size();
    m.n_conn = (int32_t)conn_kf.size(); m.n_ord = (int32_t)ord_kf.size(); m.n_target = (int32_t)target_kf.size();
    kp_point.resize(std::max<size_t>(kp_point.size(), 1), -1); pt_bad.resize(std::max<size_t>(np, 1), 0); obs.resize(std::max<size_t>(obs.size(), 1));
    conn_kf.resize(std::max<size_t>(conn_kf.size(), 1)); conn_w.resize(conn_kf.size()); ord_kf.resize(std::max<size_t>(ord_kf.size(), 1)); ord_w.resize(ord_kf.size());
    const int32_t kf_start[2] = {0, (int32_t)nk}, pt_start[2] = {0, (int32_t)np}, target_start[2] = {0, m.n_target};
    m.kf_start = kf_start; m.kf_by_key = &kf_by_key[0]; m.kf_flags = &kf_flags[0]; m.kf_parent = &kf_parent[0]; m.kp_start = &kp_start[0]; m.kp_point = &kp_point[0];
    m.pt_start = pt_start; m.pt_bad = &pt_bad[0]; m.obs_start = &obs_start[0]; m.obs = &obs[0];
    m.conn_start = &conn_start[0]; m.conn_kf = &conn_kf[0]; m.conn_w = &conn_w[0]; m.ord_start = &ord_start[0]; m.ord_kf = &ord_kf[0]; m.ord_w = &ord_w[0];
    m.target_start = target_start; m.target_kf = &target_kf[0];
    const int ccap = (int)std::max<size_t>(nk - 1, 1);               // a map never holds its own key frame: nothing overflows
    const size_t nt = target_kf.size();
    std::vector<int32_t> ck(nk * ccap), cw(nk * ccap), cn(nk), ok(nk * ccap), ow(nk * ccap), on(nk), t_parent(nt), lc(nt * ccap), n_lc(nt);
    std::vector<uint8_t> flags_out(nk), touched(nk);
    int32_t status = 0;
    viorb_covis_result r;
    std::memset(&r, 0, sizeof(r));
    r.conn_kf_out = &ck[0]; r.conn_w_out = &cw[0]; r.conn_n_out = &cn[0]; r.ord_kf_out = &ok[0]; r.ord_w_out = &ow[0]; r.ord_n_out = &on[0]; r.status = &status;
    r.kf_flags_out = &flags_out[0]; r.kf_touched = &touched[0]; r.t_parent = &t_parent[0];
    if (loop) { r.loop_conn = &lc[0]; r.n_loop_conn = &n_lc[0]; }
    check(viorb_update_connections(&m, &r, ccap, 1), "UpdateConnections");
    if (status != VIORB_OK) throw std::runtime_error("UpdateConnections: the library refused the snapshot");
    for (size_t k = 0; k < n_rows; k++) {
        if (!touched[k]) continue;
        std::unique_lock<std::mutex> lock(A::mutex(kfs[k]));
        if (touched[k] & VIORB_COVIS_MAP_CHANGED) {
            std::map<KeyFrameT*, int> w;
            for (int32_t i = 0; i < cn[k]; i++) w[kfs[ck[k * ccap + i]]] = cw[k * ccap + i];
            A::weights(kfs[k]).swap(w);
        }
        if (touched[k] & VIORB_COVIS_ORD_REBUILT) {
            std::vector<KeyFrameT*> v; std::vector<int> ws;
            for (int32_t i = 0; i < on[k]; i++) { v.push_back(kfs[ok[k * ccap + i]]); ws.push_back(ow[k * ccap + i]); }
            A::ordered(kfs[k]).swap(v); A::ordered_weights(kfs[k]).swap(ws);
        }
    }
    for (size_t t = 0; t < nt; t++) {                                // :662-667
        if (t_parent[t] < 0) continue;
        KeyFrameT* pKF = kfs[target_kf[t]];
        { std::unique_lock<std::mutex> lock(A::mutex(pKF)); A::parent(pKF) = kfs[t_parent[t]]; A::first_connection(pKF) = false; }
        kfs[t_parent[t]]->AddChild(pKF);
    }
    if (loop) for (size_t t = 0; t < nt; t++) {
        std::set<KeyFrameT*>& s = (*loop)[kfs[target_kf[t]]];
        s.clear();
        for (int32_t i = 0; i < n_lc[t]; i++) s.insert(kfs[lc[t * ccap + i]]);
    }
}

// KeyFrame::UpdateConnections (the LocalMapping and Tracking call sites, and LoopClosing.cc:458, :541)
template <class MapPointT, class KeyFrameT>
inline void update_connections(KeyFrameT* pKF) { update_connections_group<MapPointT, KeyFrameT>(std::vector<KeyFrameT*>(1, pKF), static_cast<std::map<KeyFrameT*, std::set<KeyFrameT*> >*>(0)); }

// The loop of LoopClosing.cc:574-590 over mvpCurrentConnectedKFs in one call: every UpdateConnections in order, and LoopConnections
template <class MapPointT, class KeyFrameT>
inline void update_connections_loop(const std::vector<KeyFrameT*>& group, std::map<KeyFrameT*, std::set<KeyFrameT*> >& LoopConnections) { update_connections_group<MapPointT, KeyFrameT>(group, &LoopConnections); }

// ---- key-frame removal (include/viorb_kf_removal.h) -------------------------------------------------------------------------------------------
//   void KeyFrame::SetBadFlag() { viorb_shim::set_bad_flag<MapPoint>(this); }        reference src/KeyFrame.cc:744-882
//   void KeyFrame::SetErase()   { viorb_shim::set_erase<MapPoint>(this); }           reference src/KeyFrame.cc:728-742
//   viorb_shim::remove_key_frames<KeyFrame, MapPoint>(list, kinds)                   several operations in order in one call of the library
// The templates read mnId, mvuRight, GetMapPointMatches, GetPose, GetParent, GetChilds, GetPrevKeyFrame / GetNextKeyFrame,
// MapPoint::Observations / isBad / GetReferenceKeyFrame / GetObservations, write through the two friends below, and call the reference's own
// EraseMapPointMatch(idx), SetPrevKeyFrame / SetNextKeyFrame, AppendIMUDataToFront / ComputePreInt, Map::EraseKeyFrame, Map::EraseMapPoint
// and KeyFrameDatabase::erase. KeyFrame.h and MapPoint.h name the accessors friends:
//       namespace viorb_shim { struct RemovalAccess; struct RemovalPointAccess; }      // before the classes
//       friend struct viorb_shim::RemovalAccess;                                       // inside KeyFrame
//       friend struct viorb_shim::RemovalPointAccess;                                  // inside MapPoint
struct RemovalAccess {
    template <class K> static std::map<K*, int>& weights(K* k) { return k->mConnectedKeyFrameWeights; }
    template <class K> static std::vector<K*>& ordered(K* k) { return k->mvpOrderedConnectedKeyFrames; }
    template <class K> static std::vector<int>& ordered_weights(K* k) { return k->mvOrderedWeights; }
    template <class K> static K*& parent(K* k) { return k->mpParent; }
    template <class K> static std::set<K*>& children(K* k) { return k->mspChildrens; }
    template <class K> static cv::Mat& Tcp(K* k) { return k->mTcp; }
    template <class K> static bool& bad(K* k) { return k->mbBad; }
    template <class K> static bool& not_erase(K* k) { return k->mbNotErase; }
    template <class K> static bool& to_be_erased(K* k) { return k->mbToBeErased; }
    template <class K> static bool has_loop_edges(K* k) { return !k->mspLoopEdges.empty(); }
    template <class K> static void erase_from_map_and_database(K* k) { k->mpMap->EraseKeyFrame(k); k->mpKeyFrameDB->erase(k); }
    template <class K> static std::mutex& mutex(K* k) { return k->mMutexConnections; }
};
struct RemovalPointAccess {
    template <class P, class K> static std::map<K*, size_t>& observations(P* p, K*) { return p->mObservations; }
    template <class P> static int& nobs(P* p) { return p->nObs; }
    template <class P, class K> static void set_ref(P* p, K* k) { p->mpRefKF = k; }
    template <class P> static bool& bad(P* p) { return p->mbBad; }
    template <class P> static void erase_from_map(P* p) { p->mpMap->EraseMapPoint(p); }
    template <class P> static std::mutex& mutex(P* p) { return p->mMutexFeatures; }
};

// SetBadFlag (kind 0) / SetErase (kind 1) on the key frames of `list`, in order, in one call of the library. The snapshot holds, with their
// maps and lists, the operations' key frames, the key frames of their maps and their children; as slots, their parents, prev / next, the
// key frames those maps name and the observers of their points, the observers with their keypoint tables (points the snapshot does not
// know are passed as -1: a table is only compared with a point). Pointer order enters through kf_by_key, sorted with
// std::less<KeyFrame*>. A failure throws.
template <class KeyFrameT, class MapPointT>
inline void remove_key_frames(const std::vector<KeyFrameT*>& list, const std::vector<int>& kinds) {
    typedef RemovalAccess A; typedef RemovalPointAccess PA;
    if (list.empty()) return;
    if (kinds.size() != list.size()) throw std::runtime_error("remove_key_frames: one kind per key frame");
    SlotTable<KeyFrameT> kf_slot; const std::vector<KeyFrameT*>& kfs = kf_slot.items;
    SlotTable<MapPointT> pt_slot; const std::vector<MapPointT*>& pts = pt_slot.items;
    std::vector<int32_t> op_kf; std::vector<uint8_t> op_kind;
    for (size_t j = 0; j < list.size(); j++) { op_kf.push_back(kf_slot.add(list[j])); op_kind.push_back(kinds[j] ? VIORB_KFR_SET_ERASE : VIORB_KFR_SET_BAD_FLAG); }
    const size_t n_ops = kfs.size();                                 // distinct operation key frames: slots below
    for (size_t k = 0; k < n_ops; k++) {                             // their neighbours and children bring rows too
        { std::unique_lock<std::mutex> lock(A::mutex(kfs[k]));
          const std::map<KeyFrameT*, int> w = A::weights(kfs[k]);
          for (typename std::map<KeyFrameT*, int>::const_iterator it = w.begin(); it != w.end(); ++it) kf_slot.add(it->first); }
        const std::set<KeyFrameT*> ch = kfs[k]->GetChilds();
        for (typename std::set<KeyFrameT*>::const_iterator it = ch.begin(); it != ch.end(); ++it) kf_slot.add(*it);
    }
    const size_t n_rows = kfs.size();
    std::vector<int32_t> conn_start(1, 0), conn_kf, conn_w, ord_start(1, 0), ord_kf, ord_w;
    for (size_t k = 0; k < n_rows; k++) {
        std::vector<std::pair<KeyFrameT*, int> > conn, ord;
        { std::unique_lock<std::mutex> lock(A::mutex(kfs[k]));
          conn.assign(A::weights(kfs[k]).begin(), A::weights(kfs[k]).end());          // the map's own order is key order
          for (size_t i = 0; i < A::ordered(kfs[k]).size(); i++) ord.push_back(std::make_pair(A::ordered(kfs[k])[i], A::ordered_weights(kfs[k])[i])); }
        for (size_t i = 0; i < conn.size(); i++) { conn_kf.push_back(kf_slot.add(conn[i].first)); conn_w.push_back(conn[i].second); }
        conn_start.push_back((int32_t)conn_kf.size());
        for (size_t i = 0; i < ord.size(); i++) { ord_kf.push_back(kf_slot.add(ord[i].first)); ord_w.push_back(ord[i].second); }
        ord_start.push_back((int32_t)ord_kf.size());
    }
    for (size_t k = 0; k < n_ops; k++) {                             // the parents and the links of the operations' key frames
        if (kfs[k]->GetParent()) kf_slot.add(kfs[k]->GetParent());
        if (kfs[k]->GetPrevKeyFrame()) kf_slot.add(kfs[k]->GetPrevKeyFrame());
        if (kfs[k]->GetNextKeyFrame()) kf_slot.add(kfs[k]->GetNextKeyFrame());
    }
    // the points of the operations' key frames with their observers
    std::vector<std::vector<int32_t> > table(n_ops);
    std::vector<int32_t> obs_start(1, 0), pt_nobs, pt_ref;
    std::vector<uint32_t> obs;
    std::vector<uint8_t> pt_bad;
    std::vector<std::vector<KeyFrameT*> > observers;
    for (size_t k = 0; k < n_ops; k++) {
        const std::vector<MapPointT*> vpMP = kfs[k]->GetMapPointMatches();
        for (size_t i = 0; i < vpMP.size(); i++) {
            MapPointT* pMP = vpMP[i];
            if (!pMP) { table[k].push_back(-1); continue; }
            const size_t before = pts.size();
            table[k].push_back(pt_slot.add(pMP));
            if (pts.size() == before) continue;
            pt_bad.push_back(pMP->isBad() ? 1 : 0); pt_nobs.push_back(pMP->Observations());
            KeyFrameT* ref = pMP->GetReferenceKeyFrame();
            pt_ref.push_back(ref ? kf_slot.add(ref) : -1);
            const std::map<KeyFrameT*, size_t> observations = pMP->GetObservations();
            observers.push_back(std::vector<KeyFrameT*>());
            for (typename std::map<KeyFrameT*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) {
                observers.back().push_back(it->first);
                obs.push_back((uint32_t)kf_slot.add(it->first) | (it->first->mvuRight[it->second] >= 0 ? (1u << 24) : 0u));
            }
            obs_start.push_back((int32_t)obs.size());
        }
    }
    const size_t nk = kfs.size(), np = pts.size();
    if (nk > 65535) throw std::runtime_error("remove_key_frames: more than 65535 key frames in the snapshot");
    std::vector<int32_t> kp_start(1, 0), kp_point;
    for (size_t k = 0; k < nk; k++) {                                // the tables: the operations' own, and every other key frame's as far as the snapshot knows its points
        if (k < n_ops) kp_point.insert(kp_point.end(), table[k].begin(), table[k].end());
        else {
            const std::vector<MapPointT*> vpMP = kfs[k]->GetMapPointMatches();
            for (size_t i = 0; i < vpMP.size(); i++) kp_point.push_back(vpMP[i] ? pt_slot.find(vpMP[i]) : -1);
        }
        kp_start.push_back((int32_t)kp_point.size());
    }
    conn_start.resize(nk + 1, (int32_t)conn_kf.size()); ord_start.resize(nk + 1, (int32_t)ord_kf.size());
    std::vector<uint8_t> kf_flags(nk, 0);
    std::vector<int32_t> kf_parent(nk, -1), kf_prev(nk, -1), kf_next(nk, -1);
    std::vector<float> pose12(nk * 12, 0.f);
    for (size_t k = 0; k < nk; k++) {
        KeyFrameT* K = kfs[k];
        { std::unique_lock<std::mutex> lock(A::mutex(K));
          kf_flags[k] = (uint8_t)((K->mnId == 0 ? VIORB_KFR_KF_ID0 : 0) | (A::bad(K) ? VIORB_KFR_KF_BAD : 0) | (A::not_erase(K) ? VIORB_KFR_KF_NOT_ERASE : 0)
                                  | (A::to_be_erased(K) ? VIORB_KFR_KF_TO_BE_ERASED : 0) | (A::has_loop_edges(K) ? VIORB_KFR_KF_LOOP_EDGES : 0)); }
        kf_parent[k] = K->GetParent() ? kf_slot.find(K->GetParent()) : -1;
        kf_prev[k] = K->GetPrevKeyFrame() ? kf_slot.find(K->GetPrevKeyFrame()) : -1;
        kf_next[k] = K->GetNextKeyFrame() ? kf_slot.find(K->GetNextKeyFrame()) : -1;
        const cv::Mat T = K->GetPose();
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) pose12[k * 12 + 3 * r + c] = T.template at<float>(r, c); pose12[k * 12 + 9 + r] = T.template at<float>(r, 3); }
    }
    std::vector<std::pair<KeyFrameT*, int32_t> > by_ptr;
    for (size_t k = 0; k < nk; k++) by_ptr.push_back(std::make_pair(kfs[k], (int32_t)k));
    struct Less { bool operator()(const std::pair<KeyFrameT*, int32_t>& a, const std::pair<KeyFrameT*, int32_t>& b) const { return std::less<KeyFrameT*>()(a.first, b.first); } };
    std::sort(by_ptr.begin(), by_ptr.end(), Less());
    std::vector<int32_t> kf_by_key(nk, 0);
    for (size_t j = 0; j < nk; j++) kf_by_key[j] = by_ptr[j].second;
    viorb_kfr_map m;
    m.batch = 1; m.n_kf = (int32_t)nk; m.n_kp = (int32_t)kp_point.size(); m.n_pt = (int32_t)np; m.n_obs = (int32_t)obs.size();
    m.n_conn = (int32_t)conn_kf.size(); m.n_ord = (int32_t)ord_kf.size(); m.n_op = (int32_t)op_kf.size();
    const size_t n_kp = kp_point.size(), n_obs = obs.size();
    // every array at least one element long: the library refuses a null pointer whatever the count
    kp_point.resize(std::max<size_t>(n_kp, 1), -1); pt_bad.resize(std::max<size_t>(np, 1), 0); pt_nobs.resize(pt_bad.size(), 0); pt_ref.resize(pt_bad.size(), -1);
    obs.resize(std::max<size_t>(n_obs, 1)); conn_kf.resize(std::max<size_t>(conn_kf.size(), 1)); conn_w.resize(conn_kf.size());
    ord_kf.resize(std::max<size_t>(ord_kf.size(), 1)); ord_w.resize(ord_kf.size());
    const int32_t kf_start[2] = {0, (int32_t)nk}, pt_start[2] = {0, (int32_t)np}, op_start[2] = {0, m.n_op};
    m.kf_start = kf_start; m.kf_by_key = &kf_by_key[0]; m.kf_flags = &kf_flags[0]; m.kf_parent = &kf_parent[0]; m.kf_prev = &kf_prev[0]; m.kf_next = &kf_next[0];
    m.kf_pose12 = &pose12[0]; m.kp_start = &kp_start[0]; m.kp_point = &kp_point[0]; m.pt_start = pt_start; m.pt_bad = &pt_bad[0]; m.pt_nobs = &pt_nobs[0];
    m.pt_ref = &pt_ref[0]; m.obs_start = &obs_start[0]; m.obs = &obs[0]; m.conn_start = &conn_start[0]; m.conn_kf = &conn_kf[0]; m.conn_w = &conn_w[0];
    m.ord_start = &ord_start[0]; m.ord_kf = &ord_kf[0]; m.ord_w = &ord_w[0]; m.op_start = op_start; m.op_kf = &op_kf[0]; m.op_kind = &op_kind[0];
    const int ccap = (int)std::max<size_t>(nk - 1, 1);
    const size_t nop = op_kf.size();
    std::vector<int32_t> ck(nk * ccap), cw(nk * ccap), cn(nk), ok(nk * ccap), ow(nk * ccap), on(nk), parent_out(nk), prev_out(nk), next_out(nk), nobs_out(pt_bad.size()),
        ref_out(pt_bad.size()), kp_out(kp_point.size()), reason(nop);
    std::vector<uint8_t> flags_out(nk), touched(nk), bad_out(pt_bad.size()), alive(obs.size());
    std::vector<float> Tcp(nk * 12);
    int32_t status = 0;
    viorb_kfr_result r;
    std::memset(&r, 0, sizeof(r));
    r.conn_kf_out = &ck[0]; r.conn_w_out = &cw[0]; r.conn_n_out = &cn[0]; r.ord_kf_out = &ok[0]; r.ord_w_out = &ow[0]; r.ord_n_out = &on[0]; r.status = &status;
    r.kf_parent_out = &parent_out[0]; r.kf_flags_out = &flags_out[0]; r.kf_prev_out = &prev_out[0]; r.kf_next_out = &next_out[0]; r.kf_Tcp_out = &Tcp[0]; r.kf_touched = &touched[0];
    r.pt_nobs_out = &nobs_out[0]; r.pt_bad_out = &bad_out[0]; r.obs_alive = &alive[0]; r.pt_ref_out = &ref_out[0]; r.kp_point_out = &kp_out[0]; r.op_reason = &reason[0];
    check(viorb_remove_key_frames(&m, &r, ccap), "remove_key_frames");
    if (status != VIORB_OK) throw std::runtime_error("remove_key_frames: the library refused the snapshot");
    // ---- write back ----
    for (size_t k = 0; k < nk; k++) {
        KeyFrameT* K = kfs[k];
        if (touched[k] & VIORB_KFR_PARENT_CHANGED) {                 // ChangeParent: the old parent is an operation's key frame, bad by now
            KeyFrameT* old = K->GetParent();
            if (old) { std::unique_lock<std::mutex> lock(A::mutex(old)); A::children(old).erase(K); }
            { std::unique_lock<std::mutex> lock(A::mutex(K)); A::parent(K) = kfs[parent_out[k]]; }
            { std::unique_lock<std::mutex> lock(A::mutex(kfs[parent_out[k]])); A::children(kfs[parent_out[k]]).insert(K); }
        }
        std::unique_lock<std::mutex> lock(A::mutex(K));
        if (touched[k] & VIORB_KFR_MAP_CHANGED) {
            std::map<KeyFrameT*, int> w;
            for (int32_t i = 0; i < cn[k]; i++) w[kfs[ck[k * ccap + i]]] = cw[k * ccap + i];
            A::weights(K).swap(w);
        }
        if (touched[k] & VIORB_KFR_ORD_REBUILT) {
            std::vector<KeyFrameT*> v; std::vector<int> ws;
            for (int32_t i = 0; i < on[k]; i++) { v.push_back(kfs[ok[k * ccap + i]]); ws.push_back(ow[k * ccap + i]); }
            A::ordered(K).swap(v); A::ordered_weights(K).swap(ws);
        }
        if (k < n_ops) { A::not_erase(K) = (flags_out[k] & VIORB_KFR_KF_NOT_ERASE) != 0; A::to_be_erased(K) = (flags_out[k] & VIORB_KFR_KF_TO_BE_ERASED) != 0; }
    }
    for (size_t p = 0; p < np; p++) {                                // the points: EraseObservation and, where the point went bad, SetBadFlag
        MapPointT* P = pts[p];
        bool cleared = bad_out[p] != 0, any = false;
        for (int32_t o = obs_start[p]; o < obs_start[p + 1]; o++) { cleared = cleared && !alive[o]; any = any || !alive[o]; }
        if (!any) continue;
        { std::unique_lock<std::mutex> lock(PA::mutex(P));
          for (int32_t o = obs_start[p]; o < obs_start[p + 1]; o++) if (!alive[o]) PA::observations(P, (KeyFrameT*)0).erase(observers[p][o - obs_start[p]]);
          PA::nobs(P) = nobs_out[p]; PA::bad(P) = bad_out[p] != 0;
          PA::set_ref(P, ref_out[p] >= 0 ? kfs[ref_out[p]] : (KeyFrameT*)0); }
        if (cleared && obs_start[p + 1] > obs_start[p]) PA::erase_from_map(P);
    }
    for (size_t k = 0; k < nk; k++)                                  // EraseMapPointMatch at the observers of the points that went bad
        for (int32_t i = kp_start[k]; i < kp_start[k + 1]; i++) if (kp_point[i] >= 0 && kp_out[i] < 0) kfs[k]->EraseMapPointMatch((size_t)(i - kp_start[k]));
    for (size_t j = 0; j < nop; j++) {                               // in operation order: mTcp, mbBad, the links with the IMU data, the map and the database
        KeyFrameT* K = kfs[op_kf[j]];
        if (reason[j] == VIORB_KFR_ALREADY_BAD) { A::erase_from_map_and_database(K); continue; }
        if (reason[j] != VIORB_KFR_REMOVED) continue;
        const size_t k = (size_t)op_kf[j];
        cv::Mat T(4, 4, CV_32F);
        for (int r4 = 0; r4 < 4; r4++) for (int c = 0; c < 4; c++) T.template at<float>(r4, c) = r4 < 3 ? (c < 3 ? Tcp[k * 12 + 3 * r4 + c] : Tcp[k * 12 + 9 + r4]) : (c == 3 ? 1.f : 0.f);
        KeyFrameT* par = K->GetParent();
        if (par) { std::unique_lock<std::mutex> lock(A::mutex(par)); A::children(par).erase(K); }
        { std::unique_lock<std::mutex> lock(A::mutex(K)); A::Tcp(K) = T; A::bad(K) = true; }
        KeyFrameT* pPrevKF = K->GetPrevKeyFrame(); KeyFrameT* pNextKF = K->GetNextKeyFrame();
        if (pPrevKF) pPrevKF->SetNextKeyFrame(pNextKF);
        if (pNextKF) pNextKF->SetPrevKeyFrame(pPrevKF);
        K->SetPrevKeyFrame((KeyFrameT*)0); K->SetNextKeyFrame((KeyFrameT*)0);
        if (pPrevKF && pNextKF) { pNextKF->AppendIMUDataToFront(K); pNextKF->ComputePreInt(); }
        A::erase_from_map_and_database(K);
    }
    for (size_t k = 0; k < nk; k++) {                                // the links as the library reports them: the replay above must have left the same
        if ((kfs[k]->GetPrevKeyFrame() ? kf_slot.find(kfs[k]->GetPrevKeyFrame()) : -1) != prev_out[k] || (kfs[k]->GetNextKeyFrame() ? kf_slot.find(kfs[k]->GetNextKeyFrame()) : -1) != next_out[k])
            throw std::runtime_error("remove_key_frames: the links differ from the library's report");
    }
}

// KeyFrame::SetBadFlag and KeyFrame::SetErase of one key frame
template <class MapPointT, class KeyFrameT>
inline void set_bad_flag(KeyFrameT* pKF) { remove_key_frames<KeyFrameT, MapPointT>(std::vector<KeyFrameT*>(1, pKF), std::vector<int>(1, 0)); }
template <class MapPointT, class KeyFrameT>
inline void set_erase(KeyFrameT* pKF) { remove_key_frames<KeyFrameT, MapPointT>(std::vector<KeyFrameT*>(1, pKF), std::vector<int>(1, 1)); }

} // namespace viorb_shim

#endif // VIORB_KEYFRAME_SHIM_H
