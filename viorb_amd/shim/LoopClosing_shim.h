// viorb_amd/shim/LoopClosing_shim.h — reference-side glue for the map correction (include/viorb_map_correction.h): function templates over
// the reference's KeyFrame / MapPoint / Map. Like the other shims this header includes none of the reference's headers; it is compiled
// inside the reference tree, after them (INTEGRATION.md shows the one-line bodies at the call sites).
//   LoopClosing::CorrectLoop, src/LoopClosing.cc:473-495 and :498-542 without the UpdateConnections() line:
//       viorb_shim::correct_loop_propagate<KeyFrame, MapPoint>(mpCurrentKF, mvpCurrentConnectedKFs, mg2oScw, CorrectedSim3, NonCorrectedSim3,
//                                                              sim3_get, sim3_set, to_pose);
//       for (KeyFrameAndPose::iterator mit = CorrectedSim3.begin(); mit != CorrectedSim3.end(); mit++) mit->first->UpdateConnections();
//     The caller runs UpdateConnections over CorrectedSim3 in its order afterwards (or update_connections_loop of KeyFrame_shim.h);
//     :546-561 (Replace / AddMapPoint) stays the reference's.
//   LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:712-803, and LocalMapping::TryInitVIO, src/LocalMapping.cc:824-916:
//       viorb_shim::apply_global_ba<KeyFrame, MapPoint, NavState, Vector3d, Eigen::Quaterniond, Sophus::SO3>(mpMap, nLoopKF, cvTbc, to_pose);
// sim3_get(const Sim3&, double[8]) gives r(x y z w) t s of a g2o::Sim3, sim3_set(const double[8]) builds one, to_pose(const float[12]) is
// a 4 x 4 CV_32F cv::Mat of R (row-major) and t. Both templates throw on any error of the library, flatten with SlotTable and
// std::less<KeyFrame*>, and leave locks (mMutexMapUpdate) and thread hand-shakes with the caller. MapPoint needs the accessor
// SetDescriptorNormalAndDepth's sibling
//   void SetNormalAndDepth(const cv::Mat& normal, float minDist, float maxDist)      (mNormalVector, mfMinDistance, mfMaxDistance under mMutexPos)
// and KeyFrame, for apply_global_ba, public access to mTcwGBA, mTcwBefGBA, mNavStateGBA, mNavStateBefGBA, mnBAGlobalForKF (they are public
// in the reference), SetNavState and SetPose.
#ifndef VIORB_LOOPCLOSING_SHIM_H
#define VIORB_LOOPCLOSING_SHIM_H

#include "viorb_tracking_shim.h"       // check, SlotTable, pack_navstate, unpack_navstate

namespace viorb_shim {

template <class KeyFrameT> inline std::vector<int32_t> slots_by_key(const std::vector<KeyFrameT*>& kfs) {
    std::vector<std::pair<KeyFrameT*, int32_t> > by_ptr;
    for (size_t k = 0; k < kfs.size(); k++) by_ptr.push_back(std::make_pair(kfs[k], (int32_t)k));
    struct Less { bool operator()(const std::pair<KeyFrameT*, int32_t>& a, const std::pair<KeyFrameT*, int32_t>& b) const { return std::less<KeyFrameT*>()(a.first, b.first); } };
    std::sort(by_ptr.begin(), by_ptr.end(), Less());
    std::vector<int32_t> out(kfs.size());
    for (size_t j = 0; j < kfs.size(); j++) out[j] = by_ptr[j].second;
    return out;
}
inline void pose12_of(const cv::Mat& T, float* o) {
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o[3 * r + c] = T.at<float>(r, c); o[9 + r] = T.at<float>(r, 3); }
}

// The snapshot holds the members (the covisibles and the current key frame), the points they hold, and the observers and reference key
// frames of those points. Written back: CorrectedSim3 / NonCorrectedSim3; for every corrected point SetWorldPos, mnCorrectedByKF,
// mnCorrectedReference and, where it has observations, SetNormalAndDepth; SetPose of every member, in CorrectedSim3's order.
template <class KeyFrameT, class MapPointT, class Sim3T, class KeyFrameAndPoseT, class GetS, class SetS, class ToPose>
inline void correct_loop_propagate(KeyFrameT* pCurKF, const std::vector<KeyFrameT*>& vpCurrentConnectedKFs, const Sim3T& g2oScw, KeyFrameAndPoseT& CorrectedSim3,
                                   KeyFrameAndPoseT& NonCorrectedSim3, GetS sim3_get, SetS sim3_set, ToPose to_pose) {
    SlotTable<KeyFrameT> kf_slot; const std::vector<KeyFrameT*>& kfs = kf_slot.items;
    SlotTable<MapPointT> pt_slot; const std::vector<MapPointT*>& pts = pt_slot.items;
    std::vector<int32_t> conn_kf;
    for (size_t i = 0; i < vpCurrentConnectedKFs.size(); i++) if (vpCurrentConnectedKFs[i] != pCurKF) conn_kf.push_back(kf_slot.add(vpCurrentConnectedKFs[i]));      // :462 appended it
    const int32_t cur_kf = kf_slot.add(pCurKF);
    const size_t n_members = kfs.size();
    std::vector<int32_t> kp_start(1, 0), kp_point, obs_start(1, 0), pt_ref, pt_by;
    std::vector<uint32_t> obs; std::vector<uint8_t> pt_bad; std::vector<float> pts_f;
    for (size_t k = 0; k < n_members; k++) {
        const std::vector<MapPointT*> vpMP = kfs[k]->GetMapPointMatches();
        for (size_t i = 0; i < vpMP.size(); i++) {
            MapPointT* pMP = vpMP[i];
            if (!pMP) { kp_point.push_back(-1); continue; }
            const size_t before = pts.size();
            kp_point.push_back(pt_slot.add(pMP));
            if (pts.size() == before) continue;
            pt_bad.push_back(pMP->isBad() ? 1 : 0);
            pt_by.push_back((int32_t)pMP->mnCorrectedByKF);
            int32_t ref = -1;
            float P8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (!pt_bad.back()) {
                const cv::Mat Pw = pMP->GetWorldPos();
                for (int c = 0; c < 3; c++) P8[c] = Pw.at<float>(c);
                const std::map<KeyFrameT*, size_t> observations = pMP->GetObservations();
                for (typename std::map<KeyFrameT*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it)
                    obs.push_back((uint32_t)kf_slot.add(it->first) | ((uint32_t)(it->first->mvKeysUn[it->second].octave & 0xff) << 16));
                if (!observations.empty()) ref = kf_slot.add(pMP->GetReferenceKeyFrame());
            }
            pts_f.insert(pts_f.end(), P8, P8 + 8); pt_ref.push_back(ref);
            obs_start.push_back((int32_t)obs.size());
        }
        kp_start.push_back((int32_t)kp_point.size());
    }
    const size_t nk = kfs.size(), np = pts.size(), nm = conn_kf.size() + 1;
    if (nk > 65535) throw std::runtime_error("CorrectLoop: more than 65535 key frames in the snapshot");
    kp_start.resize(nk + 1, (int32_t)kp_point.size());
    std::vector<float> pose12(nk * 12);
    for (size_t k = 0; k < nk; k++) pose12_of(kfs[k]->GetPose(), &pose12[k * 12]);
    const std::vector<int32_t> kf_by_key = slots_by_key(kfs);
    double Scw8[8];
    sim3_get(g2oScw, Scw8);
    viorb_mapping_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.nlevels = pCurKF->mnScaleLevels; cam.scale_factor = pCurKF->mfScaleFactor;
    for (int i = 0; i < 16 && i < cam.nlevels; i++) cam.scale_factors[i] = pCurKF->mvScaleFactors[i];
    viorb_correct_loop_map m;
    m.batch = 1; m.n_kf = (int32_t)nk; m.n_kp = (int32_t)kp_point.size(); m.n_pt = (int32_t)np; m.n_obs = (int32_t)obs.size(); m.n_conn = (int32_t)conn_kf.size();
    // every array at least one element long: the library refuses a null pointer whatever the count
    kp_point.resize(std::max<size_t>(kp_point.size(), 1), -1); pt_bad.resize(std::max<size_t>(np, 1), 0); obs.resize(std::max<size_t>(obs.size(), 1)); pts_f.resize(std::max<size_t>(np, 1) * 8);
    pt_ref.resize(std::max<size_t>(np, 1), -1); pt_by.resize(std::max<size_t>(np, 1), 0); conn_kf.resize(std::max<size_t>(conn_kf.size(), 1));
    const int32_t kf_start[2] = {0, (int32_t)nk}, pt_start[2] = {0, (int32_t)np}, conn_start[2] = {0, m.n_conn}, cur_id = (int32_t)pCurKF->mnId;
    m.kf_start = kf_start; m.kf_by_key = &kf_by_key[0]; m.kp_start = &kp_start[0]; m.kp_point = &kp_point[0]; m.pt_start = pt_start; m.pt_bad = &pt_bad[0];
    m.obs_start = &obs_start[0]; m.obs = &obs[0]; m.pose12 = &pose12[0]; m.pts_f = &pts_f[0]; m.pt_ref = &pt_ref[0]; m.pt_corrected_by = &pt_by[0];
    m.cur_kf = &cur_kf; m.cur_id = &cur_id; m.Scw8 = Scw8; m.conn_start = conn_start; m.conn_kf = &conn_kf[0];
    int32_t status = 0, n_member = 0;
    std::vector<int32_t> member_kf(nm), by_out(std::max<size_t>(np, 1)), ref_out(by_out.size());
    std::vector<float> f12(nm * 12), pose_out(nk * 12), Ow(nk * 3), pts_out(by_out.size() * 8);
    std::vector<double> Scw(nk * 8), Smeas(nk * 8); std::vector<uint8_t> touched(by_out.size());
    viorb_correct_loop_result r;
    r.status = &status; r.n_member = &n_member; r.member_kf = &member_kf[0]; r.Scw_f12 = &f12[0]; r.Scw_out = &Scw[0]; r.Smeas_out = &Smeas[0]; r.pose12_out = &pose_out[0];
    r.Ow_out = &Ow[0]; r.pts_f_out = &pts_out[0]; r.pt_corrected_by_out = &by_out[0]; r.pt_corrected_ref_out = &ref_out[0]; r.pt_touched = &touched[0];
    check(viorb_correct_loop(&m, &cam, &r), "CorrectLoop");
    if (status != VIORB_OK) throw std::runtime_error("CorrectLoop: the library refused the snapshot");
    for (int32_t j = 0; j < n_member; j++) {
        KeyFrameT* pKF = kfs[member_kf[j]];
        CorrectedSim3[pKF] = sim3_set(&Scw[(size_t)member_kf[j] * 8]);
        NonCorrectedSim3[pKF] = sim3_set(&Smeas[(size_t)member_kf[j] * 8]);
    }
    for (size_t p = 0; p < np; p++) {
        if (!touched[p]) continue;
        cv::Mat Pw(3, 1, CV_32F), nrm(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) { Pw.at<float>(c) = pts_out[p * 8 + c]; nrm.at<float>(c) = pts_out[p * 8 + 3 + c]; }
        pts[p]->SetWorldPos(Pw);
        pts[p]->mnCorrectedByKF = pCurKF->mnId;
        pts[p]->mnCorrectedReference = kfs[ref_out[p]]->mnId;
        if (obs_start[p + 1] > obs_start[p]) pts[p]->SetNormalAndDepth(nrm, pts_out[p * 8 + 6], pts_out[p * 8 + 7]);
    }
    for (int32_t j = 0; j < n_member; j++) kfs[member_kf[j]]->SetPose(to_pose(&pose_out[(size_t)member_kf[j] * 12]));
}

// The map update after a global bundle adjustment. The snapshot holds every key frame of the map (and whatever the origins and child sets
// name beside them) and every map point. Written back for the key frames the walk reached: mTcwGBA, mNavStateGBA, mnBAGlobalForKF,
// mTcwBefGBA, mNavStateBefGBA, SetNavState, SetPose; for the points whose position changed: SetWorldPos.
template <class KeyFrameT, class MapPointT, class NavStateT, class Vec3, class Quat, class SO3T, class MapT, class ToPose>
inline void apply_global_ba(MapT* pMap, unsigned long nLoopKF, const cv::Mat& cvTbc, ToPose to_pose) {
    SlotTable<KeyFrameT> kf_slot; const std::vector<KeyFrameT*>& kfs = kf_slot.items;
    const std::vector<KeyFrameT*> all = pMap->GetAllKeyFrames();
    for (size_t i = 0; i < all.size(); i++) kf_slot.add(all[i]);
    std::vector<int32_t> origin_kf, child_start(1, 0), child_kf;
    for (size_t i = 0; i < pMap->mvpKeyFrameOrigins.size(); i++) origin_kf.push_back(kf_slot.add(pMap->mvpKeyFrameOrigins[i]));
    for (size_t k = 0; k < kfs.size(); k++) {                           // kfs grows while the children are added
        const std::set<KeyFrameT*> sChilds = kfs[k]->GetChilds();
        for (typename std::set<KeyFrameT*>::const_iterator it = sChilds.begin(); it != sChilds.end(); ++it) child_kf.push_back(kf_slot.add(*it));
        child_start.push_back((int32_t)child_kf.size());
    }
    const std::vector<MapPointT*> pts = pMap->GetAllMapPoints();
    const size_t nk = kfs.size(), np = pts.size();
    if (nk == 0) return;
    if (nk > 65535) throw std::runtime_error("apply_global_ba: more than 65535 key frames in the map");
    std::vector<uint8_t> in_gba(nk), pt_bad(std::max<size_t>(np, 1), 0), pt_in(pt_bad.size(), 0);
    std::vector<float> pose12(nk * 12), gba12(nk * 12, 0.f), Pw(pt_bad.size() * 3, 0.f), PosGBA(Pw.size(), 0.f);
    std::vector<double> ns(nk * 22), nsg(nk * 22); std::vector<int32_t> pt_ref(pt_bad.size(), 0);
    for (size_t k = 0; k < nk; k++) {
        in_gba[k] = kfs[k]->mnBAGlobalForKF == nLoopKF ? 1 : 0;
        pose12_of(kfs[k]->GetPose(), &pose12[k * 12]);
        pack_navstate(kfs[k]->GetNavState(), &ns[k * 22]);
        pack_navstate(kfs[k]->mNavStateGBA, &nsg[k * 22]);
        if (!kfs[k]->mTcwGBA.empty()) pose12_of(kfs[k]->mTcwGBA, &gba12[k * 12]);
    }
    for (size_t p = 0; p < np; p++) {
        pt_bad[p] = pts[p]->isBad() ? 1 : 0;
        if (pt_bad[p]) continue;
        pt_in[p] = pts[p]->mnBAGlobalForKF == nLoopKF ? 1 : 0;
        const cv::Mat P = pts[p]->GetWorldPos();
        for (int c = 0; c < 3; c++) Pw[p * 3 + c] = P.at<float>(c);
        if (pt_in[p]) { for (int c = 0; c < 3; c++) PosGBA[p * 3 + c] = pts[p]->mPosGBA.template at<float>(c); continue; }
        const int ref = kf_slot.find(pts[p]->GetReferenceKeyFrame());
        if (ref < 0) throw std::runtime_error("apply_global_ba: a point's reference key frame is not in the map");
        pt_ref[p] = ref;
    }
    float Tbc12[12];
    pose12_of(cvTbc, Tbc12);
    viorb_apply_gba_map m;
    m.batch = 1; m.n_kf = (int32_t)nk; m.n_child = (int32_t)child_kf.size(); m.n_origin = (int32_t)origin_kf.size(); m.n_pt = (int32_t)np;
    child_kf.resize(std::max<size_t>(child_kf.size(), 1)); origin_kf.resize(std::max<size_t>(origin_kf.size(), 1));
    const int32_t kf_start[2] = {0, (int32_t)nk}, pt_start[2] = {0, (int32_t)np}, origin_start[2] = {0, m.n_origin};
    m.kf_start = kf_start; m.child_start = &child_start[0]; m.child_kf = &child_kf[0]; m.origin_start = origin_start; m.origin_kf = &origin_kf[0]; m.kf_in_gba = &in_gba[0];
    m.pose12 = &pose12[0]; m.TcwGBA12 = &gba12[0]; m.ns22 = &ns[0]; m.nsGBA22 = &nsg[0]; m.pt_start = pt_start; m.pt_bad = &pt_bad[0]; m.pt_in_gba = &pt_in[0];
    m.Pw = &Pw[0]; m.PosGBA = &PosGBA[0]; m.pt_ref = &pt_ref[0];
    int32_t status = 0;
    std::vector<float> pose_out(nk * 12), bef(nk * 12), gba_out(nk * 12), Pw_out(Pw.size());
    std::vector<double> ns_out(nk * 22), ns_bef(nk * 22), nsg_out(nk * 22); std::vector<uint8_t> flag(nk), reached(nk), code(pt_bad.size());
    viorb_apply_gba_result r;
    r.status = &status; r.pose12_out = &pose_out[0]; r.ns22_out = &ns_out[0]; r.TcwBef_out = &bef[0]; r.nsBef_out = &ns_bef[0]; r.TcwGBA_out = &gba_out[0]; r.nsGBA_out = &nsg_out[0];
    r.kf_in_gba_out = &flag[0]; r.kf_reached = &reached[0]; r.Pw_out = &Pw_out[0]; r.pt_code = &code[0];
    check(viorb_apply_global_ba(&m, Tbc12, &r), "apply_global_ba");
    if (status != VIORB_OK) throw std::runtime_error("apply_global_ba: the library refused the map");
    for (size_t k = 0; k < nk; k++) {
        if (!reached[k]) continue;
        KeyFrameT* pKF = kfs[k];
        if (flag[k] && !in_gba[k]) { pKF->mTcwGBA = to_pose(&gba_out[k * 12]); pKF->mnBAGlobalForKF = nLoopKF; unpack_navstate<NavStateT, Vec3, Quat, SO3T>(&nsg_out[k * 22], pKF->mNavStateGBA); }
        pKF->mTcwBefGBA = to_pose(&bef[k * 12]);
        pKF->mNavStateBefGBA = pKF->GetNavState();
        pKF->SetNavState(pKF->mNavStateGBA);
        pKF->SetPose(to_pose(&pose_out[k * 12]));                        // what UpdatePoseFromNS(cvTbc) computes
    }
    for (size_t p = 0; p < np; p++) {
        if (code[p] != VIORB_AGBA_PT_POS_GBA && code[p] != VIORB_AGBA_PT_BY_REF) continue;
        cv::Mat P(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) P.at<float>(c) = Pw_out[p * 3 + c];
        pts[p]->SetWorldPos(P);
    }
}

} // namespace viorb_shim

#endif // VIORB_LOOPCLOSING_SHIM_H
