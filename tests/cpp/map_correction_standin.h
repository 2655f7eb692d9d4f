// tests/cpp/map_correction_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for what viorb_shim::correct_loop_propagate and
// viorb_shim::apply_global_ba touch (include/KeyFrame.h, include/MapPoint.h, include/Map.h; g2o::Sim3 as eight doubles; NavState and the
// Eigen / Sophus types from global_ba_standin.h). Test scaffolding only.
#pragma once
#include <map>
#include <set>
#include <vector>
#include "global_ba_standin.h"         // cv_standin.h, standin::NavState, Vec3, Quat, SO3

namespace mcs {
struct Sim3 { double v[8]; };
struct MapPoint;
struct KeyFrame {
    long unsigned int mnId = 0, mnBAGlobalForKF = 0;
    int mnScaleLevels = 8; float mfScaleFactor = 1.2f; std::vector<float> mvScaleFactors; std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint*> mvpMapPoints; std::set<KeyFrame*> children;
    cv::Mat Tcw, mTcwGBA, mTcwBefGBA; standin::NavState ns, mNavStateGBA, mNavStateBefGBA; int pose_sets = 0;
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    std::set<KeyFrame*> GetChilds() const { return children; }
    cv::Mat GetPose() const { return Tcw; }
    void SetPose(const cv::Mat& T) { Tcw = T; pose_sets++; }
    const standin::NavState& GetNavState() const { return ns; }
    void SetNavState(const standin::NavState& n) { ns = n; }
};
struct MapPoint {
    bool bad = false; cv::Mat Pw, normal, mPosGBA; float mind = 0, maxd = 0; long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0, mnBAGlobalForKF = 0;
    std::map<KeyFrame*, size_t> mObservations; KeyFrame* ref = nullptr; int pos_sets = 0, normal_sets = 0;
    bool isBad() const { return bad; }
    cv::Mat GetWorldPos() const { return Pw; }
    void SetWorldPos(const cv::Mat& P) { Pw = P; pos_sets++; }
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
    KeyFrame* GetReferenceKeyFrame() const { return ref; }
    void SetNormalAndDepth(const cv::Mat& n, float a, float b) { normal = n; mind = a; maxd = b; normal_sets++; }
};
struct Map {
    std::vector<KeyFrame*> kfs, mvpKeyFrameOrigins; std::vector<MapPoint*> pts;
    std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; }
    std::vector<MapPoint*> GetAllMapPoints() const { return pts; }
};
}
