// tests/cpp/global_ba_se3_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for what viorb_shim::bundle_adjustment /
// global_bundle_adjustment touch (include/Map.h, include/KeyFrame.h, include/MapPoint.h). Test scaffolding only.
#pragma once
#include <map>
#include <vector>
#include "cv_standin.h"

namespace standin {
struct KeyFrame {                                                                // include/KeyFrame.h
    unsigned long mnId = 0, mnBAGlobalForKF = 0; bool bad = false;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    std::vector<cv::KeyPoint> mvKeysUn; std::vector<float> mvuRight, mvInvLevelSigma2;
    cv::Mat Tcw, mTcwGBA; int pose_sets = 0;
    bool isBad() const { return bad; }
    cv::Mat GetPose() const { return Tcw; } void SetPose(const cv::Mat& T) { Tcw = T; pose_sets++; }
};
struct MapPoint {                                                                // include/MapPoint.h
    unsigned long mnId = 0, mnBAGlobalForKF = 0; bool bad = false; cv::Mat Pw, mPosGBA; std::map<KeyFrame*, size_t> obs; int pos_sets = 0, normal_updates = 0;
    bool isBad() const { return bad; } cv::Mat GetWorldPos() const { return Pw; } std::map<KeyFrame*, size_t> GetObservations() const { return obs; }
    void SetWorldPos(const cv::Mat& P) { Pw = P; pos_sets++; } void UpdateNormalAndDepth() { normal_updates++; }
};
struct Map {                                                                     // include/Map.h
    std::vector<KeyFrame*> kfs; std::vector<MapPoint*> pts;
    std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; } std::vector<MapPoint*> GetAllMapPoints() const { return pts; }
};
}
