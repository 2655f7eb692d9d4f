// tests/cpp/essential_graph_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for what viorb_shim::optimize_essential_graph touches
// (include/Map.h, include/KeyFrame.h, include/MapPoint.h, include/LoopClosing.h, g2o::Sim3 as eight doubles). Test scaffolding only.
#pragma once
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>
#include "cv_standin.h"

namespace standin {
struct Sim3 { double v[8]; };                                                    // r(x y z w) t s
struct KeyFrame {                                                                // include/KeyFrame.h
    long unsigned int mnId = 0; bool bad = false;
    cv::Mat Rcw, tcw, Tcw, TcwNav; int pose_sets = 0, nav_updates = 0;
    KeyFrame* parent = nullptr; std::set<KeyFrame*> children, loop_edges;
    std::vector<std::pair<KeyFrame*, int> > covisibles;                          // ordered by weight in the reference; any order here
    std::map<KeyFrame*, int> weights;
    bool isBad() const { return bad; }
    cv::Mat GetRotation() const { return Rcw; } cv::Mat GetTranslation() const { return tcw; }
    KeyFrame* GetParent() const { return parent; } bool hasChild(KeyFrame* p) const { return children.count(p) != 0; }
    std::set<KeyFrame*> GetLoopEdges() const { return loop_edges; }
    std::vector<KeyFrame*> GetCovisiblesByWeight(const int& w) const { std::vector<KeyFrame*> o; for (size_t i = 0; i < covisibles.size(); i++) if (covisibles[i].second >= w) o.push_back(covisibles[i].first); return o; }
    int GetWeight(KeyFrame* p) const { std::map<KeyFrame*, int>::const_iterator it = weights.find(p); return it == weights.end() ? 0 : it->second; }
    void SetPose(const cv::Mat& T) { Tcw = T; pose_sets++; }
    void UpdateNavStatePVRFromTcw(const cv::Mat& T, const cv::Mat&) { TcwNav = T; nav_updates++; }
};
struct MapPoint {                                                                // include/MapPoint.h
    bool bad = false; cv::Mat Pw; long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0; KeyFrame* ref = nullptr; int pos_sets = 0, normal_updates = 0;
    bool isBad() const { return bad; } cv::Mat GetWorldPos() const { return Pw; } KeyFrame* GetReferenceKeyFrame() const { return ref; }
    void SetWorldPos(const cv::Mat& P) { Pw = P; pos_sets++; } void UpdateNormalAndDepth() { normal_updates++; }
};
struct Map {                                                                     // include/Map.h
    std::vector<KeyFrame*> kfs; std::vector<MapPoint*> pts; std::mutex mMutexMapUpdate;
    std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; } std::vector<MapPoint*> GetAllMapPoints() const { return pts; }
};
struct LoopClosing {                                                             // include/LoopClosing.h
    typedef std::map<KeyFrame*, Sim3> KeyFrameAndPose;
    int flag_sets = 0; bool flag = false;
    void SetMapUpdateFlagInTracking(bool b) { flag = b; flag_sets++; }
};
}
