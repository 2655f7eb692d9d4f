// tests/cpp/mapping_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for the KeyFrame / MapPoint members that
// viorb_amd/shim/LocalMapping_shim.h touches (include/KeyFrame.h, include/MapPoint.h, DBoW2's FeatureVector). Test scaffolding only.
#pragma once
#include <map>
#include <vector>
#include "cv_standin.h"

namespace standin {
struct FeatureVector : std::map<unsigned, std::vector<unsigned> > { void addFeature(unsigned id, unsigned i) { (*this)[id].push_back(i); } };
struct MapPoint;
struct KeyFrame {
    int N = 0; bool bad = false;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn; std::vector<float> mvuRight, mvDepth; cv::Mat mDescriptors, Tcw, Ow;
    FeatureVector mFeatVec; std::vector<MapPoint*> mps;
    float fx = 0, fy = 0, cx = 0, cy = 0, mb = 0, mbf = 0, mfScaleFactor = 1.2f;
    std::vector<float> mvScaleFactors, mvLevelSigma2; int mnScaleLevels = 8;
    MapPoint* GetMapPoint(size_t i) const { return mps[i]; }
    void AddMapPoint(MapPoint* p, size_t i) { mps[i] = p; }
    cv::Mat GetPose() const { return Tcw; }
    cv::Mat GetCameraCenter() const { return Ow; }
    bool isBad() const { return bad; }
};
struct MapPoint {
    cv::Mat Pw, Pn, desc; bool bad = false; float minD = 0, maxD = 0; KeyFrame* ref = nullptr; int updates = 0;
    std::map<KeyFrame*, size_t> obs;
    MapPoint() : Pw(3, 1, CV_32F), Pn(3, 1, CV_32F), desc(1, 32, CV_8U) {}
    cv::Mat GetWorldPos() const { return Pw; }
    bool isBad() const { return bad; }
    std::map<KeyFrame*, size_t> GetObservations() const { return obs; }
    KeyFrame* GetReferenceKeyFrame() const { return ref; }
    void AddObservation(KeyFrame* k, size_t i) { obs[k] = i; }
    void SetDescriptorNormalAndDepth(const cv::Mat& d, const cv::Mat& n, float mn, float mx) { desc = d; Pn = n; minD = mn; maxD = mx; updates++; }   // the accessor the shim asks for
};
}
