// tests/cpp/sim3_match_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for the KeyFrame / MapPoint members that the three Sim3
// matcher templates of viorb_amd/shim/ORBmatcher_shim.h touch (include/KeyFrame.h, include/MapPoint.h), ONLY to compile and run them in
// an image without OpenCV. Not part of the product.
#pragma once
#include <map>
#include <set>
#include <utility>
#include <vector>
#include "cv_standin.h"

namespace standin {
struct KeyFrame;
struct MapPoint {
    int id = -1; cv::Mat mWorldPos, mNormalVector, mDescriptor; bool mbBad = false; float mfMinDistance = 0, mfMaxDistance = 0;
    std::map<KeyFrame*, size_t> mObservations;
    std::vector<std::pair<KeyFrame*, size_t> > added;                  // every AddObservation call, in order
    MapPoint() : mWorldPos(3, 1, CV_32F), mNormalVector(3, 1, CV_32F), mDescriptor(1, 32, CV_8U) {}
    bool isBad() const { return mbBad; }
    cv::Mat GetWorldPos() const { return mWorldPos; }
    cv::Mat GetNormal() const { return mNormalVector; }
    cv::Mat GetDescriptor() const { return mDescriptor; }
    float GetMinDistance() const { return mfMinDistance; }             // the two accessors ORBmatcher_shim.h asks for
    float GetMaxDistance() const { return mfMaxDistance; }
    int GetIndexInKeyFrame(KeyFrame* kf) const { auto it = mObservations.find(kf); return it == mObservations.end() ? -1 : (int)it->second; }
    void AddObservation(KeyFrame* kf, size_t idx) { mObservations[kf] = idx; added.push_back(std::make_pair(kf, idx)); }
};
struct KeyFrame {
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn; cv::Mat mDescriptors, mRcw, mtcw;
    float fx = 0, fy = 0, cx = 0, cy = 0, mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
    int mnScaleLevels = 8; std::vector<float> mvScaleFactors;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    std::set<MapPoint*> GetMapPoints() const {
        std::set<MapPoint*> s;
        for (MapPoint* p : mvpMapPoints) if (p && !p->isBad()) s.insert(p);
        return s;
    }
    MapPoint* GetMapPoint(size_t i) const { return mvpMapPoints[i]; }
    void AddMapPoint(MapPoint* p, size_t i) { mvpMapPoints[i] = p; }
    cv::Mat GetRotation() const { return mRcw; }
    cv::Mat GetTranslation() const { return mtcw; }
};
}
