// tests/cpp/reloc_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for the Frame / KeyFrame / MapPoint members that the
// relocalisation templates of viorb_amd/shim (relocalization_refine, search_by_projection_reloc) touch (include/Frame.h, include/KeyFrame.h,
// include/MapPoint.h), ONLY to compile and run them in an image without OpenCV. Not part of the product.
#pragma once
#include <vector>
#include "cv_standin.h"

namespace standin {
struct MapPoint {
    int id = -1; cv::Mat mWorldPos, mDescriptor; bool mbBad = false; float mfMinDistance = 0, mfMaxDistance = 0;
    MapPoint() : mWorldPos(3, 1, CV_32F), mDescriptor(1, 32, CV_8U) {}
    bool isBad() const { return mbBad; }
    cv::Mat GetWorldPos() const { return mWorldPos; }
    cv::Mat GetDescriptor() const { return mDescriptor; }
    float GetMinDistance() const { return mfMinDistance; }
    float GetMaxDistance() const { return mfMaxDistance; }
};
struct KeyFrame {
    std::vector<cv::KeyPoint> mvKeysUn; std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
};
struct Frame {
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn; cv::Mat mDescriptors, mTcw; std::vector<float> mvuRight;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
    int mnScaleLevels = 8; std::vector<float> mvScaleFactors, mvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints; std::vector<bool> mvbOutlier;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw; }
};
}
