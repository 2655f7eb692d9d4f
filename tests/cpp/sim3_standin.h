// tests/cpp/sim3_standin.h — stand-ins for what viorb_amd/shim/Sim3Solver_shim.h reads of the reference's KeyFrame and MapPoint, and for
// the two cv::Mat operators its constructor uses (a 3 x 3 by 3 x 1 product and a sum, float products summed left to right as OpenCV's
// small-matrix path does), ONLY to compile and run the shim in an image without OpenCV. Not part of the product.
#pragma once
#include <map>
#include <vector>
#include "cv_standin.h"
namespace cv {
inline Mat operator*(const Mat& A, const Mat& B) {
    Mat C(A.rows, B.cols, CV_32F);
    for (int r = 0; r < A.rows; r++)
        for (int c = 0; c < B.cols; c++) {
            float s = A.at<float>(r, 0) * B.at<float>(0, c);
            for (int k = 1; k < A.cols; k++) s += A.at<float>(r, k) * B.at<float>(k, c);
            C.at<float>(r, c) = s;
        }
    return C;
}
inline Mat operator+(const Mat& A, const Mat& B) {
    Mat C(A.rows, A.cols, CV_32F);
    for (int i = 0; i < A.rows * A.cols; i++) C.at<float>(i) = A.at<float>(i) + B.at<float>(i);
    return C;
}
}
namespace standin {
struct Sim3 { double v[8]; };                 // stands for g2o::Sim3: r(x y z w) t s
struct KeyFrame;
struct MapPoint {
    cv::Mat mWorldPos; bool mbBad = false; std::map<const KeyFrame*, int> mObservations;
    bool isBad() const { return mbBad; }
    int GetIndexInKeyFrame(const KeyFrame* kf) const { auto it = mObservations.find(kf); return it == mObservations.end() ? -1 : it->second; }
    cv::Mat GetWorldPos() const { return mWorldPos; }
};
struct KeyFrame {
    std::vector<cv::KeyPoint> mvKeysUn; std::vector<float> mvLevelSigma2, mvInvLevelSigma2; cv::Mat mK, mRcw, mtcw; std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    cv::Mat GetRotation() const { return mRcw; }
    cv::Mat GetTranslation() const { return mtcw; }
};
}
