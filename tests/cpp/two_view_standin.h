// tests/cpp/two_view_standin.h — stand-ins for what viorb_amd/shim/Initializer_shim.h reads of the reference's Frame (mvKeysUn, mK) and
// for cv::Point3f, ONLY to compile and run the shim in an image without OpenCV. Not part of the product.
#pragma once
#include <vector>
#include "cv_standin.h"
namespace cv {
struct Point3f { float x, y, z; Point3f(float a = 0, float b = 0, float c = 0) : x(a), y(b), z(c) {} };
}
namespace standin {
struct Frame {
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mK;
};
}
