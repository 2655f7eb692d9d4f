// tests/cpp/global_ba_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for what viorb_shim::global_bundle_adjustment_navstate touches
// (include/Map.h, include/KeyFrame.h, include/MapPoint.h, src/IMU/NavState.h, src/IMU/IMUPreintegrator.h, Eigen / Sophus value types).
// Test scaffolding only.
#pragma once
#include <map>
#include <vector>
#include "cv_standin.h"

namespace standin {
struct Vec3 { double v[3]; Vec3(double x = 0, double y = 0, double z = 0) { v[0] = x; v[1] = y; v[2] = z; } double operator[](int i) const { return v[i]; } };
struct Quat { double w_, x_, y_, z_; Quat(double w = 1, double x = 0, double y = 0, double z = 0) : w_(w), x_(x), y_(y), z_(z) {}
              double x() const { return x_; } double y() const { return y_; } double z() const { return z_; } double w() const { return w_; } };
struct SO3 { Quat q; SO3() {} explicit SO3(const Quat& q_) : q(q_) {} const Quat& unit_quaternion() const { return q; } };
template <int R, int C> struct Mat { double m[R][C]; Mat() { for (auto& r : m) for (double& x : r) x = 0; } double& operator()(int r, int c) { return m[r][c]; } double operator()(int r, int c) const { return m[r][c]; } };
struct NavState {                                                                // src/IMU/NavState.h:17-60
    Vec3 P, V, bg, ba, dbg, dba; SO3 R;
    Vec3 Get_P() const { return P; } Vec3 Get_V() const { return V; } SO3 Get_R() const { return R; }
    Vec3 Get_BiasGyr() const { return bg; } Vec3 Get_BiasAcc() const { return ba; } Vec3 Get_dBias_Gyr() const { return dbg; } Vec3 Get_dBias_Acc() const { return dba; }
    void Set_Pos(const Vec3& x) { P = x; } void Set_Vel(const Vec3& x) { V = x; } void Set_Rot(const SO3& x) { R = x; }
    void Set_BiasGyr(const Vec3& x) { bg = x; } void Set_BiasAcc(const Vec3& x) { ba = x; } void Set_DeltaBiasGyr(const Vec3& x) { dbg = x; } void Set_DeltaBiasAcc(const Vec3& x) { dba = x; }
};
struct IMUPreintegrator {                                                        // src/IMU/IMUPreintegrator.h
    Vec3 dP, dV; Mat<3, 3> dR, JPg, JPa, JVg, JVa, JRg; Mat<9, 9> cov; double dt = 0;
    Vec3 getDeltaP() const { return dP; } Vec3 getDeltaV() const { return dV; } const Mat<3, 3>& getDeltaR() const { return dR; }
    const Mat<3, 3>& getJPBiasg() const { return JPg; } const Mat<3, 3>& getJPBiasa() const { return JPa; } const Mat<3, 3>& getJVBiasg() const { return JVg; }
    const Mat<3, 3>& getJVBiasa() const { return JVa; } const Mat<3, 3>& getJRBiasg() const { return JRg; } const Mat<9, 9>& getCovPVPhi() const { return cov; }
    double getDeltaTime() const { return dt; }
};
struct KeyFrame {                                                                // include/KeyFrame.h
    unsigned long mnId = 0, mnBAGlobalForKF = 0; bool bad = false; KeyFrame* prev = nullptr;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<cv::KeyPoint> mvKeysUn; std::vector<float> mvuRight, mvInvLevelSigma2;
    NavState ns, mNavStateGBA; cv::Mat mTcwGBA; IMUPreintegrator pre; int ns_sets = 0, pose_updates = 0;
    bool isBad() const { return bad; } KeyFrame* GetPrevKeyFrame() const { return prev; }
    const NavState& GetNavState() const { return ns; } void SetNavState(const NavState& x) { ns = x; ns_sets++; }
    void UpdatePoseFromNS(const cv::Mat&) { pose_updates++; } const IMUPreintegrator& GetIMUPreInt() const { return pre; }
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
