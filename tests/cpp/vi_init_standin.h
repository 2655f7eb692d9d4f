// tests/cpp/vi_init_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for what viorb_shim::try_init_vio / try_init_vio_apply touch
// (include/KeyFrame.h, include/MapPoint.h, src/IMU/imudata.h, src/IMU/IMUPreintegrator.h, Eigen / Sophus value types). Test scaffolding only.
#pragma once
#include <vector>
#include "cv_standin.h"

namespace standin {
struct Vec3 { double v[3]; Vec3(double x = 0, double y = 0, double z = 0) { v[0] = x; v[1] = y; v[2] = z; } double operator[](int i) const { return v[i]; } };
struct Quat { double w_, x_, y_, z_; Quat(double w = 1, double x = 0, double y = 0, double z = 0) : w_(w), x_(x), y_(y), z_(z) {} };
struct SO3 { Quat q; SO3() {} explicit SO3(const Quat& q_) : q(q_) {} };
template <int R, int C> struct Mat { double m[R][C]; Mat() { for (auto& r : m) for (double& x : r) x = 0; } double& operator()(int r, int c) { return m[r][c]; } double operator()(int r, int c) const { return m[r][c]; } };
struct IMUData { Vec3 _g, _a; double _t = 0; };                                   // src/IMU/imudata.h:40-42
struct IMUPreintegrator {                                                        // src/IMU/IMUPreintegrator.h
    Vec3 dP, dV; Mat<3, 3> dR, JPg, JPa, JVg, JVa, JRg; Mat<9, 9> cov; double dt = 0;
    Vec3 getDeltaP() const { return dP; } Vec3 getDeltaV() const { return dV; } const Mat<3, 3>& getDeltaR() const { return dR; }
    const Mat<3, 3>& getJPBiasg() const { return JPg; } const Mat<3, 3>& getJPBiasa() const { return JPa; } const Mat<3, 3>& getJVBiasg() const { return JVg; }
    const Mat<3, 3>& getJVBiasa() const { return JVa; } const Mat<3, 3>& getJRBiasg() const { return JRg; } const Mat<9, 9>& getCovPVPhi() const { return cov; }
    double getDeltaTime() const { return dt; }
};
struct KeyFrame {                                                                // include/KeyFrame.h:56-105, 181
    double mTimeStamp = 0; cv::Mat Tcw, Twc; IMUPreintegrator pre; std::vector<IMUData> imu;
    Vec3 P, V, bg, ba, dbg, dba; SO3 R; int pose_sets = 0, ns_sets = 0;
    cv::Mat GetPose() const { return Tcw; } cv::Mat GetPoseInverse() const { return Twc; } void SetPose(const cv::Mat& T) { Tcw = T; pose_sets++; }
    const IMUPreintegrator& GetIMUPreInt() const { return pre; } std::vector<IMUData> GetVectorIMUData() const { return imu; }
    void SetNavStatePos(const Vec3& x) { P = x; ns_sets++; } void SetNavStateVel(const Vec3& x) { V = x; ns_sets++; } void SetNavStateRot(const SO3& x) { R = x; ns_sets++; }
    void SetNavStateBiasGyr(const Vec3& x) { bg = x; ns_sets++; } void SetNavStateBiasAcc(const Vec3& x) { ba = x; ns_sets++; }
    void SetNavStateDeltaBg(const Vec3& x) { dbg = x; ns_sets++; } void SetNavStateDeltaBa(const Vec3& x) { dba = x; ns_sets++; }
};
struct MapPoint {                                                                // src/MapPoint.cc:73-78
    float Pw[3] = {0, 0, 0}, mfMinDistance = 0, mfMaxDistance = 0;
    void UpdateScale(float scale) { for (float& x : Pw) x = x * scale; mfMaxDistance *= scale; mfMinDistance *= scale; }
};
}
