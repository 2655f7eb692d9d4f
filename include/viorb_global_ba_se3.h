/* include/viorb_global_ba_se3.h — the vision-only global bundle adjustment of the C ABI. Included by viorb.h (after the NavState global
 * solve, whose viorb_gba_config and viorb_debug_gba_last_trials it shares); include viorb.h, not this file. The ctypes mirror is
 * viorb_amd/capi.py: SIGNATURES_GLOBAL_BA_SE3. */
#ifndef VIORB_GLOBAL_BA_SE3_H
#define VIORB_GLOBAL_BA_SE3_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* Optimizer::GlobalBundleAdjustemnt / Optimizer::BundleAdjustment (reference src/Optimizer.cc:3551-3747, BlockSolver_6_3; called by
 * Tracking::CreateInitialMapMonocular, src/Tracking.cc:1420, by LoopClosing::RunGlobalBundleAdjustment without TRACK_WITH_IMU,
 * src/LoopClosing.cc:681, and the only full adjustment of the stereo / RGB-D pipeline): every key frame of the map as an SE3 pose, every
 * map point, monocular and stereo observations, in one solve. Vertices: a VertexSE3Expmap (6) per key frame, fixed where fixed[i] != 0
 * (the reference fixes mnId == 0, :3589; zero, one or several fixed key frames in any position are allowed); np marginalised points; a
 * point without an edge is left out and keeps its position (:3685-3693, point_included[p] = 0); a point seen only by fixed key frames
 * is a vertex and moves. Factors: per observation one EdgeSE3ProjectXYZ (uRight < 0) or EdgeStereoSE3ProjectXYZ (uRight >= 0)
 * (Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:103-250) with information invSigma2 I. cfg->robust (bRobust): Huber sqrt(5.99) on
 * the monocular and sqrt(7.815) on the stereo edges, each delta a float squared in double (:3595-3596); without it chi2 is the plain
 * sum. Solver: ONE optimize(cfg->iterations) of g2o's Levenberg with the point block eliminated, as viorb_global_ba_navstate: no
 * classification round, no erase list, no depth gate. stop: pbStopFlag (may be NULL), polled before every iteration and after every
 * trial; raised before the call, the inputs come back unchanged with info[2] = 0 and point_included filled.
 * kfs [nk][7] = qx qy qz qw tx ty tz of Tcw (Converter::toSE3Quat, as viorb_local_ba_se3), points [np][3], edge_idx [ne][2] = (point,
 * key frame) sorted by point, edge_obs [ne][4] = u v uRight invSigma2, intr5 = fx fy cx cy bf. Outputs: kfs_out [nk][7] (fixed rows
 * copied), points_out [np][3], point_included [np], info as viorb_global_ba_navstate; viorb_debug_gba_last_trials reports this solve too.
 * VIORB_ERR_INVALID_ARG: an edge index out of range, edges not sorted by point, invSigma2 <= 0, a stereo edge with bf <= 0.
 * VIORB_ERR_CAPACITY: more than 4096 free key frames (a reduced system of order 24576), or a workspace that is too small; never a
 * truncated solve. FP64 on the calling thread's current HIP device; the host form is re-entrant. */
size_t viorb_global_ba_se3_workspace_bytes(int nk, int np, int ne);
int viorb_global_ba_se3(const viorb_gba_config* cfg, const double* kfs, int nk, const uint8_t* fixed, const double* points, int np,
                        const int32_t* edge_idx, const double* edge_obs, int ne, const double intr5[5], const volatile int* stop,
                        double* kfs_out, double* points_out, uint8_t* point_included, double info[6]);
/* The same with the arrays in device memory (kfs_out / points_out are the working states and must not alias the inputs); cfg, intr5,
 * stop and info are host pointers. workspace: viorb_global_ba_se3_workspace_bytes(nk, np, ne) bytes of device memory; its
 * contents on entry are ignored. */
int viorb_global_ba_se3_device(const viorb_gba_config* cfg, const double* kfs, int nk, const uint8_t* fixed, const double* points, int np,
                               const int32_t* edge_idx, const double* edge_obs, int ne, const double intr5[5], const volatile int* stop,
                               double* kfs_out, double* points_out, uint8_t* point_included, double info[6], void* workspace,
                               size_t workspace_bytes, void* stream);
/* Test hook (no device): one edge of the solve above from global_ba_se3_core.h compiled for the host. e3, Jp9 = d e / d point [3][3],
 * Jk18 = d e / d (omega, upsilon) [3][6], the third rows zero on a monocular edge; returns the edge's dimension (2 or 3). */
int viorb_debug_gba_se3_edge(const double* kf7, const double* pt3, const double* obs4, const double* intr5, double* e3, double* Jp9,
                             double* Jk18);

#endif /* VIORB_GLOBAL_BA_SE3_H */
