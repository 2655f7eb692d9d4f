// viorb_amd/csrc/global_ba_se3_core.h — what the vision-only global bundle adjustment (global_ba_se3.hip) shares between host and
// device: its limit, the argument predicates both forms apply, and the two binary edges from flat arrays.
//
// What is restated (reference file:line):
//   Optimizer::BundleAdjustment                          src/Optimizer.cc:3559-3747
// The SE3Quat algebra and the error of both edges (with the stereo projection's float reciprocal depth) are those of vio_core.h
// (se3_edge); the binary edges' Jacobians, the key-frame load / store and the Huber deltas those of ba_core.h, shared with the window
// solve; the Levenberg step that of global_ba_core.h.
#pragma once
#include "global_ba_core.h"

#define GBA_SE3_MAX_FREE_KF 4096       // documented limit: a reduced system of order 24576, as the NavState solve's

namespace viorb {

// the edge type's Huber delta; a stereo edge needs a baseline (VIORB_ERR_INVALID_ARG otherwise)
VIO_HD double gba_se3_delta(const double* obs4) { return ba_se3_stereo(obs4) ? ba_delta_stereo() : ba_delta_mono_map(); }
VIO_HD bool gba_se3_obs_ok(const double* obs4, double bf) { return !ba_se3_stereo(obs4) || bf > 0.0; }

// error e[3] (e[2] = 0 on a monocular edge); returns the edge's dimension
VIO_HD int gba_se3_error(const double* kf7, const double* pt3, const double* obs4, const double* intr5, double* e) {
    return se3_edge(se3_ld7(kf7), ld3(pt3), obs4[0], obs4[1], obs4[2], intr5[0], intr5[1], intr5[2], intr5[3], intr5[4], false, e, nullptr);
}
// both Jacobians of the edge (ba_se3_jac: the window solve's too)
VIO_HD void gba_se3_jac(const double* kf7, const double* pt3, const double* obs4, const double* intr5, double* Jp, double* Jk) {
    ba_se3_jac(se3_ld7(kf7), ld3(pt3), ba_se3_stereo(obs4), intr5[0], intr5[1], intr5[4], Jp, Jk);
}

} // namespace viorb
