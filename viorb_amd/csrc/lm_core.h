// viorb_amd/csrc/lm_core.h — g2o's Levenberg control, written once for the solver loops ("Where the Levenberg rule
// lives"): gba_run (global_ba.hip), lba_lambda0 / lba_decide (lba_ctl.h: both drivers of the window solves in local_ba.hip),
// k_pose_opt_vi_mp (pose_opt_mp.inc), k_pose_opt_se3 (frontend_kernels.hip), k_sim3_optimize (sim3.hip). Host and device
// (VIO_HD), no state: every function takes and returns scalars, because the sites keep lambda / ni / chi2 / the counters in a host
// struct, in a control block of doubles, in LDS words or in registers. The library is built with -ffp-contract=off and everything here
// is inlined, so an expression rounds here exactly as it did at the site it was copied from. Where the state is stored, barriers, the
// restore of a rejected trial, the stop flags, the round schedules and the summation of `scale` stay at the sites.
//
// What is restated (reference file:line):
//   OptimizationAlgorithmLevenberg::solve               Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:85-161
//   OptimizationAlgorithmLevenberg::computeLambdaInit   Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:166-180
#pragma once
#include "vio_core.h"

#define LM_TAU 1e-5                       // _tau
#define LM_GOOD_STEP_LOWER_SCALE (1. / 3.) // _goodStepLowerScale
#define LM_GOOD_STEP_UPPER_SCALE (2. / 3.) // _goodStepUpperScale
#define LM_MAX_TRIALS_AFTER_FAILURE 10    // _maxTrialsAfterFailure

namespace viorb {

// lambda_0 from the largest diagonal entry of the system (:166-180; no user lambda)
VIO_HD double lm_lambda_init(double max_diag) { return LM_TAU * max_diag; }
// chi2 of a trial: "if (! ok2) tempChi = std::numeric_limits<double>::max()" (:126-127)
VIO_HD double lm_trial_chi2(bool solved, double chi) { return solved ? chi : 1.7976931348623157e308; }
// rho = (currentChi - tempChi) / (computeScale() + 1e-3) (:129-132); scale = sum_j x_j (lambda x_j + b_j), summed by the site
VIO_HD double lm_rho(double currentChi, double tempChi, double scale) { scale += 1e-3; return (currentChi - tempChi) / scale; }
// "if (rho > 0 && g2o_isfinite(tempChi))": the trial state stays (:134)
VIO_HD bool lm_accepted(double rho, double tempChi) { return rho > 0 && isfinite(tempChi); }
// (2 rho - 1)^3 of the good-step factor, in two spellings that differ in the last bit: over 2 000 000 rho uniform in (0, 1.5) on the
// host (g++ -O2 -ffp-contract=off) the two cubes differ in 514 512 draws and the factor below in 23 034 (1.2 %). Each site keeps the
// spelling it had, so no solve changes; unifying them would (DESIGN.md lists it as open).
VIO_HD double lm_cube_pow(double t) { return pow(t, 3); }   // as g2o spells it: gba_run, k_pose_opt_se3, k_sim3_optimize
VIO_HD double lm_cube_mul(double t) { return t * t * t; }   // lba_decide, k_pose_opt_vi_mp
// an accepted trial (:135-141): lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), ni = 2; cube = lm_cube_pow / lm_cube_mul (2 * rho - 1)
VIO_HD void lm_good_step(double& lambda, double& ni, double cube) {
    lambda *= fmax(LM_GOOD_STEP_LOWER_SCALE, fmin(1. - cube, LM_GOOD_STEP_UPPER_SCALE)); ni = 2;
}
// a rejected trial (:143-147); the site restores its estimate
VIO_HD void lm_bad_step(double& lambda, double& ni) { lambda *= ni; ni *= 2; }
// "while (rho < 0 && qmax < _maxTrialsAfterFailure->value() && ! _optimizer->terminate())" (:149), qmax counted after the trial
VIO_HD bool lm_retry(double rho, int qmax) { return rho < 0 && qmax < LM_MAX_TRIALS_AFTER_FAILURE; }
// The end of an iteration: Terminate ("qmax == _maxTrialsAfterFailure->value() || rho == 0", :151-152, nBad untouched), then this fork's
// stall rule ("if ((iniChi - currentChi) * 1e3 < iniChi) _nBad++; else _nBad = 0; if (_nBad >= 3) return Terminate", :155-161)
VIO_HD bool lm_iteration_stops(double rho, int qmax, double iniChi, double currentChi, int& nBad) {
    if (qmax == LM_MAX_TRIALS_AFTER_FAILURE || rho == 0) return true;
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
    return nBad >= 3;
}

// computeScale() (:182-189) over a small dense system, in index order: k_pose_opt_se3 (6) and k_sim3_optimize (7)
template <int N> VIO_HD double lm_scale(const double* x, const double* b, double lambda) {
    double scale = 0;
    for (int j = 0; j < N; j++) scale += x[j] * (lambda * x[j] + b[j]);
    return scale;
}

} // namespace viorb
