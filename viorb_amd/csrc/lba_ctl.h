// viorb_amd/csrc/lba_ctl.h — the control block of a window solve (local_ba.hip) and the three functions that change it between trials:
// g2o's Levenberg loop (optimization_algorithm_levenberg.cpp:61-164, the rule itself from lm_core.h) inside the two optimize() calls of
// LocalBundleAdjustmentNavState / LocalBundleAdjustment (reference src/Optimizer.cc:2026-2099, :4160-4235), as a state machine over 32
// doubles. Both drivers keep the block on the device and run the same functions: the single window from the last block of
// k_ba_f_errors_decide, k_ba_lambda0 and k_ba_phase (the host takes the phase change on its copy of the block too); the lock-step batch
// from k_bab_decide, k_bab_lambda0 and k_bab_phase. Host and device (VIO_HD), plain doubles: tests/cpp/lm_core_host_test.cpp runs them on the host.
#pragma once
#include "lm_core.h"

namespace viorb {

// Word 5 (GATE) and word 30 (ABORT) are the ones every solver kernel tests before it does anything (ba_skip, BA_B_WINDOW).
enum { BA_CTL_LAMBDA = 0, BA_CTL_NI, BA_CTL_CHI, BA_CTL_INICHI, BA_CTL_NBAD,
       BA_B_GATE,                         // 0: solving; 1: this optimize() is over, gate the edges and start the second one; 2: over, final gate
       BA_CTL_IT,                         // iterations of this optimize() so far
       BA_CTL_TRIALS, BA_CTL_REJECTS,     // Levenberg trials taken / rejected (info[4], info[5])
       BA_B_DONE = 16,
       BA_B_NEED_CHI,                     // lock-step: the round computes the chi2 the optimize() starts from (the single window enqueues that itself)
       BA_B_NEED_LIN,                     // the next trial linearises first (the last one ended an iteration); 0: a retry of the same system
       BA_B_FIRST,                        // ... and is the first of its optimize(): lambda_0, nBad = 0
       BA_B_PHASE, BA_B_MONO,             // 0 / 1: first / second optimize(); robust kernel on the reprojection edges
       BA_B_QMAX,                         // trials of the current iteration so far
       BA_CTL_RHO,
       BA_B_RESTORE,                      // the last trial was rejected: the estimate goes back to its backup before anything reads it
       BA_B_ITERS,                        // 5 / 10
       BA_B_ITS0, BA_B_ITS1, BA_B_CHI0, BA_B_CHI1,   // iterations and chi2 of the two optimize() calls (info[2], [3], [0], [1])
       BA_B_ABORT,                        // lock-step: the host saw the caller's stop flag between rounds
       BA_B_N = 32 };
enum { BA_CTL_N = BA_B_N };

// the block at the start of a solve, word t
VIO_HD double lba_ctl_init(int t) {
    return (t == BA_B_NEED_CHI || t == BA_B_NEED_LIN || t == BA_B_FIRST || t == BA_B_MONO) ? 1.0 : (t == BA_B_ITERS ? 5.0 : 0.0);
}

// lambda_0 (:166-180) from the largest diagonal entry of the system, on the first linearisation of an optimize() (BA_B_FIRST)
VIO_HD void lba_lambda0(double* c, double max_diag) {
    c[BA_CTL_LAMBDA] = lm_lambda_init(max_diag); c[BA_CTL_NI] = 2.0; c[BA_CTL_NBAD] = 0.0; c[BA_B_FIRST] = 0.0;
}

// The Levenberg decisions of one trial (:129-161) and the end of an optimize() call. chi2: robust chi2 of the trial state, scale:
// computeScale(), solved: the factorisation's flag (> 0.5: ok), abort: the caller's stop flag went up during the trial ("&& !terminate()"
// in the trial loop, :149, and in the iteration loop of optimize(): no retry, the iteration ends and is counted, no further one, no second
// optimize()). Afterwards exactly one of these holds: BA_B_QMAX > 0 (another trial of the same iteration, no re-linearisation),
// BA_B_NEED_LIN (next iteration), BA_B_GATE (this optimize() is over). A rejected trial leaves BA_B_RESTORE set in all three cases: the
// driver restores the estimate before the next trial or the gate.
VIO_HD void lba_decide(double* c, double chi2, double scale, double solved, bool abort) {
    const bool ok2 = solved > 0.5;
    const double tempChi = lm_trial_chi2(ok2, chi2);
    const double rho = lm_rho(c[BA_CTL_CHI], tempChi, ok2 ? scale : 0.0);
    c[BA_CTL_RHO] = rho;
    int qmax = (int)c[BA_B_QMAX];
    c[BA_CTL_TRIALS] += 1.0;
    if (lm_accepted(rho, tempChi)) { lm_good_step(c[BA_CTL_LAMBDA], c[BA_CTL_NI], lm_cube_mul(2 * rho - 1)); c[BA_CTL_CHI] = tempChi; }
    else { lm_bad_step(c[BA_CTL_LAMBDA], c[BA_CTL_NI]); c[BA_B_RESTORE] = 1.0; c[BA_CTL_REJECTS] += 1.0; }
    qmax++;
    if (lm_retry(rho, qmax) && !abort) { c[BA_B_QMAX] = qmax; return; }
    // the iteration is over
    const int phase = (int)c[BA_B_PHASE];
    c[BA_B_ITS0 + phase] += 1.0; c[BA_B_CHI0 + phase] = c[BA_CTL_CHI];
    int nBad = (int)c[BA_CTL_NBAD];
    const bool stop_opt = lm_iteration_stops(rho, qmax, c[BA_CTL_INICHI], c[BA_CTL_CHI], nBad);
    c[BA_CTL_NBAD] = nBad;
    c[BA_CTL_IT] += 1.0; c[BA_B_QMAX] = 0.0;
    if (abort) c[BA_B_GATE] = 2.0;
    else if (stop_opt || c[BA_CTL_IT] >= c[BA_B_ITERS]) c[BA_B_GATE] = phase == 0 ? 1.0 : 2.0;
    else c[BA_B_NEED_LIN] = 1.0;
}

// After the gate: BA_B_GATE == 1 -> the second optimize(), 10 iterations without the robust kernel on the reprojection edges
// (src/Optimizer.cc:2037-2099); == 2 -> the window is finished (returns true, once).
VIO_HD bool lba_phase(double* c) {
    c[BA_B_RESTORE] = 0.0;
    if (c[BA_B_GATE] == 1.0) {
        c[BA_B_PHASE] = 1.0; c[BA_B_MONO] = 0.0; c[BA_B_ITERS] = 10.0; c[BA_CTL_IT] = 0.0; c[BA_B_QMAX] = 0.0;
        c[BA_B_NEED_CHI] = 1.0; c[BA_B_NEED_LIN] = 1.0; c[BA_B_FIRST] = 1.0; c[BA_B_GATE] = 0.0;
    } else if (c[BA_B_GATE] == 2.0) {
        c[BA_B_GATE] = 0.0; c[BA_B_DONE] = 1.0;
        return true;
    }
    return false;
}

} // namespace viorb
