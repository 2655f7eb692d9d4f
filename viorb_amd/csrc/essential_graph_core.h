// viorb_amd/csrc/essential_graph_core.h — the arithmetic of the essential-graph solve (Optimizer::OptimizeEssentialGraph), shared by the
// HIP kernels of essential_graph.hip and by the host-only hooks viorb_debug_sim3_log / viorb_debug_essential_graph_edge (the CPU
// test-suite compares them with tests/essential_graph_ref.py without a GPU; tests/cpp/essential_graph_core_host_test.cpp runs them under
// the address and undefined-behaviour sanitizers). Everything is double.
//
// What is restated (reference file:line):
//   g2o::Sim3::log (four branches, deltaR, W.lu().solve)   Thirdparty/g2o/g2o/types/sim3.h:148-230, se3_ops.hpp:27-47
//   EdgeSim3::computeError                                 Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:106-114
//   the numeric Jacobians of an edge without linearizeOplus Thirdparty/g2o/g2o/core/base_binary_edge.hpp:131-200
//   the measurement of an edge, Sji = Sjw * Swi            src/Optimizer.cc:4390-4400, :4422-4447, :4465-4474, :4496-4505
//   the write-back of key frames and points                src/Optimizer.cc:4527-4581
// The Sim3 exponential, product, inverse and oplusImpl are sim3_core.h's. Float / double placement is the audit table of DESIGN.md §2
// ("Essential graph").
#pragma once
#include "sim3_core.h"

#define EG_MAX_FREE_KF 3510            // 7 * 3510 = 24570 <= 24576, the order limit of the shared factorisation
#define EG_DELTA 1e-9                  // base_binary_edge.hpp:147

namespace viorb {

// Swaps two rows of [a b c | r] held as values when the second has the larger pivot candidate (Eigen takes the first maximum).
#define EG_ROW_SWAP_IF(cond, a0, a1, a2, r0, b0, b1, b2, r1)                                     \
    do {                                                                                        \
        const bool _s = (cond);                                                                 \
        const double _t0 = _s ? b0 : a0, _t1 = _s ? b1 : a1, _t2 = _s ? b2 : a2, _tr = _s ? r1 : r0; \
        b0 = _s ? a0 : b0; b1 = _s ? a1 : b1; b2 = _s ? a2 : b2; r1 = _s ? r0 : r1;                 \
        a0 = _t0; a1 = _t1; a2 = _t2; r0 = _tr;                                                 \
    } while (0)

// W.lu().solve(t): Eigen's PartialPivLU of a fixed 3 x 3 (the unblocked kernel: the first largest |entry| of the column at or below the
// diagonal is the pivot, the rows below are divided by it, the trailing block is updated) and the two unrolled triangular solves
// (row-wise: x_i = (b_i - sum_k L_ik x_k) [/ U_ii]). All indices are compile-time: the rows are values, a swap is six selects.
VIO_HD d3 eg_lu_solve(const m33& W, d3 t) {
    double a00 = W.a00, a01 = W.a01, a02 = W.a02, a10 = W.a10, a11 = W.a11, a12 = W.a12, a20 = W.a20, a21 = W.a21, a22 = W.a22;
    double b0 = t.x, b1 = t.y, b2 = t.z;
    // column 0: the first maximum of |a00|, |a10|, |a20|
    const bool p2 = fabs(a20) > (fabs(a10) > fabs(a00) ? fabs(a10) : fabs(a00)), p1 = !p2 && fabs(a10) > fabs(a00);
    EG_ROW_SWAP_IF(p1, a00, a01, a02, b0, a10, a11, a12, b1);
    EG_ROW_SWAP_IF(p2, a00, a01, a02, b0, a20, a21, a22, b2);
    if (a00 != 0.0) { a10 /= a00; a20 /= a00; }
    a11 -= a10 * a01; a12 -= a10 * a02; a21 -= a20 * a01; a22 -= a20 * a02;
    // column 1
    EG_ROW_SWAP_IF(fabs(a21) > fabs(a11), a10, a11, a12, b1, a20, a21, a22, b2);
    if (a11 != 0.0) a21 /= a11;
    a22 -= a21 * a12;
    // L y = P b (unit lower), U x = y
    const double y1 = b1 - a10 * b0;
    const double y2 = b2 - (a20 * b0 + a21 * y1);
    const double x2 = y2 / a22;
    const double x1 = (y1 - a12 * x2) / a11;
    const double x0 = (b0 - (a01 * x1 + a02 * x2)) / a00;
    return mk3(x0, x1, x2);
}

// Sim3::log(): res = omega, upsilon, sigma. acos(d) is not clamped (d <= 1 - 1e-5 in its branches; d < -1 gives NaN as in g2o).
VIO_HD void sim3_log(const sim3d& S, double* res) {
    const double s = S.s, sigma = log(s), eps = 0.00001;
    const m33 R = qmat(S.r);
    const double d = 0.5 * (R.a00 + R.a11 + R.a22 - 1);
    const d3 dR = mk3(R.a21 - R.a12, R.a02 - R.a20, R.a10 - R.a01);
    d3 omega;
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) { omega = dR * 0.5; A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta = acos(d), theta2 = theta * theta;
            omega = dR * (theta / (2 * sqrt(1 - d * d)));
            A = (1 - cos(theta)) / theta2; B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            omega = dR * 0.5;
            A = ((sigma - 1) * s + 1) / sigma2; B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            omega = dR * (theta / (2 * sqrt(1 - d * d)));
            const double theta2 = theta * theta, a = s * sin(theta), b = s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const m33 Om = hat3(omega);
    const m33 W = add(add(scl(Om, A), mul(scl(Om, B), Om)), scl(eye3(), C));
    const d3 ups = eg_lu_solve(W, S.t);
    res[0] = omega.x; res[1] = omega.y; res[2] = omega.z; res[3] = ups.x; res[4] = ups.y; res[5] = ups.z; res[6] = sigma;
}

// Sji = Sjw * Swi with both operands from one pose array (vertex 0 = i, vertex 1 = j)
VIO_HD sim3d eg_measurement(const sim3d& Siw, const sim3d& Sjw) { return sim3_mul(Sjw, sim3_inv(Siw)); }
// EdgeSim3::computeError: log(C * S_v0 * S_v1^-1)
VIO_HD void eg_error(const sim3d& C, const sim3d& Si, const sim3d& Sj, double* e) { sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inv(Sj)), e); }
// Column c of the numeric Jacobian of one side: scalar * (e(+delta) - e(-delta)), the step taken through oplusImpl on that vertex alone.
// side 0: vertex i, side 1: vertex j. With fix_scale, column 6 is 0 * anything finite = exactly zero (both estimates are the same).
VIO_HD void eg_jac_column(const sim3d& C, const sim3d& Si, const sim3d& Sj, int side, int c, bool fix_scale, double* col) {
    const double scalar = 1.0 / (2 * EG_DELTA);
    double ep[7], em[7];
    // the side is selected by value, not by branch: the lanes of both sides of an edge run one instruction stream
    const sim3d base = side ? Sj : Si;
    const sim3d p = sim3_perturbed(base, 2 * c, fix_scale), m = sim3_perturbed(base, 2 * c + 1, fix_scale);
    eg_error(C, side ? Si : p, side ? p : Sj, ep);
    eg_error(C, side ? Si : m, side ? m : Sj, em);
#pragma unroll
    for (int r = 0; r < 7; r++) col[r] = scalar * (ep[r] - em[r]);
}
// One edge, serially: e7, Ji / Jj [7][7] row-major (row = error row, column = increment); a fixed side gets no Jacobian (zeros).
VIO_HD void eg_edge(const sim3d& Si, const sim3d& Sj, const sim3d& C, bool fix_scale, bool fixed_i, bool fixed_j, double* e, double* Ji, double* Jj) {
    eg_error(C, Si, Sj, e);
    for (int c = 0; c < 7; c++) {
        double ci[7] = {0, 0, 0, 0, 0, 0, 0}, cj[7] = {0, 0, 0, 0, 0, 0, 0};
        if (!fixed_i) eg_jac_column(C, Si, Sj, 0, c, fix_scale, ci);
        if (!fixed_j) eg_jac_column(C, Si, Sj, 1, c, fix_scale, cj);
        for (int r = 0; r < 7; r++) { Ji[7 * r + c] = ci[r]; Jj[7 * r + c] = cj[r]; }
    }
}

// SE3 pose recovering (:4534-4542): [R | t / s], R row-major, eigt *= (1. / s)
VIO_HD void eg_recover_pose(const sim3d& S, double* T12) {
    stm(T12, qmat(S.r));
    const d3 t = S.t * (1. / S.s);
    T12[9] = t.x; T12[10] = t.y; T12[11] = t.z;
}
// correctedSwr.map(Srw.map(P)) (:4570-4577): P a float position read as double, the result rounded to float once
VIO_HD void eg_recover_point(const sim3d& Srw, const sim3d& corrected_Srw, const float* P, float* out) {
    const d3 p = sim3_map(sim3_inv(corrected_Srw), sim3_map(Srw, mk3((double)P[0], (double)P[1], (double)P[2])));
    out[0] = (float)p.x; out[1] = (float)p.y; out[2] = (float)p.z;
}
// argument predicate of one pose row: finite, scale > 0
VIO_HD bool eg_pose_ok(const double* S8) {
    bool ok = S8[7] > 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) ok = ok && (S8[k] - S8[k] == 0.0);
    return ok;
}
VIO_HD bool eg_edge_ok(int i, int j, int nk) { return i >= 0 && i < nk && j >= 0 && j < nk && i != j; }

} // namespace viorb
