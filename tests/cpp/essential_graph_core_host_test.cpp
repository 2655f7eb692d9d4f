// tests/cpp/essential_graph_core_host_test.cpp — the host build of viorb_amd/csrc/essential_graph_core.h on a few fixed cases, as a
// stand-alone program that tests/test_essential_graph_host_sanitized.py compiles with -fsanitize=address,undefined and runs as a child
// process: Sim3::log in each of its four branches and with a scale at the 1e-5 thresholds, exp(log) against the input, an edge with
// each side fixed, a zero increment, the write-back of a pose and a point. It prints one checksum line; the test requires a clean exit.
// No GPU, no library: only the header.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "essential_graph_core.h"

using namespace viorb;

static double sum = 0;
static void add(const double* v, int n) { for (int i = 0; i < n; i++) { if (!std::isfinite(v[i])) { std::printf("non-finite value\n"); std::exit(2); } sum += std::fabs(v[i]); } }

static sim3d make(double angle, double sigma, double tx, double ty, double tz) {
    const double n = std::sqrt(0.3 * 0.3 + 0.5 * 0.5 + 0.8 * 0.8), h = std::sin(angle / 2) / n;
    sim3d S; S.r = mkq(0.3 * h, -0.5 * h, 0.8 * h, std::cos(angle / 2)); S.t = mk3(tx, ty, tz); S.s = std::exp(sigma);
    return S;
}

int main() {
    // log: small / general rotation x small / general scale, and both sides of both thresholds (d = 1 - 1e-5 at 4.4721e-3 rad)
    const double angles[6] = {0.0, 1e-4, 4.46e-3, 4.48e-3, 0.8, 2.5}, sigmas[7] = {0.0, 0.9e-5, -0.9e-5, 1.1e-5, -1.1e-5, 0.35, -0.6};
    int branches = 0;
    for (int a = 0; a < 6; a++)
        for (int g = 0; g < 7; g++) {
            const sim3d S = make(angles[a], sigmas[g], 0.7, -1.3, 2.1);
            double l[7];
            sim3_log(S, l);
            add(l, 7);
            branches |= 1 << ((std::fabs(l[6]) < 1e-5 ? 0 : 2) + (angles[a] < 4.47e-3 ? 0 : 1));
            if (std::fabs(l[6] - std::log(S.s)) != 0) { std::printf("sigma\n"); return 3; }
            // exp(log(S)) == S where both take the same branch: log calls a rotation small below 4.4721e-3 rad (d > 1 - 1e-5), exp below
            // 1e-5 rad (theta < 1e-5), and between the two log's first-order omega is not what exp inverts
            if (angles[a] >= 4.47e-3 || angles[a] == 0.0) {
                double p[8], q[8];
                sim3_st(p, sim3_exp(l)); sim3_st(q, S);
                for (int k = 0; k < 8; k++) if (std::fabs(p[k] - q[k]) > 1e-9) { std::printf("exp(log) %d %d %d: %g\n", a, g, k, p[k] - q[k]); return 4; }
            }
        }
    if (branches != 15) { std::printf("branches %d\n", branches); return 5; }
    // a singular W (zero scale is refused by the entry points; a zero matrix must still not index out of range)
    { const d3 x = eg_lu_solve(zero3(), mk3(1, 2, 3)); (void)x; }
    // pivoting: every row order of one matrix gives the same solution
    {
        const double rows[3][3] = {{0.1, 2.0, -1.0}, {3.0, 0.5, 0.2}, {-0.4, 0.3, 4.0}}, b[3] = {1.0, -2.0, 0.5};
        const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        double first[3] = {0, 0, 0};
        for (int q = 0; q < 6; q++) {
            const int* p = perm[q];
            const d3 x = eg_lu_solve(mkm(rows[p[0]][0], rows[p[0]][1], rows[p[0]][2], rows[p[1]][0], rows[p[1]][1], rows[p[1]][2], rows[p[2]][0], rows[p[2]][1], rows[p[2]][2]),
                                     mk3(b[p[0]], b[p[1]], b[p[2]]));
            const double v[3] = {x.x, x.y, x.z};
            add(v, 3);
            for (int k = 0; k < 3; k++) { if (q == 0) first[k] = v[k]; else if (std::fabs(v[k] - first[k]) > 1e-14) { std::printf("pivot order %d\n", q); return 6; } }
        }
    }
    // an edge: both free, each side fixed, both fixed; free and fixed scale
    const sim3d Si = make(0.4, 0.05, 1.0, 0.2, -0.3), Sj = make(-0.7, -0.02, -0.5, 1.1, 0.4);
    const sim3d Cm = sim3_mul(eg_measurement(Si, Sj), make(0.01, 0.002, 0.01, -0.02, 0.005));
    for (int fs = 0; fs < 2; fs++)
        for (int fx = 0; fx < 4; fx++) {
            double e[7], Ji[49], Jj[49];
            eg_edge(Si, Sj, Cm, fs != 0, (fx & 1) != 0, (fx & 2) != 0, e, Ji, Jj);
            add(e, 7); add(Ji, 49); add(Jj, 49);
            for (int k = 0; k < 49; k++) {
                if ((fx & 1) && Ji[k] != 0) { std::printf("Jacobian of a fixed vertex\n"); return 7; }
                if ((fx & 2) && Jj[k] != 0) { std::printf("Jacobian of a fixed vertex\n"); return 7; }
                if (fs && k % 7 == 6 && (Ji[k] != 0 || Jj[k] != 0)) { std::printf("scale column with fix_scale\n"); return 8; }
            }
        }
    // a zero increment leaves the estimate; with fix_scale the scale is kept bit for bit
    {
        const double z[7] = {0, 0, 0, 0, 0, 0, 0}, u[7] = {0.01, -0.02, 0.03, 0.1, 0.2, -0.1, 0.05};
        double p[8], q[8];
        sim3_st(p, sim3_oplus(Si, z, false)); sim3_st(q, Si);
        for (int k = 0; k < 8; k++) if (p[k] != q[k]) { std::printf("zero increment\n"); return 9; }
        sim3_st(p, sim3_oplus(Si, u, true));
        if (p[7] != q[7]) { std::printf("scale moved with fix_scale\n"); return 10; }
        add(p, 8);
    }
    // write-back
    {
        double T[12];
        eg_recover_pose(Si, T);
        add(T, 12);
        const float P[3] = {1.5f, -0.25f, 4.0f};
        float o[3];
        eg_recover_point(Si, Si, P, o);
        for (int k = 0; k < 3; k++) if (std::fabs(o[k] - P[k]) > 1e-6f) { std::printf("point through S^-1 S\n"); return 11; }
        eg_recover_point(Si, Sj, P, o);
        const double od[3] = {o[0], o[1], o[2]};
        add(od, 3);
        const double bad[8] = {0, 0, 0, 1, 0, 0, 0, 0.0}, nan8[8] = {0, 0, 0, 1, 0, NAN, 0, 1.0}, ok8[8] = {0, 0, 0, 1, 0, 0, 0, 1.0};
        if (eg_pose_ok(bad) || eg_pose_ok(nan8) || !eg_pose_ok(ok8) || eg_edge_ok(2, 2, 5) || eg_edge_ok(-1, 2, 5) || eg_edge_ok(1, 5, 5) || !eg_edge_ok(4, 0, 5)) { std::printf("predicates\n"); return 12; }
    }
    std::printf("checksum %.12g\n", sum);
    return 0;
}
