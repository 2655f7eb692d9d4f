// tests/cpp/sim3_core_host_test.cpp — the host build of viorb_amd/csrc/sim3_core.h on a few fixed cases, as a stand-alone program that
// tests/test_sim3_host_sanitized.py compiles with -fsanitize=address,undefined and runs as a child process. It prints one checksum
// line; the test requires a clean exit. No GPU, no library: only the header.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sim3_core.h"

using namespace viorb;

static double sum = 0;
static void add(const float* v, int n) { for (int i = 0; i < n; i++) { if (!std::isfinite(v[i])) { std::printf("non-finite value\n"); std::exit(2); } sum += std::fabs((double)v[i]); } }

static unsigned rng_state = 24680u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)((rng_state >> 8) & 0xffffff) / 16777216.0f; }

int main() {
    const Sim3K k = {458.654f, 457.296f, 367.215f, 248.375f};
    // X1 = s R X2 + t with a rotation about y, s = 1.3
    const float c = std::cos(0.3f), s = std::sin(0.3f), sc = 1.3f;
    const float Rt[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, tt[3] = {0.4f, -0.1f, 0.2f};
    const int N = 70;
    std::vector<float> X1(3 * N), X2(3 * N), sig(N);
    for (int i = 0; i < N; i++) {
        float* a = &X1[3 * i]; float* b = &X2[3 * i];
        b[0] = 3 * rnd() - 1.5f; b[1] = 2 * rnd() - 1.0f; b[2] = 3 + 5 * rnd();
        for (int r = 0; r < 3; r++) a[r] = sc * (Rt[3 * r] * b[0] + Rt[3 * r + 1] * b[1] + Rt[3 * r + 2] * b[2]) + tt[r];
        if (i % 7 == 3) b[0] += 1.0f;                              // an outlier
        sig[i] = std::pow(1.44f, (float)(i % 8));
    }
    // hypotheses from consecutive triples, free and fixed scale; the inliers of each; the acceptance rule over the counts
    std::vector<int> counts;
    for (int fix = 0; fix < 2; fix++)
        for (int it = 0; it + 2 < N; it += 3) {
            float P1[3][3], P2[3][3], R[9], t[3], s12;
            for (int j = 0; j < 3; j++) for (int r = 0; r < 3; r++) { P1[j][r] = X1[3 * (it + j) + r]; P2[j][r] = X2[3 * (it + j) + r]; }
            if (sim3_horn(P1, P2, fix != 0, R, t, s12) != SIM3_SET_OK) { std::printf("unexpected reason\n"); return 4; }
            add(R, 9); add(t, 3); add(&s12, 1);
            float T16[16];
            sim3_T12(R, t, s12, T16); add(T16, 16);
            Sim3Pair T;
            sim3_transforms(R, t, s12, T);
            int cnt = 0;
            for (int i = 0; i < N; i++) {
                float p1u, p1v, p2u, p2v, e1, e2;
                sim3_to_image(k, X1[3 * i], X1[3 * i + 1], X1[3 * i + 2], p1u, p1v);
                sim3_to_image(k, X2[3 * i], X2[3 * i + 1], X2[3 * i + 2], p2u, p2v);
                cnt += sim3_is_inlier(k, k, T, &X1[3 * i], &X2[3 * i], p1u, p1v, p2u, p2v, sim3_max_error(sig[i]), sim3_max_error(sig[i]), e1, e2);
                add(&e1, 1); add(&e2, 1);
            }
            if (!fix) counts.push_back(cnt);
        }
    // the 0 / 0 set, a collinear set and coincident points
    float Z[3][3] = {{0.5f, -0.25f, 4.0f}, {-1.0f, 0.75f, 6.0f}, {1.5f, 1.0f, 3.0f}}, R[9], t[3], s12;
    const int zr = sim3_horn(Z, Z, false, R, t, s12);
    add(R, 9); add(t, 3);
    float L1[3][3] = {{0, 0, 4}, {0.5f, 0.25f, 5}, {1, 0.5f, 6}}, L2[3][3] = {{0.25f, 0.25f, 2.25f}, {0.5f, 0.375f, 2.75f}, {0.75f, 0.5f, 3.25f}};
    const int lr = sim3_horn(L1, L2, false, R, t, s12);
    add(R, 9); add(t, 3); add(&s12, 1);
    float C1[3][3] = {{1, 1, 5}, {1, 1, 5}, {1, 1, 5}};
    const int cr = sim3_horn(C1, C1, true, R, t, s12);             // every relative coordinate is zero: N = 0
    // g2o::Sim3: the exponential in its four branches, oplus with and without a fixed scale, both edges and their numeric Jacobians
    const double us[4][7] = {{1e-6, 2e-6, -1e-6, 0.3, 0.1, 0.2, 1e-6}, {0.2, -0.1, 0.3, 0.3, 0.1, 0.2, 1e-6}, {1e-6, 2e-6, -1e-6, 0.3, 0.1, 0.2, 0.1},
                             {0.2, -0.1, 0.3, 0.3, 0.1, 0.2, -0.2}};
    sim3d est = sim3_exp(us[3]);
    for (int k = 0; k < 4; k++) {
        double v8[8]; float f8[8];
        sim3_st(v8, sim3_mul(sim3_exp(us[k]), est));
        for (int i = 0; i < 8; i++) f8[i] = (float)(k == 2 ? v8[i] * 1e-6 : v8[i]);          // the third branch's translation is huge in the reference
        add(f8, 8);
    }
    const double K4[4] = {458.654, 457.296, 367.215, 248.375};
    for (int fixs = 0; fixs < 2; fixs++)
        for (int d = 0; d < 14; d++) {
            const sim3d pe = sim3_perturbed(est, d, fixs != 0);
            double e[2], e2[2]; float f4[4];
            sim3_edge_error(pe, mk3(0.3, -0.2, 5.0), K4, 300.0, 200.0, e); sim3_edge_error(sim3_inv(pe), mk3(0.5, 0.1, 4.0), K4, 310.0, 220.0, e2);
            f4[0] = (float)e[0]; f4[1] = (float)e[1]; f4[2] = (float)e2[0]; f4[3] = (float)e2[1];
            add(f4, 4);
        }
    int st[4];
    Sim3Select a = sim3_select(counts.data(), (int)counts.size(), N, 20, (int)counts.size(), 0, 0, 5);
    st[0] = a.status; st[1] = a.iterations_done;
    Sim3Select b = sim3_select(counts.data(), (int)counts.size(), N, 20, (int)counts.size(), a.iterations_done, a.best_inliers, 1000);
    st[2] = b.status; st[3] = b.iterations_done;
    const Sim3Select few = sim3_select(counts.data(), (int)counts.size(), 10, 20, 5, 0, 0, 5);
    const Sim3Select past = sim3_select(counts.data(), (int)counts.size(), N, 20, 1000, (int)counts.size() + 5, 0, 5);
    const float big = sim3_max_error(1e30f), neg = sim3_max_error(-1.0f), nan_th = sim3_max_error(NAN);
    std::printf("checksum %.6f zero %d collinear %d coincident %d select %d %d %d %d few %d past %d %d thresholds %g %g %g first count %d\n", sum, zr, lr, cr,
                st[0], st[1], st[2], st[3], few.status, past.status, past.iterations_done, (double)big, (double)neg, (double)nan_th, counts[0]);
    return (zr == SIM3_SET_ZERO_ROTATION && a.status == SIM3_FOUND && few.status == SIM3_FEW && counts[0] == 60) ? 0 : 3;
}
