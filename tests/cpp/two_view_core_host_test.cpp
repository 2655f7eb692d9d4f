// tests/cpp/two_view_core_host_test.cpp — the host build of viorb_amd/csrc/two_view_core.h on a few fixed cases, as a stand-alone program
// that tests/test_two_view_host_sanitized.py compiles with -fsanitize=address,undefined and runs as a child process. It prints one
// checksum line; the test requires a clean exit. No GPU, no library: only the header.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "two_view_core.h"

using namespace viorb;

static double sum = 0;
static void add(const float* v, int n) { for (int i = 0; i < n; i++) { if (!std::isfinite(v[i])) { std::printf("non-finite value\n"); std::exit(2); } sum += std::fabs((double)v[i]); } }

static unsigned rng_state = 12345u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)((rng_state >> 8) & 0xffffff) / 16777216.0f; }

int main() {
    const TvK k = {458.654f, 457.296f, 367.215f, 248.375f};
    // a scene in front of camera 1, camera 2 = small rotation about y and a sideways step
    const float c = std::cos(0.05f), s = std::sin(0.05f);
    const float Rt[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, tt[3] = {-0.5f, 0.02f, 0.03f};
    const int N = 60;
    std::vector<float> uv(4 * N);
    for (int i = 0; i < N; i++) {
        const float X[3] = {4 * rnd() - 2, 3 * rnd() - 1.5f, 4 + 6 * rnd()};
        const float Y[3] = {Rt[0] * X[0] + Rt[1] * X[1] + Rt[2] * X[2] + tt[0], Rt[3] * X[0] + Rt[4] * X[1] + Rt[5] * X[2] + tt[1], Rt[6] * X[0] + Rt[7] * X[1] + Rt[8] * X[2] + tt[2]};
        uv[4 * i] = k.fx * X[0] / X[2] + k.cx; uv[4 * i + 1] = k.fy * X[1] / X[2] + k.cy;
        uv[4 * i + 2] = k.fx * Y[0] / Y[2] + k.cx; uv[4 * i + 3] = k.fy * Y[1] / Y[2] + k.cy;
    }
    // Normalize of both frames
    float nrm1[4], nrm2[4];
    for (int f = 0; f < 2; f++) {
        double sx = 0, sy = 0, dx = 0, dy = 0;
        float* nrm = f ? nrm2 : nrm1;
        for (int i = 0; i < N; i++) { sx += uv[4 * i + 2 * f]; sy += uv[4 * i + 2 * f + 1]; }
        tv_norm_finish_mean(sx, sy, N, nrm);
        for (int i = 0; i < N; i++) { dx += std::fabs(uv[4 * i + 2 * f] - nrm[0]); dy += std::fabs(uv[4 * i + 2 * f + 1] - nrm[1]); }
        tv_norm_finish_dev(dx, dy, N, nrm);
        add(nrm, 4);
    }
    // one H and one F hypothesis from the first eight pairs
    float AH[16][9], AF[8][9], x[9], H21[9], H12[9], Fn[9], F21[9];
    for (int i = 0; i < 8; i++) {
        float a, b, cc, d;
        tv_norm_point(nrm1, uv[4 * i], uv[4 * i + 1], a, b); tv_norm_point(nrm2, uv[4 * i + 2], uv[4 * i + 3], cc, d);
        tv_rows_h(a, b, cc, d, AH[2 * i], AH[2 * i + 1]); tv_row_f(a, b, cc, d, AF[i]);
    }
    tv_null9_host<16>(AH, x); tv_h_denorm(x, nrm1, nrm2, H21, H12); add(H21, 9); add(H12, 9);
    tv_null9_host<8>(AF, x); tv_f_rank2(x, Fn); tv_f_denorm(Fn, nrm1, nrm2, F21); add(F21, 9);
    // scores of every match under both models
    int inl = 0;
    std::vector<unsigned char> flags(N);
    for (int i = 0; i < N; i++) {
        float chi[2]; bool in;
        sum += tv_score_h(H21, H12, uv[4 * i], uv[4 * i + 1], uv[4 * i + 2], uv[4 * i + 3], tv_inv_sigma2(1.0f), chi, in);
        sum += tv_score_f(F21, uv[4 * i], uv[4 * i + 1], uv[4 * i + 2], uv[4 * i + 3], tv_inv_sigma2(1.0f), chi, in);
        flags[i] = in; inl += in;
    }
    // both decompositions
    float R[8][9], t[8][3], d3[3];
    const bool okh = tv_decompose_h(H21, k, R, t, d3);
    for (int h = 0; h < 8; h++) { add(R[h], 9); add(t[h], 3); }
    add(d3, 3);
    tv_decompose_f(F21, k, R, t);
    for (int h = 0; h < 4; h++) { add(R[h], 9); add(t[h], 3); }
    // CheckRT of the 60 matches under the four motions, with the selection and the accept rule
    int ng[8] = {0}; float par[8] = {0};
    for (int h = 0; h < 4; h++) {
        TvPose p;
        tv_pose(k, R[h], t[h], p);
        std::vector<uint32_t> keys;
        for (int i = 0; i < N; i++) {
            float X[3], q[6];
            if (tv_check_rt_match(k, p, uv[4 * i], uv[4 * i + 1], uv[4 * i + 2], uv[4 * i + 3], tv_th2(1.0f), X, q) != TV_RT_NONE) { keys.push_back(tv_float_key(q[0])); add(X, 3); }
        }
        ng[h] = (int)keys.size();
        if (!keys.empty()) {                                        // the four-pass radix select of the kernel
            int kk = ng[h] - 1 < 50 ? ng[h] - 1 : 50;
            uint32_t prefix = 0;
            for (int pass = 0; pass < 4; pass++) {
                const int shift = 24 - 8 * pass;
                const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
                int hist[256] = {0};
                for (uint32_t key : keys) if ((key & mask) == prefix) hist[(key >> shift) & 255]++;
                int d = 0;
                while (d < 255 && kk >= hist[d]) { kk -= hist[d]; d++; }
                prefix |= (uint32_t)d << shift;
            }
            par[h] = tv_parallax_deg(tv_key_float(prefix));
        }
    }
    int reason = 0;
    const int win = tv_accept_f(ng, par, inl, 1.0f, 50, reason);
    int rh = 0;
    const int winh = tv_accept_h(ng, par, inl, 1.0f, 50, rh);
    std::printf("checksum %.6f okh %d inliers %d n_good %d %d %d %d win %d reason %d winh %d\n", sum, (int)okh, inl, ng[0], ng[1], ng[2], ng[3], win, reason, winh);
    return (win >= 0 && ng[win] == N) ? 0 : 3;
}
