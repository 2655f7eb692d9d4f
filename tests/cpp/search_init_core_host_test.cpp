// tests/cpp/search_init_core_host_test.cpp — the host build of viorb_amd/csrc/search_init_core.h on a few fixed cases, as a stand-alone
// program that tests/test_search_init_host_sanitized.py compiles with -fsanitize=address,undefined and runs as a child process. It
// prints one checksum line; the test requires a clean exit. No GPU, no library: only the header. What the header takes from match_core.h
// (window, rotation bin, three maxima) is exercised by tests/cpp/match_core_host_test.cpp.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "search_init_core.h"

using namespace viorb;

static long long sum = 0;
static unsigned rng_state = 2468u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static void fail(const char* what) { std::printf("FAILED: %s\n", what); std::exit(2); }

// the literal i1-ascending loop (:418-487) over candidate lists, to hold the sweeps against
static void literal(const std::vector<uint32_t>& cand, const std::vector<int32_t>& cn, int npts, int lcap, int nfeat, float ratio, std::vector<int32_t>& m12,
                    std::vector<int32_t>& m21, std::vector<int32_t>& md) {
    m12.assign(npts, -1); m21.assign(nfeat, -1); md.assign(nfeat, INT_MAX);
    for (int p = 0; p < npts; p++) {
        SiPick P; si_pick_init(P);
        for (int k = 0; k < cn[p]; k++) { const uint32_t e = cand[(size_t)p * lcap + k]; si_pick_visit(P, (int)(e >> 16), (int)(e & 0xffffu), md[e & 0xffffu]); }
        int why;
        if (si_decide(P, ratio, why) == SI_NONE) continue;
        if (m21[P.best] >= 0) m12[m21[P.best]] = -1;
        m12[p] = P.best; m21[P.best] = p; md[P.best] = P.dist;
    }
}

static int run_lists(const std::vector<uint32_t>& cand, const std::vector<int32_t>& cn, int npts, int lcap, int nfeat, float ratio) {
    std::vector<uint32_t> st(npts + 1), st2(npts + 1);
    std::vector<int> why(npts + 1), head(nfeat + 1), next(npts + 1);
    std::vector<int32_t> m12(npts + 1), m21(nfeat + 1), md(nfeat + 1), e12, e21, ed;
    const int sweeps = si_ordered_sweeps(cand.data(), cn.data(), npts, lcap, nfeat, ratio, st.data(), st2.data(), why.data(), head.data(), next.data());
    const int nm = si_after_loop(st.data(), npts, nfeat, m12.data(), m21.data(), md.data());
    literal(cand, cn, npts, lcap, nfeat, ratio, e12, e21, ed);
    int want = 0;
    for (int p = 0; p < npts; p++) { if (m12[p] != e12[p]) fail("matches12 differs from the literal loop"); want += e12[p] >= 0; sum += m12[p]; }
    for (int f = 0; f < nfeat; f++) if (m21[f] != e21[f] || md[f] != ed[f]) fail("matches21 / matched_distance differ from the literal loop");
    if (nm != want || sweeps < 1 || sweeps > npts + 1) fail("count or sweeps");
    return sweeps;
}

int main() {
    // random lists: 300 points, 120 features, up to 6 candidates each with low distances, so that features are fought over
    {
        const int npts = 300, nfeat = 120, lcap = 6;
        std::vector<uint32_t> cand((size_t)npts * lcap); std::vector<int32_t> cn(npts);
        for (int p = 0; p < npts; p++) { cn[p] = (int)(rnd() % (lcap + 1)); for (int k = 0; k < cn[p]; k++) cand[(size_t)p * lcap + k] = ((rnd() % 70) << 16) | (rnd() % nfeat); }
        sum += run_lists(cand, cn, npts, lcap, nfeat, 0.9f);
        sum += run_lists(cand, cn, npts, lcap, nfeat, 1.2f);
        sum += run_lists(cand, cn, 0, lcap, nfeat, 0.9f);
        sum += run_lists(cand, cn, npts, lcap, 120, 0.05f);
    }
    // both staircases of 70
    {
        const int n = 70;
        std::vector<uint32_t> down(n), up((size_t)n * 2); std::vector<int32_t> one(n, 1), two(n, 2);
        for (int k = 0; k < n; k++) { down[k] = (uint32_t)(n - 1 - k) << 16; up[2 * k] = (20u << 16) | (uint32_t)k; up[2 * k + 1] = (20u << 16) | (uint32_t)(k + 1); }
        two[0] = 1; up[0] = (20u << 16) | 1u;
        if (run_lists(down, one, n, 1, 1, 0.9f) > n + 1) fail("descending staircase");
        if (run_lists(up, two, n, 2, n + 1, 0.9f) != n + 1) fail("ascending staircase takes one sweep per link");
    }
    // pruning rule, depth and the select (the windows, the bins and the three maxima: match_core_host_test.cpp)
    {
        for (int d = 0; d <= 256; d++) sum += si_keep(d, 0.9f) + 2 * si_keep(d, 1e-9f) + 4 * si_keep(d, 1e9f);
        const int n = 1000;
        std::vector<float> z(n);
        const float pose[12] = {1, 0, 0, 0, 1, 0, 0.1f, -0.2f, 0.97f, 0, 0, 0.5f};
        for (int i = 0; i < n; i++) { const float X[3] = {(float)(rnd() % 2000) / 100.f - 10.f, (float)(rnd() % 2000) / 100.f - 10.f, (float)(rnd() % 2000) / 100.f - 5.f}; z[i] = si_depth(pose, X); }
        for (int q = 1; q <= 3; q++) {
            int k = (n - 1) / q; const int k0 = k;
            uint32_t prefix = 0;
            for (int pass = 0; pass < 4; pass++) {
                const int shift = 24 - 8 * pass;
                const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
                int h[256] = {0};
                for (int i = 0; i < n; i++) { const uint32_t key = tv_float_key(z[i]); if ((key & mask) == prefix) h[(key >> shift) & 255]++; }
                prefix |= (uint32_t)si_select_digit(h, k) << shift;
            }
            const float med = tv_key_float(prefix);
            int below = 0, equal = 0;
            for (int i = 0; i < n; i++) { below += z[i] < med; equal += z[i] == med; }
            if (!(below <= k0 && k0 < below + equal)) fail("the select is not the k-th smallest");
            sum += (long long)std::lround(med * 1000.0);
        }
    }
    std::printf("checksum %lld\n", sum);
    return 0;
}
