// tests/cpp/reloc_core_host_test.cpp — the host build of viorb_amd/csrc/reloc_core.h, as a stand-alone program that
// tests/test_reloc_host_sanitized.py compiles with -fsanitize=address,undefined and runs as a child process. The gates run on the edge
// values of ORBmatcher::SearchByProjection(Frame&, KeyFrame*, ...) (no z < 0 gate, NaN coordinates, both bounds, both distance limits) and
// against a restatement written with the reference's double casts; the serial claim plus histogram runs against the literal loop
// (a taken bitmap, 30 rotHist vectors, ComputeThreeMaxima) on random and adversarial lists; the whole matcher (gates, window scan, lists,
// claim, histogram) runs against a literal loop over an mGrid of vectors; corrupted grids, lists and counts, held in heap blocks of their
// exact size, must not send a read outside them. It prints one checksum line; the test requires a clean exit. No GPU, no library.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#include "reloc_core.h"

using namespace viorb;

static long long sum = 0;
static unsigned rng_state = 24680u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() % 100000) / 100000.f; }
static void fail(const char* what) { std::printf("FAILED: %s\n", what); std::exit(2); }

struct Kp { float x, y, size, angle, response; int octave, class_id; };

static S3mCam camera(float th, int nlevels) {
    S3mCam C;
    C.fx = 128.f; C.fy = 128.f; C.cx = 320.f; C.cy = 240.f;
    const float b4[4] = {0.f, 640.f, 0.f, 480.f};
    C.g = grid_cam(b4);
    C.th = th; C.nlevels = nlevels;
    C.log_sf = (float)std::log((double)1.2f);
    float s = 1.f;
    for (int i = 0; i < 16; i++) { C.scale[i] = s; if (i + 1 < nlevels) s *= 1.2f; }
    return C;
}

// src/ORBmatcher.cc:1477-1479, :1498-1527 with the reference's casts written out: reason, u, v, dist3D, level, radius
struct Lit { int reason, level; float u, v, dist3D, radius; };
static Lit literal_project(const S3mCam& C, const float* pose, const float* X) {
    Lit L; L.reason = S3M_MATCHED; L.level = 0; L.u = L.v = L.dist3D = L.radius = 0.f;
    float Ow[3], pc[3];
    for (int r = 0; r < 3; r++) {
        volatile float a = pose[r] * pose[9], b = pose[3 + r] * pose[10], c = pose[6 + r] * pose[11];
        volatile float ab = a + b; volatile float abc = ab + c;
        Ow[r] = -abc;
        volatile float d = pose[3 * r] * X[0], e = pose[3 * r + 1] * X[1], f = pose[3 * r + 2] * X[2];
        volatile float de = d + e; volatile float def = de + f;
        volatile float withT = def + pose[9 + r];
        pc[r] = withT;
    }
    const float invzc = (float)(1.0 / (double)pc[2]);
    volatile float fxx = C.fx * pc[0]; volatile float fxxz = fxx * invzc; volatile float u = fxxz + C.cx;
    volatile float fyy = C.fy * pc[1]; volatile float fyyz = fyy * invzc; volatile float v = fyyz + C.cy;
    L.u = u; L.v = v;
    if (u < C.g.minX || u > C.g.maxX) { L.reason = S3M_OUT_OF_IMAGE; return L; }
    if (v < C.g.minY || v > C.g.maxY) { L.reason = S3M_OUT_OF_IMAGE; return L; }
    const float PO[3] = {X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]};
    L.dist3D = (float)std::sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
    const float maxD = 1.2f * X[7], minD = 0.8f * X[6];
    if (L.dist3D < minD || L.dist3D > maxD) { L.reason = S3M_OUT_OF_RANGE; return L; }
    const float ratio = X[7] / L.dist3D;
    const float q = std::ceil(viorb_logf(ratio) / C.log_sf);
    int n = (q > -2147483648.0f && q < 2147483648.0f) ? (int)q : INT_MIN;
    if (n < 0) n = 0; else if (n >= C.nlevels) n = C.nlevels - 1;
    L.level = n;
    L.radius = C.th * C.scale[n];
    return L;
}

static bool same_float(float a, float b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

static void check_point(const S3mCam& C, const float* pose, const float* X, int want_reason) {
    S3mProj P; reloc_project(C, pose, X, P);
    const Lit L = literal_project(C, pose, X);
    if (!same_float(P.u, L.u) || !same_float(P.v, L.v)) fail("u, v differ from the literal projection");
    if (L.reason == S3M_MATCHED) {
        if (!same_float(P.dist3D, L.dist3D) || P.level != L.level || !same_float(P.radius, L.radius)) fail("dist3D / level / radius differ");
        if (P.reason != (P.rect.empty ? S3M_NO_FEATURE_IN_WINDOW : S3M_MATCHED)) fail("reason of a point that reaches the window");
        if (!P.rect.empty && (P.rect.x0 < 0 || P.rect.x1 >= GRID_COLS || P.rect.y0 < 0 || P.rect.y1 >= GRID_ROWS)) fail("cell rectangle out of the grid");
    } else if (P.reason != L.reason) fail("gate differs from the literal projection");
    if (want_reason >= 0 && P.reason != want_reason) { std::printf("point %g %g %g [%g %g]: reason %d, expected %d\n", X[0], X[1], X[2], X[6], X[7], P.reason, want_reason); fail("edge value ends at another statement"); }
    sum += P.reason * 7 + P.level;
}

static void test_gates() {
    const S3mCam C = camera(10.f, 8);
    const float I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    auto pt = [](float x, float y, float z, float mn, float mx) { std::vector<float> X = {x, y, z, 0, 0, 0, mn, mx}; return X; };
    // no z < 0 gate: a point behind the camera whose projection is inside reaches the window
    check_point(C, I, pt(1.f, 0.5f, -2.f, 0.1f, 100.f).data(), S3M_MATCHED);
    // z = 0 with x = y = 0: NaN passes `u < min || u > max`; the window is empty
    check_point(C, I, pt(0.f, 0.f, 0.f, 0.f, 1.f).data(), S3M_NO_FEATURE_IN_WINDOW);
    // z = 0 with x != 0: infinite u
    check_point(C, I, pt(1.f, 0.f, 0.f, 0.f, 10.f).data(), S3M_OUT_OF_IMAGE);
    check_point(C, I, pt(0.f, -1.f, 0.f, 0.f, 10.f).data(), S3M_OUT_OF_IMAGE);
    // exactly on each bound (128 * 2.5 = 320, 128 * 1.875 = 240) passes; a little beyond does not (one ulp of x beyond still rounds onto the bound)
    check_point(C, I, pt(-2.5f, 0.f, 1.f, 0.1f, 100.f).data(), S3M_MATCHED);
    check_point(C, I, pt(2.5f, 0.f, 1.f, 0.1f, 100.f).data(), S3M_MATCHED);
    check_point(C, I, pt(0.f, -1.875f, 1.f, 0.1f, 100.f).data(), S3M_MATCHED);
    check_point(C, I, pt(0.f, 1.875f, 1.f, 0.1f, 100.f).data(), S3M_MATCHED);
    check_point(C, I, pt(-2.5001f, 0.f, 1.f, 0.1f, 100.f).data(), S3M_OUT_OF_IMAGE);
    check_point(C, I, pt(2.5001f, 0.f, 1.f, 0.1f, 100.f).data(), S3M_OUT_OF_IMAGE);
    check_point(C, I, pt(0.f, -1.8751f, 1.f, 0.1f, 100.f).data(), S3M_OUT_OF_IMAGE);
    check_point(C, I, pt(0.f, 1.8751f, 1.f, 0.1f, 100.f).data(), S3M_OUT_OF_IMAGE);
    // dist3D equal to each limit passes: dist = 2; 0.8f * 2.5f and 1.2f * m round to 2
    if (0.8f * 2.5f != 2.0f) fail("0.8f * 2.5f");
    check_point(C, I, pt(0.f, 0.f, 2.f, 2.5f, 100.f).data(), S3M_MATCHED);
    check_point(C, I, pt(0.f, 0.f, 2.f, 2.5001f, 100.f).data(), S3M_OUT_OF_RANGE);
    float m = 2.0f / 1.2f;
    while (1.2f * m > 2.0f) m = std::nextafterf(m, 0.f);
    while (1.2f * m < 2.0f) m = std::nextafterf(m, 10.f);
    if (1.2f * m != 2.0f) fail("no float m with 1.2f * m == 2");
    check_point(C, I, pt(0.f, 0.f, 2.f, 0.1f, m).data(), S3M_MATCHED);
    float below = m;
    while (1.2f * below >= 2.0f) below = std::nextafterf(below, 0.f);
    check_point(C, I, pt(0.f, 0.f, 2.f, 0.1f, below).data(), S3M_OUT_OF_RANGE);
    // levels 0 and top; a scale factor of 1 (one level): the quotient is not finite and clamps to level 0
    { S3mProj P; reloc_project(C, I, pt(0.f, 0.f, 2.f, 0.1f, 1.9f).data(), P); if (P.level != 0 || P.radius != 10.f) fail("level 0"); }
    { S3mProj P; reloc_project(C, I, pt(0.f, 0.f, 2.f, 0.1f, 50.f).data(), P); if (P.level != 7 || P.radius != 10.f * C.scale[7]) fail("top level"); }
    { S3mCam C1 = camera(3.f, 1); C1.log_sf = 0.f; S3mProj P; reloc_project(C1, I, pt(0.f, 0.f, 2.f, 0.1f, 50.f).data(), P); if (P.level != 0) fail("one level"); }
    // non-finite inputs end somewhere, with no undefined conversion on the way
    const float bad[] = {NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 0.f, -0.f, 1e-40f};
    for (float a : bad) for (float b : bad) for (float c : bad) { check_point(C, I, pt(a, b, c, 0.f, 1e30f).data(), -1); check_point(C, I, pt(1.f, 1.f, 4.f, a, b).data(), -1); }
    // random poses and points against the restatement
    for (int it = 0; it < 20000; it++) {
        float pose[12];
        const float ax = rndf(-0.5f, 0.5f), ay = rndf(-0.5f, 0.5f);
        const float cx = std::cos(ax), sx = std::sin(ax), cy = std::cos(ay), sy = std::sin(ay);
        const float R[9] = {cy, 0, sy, sx * sy, cx, -sx * cy, -cx * sy, sx, cx * cy};
        for (int k = 0; k < 9; k++) pose[k] = R[k];
        for (int k = 0; k < 3; k++) pose[9 + k] = rndf(-2.f, 2.f);
        const float mx = rndf(0.5f, 30.f);
        check_point(C, pose, pt(rndf(-6.f, 6.f), rndf(-4.f, 4.f), rndf(-3.f, 12.f), mx / rndf(1.f, 5.f), mx).data(), -1);
    }
}

// the literal loop of :1536-1597 over candidate lists
static int literal_match(const std::vector<std::vector<std::pair<int, int>>>& cands, const std::vector<uint8_t>& taken_in, int orb_dist, bool ori,
                         const std::vector<float>& ak, const std::vector<float>& af, std::vector<int>& best, std::vector<uint8_t>& removed) {
    std::vector<uint8_t> taken(taken_in);
    std::vector<int> rotHist[HISTO_LENGTH];
    int nmatches = 0;
    best.assign(cands.size(), -1); removed.assign(cands.size(), 0);
    for (size_t p = 0; p < cands.size(); p++) {
        int bestDist = 256, bestIdx2 = -1;
        for (auto& c : cands[p]) {
            if (taken[c.second]) continue;
            if (c.first < bestDist) { bestDist = c.first; bestIdx2 = c.second; }
        }
        if (bestDist <= orb_dist) {
            taken[bestIdx2] = 1; best[p] = bestIdx2; nmatches++;
            if (ori) {
                float rot = ak[p] - af[bestIdx2];
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)std::round(rot * (1.0f / HISTO_LENGTH));
                if (bin == HISTO_LENGTH) bin = 0;
                if (bin < 0 || bin >= HISTO_LENGTH) fail("angle out of range in the test's own data");
                rotHist[bin].push_back((int)p);
            }
        }
    }
    if (ori) {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < HISTO_LENGTH; i++) {
            const int s = (int)rotHist[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
        for (int i = 0; i < HISTO_LENGTH; i++)
            if (i != ind1 && i != ind2 && i != ind3)
                for (int p : rotHist[i]) { best[p] = -1; removed[p] = 1; nmatches--; }
    }
    return nmatches;
}

static void run_lists(const std::vector<std::vector<std::pair<int, int>>>& cands, const std::vector<uint8_t>& taken, int orb_dist, bool ori,
                      const std::vector<float>& ak, const std::vector<float>& af) {
    const int npts = (int)cands.size(), nfeat = (int)taken.size();
    int lcap = 1;
    for (auto& c : cands) lcap = std::max(lcap, (int)c.size());
    // heap blocks of the exact size
    std::vector<uint32_t> cand((size_t)npts * lcap); std::vector<int32_t> cn(npts), best(npts), owner(std::max(nfeat, 1)); std::vector<uint8_t> removed(npts);
    for (int p = 0; p < npts; p++) { cn[p] = (int)cands[p].size(); for (size_t k = 0; k < cands[p].size(); k++) cand[(size_t)p * lcap + k] = ((uint32_t)cands[p][k].first << 16) | (uint32_t)cands[p][k].second; }
    const int nm = reloc_match_serial(cand.data(), cn.data(), npts, lcap, taken.data(), nfeat, orb_dist, ori, ak.data(), af.data(), best.data(), removed.data(), owner.data());
    std::vector<int> lb; std::vector<uint8_t> lr;
    const int lm = literal_match(cands, taken, orb_dist, ori, ak, af, lb, lr);
    if (nm != lm) fail("nmatches differs from the literal loop");
    for (int p = 0; p < npts; p++) { if (best[p] != lb[p] || removed[p] != lr[p]) fail("claim plus histogram differs from the literal loop"); sum += best[p] + 3 * removed[p]; }
}

static void test_lists() {
    for (int trial = 0; trial < 400; trial++) {
        const int npts = rnd() % 70, nfeat = 1 + rnd() % 30, hi = (trial % 3 == 0) ? 6 : ((trial % 3 == 1) ? 60 : 150);
        std::vector<std::vector<std::pair<int, int>>> cands(npts);
        for (auto& c : cands) { const int n = rnd() % 7; for (int k = 0; k < n; k++) { const int f = rnd() % nfeat; bool dup = false; for (auto& e : c) dup |= e.second == f; if (!dup) c.push_back({(int)(rnd() % hi), f}); } }
        std::vector<uint8_t> taken(nfeat); for (auto& t : taken) t = rnd() % 8 == 0;
        std::vector<float> ak(npts + 1), af(nfeat);
        for (auto& a : ak) a = rnd() % 10 < 7 ? 100.f : rndf(0.f, 359.9f);
        for (auto& a : af) a = rnd() % 10 < 7 ? 40.f : rndf(0.f, 359.9f);
        run_lists(cands, taken, trial % 2 ? 100 : 64, trial % 5 != 0, ak, af);
    }
    // adversarial: every point wants the same features, best first (npts sweeps); a chain where each loss moves the next
    const int n = 80;
    std::vector<std::vector<std::pair<int, int>>> all(n), chain(n);
    for (int p = 0; p < n; p++) for (int f = 0; f < n; f++) all[p].push_back({f, f});
    chain[0].push_back({0, 0});
    for (int p = 1; p < n; p++) { chain[p].push_back({1, p - 1}); chain[p].push_back({5, p}); }
    std::vector<uint8_t> none(n, 0); std::vector<float> z(n + 1, 0.f);
    run_lists(all, none, 100, true, z, z);
    run_lists(chain, none, 100, true, z, z);
    std::vector<float> spread(n + 1); for (int p = 0; p <= n; p++) spread[p] = (float)((p * 37) % 360);
    run_lists(chain, none, 100, true, spread, z);
    // corrupted lists and counts: features outside 0..nfeat-1, counts below zero and above the list; nothing may be read outside the blocks
    {
        const int npts = 9, lcap = 3, nfeat = 5;
        std::vector<uint32_t> cand((size_t)npts * lcap); std::vector<int32_t> cn(npts), best(npts), owner(nfeat); std::vector<uint8_t> removed(npts), taken(nfeat, 0);
        std::vector<float> ak(npts, NAN), af(nfeat, INFINITY);
        for (auto& c : cand) c = ((rnd() % 120) << 16) | (rnd() % 9 == 0 ? 0xffffu : rnd() % 12);
        const int counts[9] = {-5, 0, 1, 2, 3, 4, 1000, INT_MAX, INT_MIN};
        for (int p = 0; p < npts; p++) cn[p] = counts[p];
        const int nm = reloc_match_serial(cand.data(), cn.data(), npts, lcap, taken.data(), nfeat, 100, 1, ak.data(), af.data(), best.data(), removed.data(), owner.data());
        for (int p = 0; p < npts; p++) if (best[p] >= nfeat) fail("a feature outside the frame was claimed");
        sum += nm;
    }
}

// the whole matcher on the host: reloc_project + reloc_scan + lists + reloc_match_serial against the literal loop over an mGrid of vectors
static void test_matcher(bool corrupt) {
    const S3mCam C = camera(10.f, 8);
    const int N = 160, K = 140, cap = N;                               // heap blocks of the exact size
    std::vector<Kp> kp(N); std::vector<uint8_t> taken(N), kvalid(K), kfound(K);
    std::vector<std::vector<int>> mGrid(GRID_CELLS);
    std::vector<uint32_t> fdesc(N * 8), pdesc(K * 8);
    float pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1f, -0.2f, 0.05f};
    std::vector<float> X(K * 8), ak(K);
    for (int i = 0; i < K; i++) {
        float* x = &X[i * 8];
        const float z = rndf(2.f, 8.f), u = rndf(20.f, 200.f), v = rndf(20.f, 150.f);      // a small region, so that windows overlap
        x[0] = (u - C.cx) / C.fx * z - pose[9]; x[1] = (v - C.cy) / C.fy * z - pose[10]; x[2] = z - pose[11];
        const float d = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        x[7] = d * rndf(0.9f, 2.0f); x[6] = x[7] / 4.f;
        kvalid[i] = rnd() % 12 != 0; kfound[i] = rnd() % 15 == 0; ak[i] = rnd() % 10 < 7 ? 75.f : rndf(0.f, 359.9f);
        for (int w = 0; w < 8; w++) pdesc[i * 8 + w] = (i % 7) * 0x01010101u ^ (rnd() & 0x00030003u);    // few bits differ: every window feature is a candidate
    }
    for (int j = 0; j < N; j++) {
        kp[j].x = rndf(10.f, 210.f); kp[j].y = rndf(10.f, 160.f); kp[j].octave = rnd() % 4; kp[j].angle = rnd() % 10 < 7 ? 40.f : rndf(0.f, 359.9f);
        kp[j].size = 31.f; kp[j].response = 1.f; kp[j].class_id = -1;
        taken[j] = rnd() % 10 == 0;
        for (int w = 0; w < 8; w++) fdesc[j * 8 + w] = (j % 7) * 0x01010101u ^ (rnd() & 0x00300030u);
        const int px = (int)std::round((kp[j].x - C.g.minX) * C.g.wInv), py = (int)std::round((kp[j].y - C.g.minY) * C.g.hInv);
        if (px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS) mGrid[px * GRID_ROWS + py].push_back(j);
    }
    std::vector<int> cs(GRID_CELLS + 1), ci(cap, 0);
    int q = 0;
    for (int c = 0; c < GRID_CELLS; c++) { cs[c] = q; for (int j : mGrid[c]) ci[q++] = j; }
    cs[GRID_CELLS] = q;
    if (corrupt) {                                                      // a grid that was not built for these arrays
        for (int c = 0; c <= GRID_CELLS; c++) if (rnd() % 5 == 0) cs[c] = (int)(rnd() % 4000) - 2000;
        for (int k = 0; k < cap; k++) if (rnd() % 5 == 0) ci[k] = (int)(rnd() % 1000) - 300;
    }
    auto dist = [&](int i, int j) { int d = 0; for (int w = 0; w < 8; w++) d += __builtin_popcount(pdesc[i * 8 + w] ^ fdesc[j * 8 + w]); return d; };
    const int orb_dist = 100, LIST = 64;
    std::vector<uint32_t> cand((size_t)K * LIST); std::vector<int32_t> cn(K, 0), best(K), owner(N); std::vector<uint8_t> removed(K);
    std::vector<float> af(N); for (int j = 0; j < N; j++) af[j] = kp[j].angle;
    for (int i = 0; i < K; i++) {
        if (!kvalid[i] || kfound[i]) continue;
        S3mProj P; reloc_project(C, pose, &X[i * 8], P);
        if (P.reason != S3M_MATCHED) continue;
        reloc_scan(P, kp.data(), cs.data(), ci.data(), N, cap, [&](int idx) {
            if (idx < 0 || idx >= N) fail("the scan visited a feature outside the frame");
            if (taken[idx]) return;
            const int d = dist(i, idx);
            if (d <= orb_dist && cn[i] < LIST) cand[(size_t)i * LIST + cn[i]++] = ((uint32_t)d << 16) | (uint32_t)idx;
        });
    }
    const int nm = reloc_match_serial(cand.data(), cn.data(), K, LIST, taken.data(), N, orb_dist, 1, ak.data(), af.data(), best.data(), removed.data(), owner.data());
    sum += nm;
    if (corrupt) return;
    // the literal loop: Frame::GetFeaturesInArea over mGrid, the frame's map points as a vector, sAlreadyFound as a set
    std::set<int> sAlreadyFound; for (int i = 0; i < K; i++) if (kfound[i]) sAlreadyFound.insert(i);
    std::vector<int> mvp(N); for (int j = 0; j < N; j++) mvp[j] = taken[j] ? -2 : -1;
    std::vector<std::pair<int, int>> rotHist[HISTO_LENGTH];
    std::vector<int> lbest(K, -1);
    int nmatches = 0, contended = 0;
    for (int i = 0; i < K; i++) {
        if (!kvalid[i] || sAlreadyFound.count(i)) continue;
        const Lit L = literal_project(C, pose, &X[i * 8]);
        if (L.reason != S3M_MATCHED) continue;
        GridRect R; grid_window(C.g, L.u, L.v, L.radius, R);
        if (R.empty) continue;
        int bestDist = 256, bestIdx2 = -1;
        for (int ix = R.x0; ix <= R.x1; ix++) for (int iy = R.y0; iy <= R.y1; iy++) for (int j : mGrid[ix * GRID_ROWS + iy]) {
            if (kp[j].octave < L.level - 1) continue;
            if (kp[j].octave > L.level + 1) continue;
            if (!(std::fabs(kp[j].x - L.u) < L.radius && std::fabs(kp[j].y - L.v) < L.radius)) continue;
            if (mvp[j] != -1) { contended += mvp[j] >= 0; continue; }
            const int d = dist(i, j);
            if (d < bestDist) { bestDist = d; bestIdx2 = j; }
        }
        if (bestDist <= orb_dist) {
            mvp[bestIdx2] = i; lbest[i] = bestIdx2; nmatches++;
            rotHist[rot_bin(ak[i], kp[bestIdx2].angle)].push_back({bestIdx2, i});
        }
    }
    int hist[HISTO_LENGTH], keep[HISTO_LENGTH];
    for (int b = 0; b < HISTO_LENGTH; b++) hist[b] = (int)rotHist[b].size();
    three_maxima(hist, keep);
    for (int b = 0; b < HISTO_LENGTH; b++) if (!keep[b]) for (auto& e : rotHist[b]) { mvp[e.first] = -1; lbest[e.second] = -1; nmatches--; }
    if (nmatches != nm) fail("the host matcher's count differs from the literal loop");
    for (int i = 0; i < K; i++) if (best[i] != lbest[i]) fail("the host matcher differs from the literal loop");
    if (nm < 20 || contended < 20) fail("the matcher problem does not match or does not contend");
}

static void test_cascade_decisions() {
    const RelocThresholds T = {10, 50, 30};
    for (int g = -2; g < 90; g++) {
        if (reloc_after_solve1(T, g) != (g < 10 ? RELOC_FEW_INLIERS : (g < 50 ? RELOC_RUNNING : RELOC_ACCEPTED_FIRST))) fail("after the first solve");
        if (reloc_after_solve2(T, g) != ((g > 30 && g < 50) ? RELOC_RUNNING : (g >= 50 ? RELOC_ACCEPTED_SECOND : RELOC_SECOND_WEAK))) fail("after the second solve");
        if (reloc_after_solve3(T, g) != (g >= 50 ? RELOC_ACCEPTED_THIRD : RELOC_THIRD_REJECTED)) fail("after the third solve");
        for (int a = 0; a < 60; a++) {
            if (reloc_after_search1(T, g, a) != (a + g >= 50 ? RELOC_RUNNING : RELOC_COARSE_SHORT)) fail("after the coarse search");
            if (reloc_after_search2(T, g, a) != (g + a >= 50 ? RELOC_RUNNING : RELOC_NARROW_SHORT)) fail("after the narrow search");
        }
        sum += reloc_after_solve1(T, g) + reloc_after_solve2(T, g);
    }
}

int main() {
    test_gates();
    test_lists();
    for (int k = 0; k < 6; k++) test_matcher(false);
    for (int k = 0; k < 6; k++) test_matcher(true);
    test_cascade_decisions();
    std::printf("checksum %lld\n", sum);
    return 0;
}
