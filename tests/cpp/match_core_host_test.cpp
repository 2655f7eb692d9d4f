// tests/cpp/match_core_host_test.cpp — the host build of viorb_amd/csrc/match_core.h, as a stand-alone program that
// tests/test_match_core_host_sanitized.py compiles with -fsanitize=address,undefined and runs as a child process. Every helper is held
// against a literal restatement of the reference's statement (or of the form the kernels used before the helper existed); grid_scan also
// walks corrupted grids whose arrays are heap blocks of their exact size, so that the address sanitizer sees any read outside them. It
// prints one checksum line; the test requires a clean exit. No GPU, no library: only the header.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "match_core.h"

using namespace viorb;

static long long sum = 0;
static unsigned rng_state = 97531u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() % 100000) / 100000.f; }
static void fail(const char* what) { std::printf("FAILED: %s\n", what); std::exit(2); }

// (int) of a double as the reference's x86 build converts it (cvttsd2si: the "integer indefinite" INT_MIN for what no int holds)
static int x86_int(double q) { return (q > -2147483649.0 && q < 2147483648.0) ? (int)q : INT_MIN; }

// Frame::GetFeaturesInArea, src/Frame.cc:512-526, statement by statement; the fields behind an early return keep grid_window's defaults
static GridRect literal_window(const GridCam& C, float x, float y, float r) {
    GridRect R; R.x0 = R.y0 = 0; R.x1 = R.y1 = -1; R.empty = true;
    const int nMinCellX = std::max(0, x86_int(std::floor((double)((x - C.minX - r) * C.wInv))));
    R.x0 = nMinCellX;
    if (nMinCellX >= GRID_COLS) return R;
    const int nMaxCellX = std::min((int)GRID_COLS - 1, x86_int(std::ceil((double)((x - C.minX + r) * C.wInv))));
    R.x1 = nMaxCellX;
    if (nMaxCellX < 0) return R;
    const int nMinCellY = std::max(0, x86_int(std::floor((double)((y - C.minY - r) * C.hInv))));
    R.y0 = nMinCellY;
    if (nMinCellY >= GRID_ROWS) return R;
    const int nMaxCellY = std::min((int)GRID_ROWS - 1, x86_int(std::ceil((double)((y - C.minY + r) * C.hInv))));
    R.y1 = nMaxCellY;
    if (nMaxCellY < 0) return R;
    R.empty = false;
    return R;
}

static void test_window() {
    const float b4[4] = {-12.5f, 760.25f, -8.f, 487.5f};
    const GridCam C = grid_cam(b4);
    if (C.wInv != 64.f / (760.25f + 12.5f) || C.hInv != 48.f / (487.5f + 8.f) || C.minX != b4[0] || C.maxX != b4[1] || C.minY != b4[2] || C.maxY != b4[3]) fail("grid_cam");
    const float inf = INFINITY;
    const float xs[] = {-12.5f, 760.24f, 760.25f, -112.5f, -112.6f, 860.25f, 872.4f, -8.f, 487.4f, 487.5f, -108.f, -108.1f, 587.5f, 597.9f, 376.f, 0.f,
                        1e12f, -1e12f, 1e30f, -1e30f, 3e38f, -3e38f, NAN, inf, -inf};
    const float rs[] = {100.f, 10.f, 0.f, 1e30f, NAN, inf, -5.f};
    for (float x : xs) for (float y : xs) for (float r : rs) {
        GridRect R; grid_window(C, x, y, r, R);
        const GridRect L = literal_window(C, x, y, r);
        if (R.empty != L.empty || R.x0 != L.x0 || R.x1 != L.x1 || R.y0 != L.y0 || R.y1 != L.y1) fail("grid_window differs from Frame.cc:512-526");
        if (!R.empty && (R.x0 < 0 || R.x1 >= GRID_COLS || R.y0 < 0 || R.y1 >= GRID_ROWS || R.x0 > R.x1 || R.y0 > R.y1)) fail("cell rectangle out of the grid");
        sum += R.empty ? 1 : (R.x1 - R.x0 + 1) * (R.y1 - R.y0 + 1);
    }
    // in-image points: the (int)-cast expressions the kernels used before grid_window
    for (int i = 0; i < 10000; i++) {
        const float u = rndf(C.minX, C.maxX), v = rndf(C.minY, C.maxY), radius = rndf(0.5f, 250.f);
        const int x0 = std::max(0, (int)floorf((u - C.minX - radius) * C.wInv));
        const int x1 = std::min((int)GRID_COLS - 1, (int)ceilf((u - C.minX + radius) * C.wInv));
        const int y0 = std::max(0, (int)floorf((v - C.minY - radius) * C.hInv));
        const int y1 = std::min((int)GRID_ROWS - 1, (int)ceilf((v - C.minY + radius) * C.hInv));
        const bool ok = x0 < GRID_COLS && x1 >= 0 && y0 < GRID_ROWS && y1 >= 0;
        GridRect R; grid_window(C, u, v, radius, R);
        if (!ok || R.empty || R.x0 != x0 || R.x1 != x1 || R.y0 != y0 || R.y1 != y1) fail("grid_window differs from the cast form on an in-image point");
        sum += x0 + x1 + y0 + y1;
    }
    for (float q : {0.f, -0.99f, 2147483520.f, -2147483648.f, 12345.7f, -12345.7f}) if (float_to_int(q) != (int)q) fail("float_to_int in range");
    for (float q : {2147483648.f, -2147483904.f, 1e30f, -1e30f, (float)NAN, inf, -inf}) if (float_to_int(q) != INT_MIN) fail("float_to_int out of range");
}

struct Pt { float x, y; };

static void test_scan() {
    const float b4[4] = {0.f, 752.f, 0.f, 480.f};
    const GridCam C = grid_cam(b4);
    const int n = 300, cap = 320;
    std::vector<Pt> kp(n);
    std::vector<int> cell[GRID_COLS][GRID_ROWS];
    for (int i = 0; i < n; i++) {
        kp[i].x = i % 3 == 0 ? rndf(300.f, 360.f) : rndf(0.f, 752.f); kp[i].y = i % 3 == 0 ? rndf(200.f, 240.f) : rndf(0.f, 480.f);   // a crowd and a spread
        const int px = (int)roundf((kp[i].x - C.minX) * C.wInv), py = (int)roundf((kp[i].y - C.minY) * C.hInv);     // Frame::PosInGrid
        if (px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS) cell[px][py].push_back(i);
    }
    // exact-size heap blocks: cell_start [GRID_CELLS + 1], cell_idx [cap]
    std::vector<int> cs(GRID_CELLS + 1), ci(cap, 0);
    int fill = 0;
    for (int ix = 0; ix < GRID_COLS; ix++) for (int iy = 0; iy < GRID_ROWS; iy++) { cs[ix * GRID_ROWS + iy] = fill; for (int i : cell[ix][iy]) ci[fill++] = i; }
    cs[GRID_CELLS] = fill;
    const float wins[][3] = {{330.f, 220.f, 100.f}, {0.f, 0.f, 60.f}, {751.f, 479.f, 35.f}, {376.f, 240.f, 1000.f}, {376.f, 5.f, 12.f}, {-50.f, 240.f, 40.f}, {900.f, 240.f, 40.f}};
    for (const float* w : wins) {
        GridRect R; grid_window(C, w[0], w[1], w[2], R);
        std::vector<int> got, want;
        grid_scan(R, cs.data(), ci.data(), n, cap, [&](int idx) { got.push_back(idx); });
        if (!R.empty)
            for (int ix = R.x0; ix <= R.x1; ix++) for (int iy = R.y0; iy <= R.y1; iy++) for (size_t j = 0; j < cell[ix][iy].size(); j++) want.push_back(cell[ix][iy][j]);
        if (got != want) fail("grid_scan order differs from the ix / iy / insertion loop");
        sum += (long long)got.size();
    }
    // corrupted grids: every visited index in [0, n), every read inside the blocks (the address sanitizer decides)
    GridRect all; grid_window(C, 376.f, 240.f, 1000.f, all);
    for (int kind = 0; kind < 6; kind++) {
        std::vector<int> bs(cs), bi(ci);
        for (int k = 0; k <= GRID_CELLS; k++) {
            if (kind == 0 && k % 7 == 0) bs[k] = -1 - (int)(rnd() % 100000);                         // negative cell_start
            if (kind == 1 && k % 5 == 0) bs[k] = cap + 1 + (int)(rnd() % 100000);                    // entries above cap
            if (kind == 2) bs[k] = cs[GRID_CELLS - k];                                               // descending runs
            if (kind == 3) bs[k] = (int)rnd() - (1 << 23);                                           // anything
            if (kind == 5) bs[k] = k % 2 ? INT_MAX : INT_MIN;
        }
        if (kind == 4 || kind == 3) for (int q = 0; q < cap; q++) if (q % 3 == 0) bi[q] = q % 2 ? n + (int)(rnd() % 1000) : -1 - (int)(rnd() % 1000);   // cell_idx outside 0..n-1
        if (kind == 5) for (int q = 0; q < cap; q++) bi[q] = q % 2 ? INT_MAX : INT_MIN;
        int* hs = new int[GRID_CELLS + 1]; int* hi = new int[cap]; Pt* hk = new Pt[n];
        std::memcpy(hs, bs.data(), sizeof(int) * (GRID_CELLS + 1)); std::memcpy(hi, bi.data(), sizeof(int) * cap); std::memcpy(hk, kp.data(), sizeof(Pt) * n);
        long long visited = 0;
        for (const float* w : wins) {
            GridRect R; grid_window(C, w[0], w[1], w[2], R);
            grid_scan(R, hs, hi, n, cap, [&](int idx) { if (idx < 0 || idx >= n) fail("grid_scan visits an index outside 0..n-1"); visited += (long long)hk[idx].x; });
            int beg, end;
            if (!R.empty) { grid_column(hs, R.x0, R.y0, R.y1, cap, beg, end); if (beg < 0 || end < beg || end > cap) fail("grid_column clamps"); }
        }
        grid_scan(all, hs, hi, 0, cap, [&](int) { fail("grid_scan visits a feature of an empty frame"); });
        sum += visited;
        delete[] hs; delete[] hi; delete[] hk;
    }
}

static int bit_loop(const uint32_t* a, const uint32_t* b) {
    int d = 0;
    for (int w = 0; w < 8; w++) for (int k = 0; k < 32; k++) d += ((a[w] >> k) & 1u) != ((b[w] >> k) & 1u);
    return d;
}
static void check_pair(const uint32_t* a, const uint32_t* b, int want) {
    uint4 h[4];                                          // a's halves, then b as a row of a descriptor array
    std::memcpy(&h[0], a, 32); std::memcpy(&h[2], b, 32);
    const int d = desc_distance(h[0], h[1], h[2], h[3]);
    if (d != bit_loop(a, b) || (want >= 0 && d != want)) fail("desc_distance differs from the bit loop");
    if (desc_distance(h[0], h[1], reinterpret_cast<const uint8_t*>(&h[2])) != d || hamming256(a, b) != d) fail("desc_distance overloads / hamming256 disagree");
    sum += d;
}
static void test_distance() {
    uint32_t a[8], b[8];
    for (int i = 0; i < 2000; i++) { for (int w = 0; w < 8; w++) { a[w] = (rnd() << 8) ^ rnd(); b[w] = i % 4 ? (rnd() << 8) ^ rnd() : a[w] ^ (1u << (rnd() % 32)); } check_pair(a, b, -1); }
    uint32_t zero[8] = {0}, ones[8];
    for (int w = 0; w < 8; w++) ones[w] = 0xffffffffu;
    check_pair(zero, zero, 0); check_pair(ones, ones, 0); check_pair(zero, ones, 256); check_pair(ones, zero, 256);
    for (int w = 0; w < 8; w++) for (int k : {0, 1, 15, 16, 31}) {
        for (int j = 0; j < 8; j++) { a[j] = (rnd() << 8) ^ rnd(); b[j] = a[j]; }
        b[w] ^= 1u << k;
        check_pair(a, b, 1);
    }
}

static void test_rot_bin() {
    const float factor = 1.0f / HISTO_LENGTH;
    for (int i = 0; i < 5000; i++) {                     // angles as the extractor produces them, [0, 360), on a 0.01 degree lattice
        const float a1 = (float)(rnd() % 36000) / 100.f, a2 = (float)(rnd() % 36000) / 100.f;
        float rot = a1 - a2;
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * factor);             // the form of the kernels before rot_bin
        if (bin == HISTO_LENGTH) bin = 0;
        const int b = rot_bin(a1, a2);
        if (b != bin) fail("rot_bin differs from the round / wrap form");
        if (b < 0 || b > 12) fail("rot_bin outside 0..12");
        sum += b;
    }
    if (rot_bin(0.f, 0.f) != 0 || rot_bin(359.99f, 0.f) != 12 || rot_bin(0.f, 359.99f) != 0 || rot_bin(15.f, 0.f) != 1 || rot_bin(14.99f, 0.f) != 0) fail("rot_bin fixed points");
    for (float q : {(float)NAN, 1e30f, -1e30f, (float)INFINITY, -(float)INFINITY})
        if (rot_bin(q, 0.f) != 0 || rot_bin(0.f, q) != 0 || rot_bin(q, q) != 0) fail("a non-finite or huge angle must map to bin 0");
}

// ORBmatcher::ComputeThreeMaxima, src/ORBmatcher.cc:1602-1643, over vectors as the reference holds them
static void literal_maxima(const std::vector<int>* histo, int L, int& ind1, int& ind2, int& ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}
static void check_maxima(const int* hist, int want_removed, int k1, int k2, int k3) {
    std::vector<int> histo[HISTO_LENGTH];
    for (int i = 0; i < HISTO_LENGTH; i++) histo[i].assign((size_t)hist[i], 0);
    int ind1 = -1, ind2 = -1, ind3 = -1;
    literal_maxima(histo, HISTO_LENGTH, ind1, ind2, ind3);
    if (ind1 != k1 || ind2 != k2 || ind3 != k3) fail("the test's expectation differs from the literal ComputeThreeMaxima");
    int keep[HISTO_LENGTH], removed = 0;
    for (int i = 0; i < HISTO_LENGTH; i++) keep[i] = 7;
    const int got = three_maxima(hist, keep);
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int k = (i == ind1 || i == ind2 || i == ind3);
        if (keep[i] != k) fail("three_maxima keeps other bins than ComputeThreeMaxima");
        if (!k) removed += hist[i];
    }
    if (got != removed || got != want_removed) fail("three_maxima returns another count than the bins it removes hold");
    sum += got;
}
static void test_maxima() {
    int h[HISTO_LENGTH];
    auto clear = [&]() { for (int i = 0; i < HISTO_LENGTH; i++) h[i] = 0; };
    clear(); check_maxima(h, 0, -1, -1, -1);                                                        // all zero: nothing kept, nothing removed
    clear(); h[3] = h[7] = h[9] = h[11] = 5; check_maxima(h, 5, 3, 7, 9);                          // ties: the first bins win (strict >)
    clear(); h[11] = 5; h[9] = 5; h[2] = 6; h[20] = 5; check_maxima(h, 5, 2, 9, 11);               // a later larger bin shifts the earlier ones down
    clear(); h[0] = 10; h[1] = 1; h[2] = 1; h[29] = 1; check_maxima(h, 1, 0, 1, 2);                 // 1 < 0.1f * 10 is false: the ratio at equality keeps
    clear(); h[0] = 20; h[1] = 2; h[2] = 1; check_maxima(h, 1, 0, 1, -1);                            // second at equality, third below it
    clear(); h[0] = 20; h[1] = 1; h[2] = 1; check_maxima(h, 2, 0, -1, -1);                           // second below the ratio takes the third with it
    clear(); h[29] = 4; check_maxima(h, 0, 29, -1, -1);                                             // one bin: max2 = 0 < 0.4
    for (int rep = 0; rep < 200; rep++) {                // random histograms against the literal form only
        for (int i = 0; i < HISTO_LENGTH; i++) h[i] = (int)(rnd() % (rep % 2 ? 4 : 40));
        std::vector<int> histo[HISTO_LENGTH];
        for (int i = 0; i < HISTO_LENGTH; i++) histo[i].assign((size_t)h[i], 0);
        int i1 = -1, i2 = -1, i3 = -1, removed = 0;
        literal_maxima(histo, HISTO_LENGTH, i1, i2, i3);
        for (int i = 0; i < HISTO_LENGTH; i++) if (!(i == i1 || i == i2 || i == i3)) removed += h[i];
        check_maxima(h, removed, i1, i2, i3);
    }
}

int main() {
    test_window();
    test_scan();
    test_distance();
    test_rot_bin();
    test_maxima();
    std::printf("checksum %lld\n", sum);
    return 0;
}
