// viorb_amd/csrc/match_core.h — the arithmetic every matcher shares: the 64 x 48 feature grid and its search window, the descriptor
// distance, the rotation histogram. One definition each, for the HIP kernels (frontend_kernels.hip, bow_matcher.hip, sim3_match.hip,
// search_init.hip, orb_extractor.hip, hamming_matcher.hip) and for the host (the viorb_debug_* hooks; tests/cpp/match_core_host_test.cpp
// runs it under the address and undefined-behaviour sanitizers).
//
// What is restated (reference file:line):
//   FRAME_GRID_COLS / FRAME_GRID_ROWS, mfGridElementWidthInv / HeightInv     include/Frame.h:41-42, src/Frame.cc:184-185
//   Frame::GetFeaturesInArea, KeyFrame::GetFeaturesInArea (the cell rectangle) src/Frame.cc:512-526, src/KeyFrame.cc:906-925
//   the walk over the rectangle (ix outer, iy inner, insertion order)          src/Frame.cc:530-557, src/KeyFrame.cc:927-942
//   ORBmatcher::TH_LOW, TH_HIGH, HISTO_LENGTH                                  src/ORBmatcher.cc:37-39
//   ORBmatcher::DescriptorDistance                                             src/ORBmatcher.cc:1648-1664
//   the rotation bin (rot, + 360, round(rot * factor), 30 wraps to 0)          src/ORBmatcher.cc:475-480, also :238-243, :766-771, :1434-1439
//   ORBmatcher::ComputeThreeMaxima                                             src/ORBmatcher.cc:1602-1643
// Everything is integer arithmetic, float compares and individually rounded float products; nothing depends on contraction.
#pragma once
#include <limits.h>
#include "orb_math.h"

namespace viorb {

enum { GRID_COLS = 64, GRID_ROWS = 48, GRID_CELLS = GRID_COLS * GRID_ROWS, TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30 };

// The image bounds and the cells per pixel of a frame's grid.
struct GridCam { float minX, maxX, minY, maxY, wInv, hInv; };
VIORB_HD GridCam grid_cam(const float* bounds4) {                    // bounds4 = minX maxX minY maxY
    GridCam C;
    C.minX = bounds4[0]; C.maxX = bounds4[1]; C.minY = bounds4[2]; C.maxY = bounds4[3];
    C.wInv = static_cast<float>(GRID_COLS) / static_cast<float>(C.maxX - C.minX);        // Frame.cc:184-185
    C.hInv = static_cast<float>(GRID_ROWS) / static_cast<float>(C.maxY - C.minY);
    return C;
}

// (int) of a float as x86 converts it: a value no int holds (a window far outside the image, a non-finite quotient) gives INT_MIN, on the
// host, where the bare cast is undefined, and on the device, where it saturates, alike
VIORB_HD int float_to_int(float q) { return (q > -2147483648.0f && q < 2147483648.0f) ? (int)q : INT_MIN; }

// nMinCellX nMaxCellX nMinCellY nMaxCellY; empty: one of the four early returns fired (the fields behind it keep x1 = y1 = -1, y0 = 0)
struct GridRect { int x0, x1, y0, y1; bool empty; };

// GetFeaturesInArea :512-526: the float expressions, floor / ceil, the clamps and the early returns in the reference's order
VIORB_HD void grid_window(const GridCam& C, float x, float y, float r, GridRect& R) {
    R.x0 = R.y0 = 0; R.x1 = R.y1 = -1; R.empty = true;
    const int a = float_to_int(floorf((x - C.minX - r) * C.wInv));
    R.x0 = a < 0 ? 0 : a;
    if (R.x0 >= GRID_COLS) return;
    const int b = float_to_int(ceilf((x - C.minX + r) * C.wInv));
    R.x1 = b > GRID_COLS - 1 ? GRID_COLS - 1 : b;
    if (R.x1 < 0) return;
    const int c = float_to_int(floorf((y - C.minY - r) * C.hInv));
    R.y0 = c < 0 ? 0 : c;
    if (R.y0 >= GRID_ROWS) return;
    const int d = float_to_int(ceilf((y - C.minY + r) * C.hInv));
    R.y1 = d > GRID_ROWS - 1 ? GRID_ROWS - 1 : d;
    if (R.y1 < 0) return;
    R.empty = false;
}

// The entries [beg, end) of column ix of a window in the CSR grid (cell_start [GRID_CELLS + 1], cell index ix*48 + iy: the cells of one
// column are adjacent). Clamped into 0..cap, end >= beg, so that a grid that was not built for these arrays cannot send a read out of them.
VIORB_HD void grid_column(const int* cs, int ix, int y0, int y1, int cap, int& beg, int& end) {
    const int s = cs[ix * GRID_ROWS + y0], e = cs[ix * GRID_ROWS + y1 + 1];
    beg = s < 0 ? 0 : (s > cap ? cap : s);
    end = e < beg ? beg : (e > cap ? cap : e);
}

// visit(idx) for every feature of the window's cells in GetFeaturesInArea's order: columns outer, rows inner, insertion order inside a
// cell. ci [cap] holds feature indices; one outside 0..n-1 is skipped. The distance test |dx| < r, |dy| < r is the visitor's.
template <class Visit> VIORB_HD void grid_scan(const GridRect& R, const int* cs, const int* ci, int n, int cap, Visit&& visit) {
    if (R.empty) return;
    for (int ix = R.x0; ix <= R.x1; ix++) {
        int beg, end;
        grid_column(cs, ix, R.y0, R.y1, cap, beg, end);
        for (int q = beg; q < end; q++) {
            const int idx = ci[q];
            if ((unsigned)idx < (unsigned)n) visit(idx);
        }
    }
}

#if !defined(__HIPCC__)
struct alignas(16) uint4 { uint32_t x, y, z, w; };                   // the host build's stand-in for HIP's vector type
#endif

// DescriptorDistance of two 256-bit descriptors, each held as two 128-bit halves. The halves are taken by value: with references the
// candidate loop of k_search_by_bow compiled to other instructions than with the expression written in place.
VIORB_HD int desc_distance(const uint4 da, const uint4 db, const uint4 ea, const uint4 eb) {
    return __builtin_popcount(da.x ^ ea.x) + __builtin_popcount(da.y ^ ea.y) + __builtin_popcount(da.z ^ ea.z) + __builtin_popcount(da.w ^ ea.w) +
           __builtin_popcount(db.x ^ eb.x) + __builtin_popcount(db.y ^ eb.y) + __builtin_popcount(db.z ^ eb.z) + __builtin_popcount(db.w ^ eb.w);
}
// the second descriptor from its row of a descriptor array (32 bytes, 16-byte aligned)
VIORB_HD int desc_distance(const uint4 da, const uint4 db, const uint8_t* row) {
    const uint4* dc = reinterpret_cast<const uint4*>(row);
    const uint4 ea = dc[0], eb = dc[1];
    return desc_distance(da, db, ea, eb);
}

// rot = angle1 - angle2 in float, + 360 when negative, round half away from zero of rot * (1.0f / 30), 30 wraps to 0. The reference
// asserts the range (angles are in [0, 360)); a value outside it (a NaN angle) goes to bin 0 here, never out of the histogram.
VIORB_HD int rot_bin(float angle1, float angle2) {
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = angle1 - angle2;
    if (rot < 0.0f) rot += 360.0f;
    const float b = roundf(rot * factor);
    return (b >= 0.0f && b < (float)HISTO_LENGTH) ? (int)b : 0;
}

// ComputeThreeMaxima over the bins' sizes: keep[i] = bin i is one of ind1 ind2 ind3. Returns the entries of the bins it removes.
VIORB_HD int three_maxima(const int* hist, int* keep) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int sz = hist[i];
        if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
        else if (sz > max3) { max3 = sz; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
    int removed = 0;
    for (int i = 0; i < HISTO_LENGTH; i++) { const int k = (i == ind1 || i == ind2 || i == ind3); keep[i] = k; if (!k) removed += hist[i]; }
    return removed;
}

#if defined(__HIPCC__)
// The workgroup's count of `flag`, returned to every thread: the wavefronts' ballots, one LDS word per wavefront (s_part [blockDim.x / 64]).
// Every thread of the workgroup calls it.
__device__ __forceinline__ int block_count(bool flag, int* s_part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x / 64, nw = (blockDim.x + 63) / 64;
    const int c = __popcll(__ballot(flag));
    if (lane == 0) s_part[w] = c;
    __syncthreads();
    int total = 0;
    for (int k = 0; k < nw; k++) total += s_part[k];
    __syncthreads();
    return total;
}
#endif

} // namespace viorb
