// viorb_amd/csrc/search_init.hip — the monocular matcher and the scene depth of map initialisation (include/viorb_search_init.h):
//   k_si_candidates   ORBmatcher::SearchForInitialization, the window scan of every point      reference src/ORBmatcher.cc:418-442, Frame.cc:507-560
//   k_si_ordered      the point-order loop (:444-471) as sweeps, then the rotation step, prev_matched and the counts (:489-519)
//   k_si_median       KeyFrame::ComputeSceneMedianDepth                                            src/KeyFrame.cc:970-1000
// The arithmetic is search_init_core.h. Shape (DESIGN.md "Monocular matcher"): the window is 200 x 200 pixels, some 360 cells and hundreds
// of features, so the candidate pass gives a wavefront to a point and spreads the window's grid entries over its lanes; a ballot and a
// prefix rank keep GetFeaturesInArea's visiting order. The ordered phase is one workgroup per stream: a sweep evaluates every point
// against the previous sweep's states, with the points accepted on a feature chained from one LDS word per feature.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "search_init_core.h"

namespace viorb {

enum { SI_WAVE = 64, SI_POINTS = 4, SI_BLOCK = SI_WAVE * SI_POINTS, SI_LIST = 16, SI_ORDERED_THREADS = 1024, SI_MEDIAN_THREADS = 256 };

struct SiKf { const viorb_keypoint* kps; const uint8_t* desc; const int* count; const int* cell_start; const int* cell_idx; };
struct SiArgs {
    const viorb_keypoint* kps1; const uint8_t* desc1; const int* n1; SiKf kf2; float* prev;
    uint32_t* cand; int* cand_n; int* why; uint32_t* st; uint32_t* st2; int* next;     // workspace: cand [batch][SI_LIST][cap], the rest [batch][cap]
    int* matches12; int* nmatches; viorb_search_init_outputs out;             // out: every pointer may be NULL
    GridCam cam; float r, nnratio; int check_ori, cap;
};

// blockIdx = (chunk of SI_POINTS points, stream); one wavefront per point of frame 1. Writes the point's list (candidates si_keep admits,
// in visiting order; the count goes on past SI_LIST and k_si_ordered rescans the window of such a point), its first reason, xy1 and xy2.
__global__ __launch_bounds__(SI_BLOCK) void k_si_candidates(SiArgs A) {
    const int lane = threadIdx.x & (SI_WAVE - 1), b = blockIdx.y, i = blockIdx.x * SI_POINTS + threadIdx.x / SI_WAVE, cap = A.cap;
    if (i >= cap) return;                                            // the whole wavefront; the kernel has no barrier
    const int n1 = min(max(A.n1[b], 0), cap), n2 = min(max(A.kf2.count[b], 0), cap);
    const size_t o = (size_t)b * cap + i;
    const viorb_keypoint* kp2 = A.kf2.kps + (size_t)b * cap;
    if (lane < 2) {
        if (A.out.xy1) A.out.xy1[o * 2 + lane] = i < n1 ? (lane ? A.kps1[o].y : A.kps1[o].x) : 0.0f;
        if (A.out.xy2) A.out.xy2[o * 2 + lane] = i < n2 ? (lane ? kp2[i].y : kp2[i].x) : 0.0f;
    }
    int ncand = 0, why = SI_NOT_CANDIDATE;
    const int level1 = i < n1 ? A.kps1[o].octave : 1;
    if (level1 <= 0) {                                               // :422
        const float x = A.prev[o * 2], y = A.prev[o * 2 + 1], r = A.r;
        GridRect R;
        grid_window(A.cam, x, y, r, R);
        int nwin = 0;
        if (!R.empty && n2 > 0) {
            const int* cs = A.kf2.cell_start + (size_t)b * (GRID_CELLS + 1);
            const int* ci = A.kf2.cell_idx + (size_t)b * cap;
            const uint8_t* desc2 = A.kf2.desc + (size_t)b * cap * 32;
            const uint4* dl = reinterpret_cast<const uint4*>(A.desc1 + o * 32);
            const uint4 da = dl[0], db = dl[1];
            uint32_t* list = A.cand + (size_t)b * SI_LIST * cap + i;
            // lane c holds column x0 + c of the window (at most 64 columns): its run of the CSR and the run's offset in the window's sequence
            int beg = 0, len = 0;
            if (lane <= R.x1 - R.x0) { int end; grid_column(cs, R.x0 + lane, R.y0, R.y1, cap, beg, end); len = end - beg; }
            int incl = len;
#pragma unroll
            for (int s = 1; s < SI_WAVE; s <<= 1) { const int v = __shfl_up(incl, s); if (lane >= s) incl += v; }
            const int excl = incl - len, total = __shfl(incl, SI_WAVE - 1);
            for (int base = 0; base < total; base += SI_WAVE) {
                const int e = base + lane;
                int c = 0;                                           // the last column whose offset is <= e: the one that holds entry e
#pragma unroll
                for (int s = SI_WAVE / 2; s >= 1; s >>= 1) { const int v = __shfl(excl, c + s); if (v <= e) c += s; }
                const int q = __shfl(beg, c) + (e - __shfl(excl, c));
                bool pass = false;
                int idx = 0, d = 0;
                if (e < total) {
                    idx = ci[q];
                    if ((unsigned)idx < (unsigned)n2) {
                        const viorb_keypoint k = kp2[idx];
                        pass = si_level_ok(level1, k.octave) && fabsf(k.x - x) < r && fabsf(k.y - y) < r;
                    }
                }
                if (pass) d = desc_distance(da, db, desc2 + (size_t)idx * 32);
                const bool keep = pass && si_keep(d, A.nnratio);
                nwin += __popcll(__ballot(pass));
                const unsigned long long km = __ballot(keep);
                const int pos = ncand + __popcll(km & ((1ull << lane) - 1ull));
                if (keep && pos < SI_LIST) list[(size_t)pos * cap] = ((uint32_t)d << 16) | (uint32_t)idx;
                ncand += __popcll(km);
            }
        }
        why = nwin == 0 ? SI_NO_FEATURE_IN_WINDOW : SI_ABOVE_THRESHOLD;
    }
    if (lane == 0) { A.cand_n[o] = ncand; A.why[o] = why; }
}

// One workgroup per stream: the sweeps of si_ordered_sweeps (search_init_core.h) with the points of a sweep in parallel, then what follows
// the main loop. s_head[f] chains the points accepted on feature f (LDS exchange; the order of a chain does not matter to si_seen). The
// states of a sweep are read from one array and written to the other, so a run does not depend on the order of the threads.
__global__ __launch_bounds__(SI_ORDERED_THREADS) void k_si_ordered(SiArgs A) {
    extern __shared__ int s_head[];
    __shared__ int s_part[SI_ORDERED_THREADS / SI_WAVE];
    __shared__ int s_hist[HISTO_LENGTH], s_keep[HISTO_LENGTH];
    const int b = blockIdx.x, t = threadIdx.x, cap = A.cap;
    const int n1 = min(max(A.n1[b], 0), cap), n2 = min(max(A.kf2.count[b], 0), cap);
    const size_t ob = (size_t)b * cap;
    const viorb_keypoint* kp1 = A.kps1 + ob;
    const viorb_keypoint* kp2 = A.kf2.kps + ob;
    const int* cand_n = A.cand_n + ob;
    const uint32_t* cand = A.cand + (size_t)b * SI_LIST * cap;
    int* why = A.why + ob;
    int* next = A.next + ob;
    uint32_t* cur = A.st + ob;
    uint32_t* nxt = A.st2 + ob;
    for (int p = t; p < cap; p += blockDim.x) { cur[p] = SI_NONE; nxt[p] = SI_NONE; }
    if (t < HISTO_LENGTH) { s_hist[t] = 0; s_keep[t] = 1; }
    __syncthreads();
    int sweeps = 0;
    for (;;) {
        sweeps++;
        for (int f = t; f < n2; f += blockDim.x) s_head[f] = -1;
        __syncthreads();
        for (int p = t; p < n1; p += blockDim.x) { const uint32_t s = cur[p]; if (s != SI_NONE) next[p] = atomicExch(&s_head[s & 0xffffu], p); }
        __syncthreads();
        int changed = 0;
        for (int p = t; p < n1; p += blockDim.x) {
            const int nc = cand_n[p];
            if (nc == 0) continue;
            SiPick P;
            si_pick_init(P);
            if (nc <= SI_LIST) {
                for (int k = 0; k < nc; k++) {
                    const uint32_t e = cand[(size_t)k * cap + p];
                    const int f = (int)(e & 0xffffu);
                    si_pick_visit(P, (int)(e >> 16), f, si_seen(s_head, next, cur, f, p));
                }
            } else {                                                 // more candidates than the list holds: the window again, nothing left out
                const float x = A.prev[(ob + p) * 2], y = A.prev[(ob + p) * 2 + 1], r = A.r;
                const int level1 = kp1[p].octave;
                GridRect R;
                grid_window(A.cam, x, y, r, R);
                const int* cs = A.kf2.cell_start + (size_t)b * (GRID_CELLS + 1);
                const int* ci = A.kf2.cell_idx + ob;
                const uint8_t* desc2 = A.kf2.desc + ob * 32;
                const uint4* dl = reinterpret_cast<const uint4*>(A.desc1 + (ob + p) * 32);
                const uint4 da = dl[0], db = dl[1];
                grid_scan(R, cs, ci, n2, cap, [&](int idx) {
                    const viorb_keypoint k = kp2[idx];
                    if (!(si_level_ok(level1, k.octave) && fabsf(k.x - x) < r && fabsf(k.y - y) < r)) return;
                    si_pick_visit(P, desc_distance(da, db, desc2 + (size_t)idx * 32), idx, si_seen(s_head, next, cur, idx, p));
                });
            }
            int w;
            const uint32_t s = si_decide(P, A.nnratio, w);
            nxt[p] = s; why[p] = w;
            changed |= s != cur[p];
        }
        uint32_t* sw = cur; cur = nxt; nxt = sw;
        if (!__syncthreads_or(changed)) break;
        if (sweeps > n1) break;                                      // n1 + 1 sweeps always suffice (search_init_core.h); never a longer loop
    }
    // vnMatches21: the latest point accepted on each feature
    for (int f = t; f < n2; f += blockDim.x) s_head[f] = -1;
    __syncthreads();
    for (int p = t; p < n1; p += blockDim.x) { const uint32_t s = cur[p]; if (s != SI_NONE) atomicMax(&s_head[s & 0xffffu], p); }
    __syncthreads();
    if (A.check_ori) {                                               // rotHist keeps a displaced point (:482 is never undone)
        for (int p = t; p < n1; p += blockDim.x) {
            const uint32_t s = cur[p];
            if (s != SI_NONE) atomicAdd(&s_hist[rot_bin(kp1[p].angle, kp2[s & 0xffffu].angle)], 1);
        }
        __syncthreads();
        if (t == 0) three_maxima(s_hist, s_keep);
        __syncthreads();
    }
    int found = 0;
    for (int base = 0; base < cap; base += blockDim.x) {
        const int p = base + t;
        int m = -1;
        if (p < cap) {
            int reason = SI_NOT_CANDIDATE;
            if (p < n1) {
                const uint32_t s = cur[p];
                reason = why[p];
                if (s != SI_NONE) {
                    const int f = (int)(s & 0xffffu);
                    if (s_head[f] != p) reason = SI_DISPLACED;
                    else if (A.check_ori && !s_keep[rot_bin(kp1[p].angle, kp2[f].angle)]) reason = SI_ROTATION;
                    else { reason = SI_MATCHED; m = f; }
                }
            }
            A.matches12[ob + p] = m;
            if (A.out.reason) A.out.reason[ob + p] = reason;
            if (m >= 0) { A.prev[(ob + p) * 2] = kp2[m].x; A.prev[(ob + p) * 2 + 1] = kp2[m].y; }      // :515-517
        }
        found += block_count(m >= 0, s_part);
    }
    if (A.out.matches21 || A.out.matched_distance)
        for (int f = t; f < cap; f += blockDim.x) {
            const int p = f < n2 ? s_head[f] : -1;
            if (A.out.matches21) A.out.matches21[ob + f] = p;
            if (A.out.matched_distance) A.out.matched_distance[ob + f] = p >= 0 ? (int)(cur[p] >> 16) : INT_MAX;
        }
    if (A.out.rot_hist && t < HISTO_LENGTH) A.out.rot_hist[(size_t)b * HISTO_LENGTH + t] = s_hist[t];
    if (t == 0) { A.nmatches[b] = found; if (A.out.sweeps) A.out.sweeps[b] = sweeps; }
}

// One workgroup per key frame: the depths are recomputed in every pass (three products), so the kernel needs no scratch. Pass 0 counts
// the points, four passes select the (n - 1) / q-th smallest key one 8-bit digit at a time (the select of k_tv_check_rt).
__global__ __launch_bounds__(SI_MEDIAN_THREADS) void k_si_median(const float* __restrict__ pose12, const float* __restrict__ points,
                                                                 const uint8_t* __restrict__ has_point, const int* __restrict__ count, int cap, int q,
                                                                 float* __restrict__ median, int* __restrict__ n_depths) {
    __shared__ int s_hist[256];
    __shared__ int s_part[SI_MEDIAN_THREADS / SI_WAVE];
    __shared__ uint32_t s_prefix;
    __shared__ int s_k;
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = min(max(count[b], 0), cap);
    const float* pose = pose12 + (size_t)b * 12;
    const float* X = points + (size_t)b * cap * 3;
    const uint8_t* hp = has_point + (size_t)b * cap;
    int ng = 0;
    for (int base = 0; base < n; base += SI_MEDIAN_THREADS) { const int i = base + t; ng += block_count(i < n && hp[i], s_part); }
    if (ng == 0) { if (t == 0) { median[b] = -1.0f; n_depths[b] = 0; } return; }
    if (t == 0) { s_prefix = 0; s_k = (ng - 1) / q; }
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        s_hist[t] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (int i = t; i < n; i += SI_MEDIAN_THREADS)
            if (hp[i]) { const uint32_t key = tv_float_key(si_depth(pose, X + (size_t)i * 3)); if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255], 1); }
        __syncthreads();
        if (t == 0) { int k = s_k; const int d = si_select_digit(s_hist, k); s_k = k; s_prefix = prefix | ((uint32_t)d << shift); }
        __syncthreads();
    }
    if (t == 0) { median[b] = tv_key_float(s_prefix); n_depths[b] = ng; }
}

} // namespace viorb

using namespace viorb;

namespace {

struct SiLayout { uint32_t* cand; int* cand_n; int* why; uint32_t* st; uint32_t* st2; int* next; size_t total; };
SiLayout si_layout(void* base, int cap, int batch) {
    SiLayout L; WorkspaceLayout Y(base);
    const size_t n = (size_t)batch * cap;
    Y.take(&L.cand, n * SI_LIST); Y.take(&L.cand_n, n); Y.take(&L.why, n); Y.take(&L.st, n); Y.take(&L.st2, n); Y.take(&L.next, n);
    L.total = Y.end();
    return L;
}
bool si_sizes_ok(int cap, int batch) { return cap >= 1 && cap <= VIORB_S3M_MAX_FEATURES && batch >= 1 && batch <= 65535; }

int si_check_common(int cap, int batch, const float* bounds4, int window_size, float nnratio) {
    VIORB_REQUIRE(bounds4, "null array");
    VIORB_REQUIRE(cap >= 1, "cap >= 1");
    VIORB_REQUIRE(batch >= 1 && batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(window_size > 0, "window_size > 0");
    VIORB_REQUIRE(nnratio > 0, "nnratio > 0");
    VIORB_REQUIRE(bounds4[1] > bounds4[0] && bounds4[3] > bounds4[2], "empty image bounds");
    if (cap > VIORB_S3M_MAX_FEATURES) { set_error("cap %d above VIORB_S3M_MAX_FEATURES", cap); return VIORB_ERR_CAPACITY; }
    return VIORB_OK;
}

} // namespace

extern "C" {

size_t viorb_search_init_workspace_bytes(int cap, int batch) {
    if (!si_sizes_ok(cap, batch)) return 0;
    return si_layout(nullptr, cap, batch).total;
}

int viorb_search_init_shape(int32_t* out4) {
    VIORB_REQUIRE(out4, "null array");
    out4[0] = SI_POINTS; out4[1] = SI_WAVE; out4[2] = SI_LIST; out4[3] = SI_ORDERED_THREADS;
    return VIORB_OK;
}

int viorb_search_for_initialization_device(const viorb_keypoint* kps1, const uint8_t* desc1, const int32_t* n1, const viorb_s3m_keyframes* kf2,
                                           float* prev_matched, int cap, int batch, const float bounds4[4], int window_size, float nnratio,
                                           int check_orientation, int32_t* matches12, int32_t* nmatches,
                                           const viorb_search_init_outputs* out, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_TRY(si_check_common(cap, batch, bounds4, window_size, nnratio));
    VIORB_REQUIRE(kps1 && desc1 && n1 && prev_matched && matches12 && nmatches, "null array");
    VIORB_REQUIRE(kf2 && kf2->kps && kf2->desc && kf2->count && kf2->cell_start && kf2->cell_idx, "null array");
    VIORB_REQUIRE(kf2->cap == cap, "the capacity of frame 2 must equal cap");
    VIORB_REQUIRE(workspace && workspace_bytes >= si_layout(nullptr, cap, batch).total && ((uintptr_t)workspace & 255) == 0,
                  "workspace smaller than viorb_search_init_workspace_bytes or not 256-byte aligned");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const SiLayout L = si_layout(workspace, cap, batch);
    SiArgs A;
    A.kps1 = kps1; A.desc1 = desc1; A.n1 = n1; A.prev = prev_matched;
    A.kf2.kps = kf2->kps; A.kf2.desc = kf2->desc; A.kf2.count = kf2->count; A.kf2.cell_start = kf2->cell_start; A.kf2.cell_idx = kf2->cell_idx;
    A.cand = L.cand; A.cand_n = L.cand_n; A.why = L.why; A.st = L.st; A.st2 = L.st2; A.next = L.next;
    A.matches12 = matches12; A.nmatches = nmatches;
    if (out) A.out = *out; else memset(&A.out, 0, sizeof(A.out));
    A.cam = grid_cam(bounds4); A.r = (float)window_size; A.nnratio = nnratio; A.check_ori = check_orientation ? 1 : 0; A.cap = cap;
    VIORB_LAUNCH(k_si_candidates, dim3((cap + SI_POINTS - 1) / SI_POINTS, batch), SI_BLOCK, 0, st, A);
    const size_t lds = (size_t)cap * sizeof(int);                    // cap <= VIORB_S3M_MAX_FEATURES: at most 64 KiB beside the static words
    if (lds > 48 * 1024) VIORB_HIP_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(k_si_ordered), lds));
    VIORB_LAUNCH(k_si_ordered, batch, SI_ORDERED_THREADS, lds, st, A);
    return VIORB_OK;
}

int viorb_search_for_initialization(const viorb_keypoint* kps1, const uint8_t* desc1, int n1, const viorb_keypoint* kps2, const uint8_t* desc2,
                                    int n2, float* prev_matched, const float bounds4[4], int window_size, float nnratio, int check_orientation,
                                    int32_t* matches12, int32_t* nmatches, const viorb_search_init_outputs* out) {
    VIORB_REQUIRE(n1 >= 0 && n2 >= 0 && nmatches, "null array or a negative count");
    const int cap = std::max(std::max(n1, n2), 1);
    VIORB_TRY(si_check_common(cap, 1, bounds4, window_size, nnratio));
    VIORB_REQUIRE(n1 == 0 || (kps1 && desc1 && prev_matched && matches12), "null array");
    VIORB_REQUIRE(n2 == 0 || (kps2 && desc2), "null array");
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t c = (size_t)cap, m1 = (size_t)n1, m2 = (size_t)n2;
    viorb_keypoint* dk1 = B.up(kps1, m1, c); uint8_t* dd1 = B.up(desc1, m1 * 32, c * 32); int32_t* dn1 = B.up(&n1, 1);
    float* dprev = B.up(prev_matched, m1 * 2, c * 2);
    int32_t *d12 = B.zeros<int32_t>(c), *dnm = B.zeros<int32_t>(1);
    viorb_search_init_outputs D;
    D.matches21 = B.zeros<int32_t>(c); D.matched_distance = B.zeros<int32_t>(c); D.rot_hist = B.zeros<int32_t>(HISTO_LENGTH); D.reason = B.zeros<int32_t>(c);
    D.xy1 = B.zeros<float>(c * 2); D.xy2 = B.zeros<float>(c * 2); D.sweeps = B.zeros<int32_t>(1);
    const size_t wb = viorb_search_init_workspace_bytes(cap, 1);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    viorb_s3m_keyframes kf;
    VIORB_TRY(host_keyframe(B, kps2, desc2, n2, cap, bounds4, kf));
    VIORB_TRY(viorb_search_for_initialization_device(dk1, dd1, dn1, &kf, dprev, cap, 1, bounds4, window_size, nnratio, check_orientation, d12, dnm, &D,
                                                     dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_TRY(download(matches12, d12, m1)); VIORB_TRY(download(nmatches, dnm, 1)); VIORB_TRY(download(prev_matched, dprev, m1 * 2));
    if (out) {
        VIORB_TRY(download(out->matches21, D.matches21, m2)); VIORB_TRY(download(out->matched_distance, D.matched_distance, m2));
        VIORB_TRY(download(out->rot_hist, D.rot_hist, (size_t)HISTO_LENGTH)); VIORB_TRY(download(out->reason, D.reason, m1));
        VIORB_TRY(download(out->xy1, D.xy1, m1 * 2)); VIORB_TRY(download(out->xy2, D.xy2, m2 * 2)); VIORB_TRY(download(out->sweeps, D.sweeps, 1));
    }
    return VIORB_OK;
}

int viorb_scene_median_depth_device(const float* pose12, const float* points, const uint8_t* has_point, const int32_t* count, int cap, int batch,
                                    int q, float* median, int32_t* n_depths, void* stream) {
    VIORB_REQUIRE(pose12 && points && has_point && count && median && n_depths, "null array");
    VIORB_REQUIRE(cap >= 1, "cap >= 1");
    VIORB_REQUIRE(batch >= 1 && batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(q >= 1, "q >= 1");
    VIORB_TRY(require_device());
    VIORB_LAUNCH(k_si_median, batch, SI_MEDIAN_THREADS, 0, (hipStream_t)stream, pose12, points, has_point, count, cap, q, median, n_depths);
    return VIORB_OK;
}

int viorb_scene_median_depth(const float pose12[12], const float* points, const uint8_t* has_point, int n, int q, float* median, int32_t* n_depths) {
    VIORB_REQUIRE(pose12 && median && n_depths && n >= 0 && (n == 0 || (points && has_point)), "null array or a negative count");
    VIORB_REQUIRE(q >= 1, "q >= 1");
    VIORB_TRY(require_device());
    DeviceBufs B;
    const size_t m = (size_t)n, c = (size_t)std::max(n, 1);
    float* dp = B.up(pose12, 12); float* dx = B.up(points, m * 3, c * 3); uint8_t* dh = B.up(has_point, m, c); int32_t* dn = B.up(&n, 1);
    float* dm = B.zeros<float>(1); int32_t* dc = B.zeros<int32_t>(1);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_scene_median_depth_device(dp, dx, dh, dn, (int)c, 1, q, dm, dc, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_TRY(download(median, dm, 1));
    return download(n_depths, dc, 1);
}

// ---- host-only test hooks: search_init_core.h compiled for the host --------------------------------------------------------------------
int viorb_debug_search_init_ordered(const uint32_t* cand, const int32_t* cand_n, int npts, int lcap, int nfeat, float nnratio, uint32_t* state,
                                    int32_t* why, int32_t* matches12, int32_t* matches21, int32_t* matched_distance, int32_t* nmatches) {
    VIORB_REQUIRE(npts >= 0 && lcap >= 1 && nfeat >= 0 && nfeat <= 65536 && nnratio > 0 && nmatches, "null array or a size outside its range");
    VIORB_REQUIRE(npts == 0 || (cand && cand_n && state && why && matches12), "null array");
    VIORB_REQUIRE(nfeat == 0 || (matches21 && matched_distance), "null array");
    std::vector<uint32_t> st2((size_t)std::max(npts, 1));
    std::vector<int> head((size_t)std::max(nfeat, 1)), next((size_t)std::max(npts, 1));
    const int sweeps = si_ordered_sweeps(cand, cand_n, npts, lcap, nfeat, nnratio, state, st2.data(), why, head.data(), next.data());
    *nmatches = si_after_loop(state, npts, nfeat, matches12, matches21, matched_distance);
    return sweeps;
}

int viorb_debug_search_init_window(const viorb_keypoint* kps2, int n2, const int32_t* cell_start, const int32_t* cell_idx, const float bounds4[4],
                                   float x, float y, float r, int level1, int32_t* rect4, int32_t* out_idx) {
    VIORB_REQUIRE(n2 >= 0 && cell_start && bounds4 && rect4 && (n2 == 0 || (kps2 && cell_idx && out_idx)), "null array or a negative count");
    VIORB_REQUIRE(bounds4[1] > bounds4[0] && bounds4[3] > bounds4[2], "empty image bounds");
    GridRect R;
    grid_window(grid_cam(bounds4), x, y, r, R);
    rect4[0] = R.x0; rect4[1] = R.x1; rect4[2] = R.y0; rect4[3] = R.y1;
    int n = 0;
    grid_scan(R, cell_start, cell_idx, n2, n2, [&](int idx) {
        const viorb_keypoint& k = kps2[idx];
        if (si_level_ok(level1, k.octave) && fabsf(k.x - x) < r && fabsf(k.y - y) < r) out_idx[n++] = idx;
    });
    return n;
}

float viorb_debug_scene_depth(const float* pose12, const float* point3) {
    if (!pose12 || !point3) return 0.0f;
    return si_depth(pose12, point3);
}

} // extern "C"
