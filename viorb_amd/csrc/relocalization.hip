// viorb_amd/csrc/relocalization.hip — relocalisation after the PnP hypothesis (include/viorb_relocalization.h):
//   k_reloc_gates   SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist): gates + candidate lists   reference src/ORBmatcher.cc:1489-1554
//   k_reloc_claim   the point-order claim, the rotation histogram, the removals and the count                    :1536-1597
//   k_reloc_step    the bookkeeping of Tracking::Relocalization between its solves and searches                 src/Tracking.cc:2209-2273
// The arithmetic is reloc_core.h. Shape (DESIGN.md "Relocalisation"): that of the Sim3 matchers, for the same kind of workload (one lost
// frame, a handful of candidates of about a thousand points each, latency at small batch deciding): a lane per key-frame point, RELOC_BLOCK
// points per workgroup, the grid over (point chunk, hypothesis); then one workgroup per hypothesis runs the claim as the fixed-point sweeps
// k_s3m_claim runs (s3m_claim_sweeps of sim3_match_core.h, one LDS word per frame feature) and the histogram on 30 LDS counters. The result
// arrays are written with plain stores; the only atomics are on LDS scratch.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "reloc_core.h"

namespace viorb {

enum { RELOC_BLOCK = 256, RELOC_WAVE = 64, RELOC_LIST = 8, RELOC_CLAIM_THREADS = 1024, RELOC_STEP_THREADS = 256 };

struct RelocKf { const viorb_keypoint* kps; const uint8_t* desc; const int* count; const int* cell_start; const int* cell_idx; int cap; };

struct RelocArgs {
    RelocKf fr; int n_frames; const int* hyp_frame; const float* pose12;
    const float* kf_angle; const uint8_t* kf_valid; const uint8_t* kf_found; const float* pts_f; const uint8_t* pts_desc; const int* kf_count;
    const uint8_t* feat_taken;
    int* best_idx; int* nmatches; int* reason;      // reason may be NULL
    uint32_t* cand; int* cand_n;                    // [batch][RELOC_LIST][kcap] (entry k of point i at k * kcap + i), [batch][kcap]
    int kcap, orb_dist, check_ori;
    S3mCam cam;
};

// the frame of hypothesis b and its feature count: an index outside 0..n_frames-1 is a frame without features
__device__ __forceinline__ int reloc_frame(const RelocArgs& A, int b, int& n) {
    const int f = A.hyp_frame ? A.hyp_frame[b] : b;
    const bool ok = (unsigned)f < (unsigned)A.n_frames;
    n = ok ? min(max(A.fr.count[f], 0), A.fr.cap) : 0;
    return ok ? f : 0;
}

// blockIdx = (point chunk, hypothesis): a point's candidates of distance <= orb_dist that are free on entry go to its list in visiting
// order, the count goes on past RELOC_LIST (k_reloc_claim rescans the window of such a point); best_idx is left to k_reloc_claim
__global__ __launch_bounds__(RELOC_BLOCK) void k_reloc_gates(RelocArgs A) {
    const int b = blockIdx.y, i = blockIdx.x * RELOC_BLOCK + threadIdx.x, kcap = A.kcap, cap = A.fr.cap;
    if (i >= kcap) return;
    int n;
    const int f = reloc_frame(A, b, n);
    const int npts = min(max(A.kf_count[b], 0), kcap);
    const size_t o = (size_t)b * kcap + i;
    int reason = S3M_NOT_CANDIDATE, ncand = 0;
    if (i < npts && A.kf_valid[o] && !A.kf_found[o]) {
        const float* X = A.pts_f + o * 8;
        float x8[8], pose[12];
#pragma unroll
        for (int k = 0; k < 8; k++) x8[k] = X[k];
#pragma unroll
        for (int k = 0; k < 12; k++) pose[k] = A.pose12[(size_t)b * 12 + k];
        S3mProj P;
        reloc_project(A.cam, pose, x8, P);
        reason = P.reason;
        if (reason == S3M_MATCHED && n == 0) reason = S3M_NO_FEATURE_IN_WINDOW;
        if (reason == S3M_MATCHED) {
            const uint4* dl = reinterpret_cast<const uint4*>(A.pts_desc + o * 32);
            const uint4 da = dl[0], db = dl[1];
            const uint8_t* desc = A.fr.desc + (size_t)f * cap * 32;
            const uint8_t* taken = A.feat_taken + (size_t)b * cap;
            uint32_t* list = A.cand + (size_t)b * RELOC_LIST * kcap + i;
            bool any = false;
            reloc_scan(P, A.fr.kps + (size_t)f * cap, A.fr.cell_start + (size_t)f * (GRID_CELLS + 1), A.fr.cell_idx + (size_t)f * cap, n, cap, [&](int idx) {
                any = true;
                if (taken[idx]) return;
                const int dist = desc_distance(da, db, desc + (size_t)idx * 32);
                if (dist <= A.orb_dist) {
                    if (ncand < RELOC_LIST) list[(size_t)ncand * kcap] = ((uint32_t)dist << 16) | (uint32_t)idx;
                    ncand++;
                }
            });
            reason = any ? S3M_ABOVE_THRESHOLD : S3M_NO_FEATURE_IN_WINDOW;
        }
    }
    A.cand_n[o] = ncand;
    if (A.reason) A.reason[o] = reason;
}

// One workgroup per hypothesis: the point-order claim (the sweeps of s3m_claim_in_order with the points of a sweep in parallel; a point
// whose candidates exceeded its list rescans its window, so it is served exactly), then the rotation histogram of the matches on LDS
// counters, ComputeThreeMaxima by one thread, the removals and the count.
__global__ __launch_bounds__(RELOC_CLAIM_THREADS) void k_reloc_claim(RelocArgs A) {
    extern __shared__ int s_owner[];
    __shared__ int s_part[RELOC_CLAIM_THREADS / RELOC_WAVE];
    __shared__ int s_hist[HISTO_LENGTH], s_keep[HISTO_LENGTH];
    const int b = blockIdx.x, kcap = A.kcap, cap = A.fr.cap;
    int n;
    const int f = reloc_frame(A, b, n);
    const int npts = min(max(A.kf_count[b], 0), kcap);
    int* choice = A.best_idx + (size_t)b * kcap;
    const viorb_keypoint* kp = A.fr.kps + (size_t)f * cap;
    for (int p = threadIdx.x; p < kcap; p += blockDim.x) choice[p] = -1;
    if (threadIdx.x < HISTO_LENGTH) { s_hist[threadIdx.x] = 0; s_keep[threadIdx.x] = 1; }
    __syncthreads();
    s3m_claim_sweeps(s_owner, n, npts, choice, A.cand_n + (size_t)b * kcap, A.cand + (size_t)b * RELOC_LIST * kcap, (size_t)kcap, RELOC_LIST, A.orb_dist,
                     [&](int p) {
        const size_t o = (size_t)b * kcap + p;
        const float* X = A.pts_f + o * 8;
        float x8[8], pose[12];
#pragma unroll
        for (int k = 0; k < 8; k++) x8[k] = X[k];
#pragma unroll
        for (int k = 0; k < 12; k++) pose[k] = A.pose12[(size_t)b * 12 + k];
        S3mProj P;
        reloc_project(A.cam, pose, x8, P);
        const uint4* dl = reinterpret_cast<const uint4*>(A.pts_desc + o * 32);
        const uint4 da = dl[0], db = dl[1];
        const uint8_t* desc = A.fr.desc + (size_t)f * cap * 32;
        const uint8_t* taken = A.feat_taken + (size_t)b * cap;
        int best_dist = 256, c = -1;
        reloc_scan(P, kp, A.fr.cell_start + (size_t)f * (GRID_CELLS + 1), A.fr.cell_idx + (size_t)f * cap, n, cap, [&](int idx) {
            if (taken[idx] || s_owner[idx] < p) return;
            const int dist = desc_distance(da, db, desc + (size_t)idx * 32);
            if (dist < best_dist) { best_dist = dist; c = idx; }
        });
        return best_dist <= A.orb_dist ? c : -1;
    });
    // the histogram (:1561-1571), ComputeThreeMaxima (:1584), the removals (:1586-1596); choice[p] is read and written by p's own thread
    if (A.check_ori) {
        for (int p = threadIdx.x; p < npts; p += blockDim.x) {
            const int c = choice[p];
            if (c >= 0) atomicAdd(&s_hist[rot_bin(A.kf_angle[(size_t)b * kcap + p], kp[c].angle)], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) three_maxima(s_hist, s_keep);
        __syncthreads();
    }
    int found = 0;
    for (int base = 0; base < npts; base += blockDim.x) {
        const int p = base + threadIdx.x;
        bool hit = false;
        if (p < npts) {
            const int c = choice[p];
            if (c >= 0) {
                hit = !A.check_ori || s_keep[rot_bin(A.kf_angle[(size_t)b * kcap + p], kp[c].angle)];
                if (!hit) choice[p] = -1;
                if (A.reason) A.reason[(size_t)b * kcap + p] = hit ? S3M_MATCHED : RELOC_ROTATION;
            }
        }
        found += block_count(hit, s_part);
    }
    if (threadIdx.x == 0) A.nmatches[b] = found;
}

// ---- the cascade ------------------------------------------------------------------------------------------------------------------------
struct RelocStepArgs {
    RelocKf fr; int n_frames; const int* hyp_frame; const float* uright;
    const float* pose_in; const float* pts_f; const int* kf_count; int kcap;
    const int* bow_match; const uint8_t* inlier;
    // outputs of the call
    int* accepted; int* n_good; int* stage; int* counts; float* out_pose12; double* chi2; int* frame_match; uint8_t* outlier;
    // workspace
    uint8_t* kf_found; uint8_t* feat_taken; int* kf_count_eff; int* best_idx; int* nmatches;
    double* obs7; int* obs_index; int* n_obs; uint8_t* sol_outlier; double* info; float* sol_pose; int hcap;
    RelocThresholds T;
    float inv_sigma2[16]; int nlevels;
};

enum { RELOC_STEP_BEGIN = 0, RELOC_STEP_SOLVE1 = 1, RELOC_STEP_SEARCH1 = 2, RELOC_STEP_SOLVE2 = 3, RELOC_STEP_SEARCH2 = 4, RELOC_STEP_SOLVE3 = 5 };

// One workgroup per hypothesis, between two launches of the cascade. `step` names what has just run:
//   BEGIN    (a) mvpMapPoints from the inliers, sFound; then the observations of the first solve                          :2209-2224
//   SOLVE1   (c) nGood < min_good: leave, nothing nulled; (d) null the outliers; (e) accept, or prepare the coarse search   :2226-2236
//   SEARCH1  the matches of the coarse search enter mvpMapPoints; too few: leave; else the observations of the second solve :2238-2242
//   SOLVE2   (f) accept / leave, or sFound from every non-NULL entry (outliers included, none nulled) for the narrow search :2242-2252
//   SEARCH2  the matches of the narrow search enter; too few: leave; else the observations of the third solve               :2252-2257
//   SOLVE3   null the outliers, (g) accept or reject                                                                         :2257-2269
// A hypothesis that has left keeps stage != 0: its later searches get kf_count_eff = 0 and its later solves n_obs = 0.
__global__ __launch_bounds__(RELOC_STEP_THREADS) void k_reloc_step(RelocStepArgs A, int step) {
    __shared__ int s_part[RELOC_STEP_THREADS / RELOC_WAVE];
    __shared__ int s_base, s_stage;
    const int b = blockIdx.x, t = threadIdx.x, cap = A.fr.cap, kcap = A.kcap, hcap = A.hcap;
    const int fi = A.hyp_frame ? A.hyp_frame[b] : b;
    const bool fok = (unsigned)fi < (unsigned)A.n_frames;
    const int f = fok ? fi : 0;
    const int n = fok ? min(min(max(A.fr.count[f], 0), cap), hcap) : 0;
    const int npts = min(max(A.kf_count[b], 0), kcap);
    int* fm = A.frame_match + (size_t)b * cap;
    uint8_t* ol = A.outlier + (size_t)b * cap;
    uint8_t* found = A.kf_found + (size_t)b * kcap;
    uint8_t* taken = A.feat_taken + (size_t)b * cap;
    int* cnt = A.counts + (size_t)b * 8;
    const int stage_in = step == RELOC_STEP_BEGIN ? RELOC_RUNNING : A.stage[b];
    __syncthreads();                                            // every thread has read stage[b] before thread 0 may write it
    if (stage_in != RELOC_RUNNING) {                            // left earlier: nothing of it changes any more
        if (t == 0) { A.kf_count_eff[b] = 0; A.n_obs[b] = 0; }
        return;
    }
    int stage = RELOC_RUNNING;
    bool want_obs = false;
    if (step == RELOC_STEP_BEGIN) {
        for (int i = t; i < kcap; i += blockDim.x) found[i] = 0;
        __syncthreads();
        for (int j = t; j < cap; j += blockDim.x) {
            int m = -1;
            if (j < n && A.inlier[(size_t)b * cap + j]) {
                m = A.bow_match[(size_t)b * cap + j];
                if (m < 0 || m >= npts) m = -1;
            }
            fm[j] = m; ol[j] = 0;
            if (m >= 0) found[m] = 1;                           // sFound.insert: the same value from every writer
        }
        if (t < 12) { A.out_pose12[(size_t)b * 12 + t] = A.pose_in[(size_t)b * 12 + t]; }
        if (t < 8) cnt[t] = t < 5 ? -1 : 0;
        if (t == 0) { A.chi2[b] = 0.0; A.n_good[b] = 0; A.accepted[b] = 0; A.kf_count_eff[b] = 0; }
        want_obs = true;
    } else if (step == RELOC_STEP_SOLVE1 || step == RELOC_STEP_SOLVE2 || step == RELOC_STEP_SOLVE3) {
        const int nobs = min(max(A.n_obs[b], 0), hcap);
        const int good = (int)A.info[(size_t)b * 4];
        for (int k = t; k < nobs; k += blockDim.x) {            // mvbOutlier of the features that held a point (Optimizer.cc:3801, :3909-3915)
            const int j = A.obs_index[(size_t)b * hcap + k];
            if ((unsigned)j < (unsigned)cap) ol[j] = A.sol_outlier[(size_t)b * hcap + k];
        }
        if (t < 12) A.out_pose12[(size_t)b * 12 + t] = A.sol_pose[(size_t)b * 12 + t];       // SetPose
        if (t == 0) { A.chi2[b] = A.info[(size_t)b * 4 + 1]; A.n_good[b] = good; cnt[step == RELOC_STEP_SOLVE1 ? 0 : (step == RELOC_STEP_SOLVE2 ? 2 : 4)] = good; }
        stage = step == RELOC_STEP_SOLVE1 ? reloc_after_solve1(A.T, good) : (step == RELOC_STEP_SOLVE2 ? reloc_after_solve2(A.T, good) : reloc_after_solve3(A.T, good));
        __syncthreads();                                        // ol is complete
        const bool null_outliers = (step == RELOC_STEP_SOLVE1 && stage != RELOC_FEW_INLIERS) || step == RELOC_STEP_SOLVE3;
        if (null_outliers)
            for (int j = t; j < n; j += blockDim.x) if (ol[j]) fm[j] = -1;
        if (stage == RELOC_RUNNING) {                           // a search follows: mvpMapPoints != NULL on entry, sFound
            if (step == RELOC_STEP_SOLVE2) {
                for (int i = t; i < kcap; i += blockDim.x) found[i] = 0;
                __syncthreads();
                for (int j = t; j < n; j += blockDim.x) { const int m = fm[j]; if (m >= 0) found[m] = 1; }
            }
            for (int j = t; j < cap; j += blockDim.x) taken[j] = j < n && fm[j] >= 0;
            if (t == 0) A.kf_count_eff[b] = npts;
        }
    } else {                                                    // SEARCH1, SEARCH2
        const int add = A.nmatches[b], good = A.n_good[b];
        const int* bi = A.best_idx + (size_t)b * kcap;
        for (int i = t; i < npts; i += blockDim.x) {            // CurrentFrame.mvpMapPoints[bestIdx2] = pMP (:1558): one point per feature
            const int j = bi[i];
            if ((unsigned)j < (unsigned)n) fm[j] = i;
        }
        if (t == 0) { cnt[step == RELOC_STEP_SEARCH1 ? 1 : 3] = add; A.kf_count_eff[b] = 0; }
        stage = step == RELOC_STEP_SEARCH1 ? reloc_after_search1(A.T, good, add) : reloc_after_search2(A.T, good, add);
        want_obs = stage == RELOC_RUNNING;
    }
    if (t == 0) {
        s_base = 0;
        if (stage != RELOC_RUNNING) {
            A.stage[b] = stage;
            A.accepted[b] = stage == RELOC_ACCEPTED_FIRST || stage == RELOC_ACCEPTED_SECOND || stage == RELOC_ACCEPTED_THIRD;
            A.kf_count_eff[b] = 0;
        } else if (step == RELOC_STEP_BEGIN) A.stage[b] = RELOC_RUNNING;
        if (!want_obs) A.n_obs[b] = 0;
    }
    __syncthreads();                                            // fm is complete, s_base is 0
    if (!want_obs) return;
    // the edges of PoseOptimization(Frame*) in key-point order (Optimizer.cc:3792-3870): an ordered compaction, a chunk of the frame at a time
    const viorb_keypoint* kp = A.fr.kps + (size_t)f * cap;
    for (int base = 0; base < n; base += blockDim.x) {
        const int j = base + t;
        const int m = j < n ? fm[j] : -1;
        const bool has = m >= 0;
        const unsigned long long bal = __ballot(has);
        const int lane = t & 63, w = t >> 6;
        if (lane == 0) s_part[w] = __popcll(bal);
        __syncthreads();
        int k = s_base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int q = 0; q < w; q++) k += s_part[q];
        if (has) {
            const viorb_keypoint kpj = kp[j];
            const float* X = A.pts_f + ((size_t)b * kcap + m) * 8;
            double* o = A.obs7 + ((size_t)b * hcap + k) * 7;
            const int oct = min(max(kpj.octave, 0), A.nlevels - 1);
            o[0] = (double)X[0]; o[1] = (double)X[1]; o[2] = (double)X[2];
            o[3] = (double)kpj.x; o[4] = (double)kpj.y;
            o[5] = A.uright ? (double)A.uright[(size_t)f * cap + j] : -1.0;
            o[6] = (double)A.inv_sigma2[oct];
            A.obs_index[(size_t)b * hcap + k] = j;
        }
        __syncthreads();
        if (t == 0) { int s = s_base; for (int q = 0; q < RELOC_STEP_THREADS / RELOC_WAVE; q++) s += s_part[q]; s_base = s; }
        __syncthreads();
    }
    if (t == 0) A.n_obs[b] = s_base;
}

} // namespace viorb

using namespace viorb;

namespace {

struct RelocLayout { uint32_t* cand; int* cand_n; size_t total; };
RelocLayout reloc_layout(void* base, int kcap, int batch) {
    RelocLayout L; WorkspaceLayout Y(base);
    const size_t B = (size_t)batch;
    Y.take(&L.cand, B * kcap * RELOC_LIST); Y.take(&L.cand_n, B * kcap);
    L.total = Y.end();
    return L;
}
bool reloc_sizes_ok(int fcap, int kcap, int batch) { return fcap >= 1 && fcap <= VIORB_S3M_MAX_FEATURES && kcap >= 1 && batch >= 1 && batch <= 65535; }

struct RelocRefineLayout {
    uint8_t* kf_found; uint8_t* feat_taken; int* kf_count_eff; int* best_idx; int* nmatches; double* obs7; int* obs_index; int* n_obs;
    uint8_t* sol_outlier; double* info; float* sol_pose; unsigned char* match_ws; size_t match_bytes, total;
};
RelocRefineLayout reloc_refine_layout(void* base, int fcap, int kcap, int hcap, int batch) {
    RelocRefineLayout L; WorkspaceLayout Y(base);
    const size_t B = (size_t)batch;
    Y.take(&L.kf_found, B * kcap); Y.take(&L.feat_taken, B * fcap); Y.take(&L.kf_count_eff, B); Y.take(&L.best_idx, B * kcap); Y.take(&L.nmatches, B);
    Y.take(&L.obs7, B * hcap * 7); Y.take(&L.obs_index, B * hcap); Y.take(&L.n_obs, B); Y.take(&L.sol_outlier, B * hcap); Y.take(&L.info, B * 4);
    Y.take(&L.sol_pose, B * 12);
    L.match_bytes = reloc_layout(nullptr, kcap, batch).total;
    Y.take(&L.match_ws, L.match_bytes);
    L.total = Y.end();
    return L;
}

int reloc_check_cam(const viorb_mapping_camera* cam, const float* bounds4, float th, int batch, S3mCam& C) {
    VIORB_REQUIRE(cam && bounds4, "null array");
    VIORB_REQUIRE(batch >= 1 && batch <= 65535, "1 <= batch <= 65535");
    VIORB_REQUIRE(th > 0, "th > 0");
    VIORB_REQUIRE(cam->nlevels >= 1 && cam->nlevels <= 16, "nlevels must be 1..16");
    VIORB_REQUIRE(bounds4[1] > bounds4[0] && bounds4[3] > bounds4[2], "empty image bounds");
    C.fx = cam->fx; C.fy = cam->fy; C.cx = cam->cx; C.cy = cam->cy;
    C.g = grid_cam(bounds4);
    C.th = th; C.nlevels = cam->nlevels;
    C.log_sf = (float)log((double)cam->scale_factors[cam->nlevels > 1 ? 1 : 0]);
    for (int i = 0; i < 16; i++) C.scale[i] = cam->scale_factors[i < cam->nlevels ? i : cam->nlevels - 1];
    return VIORB_OK;
}

int reloc_check_frames(const viorb_s3m_keyframes* fr, int n_frames, const int32_t* hyp_frame, int batch) {
    VIORB_REQUIRE(fr && fr->kps && fr->desc && fr->count && fr->cell_start && fr->cell_idx, "null array");
    VIORB_REQUIRE(fr->cap >= 1, "fcap >= 1");
    VIORB_REQUIRE(n_frames >= 1 && (hyp_frame || n_frames >= batch), "n_frames >= 1, and >= batch without hyp_frame");
    if (fr->cap > VIORB_S3M_MAX_FEATURES) { set_error("fcap %d above VIORB_S3M_MAX_FEATURES", fr->cap); return VIORB_ERR_CAPACITY; }
    return VIORB_OK;
}
RelocKf reloc_kf(const viorb_s3m_keyframes& k) { RelocKf d; d.kps = k.kps; d.desc = k.desc; d.count = k.count; d.cell_start = k.cell_start; d.cell_idx = k.cell_idx; d.cap = k.cap; return d; }

int reloc_chunks(int n) { return (n + RELOC_BLOCK - 1) / RELOC_BLOCK; }

// the two launches of the matcher; every argument has been checked
int reloc_launch_match(const RelocArgs& A, int batch, hipStream_t st) {
    VIORB_LAUNCH(k_reloc_gates, dim3(reloc_chunks(A.kcap), batch), RELOC_BLOCK, 0, st, A);
    const size_t lds = (size_t)A.fr.cap * sizeof(int);                // fcap <= VIORB_S3M_MAX_FEATURES: at most 64 KiB beside the static words
    if (lds > 48 * 1024) VIORB_HIP_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(k_reloc_claim), lds));
    VIORB_LAUNCH(k_reloc_claim, batch, RELOC_CLAIM_THREADS, lds, st, A);
    return VIORB_OK;
}

RelocThresholds reloc_thresholds(const viorb_reloc_config& c) { RelocThresholds T; T.min_good = c.min_good; T.accept = c.accept; T.narrow_above = c.narrow_above; return T; }

} // namespace

extern "C" {

size_t viorb_relocalization_workspace_bytes(int fcap, int kcap, int batch) {
    if (!reloc_sizes_ok(fcap, kcap, batch)) return 0;
    return reloc_layout(nullptr, kcap, batch).total;
}

size_t viorb_relocalization_refine_workspace_bytes(int fcap, int kcap, int hcap, int batch) {
    if (!reloc_sizes_ok(fcap, kcap, batch) || hcap < fcap) return 0;
    return reloc_refine_layout(nullptr, fcap, kcap, hcap, batch).total;
}

int viorb_relocalization_shape(int32_t* out3) {
    VIORB_REQUIRE(out3, "null array");
    out3[0] = RELOC_BLOCK; out3[1] = RELOC_WAVE; out3[2] = RELOC_LIST;
    return VIORB_OK;
}

int viorb_reloc_config_default(viorb_reloc_config* cfg) {
    VIORB_REQUIRE(cfg, "null cfg");
    cfg->min_good = 10; cfg->accept = 50; cfg->narrow_above = 30;               // src/Tracking.cc:2228, :2236 / :2240 / :2255 / :2269, :2246
    cfg->th_coarse = 10.0f; cfg->orb_dist_coarse = 100;                         // :2238
    cfg->th_narrow = 3.0f; cfg->orb_dist_narrow = 64;                           // :2252
    cfg->check_orientation = 1;                                                 // :2182 ORBmatcher matcher2(0.9, true)
    return VIORB_OK;
}

int viorb_search_by_projection_reloc_device(const viorb_s3m_keyframes* frames, int n_frames, const int32_t* hyp_frame, const float* pose12,
                                            const float* kf_angle, const uint8_t* kf_valid, const uint8_t* kf_found, const float* pts_f,
                                            const uint8_t* pts_desc, const int32_t* kf_count, int kcap, const uint8_t* feat_taken,
                                            const viorb_mapping_camera* cam, const float bounds4[4], float th, int orb_dist, int check_orientation,
                                            int batch, int32_t* best_idx, int32_t* nmatches, int32_t* reason, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    RelocArgs A;
    VIORB_TRY(reloc_check_cam(cam, bounds4, th, batch, A.cam));
    VIORB_TRY(reloc_check_frames(frames, n_frames, hyp_frame, batch));
    VIORB_REQUIRE(pose12 && kf_angle && kf_valid && kf_found && pts_f && pts_desc && kf_count && feat_taken && best_idx && nmatches, "null array");
    VIORB_REQUIRE(kcap >= 1, "kcap >= 1");
    VIORB_REQUIRE(orb_dist >= 0 && orb_dist <= 255, "0 <= orb_dist <= 255");
    VIORB_REQUIRE(workspace && workspace_bytes >= reloc_layout(nullptr, kcap, batch).total && ((uintptr_t)workspace & 255) == 0,
                  "workspace smaller than viorb_relocalization_workspace_bytes or not 256-byte aligned");
    VIORB_TRY(require_device());
    const RelocLayout L = reloc_layout(workspace, kcap, batch);
    A.fr = reloc_kf(*frames); A.n_frames = n_frames; A.hyp_frame = hyp_frame; A.pose12 = pose12; A.kf_angle = kf_angle; A.kf_valid = kf_valid;
    A.kf_found = kf_found; A.pts_f = pts_f; A.pts_desc = pts_desc; A.kf_count = kf_count; A.feat_taken = feat_taken; A.best_idx = best_idx;
    A.nmatches = nmatches; A.reason = reason; A.cand = L.cand; A.cand_n = L.cand_n; A.kcap = kcap; A.orb_dist = orb_dist; A.check_ori = check_orientation != 0;
    return reloc_launch_match(A, batch, (hipStream_t)stream);
}

int viorb_search_by_projection_reloc(const viorb_keypoint* kps, const uint8_t* desc, int n, const float pose12[12], const float* kf_angle,
                                     const uint8_t* kf_valid, const uint8_t* kf_found, const float* pts_f, const uint8_t* pts_desc, int npts,
                                     const uint8_t* feat_taken, const viorb_mapping_camera* cam, const float bounds4[4], float th, int orb_dist,
                                     int check_orientation, int32_t* best_idx, int32_t* nmatches, int32_t* reason) {
    S3mCam C;
    VIORB_TRY(reloc_check_cam(cam, bounds4, th, 1, C));
    VIORB_REQUIRE(n >= 0 && npts >= 0 && pose12 && nmatches, "null array or a negative count");
    VIORB_REQUIRE(n == 0 || (kps && desc && feat_taken), "null array");
    VIORB_REQUIRE(npts == 0 || (kf_angle && kf_valid && kf_found && pts_f && pts_desc && best_idx), "null array");
    VIORB_REQUIRE(orb_dist >= 0 && orb_dist <= 255, "0 <= orb_dist <= 255");
    if (n > VIORB_S3M_MAX_FEATURES) { set_error("n %d above VIORB_S3M_MAX_FEATURES", n); return VIORB_ERR_CAPACITY; }
    VIORB_TRY(require_device());
    DeviceBufs B; viorb_s3m_keyframes kf;
    VIORB_TRY(host_keyframe(B, kps, desc, n, std::max(n, 1), bounds4, kf));
    const size_t pc = (size_t)std::max(npts, 1), m = (size_t)npts;
    float *dP = B.up(pose12, 12), *dang = B.up(kf_angle, m, pc), *dpf = B.up(pts_f, m * 8, pc * 8);
    uint8_t *dpd = B.up(pts_desc, m * 32, pc * 32), *dkv = B.up(kf_valid, m, pc), *dkf = B.up(kf_found, m, pc), *dft = B.up(feat_taken, (size_t)n, (size_t)kf.cap);
    int32_t *dpc = B.up(&npts, 1), *dbi = B.zeros<int32_t>(pc), *dnm = B.zeros<int32_t>(1), *dre = B.zeros<int32_t>(pc);
    const size_t wb = viorb_relocalization_workspace_bytes(kf.cap, (int)pc, 1);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_search_by_projection_reloc_device(&kf, 1, nullptr, dP, dang, dkv, dkf, dpf, dpd, dpc, (int)pc, dft, cam, bounds4, th, orb_dist,
                                                      check_orientation, 1, dbi, dnm, dre, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_TRY(download(best_idx, dbi, m)); VIORB_TRY(download(nmatches, dnm, 1));
    return download(reason, dre, m);
}

int viorb_relocalization_refine_device(viorb_frontend* h, const viorb_reloc_inputs* in, const viorb_reloc_config* cfg,
                                       const viorb_mapping_camera* cam, const float bounds4[4], double bf, int batch,
                                       const viorb_reloc_outputs* out, void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_REQUIRE(h && in && cfg && out, "null handle / inputs / config / outputs");
    RelocArgs M[2];
    VIORB_TRY(reloc_check_cam(cam, bounds4, cfg->th_coarse, batch, M[0].cam));
    VIORB_TRY(reloc_check_cam(cam, bounds4, cfg->th_narrow, batch, M[1].cam));
    VIORB_TRY(reloc_check_frames(in->frames, in->n_frames, in->hyp_frame, batch));
    VIORB_REQUIRE(in->pose12 && in->kf_angle && in->kf_valid && in->pts_f && in->pts_desc && in->kf_count && in->bow_match && in->inlier, "null array");
    VIORB_REQUIRE(out->accepted && out->n_good && out->stage && out->counts && out->out_pose12 && out->chi2 && out->frame_match && out->outlier, "null array");
    VIORB_REQUIRE(in->kcap >= 1, "kcap >= 1");
    VIORB_REQUIRE(cfg->orb_dist_coarse >= 0 && cfg->orb_dist_coarse <= 255 && cfg->orb_dist_narrow >= 0 && cfg->orb_dist_narrow <= 255, "0 <= orb_dist <= 255");
    int32_t hbatch = 0, hcap = 0;
    VIORB_TRY(viorb_frontend_capacity(h, &hbatch, &hcap));
    const int fcap = in->frames->cap, kcap = in->kcap;
    VIORB_REQUIRE(batch <= hbatch && fcap <= hcap, "batch above the handle's max_batch or fcap above its cap");
    VIORB_REQUIRE(workspace && workspace_bytes >= reloc_refine_layout(nullptr, fcap, kcap, hcap, batch).total && ((uintptr_t)workspace & 255) == 0,
                  "workspace smaller than viorb_relocalization_refine_workspace_bytes or not 256-byte aligned");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const RelocRefineLayout L = reloc_refine_layout(workspace, fcap, kcap, hcap, batch);
    const RelocLayout ML = reloc_layout(L.match_ws, kcap, batch);
    RelocStepArgs S;
    S.fr = reloc_kf(*in->frames); S.n_frames = in->n_frames; S.hyp_frame = in->hyp_frame; S.uright = in->uright; S.pose_in = in->pose12;
    S.pts_f = in->pts_f; S.kf_count = in->kf_count; S.kcap = kcap; S.bow_match = in->bow_match; S.inlier = in->inlier;
    S.accepted = out->accepted; S.n_good = out->n_good; S.stage = out->stage; S.counts = out->counts; S.out_pose12 = out->out_pose12; S.chi2 = out->chi2;
    S.frame_match = out->frame_match; S.outlier = out->outlier;
    S.kf_found = L.kf_found; S.feat_taken = L.feat_taken; S.kf_count_eff = L.kf_count_eff; S.best_idx = L.best_idx; S.nmatches = L.nmatches;
    S.obs7 = L.obs7; S.obs_index = L.obs_index; S.n_obs = L.n_obs; S.sol_outlier = L.sol_outlier; S.info = L.info; S.sol_pose = L.sol_pose; S.hcap = hcap;
    S.T = reloc_thresholds(*cfg);
    S.nlevels = cam->nlevels;
    for (int i = 0; i < 16; i++) S.inv_sigma2[i] = 1.0f / cam->level_sigma2[i < cam->nlevels ? i : cam->nlevels - 1];      // mvInvLevelSigma2
    for (int k = 0; k < 2; k++) {
        RelocArgs& A = M[k];
        A.fr = S.fr; A.n_frames = in->n_frames; A.hyp_frame = in->hyp_frame; A.pose12 = out->out_pose12; A.kf_angle = in->kf_angle; A.kf_valid = in->kf_valid;
        A.kf_found = L.kf_found; A.pts_f = in->pts_f; A.pts_desc = in->pts_desc; A.kf_count = L.kf_count_eff; A.feat_taken = L.feat_taken;
        A.best_idx = L.best_idx; A.nmatches = L.nmatches; A.reason = nullptr; A.cand = ML.cand; A.cand_n = ML.cand_n; A.kcap = kcap;
        A.orb_dist = k == 0 ? cfg->orb_dist_coarse : cfg->orb_dist_narrow; A.check_ori = cfg->check_orientation != 0;
    }
    // lock step: a solve reads the pose of out_pose12 and writes sol_pose, which the step after it copies back (the solver re-reads its
    // input pose at every round, so the two must not alias)
    for (int solve = 0; solve < 3; solve++) {
        VIORB_LAUNCH(k_reloc_step, batch, RELOC_STEP_THREADS, 0, st, S, solve == 0 ? (int)RELOC_STEP_BEGIN : (solve == 1 ? (int)RELOC_STEP_SEARCH1 : (int)RELOC_STEP_SEARCH2));
        VIORB_TRY(viorb_frontend_pose_opt_se3_device(h, out->out_pose12, L.obs7, L.n_obs, bf, batch, L.sol_pose, L.sol_outlier, L.info, stream));
        VIORB_LAUNCH(k_reloc_step, batch, RELOC_STEP_THREADS, 0, st, S, solve == 0 ? (int)RELOC_STEP_SOLVE1 : (solve == 1 ? (int)RELOC_STEP_SOLVE2 : (int)RELOC_STEP_SOLVE3));
        if (solve < 2) VIORB_TRY(reloc_launch_match(M[solve], batch, st));
    }
    return VIORB_OK;
}

int viorb_relocalization_refine(const viorb_keypoint* kps, const uint8_t* desc, const float* uright, int n, const float pose12[12],
                                const float* kf_angle, const uint8_t* kf_valid, const float* pts_f, const uint8_t* pts_desc, int npts,
                                const int32_t* bow_match, const uint8_t* inlier, const viorb_reloc_config* cfg, const viorb_mapping_camera* cam,
                                const float bounds4[4], double bf, int32_t* accepted, int32_t* n_good, int32_t* stage, int32_t* counts,
                                float* out_pose12, double* chi2, int32_t* frame_match, uint8_t* outlier) {
    S3mCam C;
    VIORB_REQUIRE(cfg, "null cfg");
    VIORB_TRY(reloc_check_cam(cam, bounds4, cfg->th_coarse, 1, C));
    VIORB_REQUIRE(n >= 0 && npts >= 0 && pose12 && accepted && n_good && stage && counts && out_pose12 && chi2, "null array or a negative count");
    VIORB_REQUIRE(n == 0 || (kps && desc && bow_match && inlier && frame_match && outlier), "null array");
    VIORB_REQUIRE(npts == 0 || (kf_angle && kf_valid && pts_f && pts_desc), "null array");
    if (n > VIORB_S3M_MAX_FEATURES) { set_error("n %d above VIORB_S3M_MAX_FEATURES", n); return VIORB_ERR_CAPACITY; }
    VIORB_TRY(require_device());
    viorb_frontend_config fc;
    memset(&fc, 0, sizeof fc);
    fc.min_x = bounds4[0]; fc.max_x = bounds4[1]; fc.min_y = bounds4[2]; fc.max_y = bounds4[3];
    fc.fx = cam->fx; fc.fy = cam->fy; fc.cx = cam->cx; fc.cy = cam->cy;
    fc.cam[0] = cam->fx; fc.cam[1] = cam->fy; fc.cam[2] = cam->cx; fc.cam[3] = cam->cy; fc.cam[4] = fc.cam[8] = fc.cam[12] = 1.0;
    fc.nlevels = cam->nlevels; fc.check_orientation = cfg->check_orientation;
    for (int i = 0; i < 16; i++) { fc.scale_factors[i] = C.scale[i]; fc.inv_level_sigma2[i] = 1.0f / cam->level_sigma2[i < cam->nlevels ? i : cam->nlevels - 1]; }
    DeviceBufs B; viorb_s3m_keyframes kf;
    VIORB_TRY(host_keyframe(B, kps, desc, n, std::max(n, 1), bounds4, kf));
    struct Handle { viorb_frontend* h = nullptr; ~Handle() { if (h) (void)viorb_frontend_destroy(h); } } H;
    int device = 0;
    VIORB_HIP_TRY(hipGetDevice(&device));
    VIORB_TRY(viorb_frontend_create(&fc, 1, kf.cap, device, &H.h));
    const size_t fc_ = (size_t)kf.cap, pc = (size_t)std::max(npts, 1), m = (size_t)npts;
    viorb_reloc_inputs I; viorb_reloc_outputs O;
    I.frames = &kf; I.n_frames = 1; I.hyp_frame = nullptr; I.uright = uright ? B.up(uright, (size_t)n, fc_) : nullptr;
    I.pose12 = B.up(pose12, 12); I.kf_angle = B.up(kf_angle, m, pc); I.kf_valid = B.up(kf_valid, m, pc); I.pts_f = B.up(pts_f, m * 8, pc * 8);
    I.pts_desc = B.up(pts_desc, m * 32, pc * 32); I.kf_count = B.up(&npts, 1); I.kcap = (int)pc;
    I.bow_match = B.up(bow_match, (size_t)n, fc_); I.inlier = B.up(inlier, (size_t)n, fc_);
    O.accepted = B.zeros<int32_t>(1); O.n_good = B.zeros<int32_t>(1); O.stage = B.zeros<int32_t>(1); O.counts = B.zeros<int32_t>(8);
    O.out_pose12 = B.zeros<float>(12); O.chi2 = B.zeros<double>(1); O.frame_match = B.zeros<int32_t>(fc_); O.outlier = B.zeros<uint8_t>(fc_);
    const size_t wb = viorb_relocalization_refine_workspace_bytes(kf.cap, (int)pc, kf.cap, 1);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_relocalization_refine_device(H.h, &I, cfg, cam, bounds4, bf, 1, &O, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_TRY(download(accepted, O.accepted, 1)); VIORB_TRY(download(n_good, O.n_good, 1)); VIORB_TRY(download(stage, O.stage, 1));
    VIORB_TRY(download(counts, O.counts, 8)); VIORB_TRY(download(out_pose12, O.out_pose12, 12)); VIORB_TRY(download(chi2, O.chi2, 1));
    VIORB_TRY(download(frame_match, O.frame_match, (size_t)n));
    return download(outlier, O.outlier, (size_t)n);
}

// ---- host-only test hooks: reloc_core.h compiled for the host ----------------------------------------------------------------------------
int viorb_debug_reloc_project(const float* pose12, const float* pt8, const viorb_mapping_camera* cam, const float bounds4[4], float th, float* out4,
                              int32_t* out6) {
    S3mCam C;
    VIORB_TRY(reloc_check_cam(cam, bounds4, th, 1, C));
    VIORB_REQUIRE(pose12 && pt8 && out4 && out6, "null array");
    S3mProj P;
    reloc_project(C, pose12, pt8, P);
    out4[0] = P.u; out4[1] = P.v; out4[2] = P.dist3D; out4[3] = P.radius;
    out6[0] = P.level; out6[1] = P.rect.x0; out6[2] = P.rect.x1; out6[3] = P.rect.y0; out6[4] = P.rect.y1; out6[5] = P.reason;
    return VIORB_OK;
}

int viorb_debug_reloc_match(const uint32_t* cand, const int32_t* cand_n, int npts, int lcap, const uint8_t* taken_in, int nfeat, int orb_dist,
                            int check_orientation, const float* angle_kf, const float* angle_f, int32_t* best_idx, uint8_t* removed,
                            int32_t* nmatches) {
    VIORB_REQUIRE(npts >= 0 && lcap >= 1 && nfeat >= 0 && nmatches && (npts == 0 || (cand && cand_n && best_idx && removed && angle_kf)) &&
                  (nfeat == 0 || (taken_in && angle_f)), "null array or a negative size");
    VIORB_REQUIRE(orb_dist >= 0 && orb_dist <= 255, "0 <= orb_dist <= 255");
    std::vector<int32_t> owner((size_t)std::max(nfeat, 1));
    *nmatches = reloc_match_serial(cand, cand_n, npts, lcap, taken_in, nfeat, orb_dist, check_orientation, angle_kf, angle_f, best_idx, removed, owner.data());
    return VIORB_OK;
}

int viorb_debug_reloc_decide(const viorb_reloc_config* cfg, int step, int n_good, int n_additional) {
    VIORB_REQUIRE(cfg && step >= 1 && step <= 5, "null cfg or a step outside 1..5");
    const RelocThresholds T = reloc_thresholds(*cfg);
    switch (step) {
        case 1: return reloc_after_solve1(T, n_good);
        case 2: return reloc_after_search1(T, n_good, n_additional);
        case 3: return reloc_after_solve2(T, n_good);
        case 4: return reloc_after_search2(T, n_good, n_additional);
        default: return reloc_after_solve3(T, n_good);
    }
}

} // extern "C"
