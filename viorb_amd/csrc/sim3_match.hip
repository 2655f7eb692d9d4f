// viorb_amd/csrc/sim3_match.hip — the loop-closing matchers that project through a similarity (include/viorb_sim3_match.h):
//   k_s3m_oneway    ORBmatcher::SearchBySim3, the two one-way searches     reference src/ORBmatcher.cc:1147-1305
//   k_s3m_mutual    ORBmatcher::SearchBySim3, the agreement check           reference src/ORBmatcher.cc:1307-1323
//   k_s3m_scw       SearchByProjection(KF, Scw) gates + candidate lists, Fuse(KF, Scw)    :311-392, :999-1096
//   k_s3m_claim     SearchByProjection(KF, Scw), the point-order claim      :370-398
//   k_s3m_counts    nfused of Fuse(KF, Scw) from the workgroups' partial counts
// The arithmetic is sim3_match_core.h. Shape (DESIGN.md "Sim3 matchers"): one lane per point, S3M_BLOCK points per workgroup, the grid
// over (point chunk, key frame, direction): the calls come one loop event at a time (one key frame and thousands of points, a handful of
// pairs), so the points of one key frame are spread over workgroups. A window holds a handful of candidates, too few to give a wavefront
// per point work for its lanes. The result arrays are written with plain stores; counts are reduced per workgroup.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "viorb_common.h"
#include "sim3_match_core.h"

namespace viorb {

enum { S3M_BLOCK = 256, S3M_WAVE = 64, S3M_LIST = 8, S3M_CLAIM_THREADS = 1024 };

struct S3mKf { const viorb_keypoint* kps; const uint8_t* desc; const int* count; const int* cell_start; const int* cell_idx; int cap; };

// KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:927-942) over the CSR grid of a key frame with n features in arrays of cap: visit(idx, octave)
// for every feature of the cell rectangle with |dx| < r and |dy| < r, in the reference's order (grid_scan).
template <class Visit>
__device__ __forceinline__ void s3m_scan(const S3mProj& P, const viorb_keypoint* __restrict__ kp, const int* __restrict__ cs, const int* __restrict__ ci,
                                         int n, int cap, Visit&& visit) {
    grid_scan(P.rect, cs, ci, n, cap, [&](int idx) {
        const viorb_keypoint k = kp[idx];
        if (fabsf(k.x - P.u) < P.radius && fabsf(k.y - P.v) < P.radius) visit(idx, k.octave);
    });
}

// ---- SearchBySim3 ----------------------------------------------------------------------------------------------------------------------
struct S3mSideDev { S3mKf kf; const float* pose12; const uint8_t* has_point; const float* pts_f; const uint8_t* pts_desc; const uint8_t* already; };
struct S3mOnewayArgs {
    S3mSideDev side[2]; const float* R12; const float* t12; const float* s12;
    int* match[2]; int* reason[2];          // match: never NULL (the caller's array or scratch); reason: may be NULL
    S3mCam cam;
};
// blockIdx = (point chunk, pair, direction): direction 0 projects the points of key frame 1 into key frame 2 (:1148-1225), 1 the reverse
__global__ __launch_bounds__(S3M_BLOCK) void k_s3m_oneway(S3mOnewayArgs A) {
    const int b = blockIdx.y, d = blockIdx.z, i = blockIdx.x * S3M_BLOCK + threadIdx.x;
    const S3mSideDev& own = A.side[d];
    const S3mSideDev& oth = A.side[1 - d];
    const int cap = own.kf.cap;
    if (i >= cap) return;
    const int n = min(max(own.kf.count[b], 0), cap), n_oth = min(max(oth.kf.count[b], 0), oth.kf.cap);
    const size_t o = (size_t)b * cap + i;
    int best = -1, reason = S3M_NOT_CANDIDATE;
    if (i < n && own.has_point[o] && !own.already[o]) {
        S3mPair T;
        s3m_pair(A.R12 + (size_t)b * 9, A.t12 + (size_t)b * 3, A.s12[b], T);
        const float* X = own.pts_f + o * 8;
        float x8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x8[k] = X[k];
        S3mProj P;
        s3m_project_pair(A.cam, own.pose12 + (size_t)b * 12, d == 0 ? T.sR21 : T.sR12, d == 0 ? T.t21 : A.t12 + (size_t)b * 3, x8, P);
        reason = P.reason;
        if (reason == S3M_MATCHED && n_oth == 0) reason = S3M_NO_FEATURE_IN_WINDOW;
        if (reason == S3M_MATCHED) {
            const uint4* dl = reinterpret_cast<const uint4*>(own.pts_desc + o * 32);
            const uint4 da = dl[0], db = dl[1];
            const uint8_t* desc = oth.kf.desc + (size_t)b * oth.kf.cap * 32;
            int best_dist = INT_MAX;
            bool any = false;
            const int lvl = P.level;
            s3m_scan(P, oth.kf.kps + (size_t)b * oth.kf.cap, oth.kf.cell_start + (size_t)b * (GRID_CELLS + 1), oth.kf.cell_idx + (size_t)b * oth.kf.cap,
                     n_oth, oth.kf.cap, [&](int idx, int octave) {
                         any = true;
                         if (octave < lvl - 1 || octave > lvl) return;
                         const int dist = desc_distance(da, db, desc + (size_t)idx * 32);
                         if (dist < best_dist) { best_dist = dist; best = idx; }
                     });
            if (best_dist > TH_HIGH) best = -1;
            reason = !any ? S3M_NO_FEATURE_IN_WINDOW : (best >= 0 ? S3M_MATCHED : S3M_ABOVE_THRESHOLD);
        }
    }
    A.match[d][o] = best;
    if (A.reason[d]) A.reason[d][o] = reason;
}

struct S3mMutualArgs { const int* match1; const int* match2; int* match12; int* nfound; int* reason1; int* reason2; int cap1, cap2; };
// one workgroup per pair: match12 and nfound (:1307-1323), and NOT_MUTUAL for the one-way matches of either direction that do not agree
__global__ __launch_bounds__(S3M_CLAIM_THREADS) void k_s3m_mutual(S3mMutualArgs A) {
    __shared__ int s_part[S3M_CLAIM_THREADS / S3M_WAVE];
    const int b = blockIdx.x;
    const int* m1 = A.match1 + (size_t)b * A.cap1;
    const int* m2 = A.match2 + (size_t)b * A.cap2;
    int found = 0;
    for (int base = 0; base < A.cap1; base += blockDim.x) {
        const int i1 = base + threadIdx.x;
        bool hit = false;
        if (i1 < A.cap1) {
            const int idx2 = m1[i1];
            hit = idx2 >= 0 && idx2 < A.cap2 && m2[idx2] == i1;
            A.match12[(size_t)b * A.cap1 + i1] = hit ? idx2 : -1;
            if (A.reason1 && idx2 >= 0 && !hit) A.reason1[(size_t)b * A.cap1 + i1] = S3M_NOT_MUTUAL;
        }
        found += block_count(hit, s_part);
    }
    if (A.reason2)
        for (int i2 = threadIdx.x; i2 < A.cap2; i2 += blockDim.x) {
            const int idx1 = m2[i2];
            if (idx1 >= 0 && !(idx1 < A.cap1 && m1[idx1] == i2)) A.reason2[(size_t)b * A.cap2 + i2] = S3M_NOT_MUTUAL;
        }
    if (threadIdx.x == 0) A.nfound[b] = found;
}

// ---- SearchByProjection(KF, Scw) and Fuse(KF, Scw) -------------------------------------------------------------------------------------
struct S3mScwArgs {
    S3mKf kf; const float* Scw; const float* pts_f; const uint8_t* pts_desc; const uint8_t* pts_valid; const int* pts_count;
    const uint8_t* feat_taken;              // ORDERED only
    int* best_idx; int* reason;             // reason may be NULL
    uint32_t* cand; int* cand_n;            // ORDERED: [batch][S3M_LIST][pcap] (entry k of point p at k * pcap + p), [batch][pcap]
    int* partial;                           // !ORDERED: [batch][gridDim.x] matches of each workgroup
    int* nmatches;                          // ORDERED: [batch], written by k_s3m_claim
    int pcap, npts_shared;                  // npts_shared >= 0: one point list shared by the batch (Fuse), pts_count unused
    S3mCam cam;
};
// blockIdx = (point chunk, key frame). ORDERED (SearchByProjection): a point's candidates of distance <= TH_LOW that are free on entry go
// to its list in visiting order, the count goes on past S3M_LIST (k_s3m_claim rescans the window of such a point); best_idx is left to
// k_s3m_claim. !ORDERED (Fuse): best_idx is final.
template <bool ORDERED>
__global__ __launch_bounds__(S3M_BLOCK) void k_s3m_scw(S3mScwArgs A) {
    __shared__ int s_part[S3M_BLOCK / S3M_WAVE];
    const int b = blockIdx.y, p = blockIdx.x * S3M_BLOCK + threadIdx.x, pcap = A.pcap, cap = A.kf.cap;
    const bool shared = A.npts_shared >= 0;
    const int npts = shared ? min(A.npts_shared, pcap) : min(max(A.pts_count[b], 0), pcap);
    const int n = min(max(A.kf.count[b], 0), cap);
    const size_t o = (size_t)b * pcap + p, op = shared ? (size_t)p : o;
    int best = -1, reason = S3M_NOT_CANDIDATE, ncand = 0;
    if (p < npts && A.pts_valid[o]) {
        S3mScw D;
        s3m_decompose(A.Scw + (size_t)b * 12, D);
        const float* X = A.pts_f + op * 8;
        float x8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x8[k] = X[k];
        S3mProj P;
        s3m_project_scw(A.cam, D, x8, P);
        reason = P.reason;
        if (reason == S3M_MATCHED && n == 0) reason = S3M_NO_FEATURE_IN_WINDOW;
        if (reason == S3M_MATCHED) {
            const uint4* dl = reinterpret_cast<const uint4*>(A.pts_desc + op * 32);
            const uint4 da = dl[0], db = dl[1];
            const uint8_t* desc = A.kf.desc + (size_t)b * cap * 32;
            const uint8_t* taken = ORDERED ? A.feat_taken + (size_t)b * cap : nullptr;
            uint32_t* list = ORDERED ? A.cand + (size_t)b * S3M_LIST * pcap + p : nullptr;
            int best_dist = 256;
            bool any = false;
            const int lvl = P.level;
            s3m_scan(P, A.kf.kps + (size_t)b * cap, A.kf.cell_start + (size_t)b * (GRID_CELLS + 1), A.kf.cell_idx + (size_t)b * cap,
                     n, cap, [&](int idx, int octave) {
                         any = true;
                         if (ORDERED && taken[idx]) return;
                         if (octave < lvl - 1 || octave > lvl) return;
                         const int dist = desc_distance(da, db, desc + (size_t)idx * 32);
                         if (ORDERED && dist <= TH_LOW) {
                             if (ncand < S3M_LIST) list[(size_t)ncand * pcap] = ((uint32_t)dist << 16) | (uint32_t)idx;
                             ncand++;
                         }
                         if (dist < best_dist) { best_dist = dist; best = idx; }
                     });
            if (best_dist > TH_LOW) best = -1;
            reason = !any ? S3M_NO_FEATURE_IN_WINDOW : (best >= 0 && !ORDERED ? S3M_MATCHED : S3M_ABOVE_THRESHOLD);
        }
    }
    if (p < pcap) {
        if (ORDERED) A.cand_n[o] = ncand; else A.best_idx[o] = best;
        if (A.reason) A.reason[o] = reason;
    }
    if (!ORDERED) {
        const int total = block_count(best >= 0, s_part);
        if (threadIdx.x == 0) A.partial[(size_t)b * gridDim.x + blockIdx.x] = total;
    }
}

// nfused[b] = the sum of the partial counts of key frame b's workgroups
__global__ __launch_bounds__(S3M_WAVE) void k_s3m_counts(const int* __restrict__ partial, int chunks, int batch, int* __restrict__ out) {
    const int b = blockIdx.x * S3M_WAVE + threadIdx.x;
    if (b >= batch) return;
    int s = 0;
    for (int k = 0; k < chunks; k++) s += partial[(size_t)b * chunks + k];
    out[b] = s;
}

// The point-order claim, one workgroup per key frame: the sweeps of s3m_claim_in_order (sim3_match_core.h) with the points of a sweep in
// parallel. s_owner[f] = the lowest point that chose feature f in the previous sweep (LDS atomics on scratch; the result arrays get plain
// stores). A point whose candidates exceeded its list rescans its window, so it is served exactly.
__global__ __launch_bounds__(S3M_CLAIM_THREADS) void k_s3m_claim(S3mScwArgs A) {
    extern __shared__ int s_owner[];
    __shared__ int s_part[S3M_CLAIM_THREADS / S3M_WAVE];
    const int b = blockIdx.x, pcap = A.pcap, cap = A.kf.cap;
    const int npts = min(max(A.pts_count[b], 0), pcap);
    const int n = min(max(A.kf.count[b], 0), cap);
    int* choice = A.best_idx + (size_t)b * pcap;
    const int* cand_n = A.cand_n + (size_t)b * pcap;
    const uint32_t* cand = A.cand + (size_t)b * S3M_LIST * pcap;
    for (int p = threadIdx.x; p < pcap; p += blockDim.x) choice[p] = -1;
    __syncthreads();
    s3m_claim_sweeps(s_owner, n, npts, choice, cand_n, cand, (size_t)pcap, S3M_LIST, TH_LOW, [&](int p) {
        S3mScw D;
        s3m_decompose(A.Scw + (size_t)b * 12, D);
        const float* X = A.pts_f + ((size_t)b * pcap + p) * 8;
        float x8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x8[k] = X[k];
        S3mProj P;
        s3m_project_scw(A.cam, D, x8, P);
        const uint4* dl = reinterpret_cast<const uint4*>(A.pts_desc + ((size_t)b * pcap + p) * 32);
        const uint4 da = dl[0], db = dl[1];
        const uint8_t* desc = A.kf.desc + (size_t)b * cap * 32;
        const uint8_t* taken = A.feat_taken + (size_t)b * cap;
        int best_dist = 256, c = -1;
        const int lvl = P.level;
        s3m_scan(P, A.kf.kps + (size_t)b * cap, A.kf.cell_start + (size_t)b * (GRID_CELLS + 1), A.kf.cell_idx + (size_t)b * cap,
                 n, cap, [&](int idx, int octave) {
                     if (taken[idx] || s_owner[idx] < p) return;
                     if (octave < lvl - 1 || octave > lvl) return;
                     const int dist = desc_distance(da, db, desc + (size_t)idx * 32);
                     if (dist < best_dist) { best_dist = dist; c = idx; }
                 });
        return best_dist <= TH_LOW ? c : -1;
    });
    int found = 0;
    for (int base = 0; base < npts; base += blockDim.x) {
        const int p = base + threadIdx.x;
        const bool hit = p < npts && choice[p] >= 0;
        if (hit && A.reason) A.reason[(size_t)b * pcap + p] = S3M_MATCHED;
        found += block_count(hit, s_part);
    }
    if (threadIdx.x == 0) A.nmatches[b] = found;
}

} // namespace viorb

using namespace viorb;

namespace {

struct S3mLayout { int* m1; int* m2; uint32_t* cand; int* cand_n; int* partial; size_t total; };
int s3m_chunks(int n) { return (n + S3M_BLOCK - 1) / S3M_BLOCK; }
S3mLayout s3m_layout(void* base, int cap, int pcap, int batch) {
    S3mLayout L; WorkspaceLayout Y(base);
    const size_t B = (size_t)batch;
    Y.take(&L.m1, B * cap); Y.take(&L.m2, B * cap);
    Y.take(&L.cand, B * pcap * S3M_LIST); Y.take(&L.cand_n, B * pcap); Y.take(&L.partial, B * s3m_chunks(pcap));
    L.total = Y.end();
    return L;
}
bool s3m_sizes_ok(int cap, int pcap, int batch) { return cap >= 1 && cap <= VIORB_S3M_MAX_FEATURES && pcap >= 1 && batch >= 1 && batch <= 65535; }

int s3m_check_cam(const viorb_mapping_camera* cam, const float* bounds4, float th, int batch, S3mCam& C) {
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

int s3m_check_kf(const viorb_s3m_keyframes* kf) {
    VIORB_REQUIRE(kf && kf->kps && kf->desc && kf->count && kf->cell_start && kf->cell_idx, "null array");
    VIORB_REQUIRE(kf->cap >= 1, "cap >= 1");
    if (kf->cap > VIORB_S3M_MAX_FEATURES) { set_error("cap %d above VIORB_S3M_MAX_FEATURES", kf->cap); return VIORB_ERR_CAPACITY; }
    return VIORB_OK;
}
S3mKf s3m_kf(const viorb_s3m_keyframes& k) { S3mKf d; d.kps = k.kps; d.desc = k.desc; d.count = k.count; d.cell_start = k.cell_start; d.cell_idx = k.cell_idx; d.cap = k.cap; return d; }

int s3m_check_workspace(void* workspace, size_t workspace_bytes, int cap, int pcap, int batch) {
    VIORB_REQUIRE(workspace && workspace_bytes >= s3m_layout(nullptr, cap, pcap, batch).total && ((uintptr_t)workspace & 255) == 0,
                  "workspace smaller than viorb_sim3_match_workspace_bytes or not 256-byte aligned");
    return VIORB_OK;
}

int s3m_check_side(const viorb_s3m_side* s) {
    VIORB_REQUIRE(s, "null array");
    VIORB_TRY(s3m_check_kf(&s->kf));
    VIORB_REQUIRE(s->pose12 && s->has_point && s->pts_f && s->pts_desc && s->already, "null array");
    return VIORB_OK;
}
S3mSideDev s3m_side(const viorb_s3m_side& s) {
    S3mSideDev d; d.kf = s3m_kf(s.kf); d.pose12 = s.pose12; d.has_point = s.has_point; d.pts_f = s.pts_f; d.pts_desc = s.pts_desc; d.already = s.already;
    return d;
}

} // namespace

extern "C" {

size_t viorb_sim3_match_workspace_bytes(int cap, int pcap, int batch) {
    if (pcap < 1) pcap = 1;
    if (!s3m_sizes_ok(cap, pcap, batch)) return 0;
    return s3m_layout(nullptr, cap, pcap, batch).total;
}

int viorb_sim3_match_shape(int32_t* out3) {
    VIORB_REQUIRE(out3, "null array");
    out3[0] = S3M_BLOCK; out3[1] = S3M_WAVE; out3[2] = S3M_LIST;
    return VIORB_OK;
}

int viorb_keyframe_grid(const viorb_keypoint* kps, int n, const float bounds4[4], int32_t* cell_start, int32_t* cell_idx) {
    VIORB_REQUIRE(n >= 0 && (n == 0 || kps) && bounds4 && cell_start && cell_idx, "null array or a negative count");
    VIORB_REQUIRE(bounds4[1] > bounds4[0] && bounds4[3] > bounds4[2], "empty image bounds");
    if (n > VIORB_S3M_MAX_FEATURES) { set_error("n %d above VIORB_S3M_MAX_FEATURES", n); return VIORB_ERR_CAPACITY; }
    VIORB_TRY(require_device());
    DeviceBufs B; viorb_s3m_keyframes kf;
    VIORB_TRY(host_keyframe(B, kps, nullptr, n, std::max(n, 1), bounds4, kf));         // the grid reads no descriptors
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_TRY(download(cell_start, kf.cell_start, (size_t)GRID_CELLS + 1));
    return download(cell_idx, kf.cell_idx, (size_t)kf.cap);
}

int viorb_search_by_sim3_device(const viorb_s3m_side* side1, const viorb_s3m_side* side2, const float* R12, const float* t12, const float* s12,
                                const viorb_mapping_camera* cam, const float bounds4[4], float th, int batch, int32_t* match12, int32_t* nfound,
                                int32_t* match1, int32_t* match2, int32_t* reason1, int32_t* reason2, void* workspace, size_t workspace_bytes,
                                void* stream) {
    S3mOnewayArgs A;
    VIORB_TRY(s3m_check_cam(cam, bounds4, th, batch, A.cam));
    VIORB_TRY(s3m_check_side(side1)); VIORB_TRY(s3m_check_side(side2));
    VIORB_REQUIRE(R12 && t12 && s12 && match12 && nfound, "null array");
    const int cap1 = side1->kf.cap, cap2 = side2->kf.cap, capm = std::max(cap1, cap2);
    VIORB_TRY(s3m_check_workspace(workspace, workspace_bytes, capm, 1, batch));
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const S3mLayout L = s3m_layout(workspace, capm, 1, batch);
    A.side[0] = s3m_side(*side1); A.side[1] = s3m_side(*side2); A.R12 = R12; A.t12 = t12; A.s12 = s12;
    A.match[0] = match1 ? match1 : L.m1; A.match[1] = match2 ? match2 : L.m2; A.reason[0] = reason1; A.reason[1] = reason2;
    VIORB_LAUNCH(k_s3m_oneway, dim3(s3m_chunks(capm), batch, 2), S3M_BLOCK, 0, st, A);
    S3mMutualArgs M; M.match1 = A.match[0]; M.match2 = A.match[1]; M.match12 = match12; M.nfound = nfound; M.reason1 = reason1; M.reason2 = reason2;
    M.cap1 = cap1; M.cap2 = cap2;
    VIORB_LAUNCH(k_s3m_mutual, batch, S3M_CLAIM_THREADS, 0, st, M);
    return VIORB_OK;
}

int viorb_search_by_sim3(const viorb_keypoint* kps1, const uint8_t* desc1, int n1, const float pose12_1[12], const uint8_t* has_point1,
                         const float* pts_f1, const uint8_t* pts_desc1, const uint8_t* already1, const viorb_keypoint* kps2, const uint8_t* desc2,
                         int n2, const float pose12_2[12], const uint8_t* has_point2, const float* pts_f2, const uint8_t* pts_desc2,
                         const uint8_t* already2, const float R12[9], const float t12[3], float s12, const viorb_mapping_camera* cam,
                         const float bounds4[4], float th, int32_t* match12, int32_t* nfound, int32_t* match1, int32_t* match2, int32_t* reason1,
                         int32_t* reason2) {
    S3mCam C;
    VIORB_TRY(s3m_check_cam(cam, bounds4, th, 1, C));
    VIORB_REQUIRE(n1 >= 0 && n2 >= 0 && pose12_1 && pose12_2 && R12 && t12 && nfound, "null array or a negative count");
    VIORB_REQUIRE(n1 == 0 || (kps1 && desc1 && has_point1 && pts_f1 && pts_desc1 && already1 && match12), "null array");
    VIORB_REQUIRE(n2 == 0 || (kps2 && desc2 && has_point2 && pts_f2 && pts_desc2 && already2), "null array");
    if (std::max(n1, n2) > VIORB_S3M_MAX_FEATURES) { set_error("n above VIORB_S3M_MAX_FEATURES"); return VIORB_ERR_CAPACITY; }
    VIORB_TRY(require_device());
    DeviceBufs B;
    viorb_s3m_side S[2];
    const viorb_keypoint* kps[2] = {kps1, kps2}; const uint8_t* desc[2] = {desc1, desc2}; const int n[2] = {n1, n2};
    const float* pose[2] = {pose12_1, pose12_2}; const uint8_t* hp[2] = {has_point1, has_point2}; const float* pf[2] = {pts_f1, pts_f2};
    const uint8_t* pd[2] = {pts_desc1, pts_desc2}; const uint8_t* al[2] = {already1, already2};
    for (int k = 0; k < 2; k++) {
        VIORB_TRY(host_keyframe(B, kps[k], desc[k], n[k], std::max(n[k], 1), bounds4, S[k].kf));
        const size_t c = (size_t)S[k].kf.cap, m = (size_t)n[k];
        S[k].pose12 = B.up(pose[k], 12); S[k].has_point = B.up(hp[k], m, c); S[k].pts_f = B.up(pf[k], m * 8, c * 8);
        S[k].pts_desc = B.up(pd[k], m * 32, c * 32); S[k].already = B.up(al[k], m, c);
    }
    const size_t c1 = (size_t)S[0].kf.cap, c2 = (size_t)S[1].kf.cap;
    float *dR = B.up(R12, 9), *dt = B.up(t12, 3), *ds = B.up(&s12, 1);
    int32_t *d12 = B.zeros<int32_t>(c1), *dnf = B.zeros<int32_t>(1), *dm1 = B.zeros<int32_t>(c1), *dm2 = B.zeros<int32_t>(c2);
    int32_t *dr1 = B.zeros<int32_t>(c1), *dr2 = B.zeros<int32_t>(c2);
    const size_t wb = viorb_sim3_match_workspace_bytes((int)std::max(c1, c2), 1, 1);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_search_by_sim3_device(&S[0], &S[1], dR, dt, ds, cam, bounds4, th, 1, d12, dnf, dm1, dm2, dr1, dr2, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_TRY(download(match12, d12, (size_t)n1)); VIORB_TRY(download(nfound, dnf, 1)); VIORB_TRY(download(match1, dm1, (size_t)n1));
    VIORB_TRY(download(match2, dm2, (size_t)n2)); VIORB_TRY(download(reason1, dr1, (size_t)n1));
    return download(reason2, dr2, (size_t)n2);
}

int viorb_search_by_projection_sim3_device(const viorb_s3m_keyframes* kf, const float* Scw, const float* pts_f, const uint8_t* pts_desc,
                                           const uint8_t* pts_valid, const int32_t* pts_count, int pcap, const uint8_t* feat_taken,
                                           const viorb_mapping_camera* cam, const float bounds4[4], float th, int batch, int32_t* best_idx,
                                           int32_t* nmatches, int32_t* reason, void* workspace, size_t workspace_bytes, void* stream) {
    S3mScwArgs A;
    VIORB_TRY(s3m_check_cam(cam, bounds4, th, batch, A.cam));
    VIORB_TRY(s3m_check_kf(kf));
    VIORB_REQUIRE(Scw && pts_f && pts_desc && pts_valid && pts_count && feat_taken && best_idx && nmatches, "null array");
    VIORB_REQUIRE(pcap >= 1, "pcap >= 1");
    VIORB_TRY(s3m_check_workspace(workspace, workspace_bytes, kf->cap, pcap, batch));
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const S3mLayout L = s3m_layout(workspace, kf->cap, pcap, batch);
    A.kf = s3m_kf(*kf); A.Scw = Scw; A.pts_f = pts_f; A.pts_desc = pts_desc; A.pts_valid = pts_valid; A.pts_count = pts_count; A.feat_taken = feat_taken;
    A.best_idx = best_idx; A.reason = reason; A.cand = L.cand; A.cand_n = L.cand_n; A.partial = nullptr; A.nmatches = nmatches; A.pcap = pcap; A.npts_shared = -1;
    VIORB_LAUNCH(k_s3m_scw<true>, dim3(s3m_chunks(pcap), batch), S3M_BLOCK, 0, st, A);
    const size_t lds = (size_t)kf->cap * sizeof(int);                // cap <= VIORB_S3M_MAX_FEATURES: at most 64 KiB beside the static words
    if (lds > 48 * 1024) VIORB_HIP_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(k_s3m_claim), lds));
    VIORB_LAUNCH(k_s3m_claim, batch, S3M_CLAIM_THREADS, lds, st, A);
    return VIORB_OK;
}

int viorb_search_by_projection_sim3(const viorb_keypoint* kps, const uint8_t* desc, int n, const float Scw[12], const float* pts_f,
                                    const uint8_t* pts_desc, const uint8_t* pts_valid, int npts, const uint8_t* feat_taken,
                                    const viorb_mapping_camera* cam, const float bounds4[4], float th, int32_t* best_idx, int32_t* nmatches,
                                    int32_t* reason) {
    S3mCam C;
    VIORB_TRY(s3m_check_cam(cam, bounds4, th, 1, C));
    VIORB_REQUIRE(n >= 0 && npts >= 0 && Scw && nmatches, "null array or a negative count");
    VIORB_REQUIRE(n == 0 || (kps && desc && feat_taken), "null array");
    VIORB_REQUIRE(npts == 0 || (pts_f && pts_desc && pts_valid && best_idx), "null array");
    if (n > VIORB_S3M_MAX_FEATURES) { set_error("n %d above VIORB_S3M_MAX_FEATURES", n); return VIORB_ERR_CAPACITY; }
    VIORB_TRY(require_device());
    DeviceBufs B; viorb_s3m_keyframes kf;
    VIORB_TRY(host_keyframe(B, kps, desc, n, std::max(n, 1), bounds4, kf));
    const size_t pc = (size_t)std::max(npts, 1), m = (size_t)npts;
    float *dS = B.up(Scw, 12), *dpf = B.up(pts_f, m * 8, pc * 8);
    uint8_t *dpd = B.up(pts_desc, m * 32, pc * 32), *dpv = B.up(pts_valid, m, pc), *dft = B.up(feat_taken, (size_t)n, (size_t)kf.cap);
    int32_t *dpc = B.up(&npts, 1), *dbi = B.zeros<int32_t>(pc), *dnm = B.zeros<int32_t>(1), *dre = B.zeros<int32_t>(pc);
    const size_t wb = viorb_sim3_match_workspace_bytes(kf.cap, (int)pc, 1);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_search_by_projection_sim3_device(&kf, dS, dpf, dpd, dpv, dpc, (int)pc, dft, cam, bounds4, th, 1, dbi, dnm, dre, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_TRY(download(best_idx, dbi, m)); VIORB_TRY(download(nmatches, dnm, 1));
    return download(reason, dre, m);
}

int viorb_fuse_sim3_device(const viorb_s3m_keyframes* kf, const float* Scw, const float* pts_f, const uint8_t* pts_desc, const uint8_t* pts_valid,
                           int npts, int pcap, const viorb_mapping_camera* cam, const float bounds4[4], float th, int batch, int32_t* best_idx,
                           int32_t* nfused, int32_t* reason, void* workspace, size_t workspace_bytes, void* stream) {
    S3mScwArgs A;
    VIORB_TRY(s3m_check_cam(cam, bounds4, th, batch, A.cam));
    VIORB_TRY(s3m_check_kf(kf));
    VIORB_REQUIRE(Scw && pts_f && pts_desc && pts_valid && best_idx && nfused, "null array");
    VIORB_REQUIRE(pcap >= 1 && npts >= 0 && npts <= pcap, "pcap >= 1, 0 <= npts <= pcap");
    VIORB_TRY(s3m_check_workspace(workspace, workspace_bytes, kf->cap, pcap, batch));
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    const S3mLayout L = s3m_layout(workspace, kf->cap, pcap, batch);
    A.kf = s3m_kf(*kf); A.Scw = Scw; A.pts_f = pts_f; A.pts_desc = pts_desc; A.pts_valid = pts_valid; A.pts_count = nullptr; A.feat_taken = nullptr;
    A.best_idx = best_idx; A.reason = reason; A.cand = nullptr; A.cand_n = nullptr; A.partial = L.partial; A.nmatches = nullptr; A.pcap = pcap; A.npts_shared = npts;
    const int chunks = s3m_chunks(pcap);
    VIORB_LAUNCH(k_s3m_scw<false>, dim3(chunks, batch), S3M_BLOCK, 0, st, A);
    VIORB_LAUNCH(k_s3m_counts, (batch + S3M_WAVE - 1) / S3M_WAVE, S3M_WAVE, 0, st, L.partial, chunks, batch, nfused);
    return VIORB_OK;
}

int viorb_fuse_sim3(const viorb_keypoint* kps, const uint8_t* desc, int n, const float Scw[12], const float* pts_f, const uint8_t* pts_desc,
                    const uint8_t* pts_valid, int npts, const viorb_mapping_camera* cam, const float bounds4[4], float th, int32_t* best_idx,
                    int32_t* nfused, int32_t* reason) {
    S3mCam C;
    VIORB_TRY(s3m_check_cam(cam, bounds4, th, 1, C));
    VIORB_REQUIRE(n >= 0 && npts >= 0 && Scw && nfused, "null array or a negative count");
    VIORB_REQUIRE(n == 0 || (kps && desc), "null array");
    VIORB_REQUIRE(npts == 0 || (pts_f && pts_desc && pts_valid && best_idx), "null array");
    if (n > VIORB_S3M_MAX_FEATURES) { set_error("n %d above VIORB_S3M_MAX_FEATURES", n); return VIORB_ERR_CAPACITY; }
    VIORB_TRY(require_device());
    DeviceBufs B; viorb_s3m_keyframes kf;
    VIORB_TRY(host_keyframe(B, kps, desc, n, std::max(n, 1), bounds4, kf));
    const size_t pc = (size_t)std::max(npts, 1), m = (size_t)npts;
    float *dS = B.up(Scw, 12), *dpf = B.up(pts_f, m * 8, pc * 8);
    uint8_t *dpd = B.up(pts_desc, m * 32, pc * 32), *dpv = B.up(pts_valid, m, pc);
    int32_t *dbi = B.zeros<int32_t>(pc), *dnf = B.zeros<int32_t>(1), *dre = B.zeros<int32_t>(pc);
    const size_t wb = viorb_sim3_match_workspace_bytes(kf.cap, (int)pc, 1);
    unsigned char* dw = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    VIORB_TRY(viorb_fuse_sim3_device(&kf, dS, dpf, dpd, dpv, npts, (int)pc, cam, bounds4, th, 1, dbi, dnf, dre, dw, wb, nullptr));
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_TRY(download(best_idx, dbi, m)); VIORB_TRY(download(nfused, dnf, 1));
    return download(reason, dre, m);
}

// ---- host-only test hooks: sim3_match_core.h compiled for the host ---------------------------------------------------------------------
int viorb_debug_sim3_decompose(const float* Scw12, float* out16) {
    VIORB_REQUIRE(Scw12 && out16, "null array");
    S3mScw D;
    s3m_decompose(Scw12, D);
    out16[0] = D.scw;
    for (int k = 0; k < 9; k++) out16[1 + k] = D.R[k];
    for (int k = 0; k < 3; k++) { out16[10 + k] = D.t[k]; out16[13 + k] = D.Ow[k]; }
    return VIORB_OK;
}

int viorb_debug_sim3_pair(const float* R12, const float* t12, float s12, float* out21) {
    VIORB_REQUIRE(R12 && t12 && out21, "null array");
    S3mPair T;
    s3m_pair(R12, t12, s12, T);
    for (int k = 0; k < 9; k++) { out21[k] = T.sR12[k]; out21[9 + k] = T.sR21[k]; }
    for (int k = 0; k < 3; k++) out21[18 + k] = T.t21[k];
    return VIORB_OK;
}

int viorb_debug_sim3_project(int which, const float* T12, const float* sR9, const float* t3, const float* pt8, const viorb_mapping_camera* cam,
                             const float bounds4[4], float th, float* out4, int32_t* out6) {
    S3mCam C;
    VIORB_TRY(s3m_check_cam(cam, bounds4, th, 1, C));
    VIORB_REQUIRE(which >= S3M_FN_SEARCH_BY_SIM3 && which <= S3M_FN_FUSE, "which must be 0, 1 or 2");
    VIORB_REQUIRE(T12 && pt8 && out4 && out6 && (which != S3M_FN_SEARCH_BY_SIM3 || (sR9 && t3)), "null array");
    S3mProj P;
    if (which == S3M_FN_SEARCH_BY_SIM3) s3m_project_pair(C, T12, sR9, t3, pt8, P);
    else { S3mScw D; s3m_decompose(T12, D); s3m_project_scw(C, D, pt8, P); }
    out4[0] = P.u; out4[1] = P.v; out4[2] = P.dist3D; out4[3] = P.radius;
    out6[0] = P.level; out6[1] = P.rect.x0; out6[2] = P.rect.x1; out6[3] = P.rect.y0; out6[4] = P.rect.y1; out6[5] = P.reason;
    return VIORB_OK;
}

int viorb_debug_claim_in_order(const uint32_t* cand, const int32_t* cand_n, int npts, int lcap, const uint8_t* taken_in, int nfeat, int32_t* best_idx,
                               int32_t* nmatches) {
    VIORB_REQUIRE(npts >= 0 && lcap >= 1 && nfeat >= 0 && nmatches && (npts == 0 || (cand && cand_n && best_idx)) && (nfeat == 0 || taken_in),
                  "null array or a negative size");
    std::vector<int32_t> owner((size_t)std::max(nfeat, 1));
    const int sweeps = s3m_claim_in_order(cand, cand_n, npts, lcap, taken_in, nfeat, best_idx, owner.data());
    int m = 0;
    for (int p = 0; p < npts; p++) m += best_idx[p] >= 0;
    *nmatches = m;
    return sweeps;
}

} // extern "C"
