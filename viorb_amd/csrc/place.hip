// viorb_amd/csrc/place.hip — place recognition on the device: the BowVector of a frame, ORBVocabulary::score for lists of pairs and the
// key-frame database (KeyFrameDatabase::add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates). Kernels first, then
// the C ABI of include/viorb.h. The scalar pieces are place_core.h; reference lines are cited there and in DESIGN.md §1.
// Every result is bit-exact: integers, float compares and, per value, ONE ordered chain of double (score, norm) or float (accScore)
// additions. No floating-point atomics; the integer atomics only count, take a max / min or hand out positions that a sort then orders.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "viorb_common.h"
#include "place_core.h"

using namespace viorb;

struct viorb_kfdb {
    int n_words = 0;
    long long* d_off = nullptr;          // [slot_cap + 1], d_off[0] = 0; entries of slot s are d_off[s] .. d_off[s + 1]
    int32_t* d_words = nullptr;          // [entry_cap]
    double* d_vals = nullptr;            // [entry_cap]
    uint8_t* d_alive = nullptr;          // [slot_cap]
    size_t slot_cap = 0, entry_cap = 0, slot_hint = 0, entry_hint = 0;
    int n_slots = 0, n_alive = 0;
    long long fill_ub = 0;               // an upper bound of d_off[n_slots] (exact after a host-form add or a growth check)
    std::vector<uint8_t> alive;          // the host's copy (bookkeeping of erase / size)
    std::vector<int> pending_erase;      // slots erased since the last query: their d_alive bytes are cleared on the next query's stream
};

namespace {

constexpr int BOW_LDS_FEATURES = VIORB_BOW_VECTOR_MAX_FEATURES;     // k_bow_vector sorts this many 64-bit keys in LDS (64 KB)
constexpr int QUERY_LDS_WORDS = 8192;                               // k_kfdb_common<false> stages this many query words in LDS (32 KB)

// The rank of a set flag among the set flags of the block's 256 threads, in thread order, and their number. red: 4 ints of LDS.
__device__ int block_rank(bool flag, int* red, int* total) {
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                     // the previous call's readers are done with red
    if (lane == 0) red[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < 4; k++) { if (k < w) off += red[k]; tot += red[k]; }
    *total = tot;
    return off + before;
}

// Ascending bitonic sort of a[0..P), P a power of two, by the whole block. The keys are unique, so the result does not depend on the network.
__device__ void block_bitonic(unsigned long long* a, int P) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                const unsigned long long x = a[i], y = a[l];
                if ((x > y) == up) { a[i] = y; a[l] = x; }
            }
        }
    __syncthreads();
}

__device__ __forceinline__ int pow2_at_least(int n) { int P = 1; while (P < n) P <<= 1; return P; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- BowVector::addWeight in feature order + normalize(L1) (Thirdparty/DBoW2/DBoW2/BowVector.cpp:36-85). One workgroup per frame: a sort
// by (word, feature index) in LDS — the index makes the keys unique and the sort stable —, one lane per word sums that word's weights in
// feature order, then one lane sums the norm over the words in ascending order.
__global__ __launch_bounds__(256) void k_bow_vector(const int32_t* word, const double* weight, const int32_t* count, int cap, int32_t* bow_word,
                                                    double* bow_val, int32_t* bow_count) {
    extern __shared__ unsigned long long s_key[];
    __shared__ int s_red[4];
    __shared__ int s_m;
    __shared__ double s_norm;
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)b * cap;
    const int n = clampi(count[b], 0, cap), P = pow2_at_least(n);
    if (tid == 0) s_m = 0;
    __syncthreads();
    for (int i = tid; i < P; i += 256) {
        const bool ok = i < n && weight[base + i] > 0.0;
        s_key[i] = ok ? place_order_key(word[base + i], i) : ~0ull;
        if (ok) atomicAdd(&s_m, 1);
    }
    block_bitonic(s_key, P);
    const int m = s_m;
    int nout = 0;
    for (int t0 = 0; t0 < m; t0 += 256) {
        const int j = t0 + tid;
        bool head = false;
        int w = 0;
        if (j < m) { w = (int)(s_key[j] >> 32); head = j == 0 || (int)(s_key[j - 1] >> 32) != w; }
        int tot;
        const int r = block_rank(head, s_red, &tot);
        if (head) {
            double s = weight[base + (uint32_t)s_key[j]];
            for (int e = j + 1; e < m && (int)(s_key[e] >> 32) == w; e++) s += weight[base + (uint32_t)s_key[e]];
            bow_word[base + nout + r] = w;
            bow_val[base + nout + r] = s;
        }
        nout += tot;
    }
    __syncthreads();
    double* s_val = reinterpret_cast<double*>(s_key);            // nout <= m <= P
    for (int j = tid; j < nout; j += 256) s_val[j] = bow_val[base + j];
    __syncthreads();
    if (tid == 0) {
        double nm = 0.0;
        for (int j = 0; j < nout; j++) nm += fabs(s_val[j]);
        s_norm = nm;
        bow_count[b] = nout;
    }
    __syncthreads();
    const double nm = s_norm;
    if (nm > 0.0)
        for (int j = tid; j < nout; j += 256) bow_val[base + j] = s_val[j] / nm;
}

// ---- L1Scoring::score by one wavefront: 64 entries of the shorter vector per trip, each lane binary-searches the longer one, and the
// terms of the hits are added in lane order — the ascending order of the common words — by every lane alike.
__device__ double wave_score(const int32_t* aw, const double* av, int na, const int32_t* bw, const double* bv, int nb) {
    const int lane = threadIdx.x & 63;
    const bool a_short = na <= nb;
    const int32_t* sw = a_short ? aw : bw;
    const int32_t* lw = a_short ? bw : aw;
    const int ns = a_short ? na : nb, nl = a_short ? nb : na;
    double s = 0.0;
    for (int t0 = 0; t0 < ns; t0 += 64) {
        const int i = t0 + lane;
        double term = 0.0;
        bool hit = false;
        if (i < ns) {
            const int j = place_find(lw, nl, sw[i]);
            if (j >= 0) { hit = true; term = a_short ? place_score_term(av[i], bv[j]) : place_score_term(av[j], bv[i]); }
        }
        unsigned long long m = __ballot(hit);
        while (m) {
            s += __shfl(term, __ffsll((long long)m) - 1);
            m &= m - 1;
        }
    }
    return place_score_finish(s);
}

__global__ __launch_bounds__(256) void k_bow_score(const int32_t* a_word, const double* a_val, const int32_t* a_count, int a_cap, const int32_t* b_word,
                                                   const double* b_val, const int32_t* b_count, int b_cap, const int32_t* pair_a,
                                                   const int32_t* pair_b, int n_pairs, double* score) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_pairs) return;
    const int ia = pair_a[p], ib = pair_b[p];
    const size_t oa = (size_t)ia * a_cap, ob = (size_t)ib * b_cap;
    const double s = wave_score(a_word + oa, a_val + oa, clampi(a_count[ia], 0, a_cap), b_word + ob, b_val + ob, clampi(b_count[ib], 0, b_cap));
    if ((threadIdx.x & 63) == 0) score[p] = s;
}

// ---- the key-frame database ------------------------------------------------------------------------------------------------------
__global__ void k_kfdb_append_offsets(long long* off, int first, const int32_t* bow_count, int cap, int n) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long o = off[first];
    for (int i = 0; i < n; i++) { o += clampi(bow_count[i], 0, cap); off[first + 1 + i] = o; }
}

__global__ __launch_bounds__(256) void k_kfdb_append_copy(const long long* off, int first, const int32_t* bow_word, const double* bow_val, int cap,
                                                          int32_t* words, double* vals, long long entry_cap) {
    const int i = blockIdx.x;
    const long long o = off[first + i], c = off[first + i + 1] - o;
    if (c < 0 || c > cap || o < 0 || o + c > entry_cap) return;          // the host keeps the arena large enough; never write past it
    for (int j = threadIdx.x; j < (int)c; j += 256) {
        words[o + j] = bow_word[(size_t)i * cap + j];
        vals[o + j] = bow_val[(size_t)i * cap + j];
    }
}

struct QueryArgs {
    const long long* off; const int32_t* words; const double* vals; const uint8_t* alive; int n_slots;
    int mode, q_cap, cand_cap, P;
    const int32_t* q_word; const double* q_val; const int32_t* q_count;
    const float* min_score; const int32_t* excl_start; const int32_t* excl_slot; const int32_t* covis10;
    int32_t *cand, *n_cand, *stats, *common_out; float* score_out;
    int32_t *common, *min_word, *first_pos, *best, *thr; float *score, *acc; unsigned long long* keys;      // workspace
};

// Pass 1 (src/KeyFrameDatabase.cc:86-104, :207-222 as a count per key frame): a wavefront streams one key frame's words, 64 per trip, and
// every lane binary-searches the query's words (in LDS; GLOBAL: in memory, for a query that does not fit). Integer only.
template <bool GLOBAL> __global__ __launch_bounds__(256) void k_kfdb_common(QueryArgs A) {
    extern __shared__ int32_t s_q[];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, S = A.n_slots;
    const int nq = clampi(A.q_count[q], 0, A.q_cap);
    const int32_t* qw = A.q_word + (size_t)q * A.q_cap;
    if (!GLOBAL) {
        for (int i = tid; i < nq; i += 256) s_q[i] = qw[i];
        __syncthreads();
    }
    const int32_t* sq = GLOBAL ? qw : s_q;
    const bool loop = A.mode == PLACE_LOOP;
    const int e0 = loop ? A.excl_start[q] : 0, e1 = loop ? A.excl_start[q + 1] : 0;
    for (int s = blockIdx.x * 4 + wave; s < S; s += gridDim.x * 4) {
        bool skip = A.alive[s] == 0;
        if (!skip && loop) {
            bool ex = false;
            for (int e = e0 + lane; e < e1; e += 64) ex |= A.excl_slot[e] == s;
            skip = __ballot(ex) != 0ull;
        }
        int cnt = 0, minw = -1;
        if (!skip) {
            const long long o1 = A.off[s + 1];
            for (long long o = A.off[s]; o < o1; o += 64) {
                bool hit = false;
                int w = 0;
                if (o + lane < o1) { w = A.words[o + lane]; hit = place_find(sq, nq, w) >= 0; }
                const unsigned long long m = __ballot(hit);
                if (m) {
                    const int first = __shfl(w, __ffsll((long long)m) - 1);
                    if (cnt == 0) minw = first;
                    cnt += __popcll(m);
                }
            }
        }
        if (lane == 0) {
            const size_t idx = (size_t)q * S + s;
            A.common[idx] = cnt; A.min_word[idx] = minw; A.score[idx] = -1.0f; A.first_pos[idx] = INT_MAX;
            if (A.common_out) A.common_out[idx] = cnt;
            if (A.score_out) A.score_out[idx] = -1.0f;
        }
    }
}

// maxCommonWords, minCommonWords and the number of key frames sharing a word (:113-120, :228-235)
__global__ __launch_bounds__(256) void k_kfdb_threshold(QueryArgs A) {
    __shared__ int s_max, s_cnt;
    const int q = blockIdx.x, tid = threadIdx.x, S = A.n_slots;
    if (tid == 0) { s_max = 0; s_cnt = 0; }
    __syncthreads();
    int mx = 0, c = 0;
    for (int s = tid; s < S; s += 256) { const int v = A.common[(size_t)q * S + s]; mx = v > mx ? v : mx; c += v >= 1; }
    atomicMax(&s_max, mx);
    atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid == 0) {
        A.thr[q * 2] = s_max; A.thr[q * 2 + 1] = place_min_common(s_max);
        A.stats[q * 4] = s_cnt; A.stats[q * 4 + 1] = s_max;
    }
}

// si = (float)score(query, key frame) for the key frames above the threshold (:125-139, :242-253); every other wavefront leaves at once
__global__ __launch_bounds__(256) void k_kfdb_score(QueryArgs A) {
    const int q = blockIdx.y, s = blockIdx.x * 4 + (threadIdx.x >> 6), S = A.n_slots;
    if (s >= S) return;
    const size_t idx = (size_t)q * S + s;
    if (A.common[idx] <= A.thr[q * 2 + 1]) return;
    const size_t oq = (size_t)q * A.q_cap;
    const long long o = A.off[s];
    const double sc = wave_score(A.q_word + oq, A.q_val + oq, clampi(A.q_count[q], 0, A.q_cap), A.words + o, A.vals + o, (int)(A.off[s + 1] - o));
    if ((threadIdx.x & 63) == 0) {
        A.score[idx] = (float)sc;
        if (A.score_out) A.score_out[idx] = (float)sc;
    }
}

// Steps 3-6 of one query by one workgroup: the scored key frames in the reference's list order (a sort by (smallest common word, slot)),
// the covisibility groups (:148-173, :262-287), bestAccScore by a max, the first occurrence of every best key frame by an integer min and
// an ordered compaction (:176-193, :290-306).
__global__ __launch_bounds__(256) void k_kfdb_select(QueryArgs A) {
    __shared__ int s_red[4];
    __shared__ int s_n, s_kept;
    __shared__ float s_max[256];
    const int q = blockIdx.x, tid = threadIdx.x, S = A.n_slots;
    const size_t row = (size_t)q * S;
    const int32_t* common = A.common + row;
    const float* score = A.score + row;
    int32_t* first_pos = A.first_pos + row;
    int32_t* best = A.best + row;
    float* acc = A.acc + row;
    unsigned long long* keys = A.keys + (size_t)q * A.P;
    const int minc = A.thr[q * 2 + 1];
    if (tid == 0) { s_n = 0; s_kept = 0; }
    __syncthreads();
    for (int s = tid; s < S; s += 256)
        if (common[s] > minc) keys[atomicAdd(&s_n, 1)] = place_order_key(A.min_word[row + s], s);
    __syncthreads();
    const int n = s_n, P2 = pow2_at_least(n);                     // n <= S <= A.P
    for (int i = n + tid; i < P2; i += 256) keys[i] = ~0ull;
    block_bitonic(keys, P2);
    const bool loop = A.mode == PLACE_LOOP;
    const float ms = loop ? A.min_score[q] : 0.0f;
    float mx = ms;                                                // bestAccScore = minScore (:145) or 0 (:259)
    int kept = 0;
    for (int i = tid; i < n; i += 256) {
        const int s = (int)(uint32_t)keys[i];
        float a = 0.0f;
        int b = -1;
        if (!loop || score[s] >= ms) {
            place_group(s, common, score, minc, A.covis10, S, &a, &b);
            mx = a > mx ? a : mx;
            kept++;
        }
        acc[i] = a; best[i] = b;
    }
    s_max[tid] = mx;
    atomicAdd(&s_kept, kept);
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) s_max[tid] = s_max[tid + k] > s_max[tid] ? s_max[tid + k] : s_max[tid];
        __syncthreads();
    }
    const float retain = 0.75f * s_max[0];
    for (int i = tid; i < n; i += 256)
        if (best[i] >= 0 && acc[i] > retain) atomicMin(&first_pos[best[i]], i);
    __syncthreads();
    int nout = 0;
    for (int t0 = 0; t0 < n; t0 += 256) {
        const int i = t0 + tid;
        const bool emit = i < n && best[i] >= 0 && acc[i] > retain && __hip_atomic_load(&first_pos[best[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i;
        int tot;
        const int r = block_rank(emit, s_red, &tot);
        if (emit && nout + r < A.cand_cap) A.cand[(size_t)q * A.cand_cap + nout + r] = best[i];
        nout += tot;
    }
    if (tid == 0) { A.n_cand[q] = nout; A.stats[q * 4 + 2] = n; A.stats[q * 4 + 3] = s_kept; }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
size_t pow2_host(size_t n) { size_t P = 1; while (P < n) P <<= 1; return P; }

size_t query_layout(void* ws, int n_slots, int n_q, QueryArgs* A) {
    WorkspaceLayout L(ws);
    const size_t qs = (size_t)n_q * (size_t)n_slots, P = pow2_host((size_t)std::max(n_slots, 1));
    L.take(A ? &A->common : nullptr, qs); L.take(A ? &A->min_word : nullptr, qs); L.take(A ? &A->first_pos : nullptr, qs);
    L.take(A ? &A->best : nullptr, qs); L.take(A ? &A->score : nullptr, qs); L.take(A ? &A->acc : nullptr, qs);
    L.take(A ? &A->thr : nullptr, 2 * (size_t)n_q); L.take(A ? &A->keys : nullptr, (size_t)n_q * P);
    if (A) A->P = (int)P;
    return L.end();
}

// Room for add_slots more key frames and add_entries more entries. Growth copies on the caller's stream and waits for it once.
int kfdb_reserve(viorb_kfdb* db, size_t add_slots, size_t add_entries, hipStream_t st) {
    const size_t need_slots = (size_t)db->n_slots + add_slots;
    if (need_slots > db->slot_cap || !db->d_off) {
        const size_t cap = std::max(std::max(2 * db->slot_cap, need_slots), std::max<size_t>(db->slot_hint, 1));
        long long* off = nullptr;
        uint8_t* alive = nullptr;
        VIORB_HIP_TRY(hipMalloc((void**)&off, (cap + 1) * sizeof(long long)));
        if (hipMalloc((void**)&alive, cap) != hipSuccess) { (void)hipFree(off); set_error("device allocation failed"); return VIORB_ERR_HIP; }
        hipError_t e = hipMemsetAsync(off, 0, (cap + 1) * sizeof(long long), st);
        if (e == hipSuccess) e = hipMemsetAsync(alive, 0, cap, st);
        if (e == hipSuccess && db->d_off) e = hipMemcpyAsync(off, db->d_off, ((size_t)db->n_slots + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && db->d_alive && db->n_slots > 0) e = hipMemcpyAsync(alive, db->d_alive, (size_t)db->n_slots, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(off); (void)hipFree(alive); set_error("growing the key-frame table failed: %s", hipGetErrorString(e)); return VIORB_ERR_HIP; }
        (void)hipFree(db->d_off); (void)hipFree(db->d_alive);
        db->d_off = off; db->d_alive = alive; db->slot_cap = cap;
    }
    if ((size_t)db->fill_ub + add_entries > db->entry_cap || !db->d_words) {
        if (db->n_slots > 0) {                                    // the exact fill replaces the bound before anything is grown
            VIORB_HIP_TRY(hipStreamSynchronize(st));
            VIORB_HIP_TRY(hipMemcpy(&db->fill_ub, db->d_off + db->n_slots, sizeof(long long), hipMemcpyDeviceToHost));
        }
        const size_t need = (size_t)db->fill_ub + add_entries;
        if (need > db->entry_cap || !db->d_words) {
            const size_t cap = std::max(std::max(2 * db->entry_cap, need), std::max<size_t>(db->entry_hint, 1));
            int32_t* w = nullptr;
            double* v = nullptr;
            VIORB_HIP_TRY(hipMalloc((void**)&w, cap * sizeof(int32_t)));
            if (hipMalloc((void**)&v, cap * sizeof(double)) != hipSuccess) { (void)hipFree(w); set_error("device allocation failed"); return VIORB_ERR_HIP; }
            hipError_t e = hipSuccess;
            if (db->d_words && db->fill_ub > 0) {
                e = hipMemcpyAsync(w, db->d_words, (size_t)db->fill_ub * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
                if (e == hipSuccess) e = hipMemcpyAsync(v, db->d_vals, (size_t)db->fill_ub * sizeof(double), hipMemcpyDeviceToDevice, st);
                if (e == hipSuccess) e = hipStreamSynchronize(st);
            }
            if (e != hipSuccess) { (void)hipFree(w); (void)hipFree(v); set_error("growing the key-frame arena failed: %s", hipGetErrorString(e)); return VIORB_ERR_HIP; }
            (void)hipFree(db->d_words); (void)hipFree(db->d_vals);
            db->d_words = w; db->d_vals = v; db->entry_cap = cap;
        }
    }
    return VIORB_OK;
}

bool ascending_below(const int32_t* w, int n, int limit) {
    for (int i = 0; i < n; i++)
        if (w[i] < 0 || w[i] >= limit || (i > 0 && w[i] <= w[i - 1])) return false;
    return true;
}

} // namespace

extern "C" {

int viorb_bow_vector_device(const int32_t* word, const double* weight, const int32_t* count, int cap, int batch, int32_t* bow_word,
                            double* bow_val, int32_t* bow_count, void* stream) {
    VIORB_REQUIRE(cap >= 1 && batch >= 0, "cap >= 1, batch >= 0");
    if (batch == 0) return VIORB_OK;
    VIORB_REQUIRE(word && weight && count && bow_word && bow_val && bow_count, "null array");
    if (cap > BOW_LDS_FEATURES) {
        set_error("cap = %d features per frame is above VIORB_BOW_VECTOR_MAX_FEATURES = %d", cap, BOW_LDS_FEATURES);
        return VIORB_ERR_CAPACITY;
    }
    VIORB_TRY(require_device());
    const size_t lds = pow2_host((size_t)cap) * sizeof(unsigned long long);
    VIORB_HIP_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(&k_bow_vector), lds));
    VIORB_LAUNCH(k_bow_vector, batch, 256, lds, (hipStream_t)stream, word, weight, count, cap, bow_word, bow_val, bow_count);
    return VIORB_OK;
}

int viorb_bow_vector(const int32_t* word, const double* weight, int n, int32_t* bow_word, double* bow_val, int* bow_count) {
    VIORB_REQUIRE(n >= 0 && bow_count, "n >= 0, bow_count != NULL");
    *bow_count = 0;
    if (n == 0) return VIORB_OK;
    VIORB_REQUIRE(word && weight && bow_word && bow_val, "null array");
    if (n > BOW_LDS_FEATURES) {
        set_error("n = %d features is above VIORB_BOW_VECTOR_MAX_FEATURES = %d", n, BOW_LDS_FEATURES);
        return VIORB_ERR_CAPACITY;
    }
    VIORB_TRY(require_device());
    DeviceBufs B;
    int32_t *dw = B.up(word, n), *dc = B.up(&n, 1), *dbw = B.zeros<int32_t>(n), *dbc = B.zeros<int32_t>(1);
    double *dv = B.up(weight, n), *dbv = B.zeros<double>(n);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_bow_vector_device(dw, dv, dc, n, 1, dbw, dbv, dbc, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_HIP_TRY(hipMemcpy(bow_count, dbc, sizeof(int), hipMemcpyDeviceToHost));
    if (*bow_count > 0) {
        VIORB_HIP_TRY(hipMemcpy(bow_word, dbw, sizeof(int32_t) * (size_t)*bow_count, hipMemcpyDeviceToHost));
        VIORB_HIP_TRY(hipMemcpy(bow_val, dbv, sizeof(double) * (size_t)*bow_count, hipMemcpyDeviceToHost));
    }
    return VIORB_OK;
}

int viorb_bow_score_device(const int32_t* a_word, const double* a_val, const int32_t* a_count, int a_cap, const int32_t* b_word,
                           const double* b_val, const int32_t* b_count, int b_cap, const int32_t* pair_a, const int32_t* pair_b,
                           int n_pairs, double* score, void* stream) {
    VIORB_REQUIRE(a_cap >= 1 && b_cap >= 1 && n_pairs >= 0, "a_cap >= 1, b_cap >= 1, n_pairs >= 0");
    if (n_pairs == 0) return VIORB_OK;
    VIORB_REQUIRE(a_word && a_val && a_count && b_word && b_val && b_count && pair_a && pair_b && score, "null array");
    VIORB_TRY(require_device());
    VIORB_LAUNCH(k_bow_score, (n_pairs + 3) / 4, 256, 0, (hipStream_t)stream, a_word, a_val, a_count, a_cap, b_word, b_val, b_count, b_cap, pair_a, pair_b,
                 n_pairs, score);
    return VIORB_OK;
}

int viorb_bow_score(const int32_t* a_word, const double* a_val, const int32_t* a_count, int a_cap, int na, const int32_t* b_word,
                    const double* b_val, const int32_t* b_count, int b_cap, int nb, const int32_t* pair_a, const int32_t* pair_b,
                    int n_pairs, double* score) {
    VIORB_REQUIRE(a_cap >= 1 && b_cap >= 1 && na >= 0 && nb >= 0 && n_pairs >= 0, "a_cap >= 1, b_cap >= 1, na, nb, n_pairs >= 0");
    if (n_pairs == 0) return VIORB_OK;
    VIORB_REQUIRE(a_word && a_val && a_count && b_word && b_val && b_count && pair_a && pair_b && score, "null array");
    for (int i = 0; i < na; i++)
        VIORB_REQUIRE(a_count[i] >= 0 && a_count[i] <= a_cap && ascending_below(a_word + (size_t)i * a_cap, a_count[i], INT_MAX), "a: counts in 0..a_cap, ascending words");
    for (int i = 0; i < nb; i++)
        VIORB_REQUIRE(b_count[i] >= 0 && b_count[i] <= b_cap && ascending_below(b_word + (size_t)i * b_cap, b_count[i], INT_MAX), "b: counts in 0..b_cap, ascending words");
    for (int p = 0; p < n_pairs; p++) VIORB_REQUIRE(pair_a[p] >= 0 && pair_a[p] < na && pair_b[p] >= 0 && pair_b[p] < nb, "pair index out of range");
    VIORB_TRY(require_device());
    DeviceBufs B;
    int32_t *daw = B.up(a_word, (size_t)na * a_cap), *dac = B.up(a_count, na), *dbw = B.up(b_word, (size_t)nb * b_cap), *dbc = B.up(b_count, nb);
    int32_t *dpa = B.up(pair_a, n_pairs), *dpb = B.up(pair_b, n_pairs);
    double *dav = B.up(a_val, (size_t)na * a_cap), *dbv = B.up(b_val, (size_t)nb * b_cap), *ds = B.zeros<double>(n_pairs);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_bow_score_device(daw, dav, dac, a_cap, dbw, dbv, dbc, b_cap, dpa, dpb, n_pairs, ds, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_HIP_TRY(hipMemcpy(score, ds, sizeof(double) * (size_t)n_pairs, hipMemcpyDeviceToHost));
    return VIORB_OK;
}

int viorb_kfdb_create(int n_words, int kf_capacity_hint, int entry_capacity_hint, viorb_kfdb** out) {
    VIORB_REQUIRE(out, "out == NULL");
    *out = nullptr;
    VIORB_REQUIRE(n_words >= 1 && kf_capacity_hint >= 0 && entry_capacity_hint >= 0, "n_words >= 1, capacity hints >= 0");
    viorb_kfdb* db = new (std::nothrow) viorb_kfdb();
    VIORB_REQUIRE(db, "out of host memory");
    db->n_words = n_words; db->slot_hint = (size_t)kf_capacity_hint; db->entry_hint = (size_t)entry_capacity_hint;
    *out = db;                                                    // device memory is allocated by the first add
    return VIORB_OK;
}

int viorb_kfdb_destroy(viorb_kfdb* db) {
    if (!db) return VIORB_OK;
    (void)hipFree(db->d_off); (void)hipFree(db->d_words); (void)hipFree(db->d_vals); (void)hipFree(db->d_alive);
    delete db;
    return VIORB_OK;
}

int viorb_kfdb_add_device(viorb_kfdb* db, const int32_t* bow_word, const double* bow_val, const int32_t* bow_count, int cap, int n,
                          int* first_slot_out, void* stream) {
    VIORB_REQUIRE(db && cap >= 1 && n >= 0, "db != NULL, cap >= 1, n >= 0");
    if (n == 0) { if (first_slot_out) *first_slot_out = db->n_slots; return VIORB_OK; }
    VIORB_REQUIRE(bow_word && bow_val && bow_count, "null array");
    VIORB_REQUIRE((long long)db->n_slots + n <= INT_MAX, "more than 2^31 - 1 key frames");
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    VIORB_TRY(kfdb_reserve(db, (size_t)n, (size_t)n * (size_t)cap, st));
    const int first = db->n_slots;
    VIORB_LAUNCH(k_kfdb_append_offsets, 1, 64, 0, st, db->d_off, first, bow_count, cap, n);
    VIORB_LAUNCH(k_kfdb_append_copy, n, 256, 0, st, db->d_off, first, bow_word, bow_val, cap, db->d_words, db->d_vals, (long long)db->entry_cap);
    VIORB_HIP_TRY(hipMemsetAsync(db->d_alive + first, 1, (size_t)n, st));
    db->n_slots += n; db->n_alive += n; db->fill_ub += (long long)n * cap;
    db->alive.resize((size_t)db->n_slots, 1);
    if (first_slot_out) *first_slot_out = first;
    return VIORB_OK;
}

int viorb_kfdb_add(viorb_kfdb* db, const int32_t* words, const double* vals, int n_entries, int* slot) {
    VIORB_REQUIRE(db && n_entries >= 0 && (n_entries == 0 || (words && vals)), "db != NULL, n_entries >= 0, arrays");
    VIORB_REQUIRE(ascending_below(words, n_entries, db->n_words), "words must ascend strictly and lie in 0 .. n_words - 1");
    for (int i = 0; i < n_entries; i++) VIORB_REQUIRE(std::isfinite(vals[i]) && vals[i] > 0.0, "values must be finite and positive");
    VIORB_TRY(require_device());
    DeviceBufs B;
    int32_t *dw = B.up(words, n_entries), *dc = B.up(&n_entries, 1);
    double* dv = B.up(vals, n_entries);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_kfdb_add_device(db, dw, dv, dc, std::max(n_entries, 1), 1, slot, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
    return VIORB_OK;
}

int viorb_kfdb_erase(viorb_kfdb* db, int slot) {
    VIORB_REQUIRE(db && slot >= 0 && slot < db->n_slots, "db != NULL, 0 <= slot < n_slots");
    if (db->alive[slot]) { db->alive[slot] = 0; db->n_alive--; db->pending_erase.push_back(slot); }
    return VIORB_OK;
}

int viorb_kfdb_clear(viorb_kfdb* db) {
    VIORB_REQUIRE(db, "db == NULL");
    db->n_slots = 0; db->n_alive = 0; db->fill_ub = 0; db->alive.clear(); db->pending_erase.clear();     // d_off[0] stays 0
    return VIORB_OK;
}

int viorb_kfdb_size(const viorb_kfdb* db, int* n_slots, int* n_alive) {
    VIORB_REQUIRE(db && n_slots && n_alive, "null argument");
    *n_slots = db->n_slots; *n_alive = db->n_alive;
    return VIORB_OK;
}

size_t viorb_kfdb_query_workspace_bytes(const viorb_kfdb* db, int n_q) {
    if (!db || n_q < 1) return 0;
    return query_layout(nullptr, db->n_slots, n_q, nullptr);
}

int viorb_kfdb_query_device(viorb_kfdb* db, int mode, int n_q, const int32_t* q_word, const double* q_val, const int32_t* q_count, int q_cap,
                            const float* min_score, const int32_t* excl_start, const int32_t* excl_slot, const int32_t* covis10,
                            int cand_cap, int32_t* cand, int32_t* n_cand, int32_t* stats, int32_t* common_out, float* score_out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    VIORB_REQUIRE(db && (mode == VIORB_KFDB_LOOP || mode == VIORB_KFDB_RELOC), "db != NULL, mode = VIORB_KFDB_LOOP or VIORB_KFDB_RELOC");
    VIORB_REQUIRE(n_q >= 0 && n_q <= 65535 && q_cap >= 1 && cand_cap >= 1, "0 <= n_q <= 65535, q_cap >= 1, cand_cap >= 1");
    if (n_q == 0) return VIORB_OK;
    VIORB_REQUIRE(q_word && q_val && q_count && cand && n_cand && stats, "null array");
    VIORB_REQUIRE(mode != VIORB_KFDB_LOOP || (min_score && excl_start && excl_slot), "loop mode needs min_score, excl_start and excl_slot");
    const int S = db->n_slots;
    QueryArgs A;
    memset(&A, 0, sizeof(A));
    if (S > 0) {
        VIORB_REQUIRE(covis10 && workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= query_layout(nullptr, S, n_q, nullptr),
                      "covis10 == NULL, or workspace smaller than viorb_kfdb_query_workspace_bytes or not 256-byte aligned");
        query_layout(workspace, S, n_q, &A);
    }
    VIORB_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    VIORB_HIP_TRY(hipMemsetAsync(n_cand, 0, sizeof(int32_t) * (size_t)n_q, st));
    VIORB_HIP_TRY(hipMemsetAsync(stats, 0, sizeof(int32_t) * 4 * (size_t)n_q, st));
    if (S == 0) return VIORB_OK;
    for (int slot : db->pending_erase) VIORB_HIP_TRY(hipMemsetAsync(db->d_alive + slot, 0, 1, st));      // a few bytes per culled key frame, no wait
    db->pending_erase.clear();
    A.off = db->d_off; A.words = db->d_words; A.vals = db->d_vals; A.alive = db->d_alive; A.n_slots = S;
    A.mode = mode; A.q_cap = q_cap; A.cand_cap = cand_cap;
    A.q_word = q_word; A.q_val = q_val; A.q_count = q_count; A.min_score = min_score; A.excl_start = excl_start; A.excl_slot = excl_slot;
    A.covis10 = covis10; A.cand = cand; A.n_cand = n_cand; A.stats = stats; A.common_out = common_out; A.score_out = score_out;
    const unsigned per_wave = (unsigned)((S + 3) / 4);
    const dim3 g1(std::min(per_wave, 256u), (unsigned)n_q), g3(per_wave, (unsigned)n_q);
    if (q_cap <= QUERY_LDS_WORDS) {
        ProfScope ps("k_kfdb_common", st);
        hipLaunchKernelGGL(k_kfdb_common<false>, g1, dim3(256), sizeof(int32_t) * (size_t)q_cap, st, A);
    } else {
        ProfScope ps("k_kfdb_common_global", st);
        hipLaunchKernelGGL(k_kfdb_common<true>, g1, dim3(256), 0, st, A);
    }
    VIORB_HIP_TRY(hipGetLastError());
    VIORB_LAUNCH(k_kfdb_threshold, n_q, 256, 0, st, A);
    VIORB_LAUNCH(k_kfdb_score, g3, 256, 0, st, A);
    VIORB_LAUNCH(k_kfdb_select, n_q, 256, 0, st, A);
    return VIORB_OK;
}

int viorb_kfdb_query(viorb_kfdb* db, int mode, int n_q, const int32_t* q_word, const double* q_val, const int32_t* q_count, int q_cap,
                     const float* min_score, const int32_t* excl_start, const int32_t* excl_slot, const int32_t* covis10, int cand_cap,
                     int32_t* cand, int32_t* n_cand, int32_t* stats, int32_t* common_out, float* score_out) {
    VIORB_REQUIRE(db && (mode == VIORB_KFDB_LOOP || mode == VIORB_KFDB_RELOC), "db != NULL, mode = VIORB_KFDB_LOOP or VIORB_KFDB_RELOC");
    VIORB_REQUIRE(n_q >= 0 && n_q <= 65535 && q_cap >= 1 && cand_cap >= 1, "0 <= n_q <= 65535, q_cap >= 1, cand_cap >= 1");
    if (n_q == 0) return VIORB_OK;
    VIORB_REQUIRE(q_word && q_val && q_count && cand && n_cand && stats, "null array");
    const bool loop = mode == VIORB_KFDB_LOOP;
    const int S = db->n_slots;
    VIORB_REQUIRE(!loop || (min_score && excl_start), "loop mode needs min_score and excl_start");
    VIORB_REQUIRE(S == 0 || covis10, "covis10 == NULL");
    for (int q = 0; q < n_q; q++)
        VIORB_REQUIRE(q_count[q] >= 0 && q_count[q] <= q_cap && ascending_below(q_word + (size_t)q * q_cap, q_count[q], db->n_words),
                      "query: counts in 0..q_cap, words ascending strictly and in 0 .. n_words - 1");
    int n_excl = 0;
    if (loop) {
        VIORB_REQUIRE(excl_start[0] == 0, "excl_start[0] must be 0");
        for (int q = 0; q < n_q; q++) VIORB_REQUIRE(excl_start[q + 1] >= excl_start[q], "excl_start must not decrease");
        n_excl = excl_start[n_q];
        VIORB_REQUIRE(n_excl == 0 || excl_slot, "excl_slot == NULL");
    }
    for (size_t i = 0; i < (size_t)S * PLACE_COVIS; i++) VIORB_REQUIRE(covis10[i] >= -1 && covis10[i] < S, "covis10 entries must be -1 or a slot");
    VIORB_TRY(require_device());
    const size_t qs = (size_t)n_q * (size_t)S, wb = viorb_kfdb_query_workspace_bytes(db, n_q);
    DeviceBufs B;
    int32_t *dqw = B.up(q_word, (size_t)n_q * q_cap), *dqc = B.up(q_count, n_q), *des = B.up(loop ? excl_start : nullptr, loop ? (size_t)n_q + 1 : 0, (size_t)n_q + 1);
    int32_t *dex = B.up(loop ? excl_slot : nullptr, (size_t)n_excl), *dcv = B.up(covis10, (size_t)S * PLACE_COVIS);
    double* dqv = B.up(q_val, (size_t)n_q * q_cap);
    float *dms = B.up(loop ? min_score : nullptr, loop ? (size_t)n_q : 0, (size_t)n_q), *dso = B.zeros<float>(qs);
    int32_t *dcand = B.zeros<int32_t>((size_t)n_q * cand_cap), *dnc = B.zeros<int32_t>(n_q), *dst = B.zeros<int32_t>(4 * (size_t)n_q), *dco = B.zeros<int32_t>(qs);
    unsigned char* dws = B.zeros<unsigned char>(wb);
    if (!B.ok) { set_error("device allocation / upload failed"); return VIORB_ERR_HIP; }
    const int rc = viorb_kfdb_query_device(db, mode, n_q, dqw, dqv, dqc, q_cap, dms, des, dex, dcv, cand_cap, dcand, dnc, dst, dco, dso, dws, wb, nullptr);
    if (rc != VIORB_OK) return rc;
    VIORB_HIP_TRY(hipDeviceSynchronize());
    VIORB_HIP_TRY(hipMemcpy(cand, dcand, sizeof(int32_t) * (size_t)n_q * cand_cap, hipMemcpyDeviceToHost));
    VIORB_HIP_TRY(hipMemcpy(n_cand, dnc, sizeof(int32_t) * (size_t)n_q, hipMemcpyDeviceToHost));
    VIORB_HIP_TRY(hipMemcpy(stats, dst, sizeof(int32_t) * 4 * (size_t)n_q, hipMemcpyDeviceToHost));
    if (common_out && qs) VIORB_HIP_TRY(hipMemcpy(common_out, dco, sizeof(int32_t) * qs, hipMemcpyDeviceToHost));
    if (score_out && qs) VIORB_HIP_TRY(hipMemcpy(score_out, dso, sizeof(float) * qs, hipMemcpyDeviceToHost));
    for (int q = 0; q < n_q; q++)
        if (n_cand[q] > cand_cap) {
            set_error("query %d has %d candidates, cand_cap = %d; n_cand holds the numbers", q, n_cand[q], cand_cap);
            return VIORB_ERR_CAPACITY;
        }
    return VIORB_OK;
}

// ---- host-only test hooks: place_core.h compiled for the host --------------------------------------------------------------------------
double viorb_debug_place_score(const int32_t* a_word, const double* a_val, int na, const int32_t* b_word, const double* b_val, int nb) {
    return place_score(a_word, a_val, na, b_word, b_val, nb);
}

int viorb_debug_place_select(int mode, int n_slots, const int32_t* common, const int32_t* min_word, const float* score, float min_score,
                             const int32_t* covis10, int cand_cap, int32_t* cand, int32_t* n_cand, int32_t* stats4) {
    VIORB_REQUIRE((mode == VIORB_KFDB_LOOP || mode == VIORB_KFDB_RELOC) && n_slots >= 0 && cand_cap >= 1 && n_cand && stats4, "mode, n_slots >= 0, cand_cap >= 1");
    VIORB_REQUIRE(n_slots == 0 || (common && min_word && score && covis10 && cand), "null array");
    int mx = 0, sharing = 0;
    for (int s = 0; s < n_slots; s++) { mx = std::max(mx, common[s]); sharing += common[s] >= 1; }
    const int minc = place_min_common(mx);
    std::vector<unsigned long long> keys;
    for (int s = 0; s < n_slots; s++)
        if (common[s] > minc) keys.push_back(place_order_key(min_word[s], s));
    std::sort(keys.begin(), keys.end());
    const bool loop = mode == VIORB_KFDB_LOOP;
    const float ms = loop ? min_score : 0.0f;
    float best_acc = ms;
    std::vector<float> acc(keys.size(), 0.0f);
    std::vector<int> best(keys.size(), -1);
    int kept = 0;
    for (size_t i = 0; i < keys.size(); i++) {
        const int s = (int)(uint32_t)keys[i];
        if (loop && !(score[s] >= ms)) continue;
        place_group(s, common, score, minc, covis10, n_slots, &acc[i], &best[i]);
        if (acc[i] > best_acc) best_acc = acc[i];
        kept++;
    }
    const float retain = 0.75f * best_acc;
    std::vector<uint8_t> added((size_t)std::max(n_slots, 1), 0);
    int nout = 0;
    for (size_t i = 0; i < keys.size(); i++)
        if (best[i] >= 0 && acc[i] > retain && !added[best[i]]) {
            added[best[i]] = 1;
            if (nout < cand_cap) cand[nout] = best[i];
            nout++;
        }
    *n_cand = nout;
    stats4[0] = sharing; stats4[1] = mx; stats4[2] = (int)keys.size(); stats4[3] = kept;
    if (nout > cand_cap) { set_error("%d candidates, cand_cap = %d", nout, cand_cap); return VIORB_ERR_CAPACITY; }
    return VIORB_OK;
}

} // extern "C"
