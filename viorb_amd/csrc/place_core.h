// viorb_amd/csrc/place_core.h — the scalar pieces of place recognition, shared by the HIP kernels of place.hip and by the host-only hooks
// viorb_debug_place_score / viorb_debug_place_select (the CPU test-suite compares them with tests/place_ref.py without a GPU).
//
// What is restated (reference file:line):
//   L1Scoring::score                                    Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
//   KeyFrameDatabase::DetectLoopCandidates              src/KeyFrameDatabase.cc:76-197
//   KeyFrameDatabase::DetectRelocalizationCandidates    src/KeyFrameDatabase.cc:199-309
// Everything here is integer, float or one ordered chain of double additions: the parity bar is bit-exactness.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLACE_HD __host__ __device__ __forceinline__
#else
#define PLACE_HD inline
#endif

namespace viorb {

enum { PLACE_LOOP = 0, PLACE_RELOC = 1, PLACE_COVIS = 10 };

// index of `key` in the ascending array a[0..n), or -1
PLACE_HD int place_find(const int32_t* a, int n, int32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < n && a[lo] == key) ? lo : -1;
}

// one common word of L1Scoring::score: vi from the first vector, wi from the second (the two subtractions do not commute bit-wise)
PLACE_HD double place_score_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
PLACE_HD double place_score_finish(double s) { return -s / 2.0; }

// L1Scoring::score over two ascending (word, value) lists: the common words in ascending order, one chain of additions from 0.0
PLACE_HD double place_score(const int32_t* aw, const double* av, int na, const int32_t* bw, const double* bv, int nb) {
    double s = 0.0;
    int i = 0, j = 0;
    while (i < na && j < nb) {
        if (aw[i] == bw[j]) { s += place_score_term(av[i], bv[j]); i++; j++; }
        else if (aw[i] < bw[j]) i++;
        else j++;
    }
    return place_score_finish(s);
}

// int minCommonWords = maxCommonWords*0.8f (src/KeyFrameDatabase.cc:120, :235)
PLACE_HD int place_min_common(int max_common) { return (int)((float)max_common * 0.8f); }

// The covisibility group of one kept slot (src/KeyFrameDatabase.cc:148-173, :262-287): accScore and the best-scoring key frame over the
// slot and those of its ten best covisibles that were scored in this query (common > min_common; DESIGN.md §2 has the relocalisation
// deviation). common / score: the rows of this query, n_slots long.
PLACE_HD void place_group(int slot, const int32_t* common, const float* score, int min_common, const int32_t* covis10, int n_slots,
                          float* acc_out, int* best_out) {
    float best_score = score[slot], acc = score[slot];
    int best = slot;
    for (int k = 0; k < PLACE_COVIS; k++) {
        const int nb = covis10[(size_t)slot * PLACE_COVIS + k];
        if (nb < 0 || nb >= n_slots) continue;
        if (common[nb] > min_common) {
            acc += score[nb];
            if (score[nb] > best_score) { best = nb; best_score = score[nb]; }
        }
    }
    *acc_out = acc; *best_out = best;
}

// the order of first encounter while the query's words are walked ascending and each word's list in add order: (smallest common word, slot)
PLACE_HD unsigned long long place_order_key(int32_t min_word, int32_t slot) {
    return ((unsigned long long)(uint32_t)min_word << 32) | (uint32_t)slot;
}

} // namespace viorb
