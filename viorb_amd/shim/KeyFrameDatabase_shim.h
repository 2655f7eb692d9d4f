// viorb_amd/shim/KeyFrameDatabase_shim.h — the reference's KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:40-309)
// as a class template over its own KeyFrame / Frame, on top of the viorb_kfdb handle of include/viorb.h. It keeps the map
// KeyFrame* <-> slot; the inverted file, the scoring and the covisibility accumulation run on the device. A GPU failure is thrown with
// viorb_last_error() (viorb_shim::check), never reported as "no candidates", which LoopClosing / Tracking would read as a plain miss.
//
//   add / erase / clear                  KeyFrameDatabase::add, erase, clear                               src/KeyFrameDatabase.cc:40-73
//   DetectLoopCandidates                 KeyFrameDatabase::DetectLoopCandidates(pKF, minScore)             :76-197
//   DetectRelocalizationCandidates       KeyFrameDatabase::DetectRelocalizationCandidates(F)               :199-309
//   loop_min_score                       the lowest score to a connected key frame, LoopClosing::DetectLoop  src/LoopClosing.cc:148-162
//
// Members read: KeyFrame::mBowVec, mnId (in messages only), isBad(), GetConnectedKeyFrames(), GetBestCovisibilityKeyFrames(10);
// Frame::mBowVec. The constructor takes the vocabulary's size (mpVoc->size()). A query asks every stored key frame for its ten best
// covisibles (the device needs the table before it knows which key frames are kept); key frames that are not in the database map to -1.
// One deviation from the reference, DESIGN.md §2: in DetectRelocalizationCandidates a covisible that was not scored adds nothing.
#ifndef VIORB_KEYFRAMEDATABASE_SHIM_H
#define VIORB_KEYFRAMEDATABASE_SHIM_H

#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <vector>
#include "viorb_tracking_shim.h"

namespace viorb_shim {

// DBoW2::BowVector (a std::map<WordId, WordValue>) as ascending words and values
template <class BowVectorT> inline void flatten_bow(const BowVectorT& bow, std::vector<int32_t>& words, std::vector<double>& vals) {
    words.clear(); vals.clear();
    for (typename BowVectorT::const_iterator it = bow.begin(); it != bow.end(); ++it) { words.push_back((int32_t)it->first); vals.push_back((double)it->second); }
}

template <class KeyFrameT, class FrameT> class KeyFrameDatabase {
public:
    explicit KeyFrameDatabase(int n_words, int kf_capacity_hint = 1024, int entry_capacity_hint = 1 << 20) : db_(nullptr) {
        check(viorb_kfdb_create(n_words, kf_capacity_hint, entry_capacity_hint, &db_), "viorb_kfdb_create");
    }
    ~KeyFrameDatabase() { viorb_kfdb_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(KeyFrameT* pKF) {
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int32_t> w; std::vector<double> v;
        flatten_bow(pKF->mBowVec, w, v);
        int slot = -1;
        check(viorb_kfdb_add(db_, w.data(), v.data(), (int)w.size(), &slot), "viorb_kfdb_add");
        slot_of_[pKF] = slot;
        if ((int)kf_of_.size() <= slot) kf_of_.resize(slot + 1, nullptr);
        kf_of_[slot] = pKF;
    }
    void erase(KeyFrameT* pKF) {
        std::unique_lock<std::mutex> lock(mMutex);
        typename std::map<KeyFrameT*, int>::iterator it = slot_of_.find(pKF);
        if (it == slot_of_.end()) return;                          // the reference's erase of an absent key frame changes nothing either
        check(viorb_kfdb_erase(db_, it->second), "viorb_kfdb_erase");
        kf_of_[it->second] = nullptr;
        slot_of_.erase(it);
    }
    void clear() {
        std::unique_lock<std::mutex> lock(mMutex);
        check(viorb_kfdb_clear(db_), "viorb_kfdb_clear");
        slot_of_.clear(); kf_of_.clear();
    }

    std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore) {
        const std::set<KeyFrameT*> spConnected = pKF->GetConnectedKeyFrames();
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int32_t> excl;
        for (typename std::set<KeyFrameT*>::const_iterator it = spConnected.begin(); it != spConnected.end(); ++it) {
            const int s = slot(*it);
            if (s >= 0) excl.push_back(s);
        }
        return query(VIORB_KFDB_LOOP, pKF->mBowVec, minScore, excl);
    }
    std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F) {
        std::unique_lock<std::mutex> lock(mMutex);
        return query(VIORB_KFDB_RELOC, F->mBowVec, 0.f, std::vector<int32_t>());
    }

    // float minScore = 1; for every connected key frame that is not bad: score = mpORBVocabulary->score(CurrentBowVec, BowVec), the minimum
    float loop_min_score(KeyFrameT* pKF, const std::vector<KeyFrameT*>& vpConnected) const {
        std::vector<int32_t> aw, w, bw, bc, pa, pb; std::vector<double> av, v, bv;
        flatten_bow(pKF->mBowVec, aw, av);
        std::vector<KeyFrameT*> good;
        size_t cap = 1;
        for (size_t i = 0; i < vpConnected.size(); i++)
            if (!vpConnected[i]->isBad()) { good.push_back(vpConnected[i]); cap = std::max(cap, (size_t)vpConnected[i]->mBowVec.size()); }
        if (good.empty()) return 1.f;
        bw.assign(good.size() * cap, 0); bv.assign(good.size() * cap, 0.0);
        for (size_t i = 0; i < good.size(); i++) {
            flatten_bow(good[i]->mBowVec, w, v);
            std::copy(w.begin(), w.end(), bw.begin() + i * cap); std::copy(v.begin(), v.end(), bv.begin() + i * cap);
            bc.push_back((int32_t)w.size()); pa.push_back(0); pb.push_back((int32_t)i);
        }
        const int32_t na = (int32_t)aw.size();
        if (aw.empty()) { aw.push_back(0); av.push_back(0.0); }
        std::vector<double> s(good.size(), 0.0);
        check(viorb_bow_score(aw.data(), av.data(), &na, (int)aw.size(), 1, bw.data(), bv.data(), bc.data(), (int)cap, (int)good.size(), pa.data(), pb.data(),
                              (int)good.size(), s.data()), "viorb_bow_score");
        float minScore = 1.f;
        for (size_t i = 0; i < s.size(); i++) { const float score = (float)s[i]; if (score < minScore) minScore = score; }
        return minScore;
    }

    int slot(KeyFrameT* pKF) const {
        typename std::map<KeyFrameT*, int>::const_iterator it = slot_of_.find(pKF);
        return it == slot_of_.end() ? -1 : it->second;
    }

private:
    template <class BowVectorT> std::vector<KeyFrameT*> query(int mode, const BowVectorT& bow, float minScore, const std::vector<int32_t>& excl) {
        std::vector<int32_t> qw; std::vector<double> qv;
        flatten_bow(bow, qw, qv);
        const int32_t nq = (int32_t)qw.size();
        if (qw.empty()) { qw.push_back(0); qv.push_back(0.0); }
        const int S = (int)kf_of_.size();
        std::vector<int32_t> covis((size_t)std::max(S, 1) * 10, -1), cand((size_t)std::max(S, 1), -1);
        for (int s = 0; s < S; s++) {
            if (!kf_of_[s]) continue;
            const std::vector<KeyFrameT*> vpNeighs = kf_of_[s]->GetBestCovisibilityKeyFrames(10);
            for (size_t k = 0; k < vpNeighs.size() && k < 10; k++) covis[(size_t)s * 10 + k] = slot(vpNeighs[k]);
        }
        const int32_t excl_start[2] = {0, (int32_t)excl.size()};
        std::vector<int32_t> ex(excl);
        if (ex.empty()) ex.push_back(-1);
        int32_t n_cand = 0, stats[4] = {0, 0, 0, 0};
        const bool loop = mode == VIORB_KFDB_LOOP;
        check(viorb_kfdb_query(db_, mode, 1, qw.data(), qv.data(), &nq, (int)qw.size(), loop ? &minScore : nullptr, loop ? excl_start : nullptr,
                               loop ? ex.data() : nullptr, covis.data(), (int)cand.size(), cand.data(), &n_cand, stats, nullptr, nullptr), "viorb_kfdb_query");
        std::vector<KeyFrameT*> out;
        out.reserve(n_cand);
        for (int i = 0; i < n_cand; i++) out.push_back(kf_of_[cand[i]]);
        return out;
    }

    viorb_kfdb* db_;
    std::map<KeyFrameT*, int> slot_of_;
    std::vector<KeyFrameT*> kf_of_;
    std::mutex mMutex;
};

} // namespace viorb_shim
#endif
