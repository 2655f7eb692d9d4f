// tests/cpp/place_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for what viorb_shim::KeyFrameDatabase touches
// (include/KeyFrame.h, include/Frame.h, DBoW2::BowVector). Test scaffolding only.
#pragma once
#include <map>
#include <set>
#include <vector>
#include "cv_standin.h"

namespace standin {
typedef std::map<unsigned int, double> BowVector;                                // Thirdparty/DBoW2/DBoW2/BowVector.h:54
struct KeyFrame {                                                                // include/KeyFrame.h
    unsigned long mnId = 0; bool bad = false; BowVector mBowVec;
    std::set<KeyFrame*> connected; std::vector<KeyFrame*> covisible;             // ordered by weight, best first
    bool isBad() const { return bad; }
    std::set<KeyFrame*> GetConnectedKeyFrames() const { return connected; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(int N) const {
        return (int)covisible.size() < N ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
    }
};
struct Frame { unsigned long mnId = 0; BowVector mBowVec; };                     // include/Frame.h
}
