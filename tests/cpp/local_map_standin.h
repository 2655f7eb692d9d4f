// tests/cpp/local_map_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for the Frame / KeyFrame / MapPoint members that
// viorb_shim::update_local_map (viorb_amd/shim/viorb_tracking_shim.h) touches. Test scaffolding only.
#pragma once
#include <map>
#include <set>
#include <vector>
#include "cv_standin.h"

namespace standin {
struct LmKeyFrame;
struct LmMapPoint {
    int id = -1; bool mbBad = false;
    std::map<LmKeyFrame*, size_t> mObservations;
    bool isBad() const { return mbBad; }
    std::map<LmKeyFrame*, size_t> GetObservations() const { return mObservations; }
};
struct LmKeyFrame {
    int id = -1; bool mbBad = false;
    LmKeyFrame *mpParent = nullptr, *mpPrevKeyFrame = nullptr, *mpNextKeyFrame = nullptr;
    std::vector<LmKeyFrame*> mvpOrderedConnectedKeyFrames; std::set<LmKeyFrame*> mspChildrens; std::vector<LmMapPoint*> mvpMapPoints;
    bool isBad() const { return mbBad; }
    std::vector<LmKeyFrame*> GetBestCovisibilityKeyFrames(const int& N) const {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<LmKeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::set<LmKeyFrame*> GetChilds() const { return mspChildrens; }
    LmKeyFrame* GetParent() const { return mpParent; }
    LmKeyFrame* GetPrevKeyFrame() const { return mpPrevKeyFrame; }
    LmKeyFrame* GetNextKeyFrame() const { return mpNextKeyFrame; }
    std::vector<LmMapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
};
struct LmFrame {
    int N = 0; long unsigned int mnId = 0;
    std::vector<LmMapPoint*> mvpMapPoints; LmKeyFrame* mpReferenceKF = nullptr;
};
}
