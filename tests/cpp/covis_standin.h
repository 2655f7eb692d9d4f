// tests/cpp/covis_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for the KeyFrame / MapPoint members that
// viorb_shim::update_connections and update_connections_loop (viorb_amd/shim/KeyFrame_shim.h) touch. The covisibility members are
// protected, as in the reference, and reached through the friend the shim asks for. Test scaffolding only.
#pragma once
#include <map>
#include <mutex>
#include <set>
#include <vector>
#include "cv_standin.h"               // viorb_tracking_shim.h, which KeyFrame_shim.h builds on, names cv types

namespace viorb_shim { struct CovisAccess; }

namespace standin {
struct CvKeyFrame;
struct CvMapPoint {
    int id = -1; bool mbBad = false;
    std::map<CvKeyFrame*, size_t> mObservations;
    bool isBad() const { return mbBad; }
    std::map<CvKeyFrame*, size_t> GetObservations() const { return mObservations; }
};
struct CvKeyFrame {
    friend struct viorb_shim::CovisAccess;
    int id = -1; long unsigned int mnId = 0;
    std::vector<CvMapPoint*> mvpMapPoints;
    std::vector<CvMapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    void AddChild(CvKeyFrame* pKF) { std::unique_lock<std::mutex> lock(mMutexConnections); mspChildrens.insert(pKF); }
    // what the test program sets up and reads back
    void set_graph(const std::map<CvKeyFrame*, int>& w, const std::vector<CvKeyFrame*>& o, const std::vector<int>& ow, bool first, CvKeyFrame* parent) {
        mConnectedKeyFrameWeights = w; mvpOrderedConnectedKeyFrames = o; mvOrderedWeights = ow; mbFirstConnection = first; mpParent = parent;
    }
    const std::map<CvKeyFrame*, int>& weights() const { return mConnectedKeyFrameWeights; }
    const std::vector<CvKeyFrame*>& ordered() const { return mvpOrderedConnectedKeyFrames; }
    const std::vector<int>& ordered_weights() const { return mvOrderedWeights; }
    bool first_connection() const { return mbFirstConnection; }
    CvKeyFrame* parent() const { return mpParent; }
    const std::set<CvKeyFrame*>& children() const { return mspChildrens; }
protected:
    std::map<CvKeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<CvKeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true;
    CvKeyFrame* mpParent = nullptr;
    std::set<CvKeyFrame*> mspChildrens;
    std::mutex mMutexConnections;
};
}
