// tests/cpp/culling_standin.h — stand-ins WITH THE REFERENCE'S MEMBER NAMES for the KeyFrame / MapPoint members that
// viorb_shim::key_frame_culling and viorb_shim::map_point_culling (viorb_amd/shim/LocalMapping_shim.h) touch. SetBadFlag and
// EraseObservation carry the reference's semantics as far as culling sees them (src/KeyFrame.cc:744-882, src/MapPoint.cc:118-175): the
// map they leave is what the test compares with the state the library reports. Test scaffolding only.
#pragma once
#include <map>
#include <vector>
#include "cv_standin.h"

namespace standin {
struct CullKeyFrame;
struct CullMapPoint {
    int nObs = 0, mnFound = 1, mnVisible = 1, id = -1; long int mnFirstKFid = 0; bool mbBad = false;
    std::map<CullKeyFrame*, size_t> mObservations;
    int Observations() const { return nObs; }
    bool isBad() const { return mbBad; }
    int GetFound() const { return mnFound; }
    int GetVisible() const { return mnVisible; }                    // the accessor the shim asks for
    std::map<CullKeyFrame*, size_t> GetObservations() const { return mObservations; }
    inline void EraseObservation(CullKeyFrame* pKF);
    inline void SetBadFlag();
};
struct CullKeyFrame {
    unsigned long mnId = 1; double mTimeStamp = 0; float mThDepth = 40.f; int id = -1, preint_calls = 0;
    bool mbNotErase = false, mbToBeErased = false, mbBad = false;
    CullKeyFrame *mpPrevKeyFrame = nullptr, *mpNextKeyFrame = nullptr;
    std::vector<cv::KeyPoint> mvKeysUn; std::vector<float> mvuRight, mvDepth; std::vector<CullMapPoint*> mvpMapPoints;
    std::vector<CullKeyFrame*> covisible, appended;                 // appended: AppendIMUDataToFront(pKF) calls in order
    std::vector<CullKeyFrame*> GetVectorCovisibleKeyFrames() const { return covisible; }
    std::vector<CullMapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    CullKeyFrame* GetPrevKeyFrame() const { return mpPrevKeyFrame; }
    CullKeyFrame* GetNextKeyFrame() const { return mpNextKeyFrame; }
    bool GetNotErase() const { return mbNotErase; }                 // the accessor the shim asks for
    void EraseMapPointMatch(size_t idx) { mvpMapPoints[idx] = nullptr; }
    void SetBadFlag() {
        if (mbBad || mnId == 0) return;
        if (mbNotErase) { mbToBeErased = true; return; }
        for (size_t i = 0; i < mvpMapPoints.size(); i++) if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
        mbBad = true;
        CullKeyFrame *pPrevKF = mpPrevKeyFrame, *pNextKF = mpNextKeyFrame;
        if (pPrevKF) pPrevKF->mpNextKeyFrame = pNextKF;
        if (pNextKF) pNextKF->mpPrevKeyFrame = pPrevKF;
        mpPrevKeyFrame = mpNextKeyFrame = nullptr;
        if (pPrevKF && pNextKF) { pNextKF->appended.push_back(this); pNextKF->preint_calls++; }
    }
};
inline void CullMapPoint::EraseObservation(CullKeyFrame* pKF) {
    bool bBad = false;
    if (mObservations.count(pKF)) {
        const size_t idx = mObservations[pKF];
        if (pKF->mvuRight[idx] >= 0) nObs -= 2; else nObs--;
        mObservations.erase(pKF);
        if (nObs <= 2) bBad = true;
    }
    if (bBad) SetBadFlag();
}
inline void CullMapPoint::SetBadFlag() {
    const std::map<CullKeyFrame*, size_t> obs = mObservations;
    mbBad = true; mObservations.clear();
    for (std::map<CullKeyFrame*, size_t>::const_iterator mit = obs.begin(); mit != obs.end(); ++mit) mit->first->EraseMapPointMatch(mit->second);
}
}
