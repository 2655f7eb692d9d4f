"""A literal Python restatement of LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:1694-1821) with KeyFrame::SetBadFlag
(src/KeyFrame.cc:744-882), MapPoint::EraseObservation and MapPoint::SetBadFlag (src/MapPoint.cc:118-175) as far as they change what a
later candidate sees, and of LocalMapping::MapPointCulling (:1198-1233). Objects, dictionaries and in-place mutation, one statement of
the reference after the other; it shares no structure with the device form. The checker of tests/test_kf_culling_ref.py and
tests/test_gpu_culling.py; product code never imports it.

A scene is the dict of viorb_amd/culling.py. What the snapshot does not carry: the keypoint index of an observation, so
KeyFrame::EraseMapPointMatch (a bad point leaving the tables of its observers) is not replayed; the tables keep the pointer to the bad
point, which the count skips through isBad() exactly as it skips a null entry."""
import numpy as np

FIRST_KF, TIME_GAP, BEFORE_CURRENT, RECENT, KEPT, CULLED, DEFERRED = range(7)
REASON_NAMES = ("FIRST_KF", "TIME_GAP", "BEFORE_CURRENT", "RECENT", "KEPT", "CULLED", "DEFERRED")
MPC_KEEP, MPC_DROP_BAD, MPC_CULL_FOUND_RATIO, MPC_CULL_FEW_OBS, MPC_RETIRE = range(5)
MPC_NAMES = ("KEEP", "DROP_BAD", "CULL_FOUND_RATIO", "CULL_FEW_OBS", "RETIRE")


class MapPoint:
    def __init__(self, nobs, bad):
        self.nObs, self.mbBad, self.mObservations = int(nobs), bool(bad), {}        # KeyFrame -> (octave of its keypoint, mvuRight >= 0, position)

    def EraseObservation(self, pKF):                                                 # MapPoint.cc:118-144
        bBad = False
        if pKF in self.mObservations:
            if self.mObservations[pKF][1]:
                self.nObs -= 2
            else:
                self.nObs -= 1
            del self.mObservations[pKF]
            if self.nObs <= 2:
                bBad = True
        if bBad:
            self.SetBadFlag()

    def SetBadFlag(self):                                                            # :158-175
        self.mbBad = True
        self.mObservations.clear()


class KeyFrame:
    def __init__(self, slot, flags, t):
        self.slot, self.first, self.mbNotErase, self.mTimeStamp = slot, bool(flags & 1), bool(flags & 2), float(t)
        self.mpPrevKeyFrame = self.mpNextKeyFrame = None
        self.mbBad = self.mbToBeErased = self.repreint = False
        self.mvpMapPoints, self.octave, self.mvDepth = [], [], []

    def SetBadFlag(self, culled):                                                    # KeyFrame.cc:744-882; True when it went through
        if self.first:
            return False
        if self.mbNotErase:
            self.mbToBeErased = True
            return False
        for pMP in self.mvpMapPoints:
            if pMP is not None:
                pMP.EraseObservation(self)
        self.mbBad = True
        pPrevKF, pNextKF = self.mpPrevKeyFrame, self.mpNextKeyFrame
        if pPrevKF is not None:
            pPrevKF.mpNextKeyFrame = pNextKF
        if pNextKF is not None:
            pNextKF.mpPrevKeyFrame = pPrevKF
        self.mpPrevKeyFrame = self.mpNextKeyFrame = None
        if pPrevKF is not None and pNextKF is not None:
            pNextKF.repreint = True                                                  # AppendIMUDataToFront(this); ComputePreInt()
        culled.append(self)
        return True


def build(scene):
    """The objects of a scene: (key frames, candidates in order, points)."""
    kfs = [KeyFrame(k, int(scene["kf_flags"][k]), scene["kf_time"][k]) for k in range(len(scene["kf_flags"]))]
    for k, kf in enumerate(kfs):
        p, n = int(scene["kf_prev"][k]), int(scene["kf_next"][k])
        kf.mpPrevKeyFrame, kf.mpNextKeyFrame = (kfs[p] if p >= 0 else None), (kfs[n] if n >= 0 else None)
    pts = []
    for p in range(len(scene["pt_nobs"])):
        mp = MapPoint(scene["pt_nobs"][p], scene["pt_bad"][p])
        for o in range(int(scene["obs_start"][p]), int(scene["obs_start"][p + 1])):
            w = int(scene["obs"][o])
            mp.mObservations[kfs[w & 0xffff]] = ((w >> 16) & 0xff, bool(w & (1 << 24)), o)
        pts.append(mp)
    cands = []
    for j, c in enumerate(scene["cand_kf"]):
        kf = kfs[int(c)]
        for i in range(int(scene["kp_start"][j]), int(scene["kp_start"][j + 1])):
            q = int(scene["kp_point"][i])
            kf.mvpMapPoints.append(pts[q] if q >= 0 else None)
            kf.octave.append(int(scene["kp_octave"][i]))
            kf.mvDepth.append(np.float32(scene["kp_depth"][i]))
        cands.append(kf)
    return kfs, cands, pts


def count(pKF, mbMonocular, mThDepth):
    """:1766-1817: (nRedundantObservations, nMPs)."""
    thObs = 3
    nRedundantObservations = nMPs = 0
    for i, pMP in enumerate(pKF.mvpMapPoints):
        if pMP is not None:
            if not pMP.mbBad:
                if not mbMonocular:
                    if pKF.mvDepth[i] > np.float32(mThDepth) or pKF.mvDepth[i] < 0:
                        continue
                nMPs += 1
                if pMP.nObs > thObs:
                    scaleLevel = pKF.octave[i]
                    nObs = 0
                    for pKFi, (scaleLeveli, _, _) in pMP.mObservations.items():
                        if pKFi is pKF:
                            continue
                        if scaleLeveli <= scaleLevel + 1:
                            nObs += 1
                            if nObs >= thObs:
                                break
                    if nObs >= thObs:
                        nRedundantObservations += 1
    return nRedundantObservations, nMPs


def skip_reason(pKF, cur, vins_inited):
    """:1697-1750: the reason of a skipped candidate or None."""
    if pKF.first:
        return FIRST_KF
    pPrevKF, pNextKF = pKF.mpPrevKeyFrame, pKF.mpNextKeyFrame
    if pPrevKF is not None and pNextKF is not None and not vins_inited:
        if abs(pNextKF.mTimeStamp - pPrevKF.mTimeStamp) > 0.5:
            return TIME_GAP
    if pKF.mpNextKeyFrame is cur:
        return BEFORE_CURRENT
    if pKF.mTimeStamp >= cur.mTimeStamp - 0.2:
        return RECENT
    return None


def key_frame_culling(scene, monocular, frozen=False):
    """The loop over one scene. frozen=True: every candidate is judged on the snapshot state (no SetBadFlag takes effect): what a form
    without the ordered phase would answer. Returns the fields of viorb_cull_result for the stream."""
    kfs, cands, pts = build(scene)
    cur = kfs[int(scene["cur"])]
    nc = len(cands)
    reason, red, mps, culled = np.zeros(nc, np.int32), np.zeros(nc, np.int32), np.zeros(nc, np.int32), []
    for j, pKF in enumerate(cands):
        r = skip_reason(pKF, cur, scene["vins_inited"])
        if r is not None:
            reason[j] = r
            continue
        nRedundantObservations, nMPs = count(pKF, monocular, scene["th_depth"])
        red[j], mps[j] = nRedundantObservations, nMPs
        reason[j] = KEPT
        if nRedundantObservations > 0.9 * nMPs:
            if frozen:
                reason[j] = DEFERRED if pKF.mbNotErase else CULLED
            elif pKF.SetBadFlag(culled):
                reason[j] = CULLED
            else:
                reason[j] = DEFERRED
    alive = np.zeros(len(scene["obs"]), np.uint8)
    for mp in pts:
        for _, (_, _, o) in mp.mObservations.items():
            alive[o] = 1
    slot = lambda kf: -1 if kf is None else kf.slot
    return dict(cand_reason=reason, cand_redundant=red, cand_mps=mps, n_culled=len(culled),
                culled_order=np.array([cands.index(k) for k in culled], np.int32),
                kf_bad=np.array([k.mbBad for k in kfs], np.uint8), kf_to_be_erased=np.array([k.mbToBeErased for k in kfs], np.uint8),
                kf_prev_out=np.array([slot(k.mpPrevKeyFrame) for k in kfs], np.int32), kf_next_out=np.array([slot(k.mpNextKeyFrame) for k in kfs], np.int32),
                kf_repreint=np.array([k.repreint for k in kfs], np.uint8), pt_nobs_out=np.array([p.nObs for p in pts], np.int32),
                pt_bad_out=np.array([p.mbBad for p in pts], np.uint8), obs_alive=alive)


def map_point_culling(bad, found, visible, first_kf_id, nobs, cur_kf_id, monocular):
    """:1198-1233 over a list: the branch each point takes. GetFoundRatio() is float(mnFound) / mnVisible in float arithmetic."""
    cnThObs = 2 if monocular else 3
    code = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(len(bad)):
            ratio = np.float32(found[i]) / np.float32(visible[i])
            if bad[i]:
                code.append(MPC_DROP_BAD)
            elif ratio < np.float32(0.25):
                code.append(MPC_CULL_FOUND_RATIO)
            elif int(cur_kf_id) - int(first_kf_id[i]) >= 2 and nobs[i] <= cnThObs:
                code.append(MPC_CULL_FEW_OBS)
            elif int(cur_kf_id) - int(first_kf_id[i]) >= 3:
                code.append(MPC_RETIRE)
            else:
                code.append(MPC_KEEP)
    return np.array(code, np.int32)
