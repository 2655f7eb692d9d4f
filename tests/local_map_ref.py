"""A literal Python restatement of Tracking::UpdateLocalKeyFrames (reference src/Tracking.cc:1996-2125) and Tracking::UpdateLocalPoints
(:1970-1993): objects, dictionaries iterated by key position, mnTrackReferenceForFrame members and in-place mutation, one statement of
the reference after the other; it shares no structure with the device form. The checker of tests/test_local_map_ref.py and
tests/test_gpu_local_map.py; product code never imports it.

A scene is the dict of viorb_amd/local_map.py. std::map<KeyFrame*, int> iterates in pointer order: a key frame's `key` is its position
in kf_by_key, and the dictionaries are walked in ascending key. The index semantics of the neighbour loop are followed (itEndKF is taken
before the loop; push_back does not move it)."""
import numpy as np

OK, NO_VOTES, OVERFLOW, INVALID = 0, 1, 2, -1
FRAME_ID = 1234                                                       # mCurrentFrame.mnId; every mark starts at another value


class MapPoint:
    def __init__(self, idx, bad):
        self.idx, self.mbBad, self.mObservations, self.mnTrackReferenceForFrame = idx, bool(bad), {}, 0

    def isBad(self):
        return self.mbBad

    def GetObservations(self):
        return sorted(self.mObservations.items(), key=lambda kv: kv[0].key)


class KeyFrame:
    def __init__(self, slot, bad):
        self.slot, self.mbBad, self.key, self.mnTrackReferenceForFrame = slot, bool(bad), -1, 0
        self.mpParent = self.mpPrevKeyFrame = self.mpNextKeyFrame = None
        self.neighbours, self.mspChildrens, self.mvpMapPoints = [], [], []

    def isBad(self):
        return self.mbBad


def build(s):
    """The objects of a scene: (key frames by slot, points by index, mCurrentFrame.mvpMapPoints)."""
    nk, npt = len(s["kf_bad"]), len(s["pt_bad"])
    kfs = [KeyFrame(k, s["kf_bad"][k]) for k in range(nk)]
    pts = [MapPoint(p, s["pt_bad"][p]) for p in range(npt)]
    link = lambda v: kfs[v] if v >= 0 else None
    covis = np.asarray(s["covis10"]).reshape(nk, 10)
    for j, k in enumerate(s["kf_by_key"]):
        kfs[k].key = j
    for k, K in enumerate(kfs):
        K.mpParent, K.mpPrevKeyFrame, K.mpNextKeyFrame = link(s["kf_parent"][k]), link(s["kf_prev"][k]), link(s["kf_next"][k])
        K.neighbours = [kfs[c] for c in covis[k] if c >= 0]
        K.mspChildrens = [kfs[c] for c in s["child_kf"][s["child_start"][k]:s["child_start"][k + 1]]]
        K.mvpMapPoints = [pts[p] if p >= 0 else None for p in s["kp_point"][s["kp_start"][k]:s["kp_start"][k + 1]]]
    for p, P in enumerate(pts):
        for o in s["obs"][s["obs_start"][p]:s["obs_start"][p + 1]]:
            P.mObservations[kfs[int(o) & 0xffff]] = 0
    return kfs, pts, [pts[p] if p >= 0 else None for p in s["frame_point"]]


def update_local_map(s, lcap=None, pcap=None):
    """Every output of viorb_local_map_result for one scene, as split() of viorb_amd/local_map.py returns it (lkf / lpt cut to what fits
    in lcap / pcap when given)."""
    kfs, pts, mvpMapPoints = build(s)
    mvpLocalKeyFrames = [kfs[k] for k in s["prev_lkf"]]
    mpReferenceKF = kfs[s["prev_ref"]] if s["prev_ref"] >= 0 else None
    status, n_voted = OK, 0

    # ---- UpdateLocalKeyFrames (:1996-2125)
    keyframeCounter = {}
    for i in range(len(mvpMapPoints)):
        if mvpMapPoints[i]:
            pMP = mvpMapPoints[i]
            if not pMP.isBad():
                for pKF, _ in pMP.GetObservations():
                    keyframeCounter[pKF] = keyframeCounter.get(pKF, 0) + 1
            else:
                mvpMapPoints[i] = None
    if not keyframeCounter:
        status = NO_VOTES                                             # return (:2019)
    else:
        max_, pKFmax = 0, None
        mvpLocalKeyFrames = []
        for pKF, n in sorted(keyframeCounter.items(), key=lambda kv: kv[0].key):
            if pKF.isBad():
                continue
            if n > max_:
                max_, pKFmax = n, pKF
            mvpLocalKeyFrames.append(pKF)
            pKF.mnTrackReferenceForFrame = FRAME_ID
        n_voted = len(mvpLocalKeyFrames)
        for it in range(n_voted):                                     # itEndKF: the end before the loop
            if len(mvpLocalKeyFrames) > 80:
                break
            pKF = mvpLocalKeyFrames[it]
            for pNeighKF in pKF.neighbours:
                if not pNeighKF.isBad():
                    if pNeighKF.mnTrackReferenceForFrame != FRAME_ID:
                        mvpLocalKeyFrames.append(pNeighKF)
                        pNeighKF.mnTrackReferenceForFrame = FRAME_ID
                        break
            for pChildKF in pKF.mspChildrens:
                if not pChildKF.isBad():
                    if pChildKF.mnTrackReferenceForFrame != FRAME_ID:
                        mvpLocalKeyFrames.append(pChildKF)
                        pChildKF.mnTrackReferenceForFrame = FRAME_ID
                        break
            for pLink in (pKF.mpParent, pKF.mpPrevKeyFrame, pKF.mpNextKeyFrame):
                if pLink:
                    if pLink.mnTrackReferenceForFrame != FRAME_ID:
                        mvpLocalKeyFrames.append(pLink)
                        pLink.mnTrackReferenceForFrame = FRAME_ID
        if pKFmax:
            mpReferenceKF = pKFmax

    # ---- UpdateLocalPoints (:1970-1993)
    mvpLocalMapPoints = []
    for pKF in mvpLocalKeyFrames:
        for pMP in pKF.mvpMapPoints:
            if not pMP:
                continue
            if pMP.mnTrackReferenceForFrame == FRAME_ID:
                continue
            if not pMP.isBad():
                mvpLocalMapPoints.append(pMP)
                pMP.mnTrackReferenceForFrame = FRAME_ID

    votes = np.zeros(len(kfs), np.int32)
    for pKF, n in keyframeCounter.items():
        votes[pKF.slot] = n
    lkf = np.array([K.slot for K in mvpLocalKeyFrames], np.int32)
    lpt = np.array([P.idx for P in mvpLocalMapPoints], np.int32)
    r = dict(status=status, n_lkf=len(lkf), n_voted=n_voted, ref_kf=mpReferenceKF.slot if mpReferenceKF else -1, n_lpt=len(lpt),
             frame_point_out=np.array([P.idx if P else -1 for P in mvpMapPoints], np.int32), kf_votes=votes)
    if (lcap is not None and len(lkf) > lcap) or (pcap is not None and len(lpt) > pcap):
        r["status"] = OVERFLOW
    r["lkf"] = lkf if lcap is None else lkf[:lcap]
    r["lpt"] = lpt if pcap is None else lpt[:pcap]
    return r


def differences(got, want, cap=None):
    """The names of the outputs of one stream (split() of viorb_amd/local_map.py) that differ from the checker's: exact equality of every
    field, the -1 padding of the three rows included."""
    bad = [f for f in ("status", "n_lkf", "n_voted", "ref_kf", "n_lpt") if got[f] != want[f]]
    bad += [f for f in ("lkf", "lpt", "kf_votes") if not np.array_equal(got[f], want[f])]
    n = len(want["frame_point_out"])
    if not (np.array_equal(got["frame_point_out"][:n], want["frame_point_out"]) and (got["frame_point_out"][n:] == -1).all()):
        bad.append("frame_point_out")
    if not ((got["lkf_tail"] == -1).all() and (got["lpt_tail"] == -1).all()):
        bad.append("padding")
    return bad
