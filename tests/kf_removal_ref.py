"""A literal Python restatement of KeyFrame::SetErase and KeyFrame::SetBadFlag (reference src/KeyFrame.cc:728-882), EraseConnection
(:890-904), UpdateBestCovisibles (:429-448), GetWeight (:492-500), ChangeParent / AddChild / EraseChild (:672-689) and
MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:118-175): objects, dictionaries iterated by key position, in-place mutation, one
statement of the reference after the other; it shares no structure with the device form. The checker of tests/test_kf_removal_ref.py,
tests/test_gpu_kf_removal.py and tests/test_gpu_kf_removal_shim.py; product code never imports it.

A scene is the dict of viorb_amd/kf_removal.py. std::map<KeyFrame*, ...> and std::set<KeyFrame*> iterate in pointer order: a key frame's
`key` is its position in kf_by_key. mspChildrens is built from the (parent, bad) rule of the header and then kept by the reference's own
statements. mObservations maps a key frame to the index of the point in its mvpMapPoints (None when the table does not hold it)."""
import numpy as np

OK, INVALID = 0, -1
KF_ID0, KF_BAD, KF_NOT_ERASE, KF_TO_BE_ERASED, KF_LOOP_EDGES = 1, 2, 4, 8, 16
SET_BAD_FLAG, SET_ERASE = 0, 1
REMOVED, ALREADY_BAD, FIRST_KF, DEFERRED, RELEASED = 0, 1, 2, 3, 4
MAP_CHANGED, ORD_REBUILT, PARENT_CHANGED = 1, 2, 4
EVENTS = ("adopted-by-adopted-child", "fallback", "tie-by-order-permuted", "rebuild-pulls-sub-threshold", "point-bad", "point-survives", "ref-moves",
          "stereo-decrement", "deferred", "already-bad", "first-kf", "released", "set-erase-removes", "parent-assigned-earlier", "adjacent-removals")
F32 = np.float32


class Ctx:
    """What one call counts and reports."""

    def __init__(self, events):
        self.events = events
        self.op = None                                                # the counters of the running operation
        self.removed = []

    def count(self, what):
        if self.events is not None:
            self.events[what] = self.events.get(what, 0) + 1


class MapPoint:
    def __init__(self, index, bad, nobs):
        self.index, self.mbBad, self.nObs, self.mObservations, self.mpRefKF, self.stereo = index, bool(bad), int(nobs), {}, None, {}

    def EraseObservation(self, pKF, ctx):                             # MapPoint.cc:118-144
        bBad, found = False, pKF in self.mObservations
        if found:
            if self.stereo[pKF]:                                      # pKF->mvuRight[idx] >= 0
                self.nObs -= 2
                ctx.count("stereo-decrement")
            else:
                self.nObs -= 1
            del self.mObservations[pKF]
            if self.mpRefKF is pKF:
                obs = sorted(self.mObservations, key=lambda K: K.key)
                self.mpRefKF = obs[0] if obs else None                # begin() == end(): the point goes bad below
                ctx.count("ref-moves")
            if self.nObs <= 2:
                bBad = True
        if bBad:
            self.SetBadFlag(ctx)
        elif found:
            ctx.count("point-survives")

    def SetBadFlag(self, ctx):                                        # MapPoint.cc:158-175
        self.mbBad = True
        obs = dict(self.mObservations)
        self.mObservations.clear()
        for pKF, idx in sorted(obs.items(), key=lambda kv: kv[0].key):
            if idx is not None:
                pKF.mvpMapPoints[idx] = None                          # EraseMapPointMatch(idx)
        ctx.op["points_bad"] += 1
        ctx.count("point-bad")


class KeyFrame:
    def __init__(self, slot, flags, key, pose12):
        self.slot, self.key = slot, key
        self.mnId = 0 if flags & KF_ID0 else slot + 1
        self.mbBad, self.mbNotErase, self.mbToBeErased = bool(flags & KF_BAD), bool(flags & KF_NOT_ERASE), bool(flags & KF_TO_BE_ERASED)
        self.mspLoopEdges = {"edge"} if flags & KF_LOOP_EDGES else set()
        self.mpParent, self.mspChildrens, self.mvpMapPoints = None, set(), []
        self.mConnectedKeyFrameWeights, self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = {}, [], []
        self.mpPrevKeyFrame, self.mpNextKeyFrame = None, None
        self.Tcw = np.asarray(pose12, F32)
        self.mTcp, self.touched, self.repreint, self.assigned_in_call = None, 0, 0, False

    def isBad(self):
        return self.mbBad

    def _map_items(self):                                             # the iteration order of std::map<KeyFrame*, int>
        return sorted(self.mConnectedKeyFrameWeights.items(), key=lambda kv: kv[0].key)

    def GetPoseInverse(self):                                         # Twc as SetPose builds it: Rwc = Rcw^T, Ow = -Rwc * tcw, float
        Rcw, tcw = self.Tcw[:9].reshape(3, 3), self.Tcw[9:]
        Twc = np.zeros((4, 4), F32)
        Twc[:3, :3] = Rcw.T
        for r in range(3):
            Twc[r, 3] = F32(F32(F32(-Rcw[0, r]) * tcw[0]) + F32(F32(-Rcw[1, r]) * tcw[1])) + F32(F32(-Rcw[2, r]) * tcw[2])
        Twc[3, 3] = F32(1)
        return Twc

    def UpdateBestCovisibles(self, ctx):                              # :429-448
        vPairs = []
        for pKF, w in self._map_items():
            vPairs.append((w, pKF))
        vPairs.sort(key=lambda p: (p[0], p[1].key))
        lKFs, lWs = [], []
        for w, pKF in vPairs:
            lKFs.insert(0, pKF)
            lWs.insert(0, w)
        before = set(self.mvpOrderedConnectedKeyFrames)
        if any(w < 15 and pKF not in before for w, pKF in vPairs):
            ctx.count("rebuild-pulls-sub-threshold")
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = lKFs, lWs
        self.touched |= ORD_REBUILT

    def EraseConnection(self, pKF, ctx):                              # :890-904
        bUpdate = False
        if pKF in self.mConnectedKeyFrameWeights:
            del self.mConnectedKeyFrameWeights[pKF]
            bUpdate = True
        if bUpdate:
            self.touched |= MAP_CHANGED
            ctx.op["rebuilt"] += 1
            self.UpdateBestCovisibles(ctx)

    def GetWeight(self, pKF):                                         # :492-500
        if pKF in self.mConnectedKeyFrameWeights:
            return self.mConnectedKeyFrameWeights[pKF]
        return 0

    def ChangeParent(self, pKF):                                      # :684-689
        self.mpParent = pKF
        pKF.mspChildrens.add(self)
        self.touched |= PARENT_CHANGED
        self.assigned_in_call = True

    def SetErase(self, ctx):                                          # :728-742
        if not self.mspLoopEdges:
            self.mbNotErase = False
        if self.mbToBeErased:
            r = self.SetBadFlag(ctx)
            if r == REMOVED:
                ctx.count("set-erase-removes")
            return r
        ctx.count("released")
        return RELEASED

    def SetBadFlag(self, ctx):                                        # :744-882
        if self.mbBad:
            ctx.count("already-bad")
            return ALREADY_BAD
        if self.mnId == 0:
            ctx.count("first-kf")
            return FIRST_KF
        elif self.mbNotErase:
            self.mbToBeErased = True
            ctx.count("deferred")
            return DEFERRED
        if self.assigned_in_call:
            ctx.count("parent-assigned-earlier")
        for pKF, _ in self._map_items():
            pKF.EraseConnection(self, ctx)
        for i in range(len(self.mvpMapPoints)):
            if self.mvpMapPoints[i] is not None:
                self.mvpMapPoints[i].EraseObservation(self, ctx)
        self.mConnectedKeyFrameWeights.clear()
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = [], []
        self.touched |= MAP_CHANGED | ORD_REBUILT
        sParentCandidates = {self.mpParent}
        ctx.op["children"] = len(self.mspChildrens)
        rounds = 0
        while self.mspChildrens:
            bContinue = False
            mx, pC, pP = -1, None, None
            hits = []
            for pKF in sorted(self.mspChildrens, key=lambda K: K.key):
                if pKF.isBad():
                    continue
                vpConnected = list(pKF.mvpOrderedConnectedKeyFrames)
                for i in range(len(vpConnected)):
                    for cand in sorted(sParentCandidates, key=lambda K: K.key):
                        if vpConnected[i].mnId == cand.mnId:
                            w = pKF.GetWeight(vpConnected[i])
                            hits.append(w)
                            if w > mx:
                                pC, pP, mx = pKF, vpConnected[i], w
                                bContinue = True
            if bContinue:
                if hits.count(mx) > 1 and ctx.permuted:
                    ctx.count("tie-by-order-permuted")
                if rounds >= 1 and pP is not self.mpParent:
                    ctx.count("adopted-by-adopted-child")
                pC.ChangeParent(pP)
                sParentCandidates.add(pC)
                self.mspChildrens.discard(pC)
                rounds += 1
            else:
                break
        if self.mspChildrens:
            for pKF in sorted(self.mspChildrens, key=lambda K: K.key):
                pKF.ChangeParent(self.mpParent)
                ctx.op["fallback"] += 1
                ctx.count("fallback")
        self.mpParent.mspChildrens.discard(self)                      # EraseChild
        Twc = self.mpParent.GetPoseInverse()
        Tcw = np.zeros((4, 4), F32)
        Tcw[:3, :3], Tcw[:3, 3], Tcw[3, 3] = self.Tcw[:9].reshape(3, 3), self.Tcw[9:], F32(1)
        T = np.zeros((4, 4), F32)
        for r in range(4):
            for c in range(4):                                        # four float products summed left to right
                T[r, c] = F32(F32(F32(Tcw[r, 0] * Twc[0, c]) + F32(Tcw[r, 1] * Twc[1, c])) + F32(Tcw[r, 2] * Twc[2, c])) + F32(Tcw[r, 3] * Twc[3, c])
        self.mTcp = np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(F32)
        self.mbBad = True
        pPrevKF, pNextKF = self.mpPrevKeyFrame, self.mpNextKeyFrame
        if pPrevKF:
            pPrevKF.mpNextKeyFrame = pNextKF
        if pNextKF:
            pNextKF.mpPrevKeyFrame = pPrevKF
        self.mpPrevKeyFrame, self.mpNextKeyFrame = None, None
        if pPrevKF and pNextKF:
            pNextKF.repreint = 1                                      # AppendIMUDataToFront(this), ComputePreInt()
        if any(self in links for _, links in ctx.removed):              # it was the prev or the next of a key frame removed earlier in the call
            ctx.count("adjacent-removals")
        ctx.removed.append((self, (pPrevKF, pNextKF)))
        return REMOVED


def build(s):
    """The objects of a scene: (key frames by slot, points by index)."""
    nk = len(s["kf_flags"])
    key = np.zeros(nk, np.int64)
    key[np.asarray(s["kf_by_key"], np.int64)] = np.arange(nk)
    kfs = [KeyFrame(k, int(s["kf_flags"][k]), int(key[k]), s["kf_pose12"][k]) for k in range(nk)]
    pts = [MapPoint(p, s["pt_bad"][p], s["pt_nobs"][p]) for p in range(len(s["pt_bad"]))]
    for k, K in enumerate(kfs):
        K.mpParent = kfs[s["kf_parent"][k]] if s["kf_parent"][k] >= 0 else None
        K.mpPrevKeyFrame = kfs[s["kf_prev"][k]] if s["kf_prev"][k] >= 0 else None
        K.mpNextKeyFrame = kfs[s["kf_next"][k]] if s["kf_next"][k] >= 0 else None
        K.mvpMapPoints = [pts[p] if p >= 0 else None for p in s["kp_point"][s["kp_start"][k]:s["kp_start"][k + 1]]]
        a, e = s["conn_start"][k], s["conn_start"][k + 1]
        K.mConnectedKeyFrameWeights = {kfs[c]: int(w) for c, w in zip(s["conn_kf"][a:e], s["conn_w"][a:e])}
        a, e = s["ord_start"][k], s["ord_start"][k + 1]
        K.mvpOrderedConnectedKeyFrames, K.mvOrderedWeights = [kfs[c] for c in s["ord_kf"][a:e]], [int(w) for w in s["ord_w"][a:e]]
    for K in kfs:                                                     # the rule of the header
        if K.mpParent is not None and not K.mbBad and not K.mpParent.mbBad:
            K.mpParent.mspChildrens.add(K)
    for p, P in enumerate(pts):
        P.mpRefKF = kfs[s["pt_ref"][p]] if s["pt_ref"][p] >= 0 else None
        for o in s["obs"][s["obs_start"][p]:s["obs_start"][p + 1]]:
            K = kfs[int(o) & 0xffff]
            P.mObservations[K] = K.mvpMapPoints.index(P) if P in K.mvpMapPoints else None
            P.stereo[K] = bool(int(o) & (1 << 24))
    return kfs, pts


def children_by_rule(kfs):
    """mspChildrens of every good key frame from (parent, bad) alone."""
    return [sorted(c.slot for c in kfs if c.mpParent is K and not c.mbBad) if not K.mbBad else None for K in kfs]


def remove_key_frames(s, ccap=None, events=None, objects=False):
    """Every output of viorb_kfr_result for one scene, as split() of viorb_amd/kf_removal.py returns it. ccap: the row length (default: key
    frames - 1, at least 1). events: a dict that receives the counts of the situations named in EVENTS."""
    kfs, pts = build(s)
    nk, n_op = len(kfs), len(s["op_kf"])
    cc = int(ccap or max(1, nk - 1))
    ctx = Ctx(events)
    ctx.permuted = not np.array_equal(s["kf_by_key"], np.arange(nk))
    alive0 = [list(P.mObservations) for P in pts]
    op = {f: np.zeros(n_op, np.int32) for f in ("op_reason", "op_children", "op_fallback", "op_rebuilt", "op_points_bad")}
    for j, (x, kind) in enumerate(zip(s["op_kf"], s["op_kind"])):
        ctx.op = dict(children=0, fallback=0, rebuilt=0, points_bad=0)
        op["op_reason"][j] = kfs[x].SetErase(ctx) if kind == SET_ERASE else kfs[x].SetBadFlag(ctx)
        if op["op_reason"][j] == REMOVED:
            for f in ("children", "fallback", "rebuilt", "points_bad"):
                op["op_" + f][j] = ctx.op[f]
    r = dict(status=OK, **op)
    for f in ("conn_kf_out", "conn_w_out", "ord_kf_out", "ord_w_out"):
        r[f] = np.full((nk, cc), -1, np.int32)
    r["conn_n_out"], r["ord_n_out"] = np.zeros(nk, np.int32), np.zeros(nk, np.int32)
    for k, K in enumerate(kfs):
        items = K._map_items()
        r["conn_n_out"][k], r["ord_n_out"][k] = len(items), len(K.mvpOrderedConnectedKeyFrames)
        r["conn_kf_out"][k, :len(items)], r["conn_w_out"][k, :len(items)] = [c.slot for c, _ in items], [w for _, w in items]
        r["ord_kf_out"][k, :r["ord_n_out"][k]], r["ord_w_out"][k, :r["ord_n_out"][k]] = [c.slot for c in K.mvpOrderedConnectedKeyFrames], K.mvOrderedWeights
    slot = lambda K: K.slot if K is not None else -1
    r["kf_parent_out"] = np.array([slot(K.mpParent) for K in kfs], np.int32)
    r["kf_prev_out"] = np.array([slot(K.mpPrevKeyFrame) for K in kfs], np.int32)
    r["kf_next_out"] = np.array([slot(K.mpNextKeyFrame) for K in kfs], np.int32)
    r["kf_flags_out"] = np.array([(KF_ID0 if K.mnId == 0 else 0) | (KF_BAD if K.mbBad else 0) | (KF_NOT_ERASE if K.mbNotErase else 0)
                                  | (KF_TO_BE_ERASED if K.mbToBeErased else 0) | (KF_LOOP_EDGES if K.mspLoopEdges else 0) for K in kfs], np.uint8)
    r["kf_repreint"] = np.array([K.repreint for K in kfs], np.uint8)
    r["kf_touched"] = np.array([K.touched for K in kfs], np.uint8)
    r["kf_Tcp"] = [K.mTcp for K in kfs]                               # None where the key frame was not removed in this call
    r["pt_nobs_out"] = np.array([P.nObs for P in pts], np.int32)
    r["pt_bad_out"] = np.array([P.mbBad for P in pts], np.uint8)
    r["pt_ref_out"] = np.array([slot(P.mpRefKF) for P in pts], np.int32)
    r["obs_alive"] = np.array([K in P.mObservations for P, a in zip(pts, alive0) for K in a], np.uint8)
    r["kp_point_out"] = np.array([P.index if P is not None else -1 for K in kfs for P in K.mvpMapPoints], np.int32)
    r["children"] = [sorted(c.slot for c in K.mspChildrens) if not K.mbBad else None for K in kfs]
    r["children_by_rule"] = children_by_rule(kfs)
    if objects:
        r["objects"] = (kfs, pts)
    return r


FIELDS = ("conn_kf_out", "conn_w_out", "conn_n_out", "ord_kf_out", "ord_w_out", "ord_n_out", "kf_parent_out", "kf_flags_out", "kf_prev_out", "kf_next_out",
          "kf_repreint", "kf_touched", "pt_nobs_out", "pt_bad_out", "obs_alive", "pt_ref_out", "kp_point_out",
          "op_reason", "op_children", "op_fallback", "op_rebuilt", "op_points_bad", "kf_Tcp_out")
FILL = 77


def differences(got, want, fields=FIELDS):
    """The names of the outputs of one stream (split() of viorb_amd/kf_removal.py) that differ from the checker's: exact equality of every
    array, the -1 padding of the rows included; kf_Tcp_out bit for bit on the removed key frames and untouched (the fill) on the others."""
    bad = ["status"] if got["status"] != want["status"] else []
    if bad:
        return bad
    for f in fields:
        if f == "kf_Tcp_out":
            for k, T in enumerate(want["kf_Tcp"]):
                g = np.asarray(got[f][k], F32)
                if not (np.array_equal(g.view(np.uint32), T.view(np.uint32)) if T is not None else (g == FILL).all()):
                    bad.append("%s[%d]" % (f, k))
        elif not (np.asarray(got[f]).shape == np.asarray(want[f]).shape and np.array_equal(got[f], want[f])):
            bad.append(f)
    return bad
