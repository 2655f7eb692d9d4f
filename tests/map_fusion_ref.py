"""A literal Python checker for map fusion: dicts for mObservations, lists for mvpMapPoints, the reference's statements in their order
(src/ORBmatcher.cc:842-972 without the search and :993-1097, src/LoopClosing.cc:632-640, src/MapPoint.cc:105-116, :184-222, :258,
:272-274). It shares nothing with viorb_amd/csrc/map_fusion_core.h but the scene format of viorb_amd/map_fusion.py, and keeps event
counters so that a test set can show which situations it holds."""
import numpy as np

OK, OVERFLOW, INVALID = 0, 1, -1
POSE, SIM3 = 0, 1
ADDED, REPLACED_KF_POINT, REPLACED_CANDIDATE, COUNTED_ONLY, SKIP_BAD, SKIP_IN_KF, NONE, NULL_POINT = range(8)
EVENTS = ("add-mono", "add-stereo", "replace-kf-point", "replace-candidate", "replace-tie", "counted-only", "shared-observer-erased", "same-point",
          "duplicate-went-bad", "duplicate-entered-kf", "null-entry", "sim3-lands-on-filled-feature", "sim3-replace-of-bad-point", "sim3-already-found",
          "sim3-add-observation-early-return", "second-call-reads-first", "wrap-found", "dirty-observer-bad-left-out", "survivor-of-survivor")


class MapPoint:
    def __init__(self, idx, bad, nobs, found, visible):
        self.idx, self.bad, self.nobs, self.found, self.visible = idx, bool(bad), int(nobs), int(found) & 0xffffffff, int(visible) & 0xffffffff
        self.obs = {}                   # mObservations: slot -> feature index
        self.replaced, self.dirty, self.absorbed = -1, False, False


class World:
    def __init__(self, s):
        self.s = s
        nk = len(s["kf_bad"])
        self.kp = [[int(p) for p in s["kp_point"][s["kp_start"][k]:s["kp_start"][k + 1]]] for k in range(nk)]          # mvpMapPoints
        self.stereo = [[int(v) for v in s["kp_stereo"][s["kp_start"][k]:s["kp_start"][k + 1]]] for k in range(nk)]
        self.octave = [[int(v) for v in s["kp_octave"][s["kp_start"][k]:s["kp_start"][k + 1]]] for k in range(nk)]
        self.pts = [MapPoint(p, s["pt_bad"][p], s["pt_nobs"][p], s["pt_found"][p], s["pt_visible"][p]) for p in range(len(s["pt_bad"]))]
        self.origin = {}                # (point, slot) -> index of the input observation
        for p, mp in enumerate(self.pts):
            for o in range(s["obs_start"][p], s["obs_start"][p + 1]):
                k = int(s["obs"][o]) & 0xffff
                assert k not in mp.obs
                mp.obs[k] = int(s["obs_feat"][o])
                self.origin[(p, k)] = o
        self.touched = np.zeros(len(s["obs"]), np.uint8)
        self.events = {}

    def ev(self, what):
        self.events[what] = self.events.get(what, 0) + 1

    def add_observation(self, mp, k, idx):                          # MapPoint.cc:105-116
        if k in mp.obs:
            return False
        mp.obs[k] = idx
        mp.nobs += 2 if self.stereo[k][idx] else 1
        return True

    def replace(self, a, s):                                        # a->Replace(s), MapPoint.cc:184-222
        if a.idx == s.idx:
            self.ev("same-point")
            return
        obs, a.obs = a.obs, {}
        a.bad = True
        nvisible, nfound = a.visible, a.found
        a.replaced = s.idx
        for k in sorted(obs, key=lambda k: self.rank[k]):
            idx = obs[k]
            o = self.origin.pop((a.idx, k), None)
            if o is not None:
                self.touched[o] = 1
            if k not in s.obs:
                self.kp[k][idx] = s.idx                             # ReplaceMapPointMatch
                self.add_observation(s, k, idx)
                if o is not None:
                    self.origin[(s.idx, k)] = o
            else:
                self.kp[k][idx] = -1                                # EraseMapPointMatch
                self.ev("shared-observer-erased")
        if s.found + nfound > 0xffffffff or s.visible + nvisible > 0xffffffff:
            self.ev("wrap-found")
        s.found, s.visible = (s.found + nfound) & 0xffffffff, (s.visible + nvisible) & 0xffffffff
        if s.absorbed:
            self.ev("survivor-of-survivor")
        s.absorbed = True
        s.dirty = True                                              # ComputeDistinctiveDescriptors

    def fuse_pose(self, kf, points, feats, reasons, others, seen):
        nfused = 0
        for i, (p, f) in enumerate(zip(points, feats)):
            if p < 0:
                reasons[i] = NULL_POINT
                self.ev("null-entry")
                continue
            mp = self.pts[p]
            if mp.bad or kf in mp.obs:
                reasons[i] = SKIP_BAD if mp.bad else SKIP_IN_KF
                if p in seen and seen[p] != reasons[i]:
                    self.ev("duplicate-went-bad" if mp.bad else "duplicate-entered-kf")
                continue
            seen.setdefault(p, -1)
            if f < 0:
                reasons[i] = NONE
                continue
            q = self.kp[kf][f]
            others[i] = q
            if q >= 0:
                mq = self.pts[q]
                if not mq.bad:
                    if mq.nobs > mp.nobs:
                        reasons[i] = REPLACED_CANDIDATE
                        self.ev("replace-candidate")
                        self.replace(mp, mq)
                    else:
                        reasons[i] = REPLACED_KF_POINT
                        self.ev("replace-tie" if mq.nobs == mp.nobs and q != p else "replace-kf-point")
                        self.replace(mq, mp)
                else:
                    reasons[i] = COUNTED_ONLY
                    self.ev("counted-only")
            else:
                reasons[i] = ADDED
                self.ev("add-stereo" if self.stereo[kf][f] else "add-mono")
                self.add_observation(mp, kf, f)
                self.kp[kf][f] = p                                  # AddMapPoint
            nfused += 1
        return nfused

    def fuse_sim3(self, kf, points, feats, reasons, others):
        already = {q for q in self.kp[kf] if q >= 0 and not self.pts[q].bad}           # GetMapPoints
        nfused, rep, filled = 0, [None] * len(points), set()
        for i, (p, f) in enumerate(zip(points, feats)):
            if p < 0:
                reasons[i] = NULL_POINT
                self.ev("null-entry")
                continue
            mp = self.pts[p]
            if mp.bad or p in already:
                reasons[i] = SKIP_BAD if mp.bad else SKIP_IN_KF
                if not mp.bad:
                    self.ev("sim3-already-found")
                continue
            if f < 0:
                reasons[i] = NONE
                continue
            q = self.kp[kf][f]
            others[i] = q
            if q >= 0:
                if not self.pts[q].bad:
                    reasons[i] = REPLACED_KF_POINT
                    rep[i] = self.pts[q]
                    if f in filled:
                        self.ev("sim3-lands-on-filled-feature")
                else:
                    reasons[i] = COUNTED_ONLY
                    self.ev("counted-only")
            else:
                reasons[i] = ADDED
                self.ev("add-stereo" if self.stereo[kf][f] else "add-mono")
                if not self.add_observation(mp, kf, f):
                    self.ev("sim3-add-observation-early-return")
                self.kp[kf][f] = p
                filled.add(f)
            nfused += 1
        for i, p in enumerate(points):                              # LoopClosing.cc:633-640
            if rep[i] is not None:
                if rep[i].bad and rep[i].idx != p:
                    self.ev("sim3-replace-of-bad-point")
                self.replace(rep[i], self.pts[p])
        return nfused


def apply_fuse(s, region=None):
    """The calls of one scene in order. Returns the fields viorb_amd.map_fusion.split produces, plus `events`."""
    w = World(s)
    nk = len(s["kf_bad"])
    w.rank = {int(k): j for j, k in enumerate(s["kf_by_key"])}
    n_op = int(s["call_n"].sum())
    reasons, others, nfused = np.full(n_op, -9, np.int32), np.full(n_op, -1, np.int32), []
    j = 0
    changed_before = False
    for c in range(len(s["call_kf"])):
        kf, n = int(s["call_kf"][c]), int(s["call_n"][c])
        points = [int(p) for p in s["list_point"][s["call_list"][c]:s["call_list"][c] + n]]
        feats = [int(f) for f in s["op_feat"][s["call_feat"][c]:s["call_feat"][c] + n]]
        snapshot = ([list(r) for r in w.kp], [(p.bad, p.nobs, dict(p.obs)) for p in w.pts])
        if s["call_kind"][c] == POSE:
            nfused.append(w.fuse_pose(kf, points, feats, reasons[j:j + n], others[j:j + n], {}))
        else:
            nfused.append(w.fuse_sim3(kf, points, feats, reasons[j:j + n], others[j:j + n]))
        now = ([list(r) for r in w.kp], [(p.bad, p.nobs, dict(p.obs)) for p in w.pts])
        if changed_before and now != snapshot:
            w.ev("second-call-reads-first")
        changed_before = changed_before or now != snapshot
        j += n
    by_rank = lambda mp: sorted(mp.obs, key=lambda k: w.rank[k])
    r = dict(status=OK, events=w.events)
    r["kp_point_out"] = np.array([p for row in w.kp for p in row], np.int32)
    r["pt_bad_out"] = np.array([p.bad for p in w.pts], np.uint8)
    r["pt_nobs_out"] = np.array([p.nobs for p in w.pts], np.int32)
    r["pt_found_out"] = np.array([p.found for p in w.pts], np.uint32).view(np.int32)
    r["pt_visible_out"] = np.array([p.visible for p in w.pts], np.uint32).view(np.int32)
    r["pt_replaced_out"] = np.array([p.replaced for p in w.pts], np.int32)
    r["pt_dirty"] = np.array([p.dirty for p in w.pts], np.uint8)
    r["obs"] = [[(k, w.octave[k][mp.obs[k]], w.stereo[k][mp.obs[k]], mp.obs[k]) for k in by_rank(mp)] for mp in w.pts]
    r["need"] = sum(len(o) for o in r["obs"])
    r["dirty"] = [[(k, mp.obs[k]) for k in by_rank(mp) if not s["kf_bad"][k]] if mp.dirty and not mp.bad else [] for mp in w.pts]
    if any(mp.dirty and not mp.bad and any(s["kf_bad"][k] for k in mp.obs) for mp in w.pts):
        w.ev("dirty-observer-bad-left-out")
    alive = set(w.origin.values())
    r["obs_touched"] = w.touched
    assert all(w.touched[o] for o in range(len(s["obs"])) if o not in alive)
    r["op_reason"], r["op_other"], r["call_nfused"] = reasons, others, np.array(nfused, np.int32)
    if region is not None and r["need"] > region:
        r["status"] = OVERFLOW
        del r["obs"]
        r["dirty"] = [[] for _ in w.pts]
    return r


FIELDS = ("kp_point_out", "pt_bad_out", "pt_nobs_out", "pt_found_out", "pt_visible_out", "pt_replaced_out", "pt_dirty", "obs_touched", "op_reason", "op_other", "call_nfused")


def differences(got, exp, fields=FIELDS + ("need", "obs", "dirty")):
    """The names of the fields in which a result of viorb_amd.map_fusion differs from the checker's."""
    if got["status"] != exp["status"]:
        return ["status %d != %d" % (got["status"], exp["status"])]
    d = [f for f in fields if f in FIELDS and f in got and not np.array_equal(np.asarray(got[f]), np.asarray(exp[f]))]
    d += [f for f in ("need", "obs", "dirty") if f in fields and f in got and f in exp and got[f] != exp[f]]
    if exp["status"] == OK and "obs" in fields and "obs" not in got:
        d.append("obs missing")
    return d
