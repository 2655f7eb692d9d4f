"""numpy restatement (float32, with the reference's casts) of ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
(src/ORBmatcher.cc:1473-1600) with Frame::GetFeaturesInArea (src/Frame.cc:507-560), MapPoint::PredictScale (src/MapPoint.cc:409-424) and
ORBmatcher::ComputeThreeMaxima (:1602-1643), as the literal loop in the order of vpMPs: a `set` for sAlreadyFound, an mGrid of lists, the 30
rotHist vectors; and of the cascade of Tracking::Relocalization (src/Tracking.cc:2209-2273) statement by statement, with
oracle.binding.pose_opt_se3 as Optimizer::PoseOptimization. The checker of tests/test_reloc_ref.py and tests/test_gpu_relocalization.py;
product code never imports it. A map point is identified by the index of the key-frame feature that holds it.

Casts (see sim3_match_ref.py): a 3 x 3 product is the small-matrix gemm (m0 x0 + m1 x1) + m2 x2 in float and `Rcw*x3Dw+tcw` adds tcw in
float; `1.0/z` is a double quotient stored to float; `fx*xc*invzc+cx` is three float operations from the left; cv::norm works in double
and is stored to float; a float no int holds converts as x86 converts it (INT_MIN)."""
import numpy as np
import sim3_match_ref as S
from sim3_match_ref import Camera, KeyFrame as Frame, hamming  # noqa: F401  (Frame: mvKeysUn, mDescriptors, mGrid of lists)

f32, f64 = np.float32, np.float64
MATCHED, NOT_CANDIDATE, BEHIND, OUT_OF_IMAGE, OUT_OF_RANGE, VIEW_ANGLE, NO_FEATURE_IN_WINDOW, ABOVE_THRESHOLD, NOT_MUTUAL, ROTATION = range(10)
REASON_NAMES = S.REASON_NAMES + ("ROTATION",)
POSSIBLE_REASONS = (MATCHED, NOT_CANDIDATE, OUT_OF_IMAGE, OUT_OF_RANGE, NO_FEATURE_IN_WINDOW, ABOVE_THRESHOLD, ROTATION)
RUNNING, FEW_INLIERS, ACCEPTED_FIRST, COARSE_SHORT, SECOND_WEAK, ACCEPTED_SECOND, NARROW_SHORT, THIRD_REJECTED, ACCEPTED_THIRD = range(9)
STAGE_NAMES = ("RUNNING", "FEW_INLIERS", "ACCEPTED_FIRST", "COARSE_SHORT", "SECOND_WEAK", "ACCEPTED_SECOND", "NARROW_SHORT", "THIRD_REJECTED", "ACCEPTED_THIRD")
HISTO_LENGTH = 30
COLS, ROWS, INT_MIN = S.COLS, S.ROWS, S.INT_MIN


def _to_int(q):
    """(int) of a float as x86 converts it."""
    q = f64(q)
    return int(q) if np.isfinite(q) and -2.0 ** 31 < q < 2.0 ** 31 else INT_MIN


def cell_rect(c, x, y, r):
    """Frame::GetFeaturesInArea :512-526, or None where it returns early."""
    with np.errstate(all="ignore"):
        x0 = max(0, _to_int(np.floor((x - c.minX - r) * c.wInv)))
        if x0 >= COLS:
            return None
        x1 = min(COLS - 1, _to_int(np.ceil((x - c.minX + r) * c.wInv)))
        if x1 < 0:
            return None
        y0 = max(0, _to_int(np.floor((y - c.minY - r) * c.hInv)))
        if y0 >= ROWS:
            return None
        y1 = min(ROWS - 1, _to_int(np.ceil((y - c.minY + r) * c.hInv)))
        if y1 < 0:
            return None
    return x0, x1, y0, y1


def get_features_in_area(frame, x, y, r, minLevel, maxLevel):
    """Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel)."""
    vIndices = []
    rect = cell_rect(frame.cam, x, y, r)
    if rect is None:
        return vIndices
    nMinCellX, nMaxCellX, nMinCellY, nMaxCellY = rect
    bCheckLevels = (minLevel > 0) or (maxLevel >= 0)
    for ix in range(nMinCellX, nMaxCellX + 1):
        for iy in range(nMinCellY, nMaxCellY + 1):
            vCell = frame.grid[ix][iy]
            if not vCell:
                continue
            for j in vCell:
                if bCheckLevels:
                    if frame.octave[j] < minLevel:
                        continue
                    if maxLevel >= 0:
                        if frame.octave[j] > maxLevel:
                            continue
                distx = frame.x[j] - x
                disty = frame.y[j] - y
                if abs(distx) < r and abs(disty) < r:
                    vIndices.append(j)
    return vIndices


def compute_three_maxima(histo, L):
    """ORBmatcher::ComputeThreeMaxima: (ind1, ind2, ind3)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i in range(L):
        s = len(histo[i])
        if s > max1:
            max3 = max2; max2 = max1; max1 = s
            ind3 = ind2; ind2 = ind1; ind1 = i
        elif s > max2:
            max3 = max2; max2 = s
            ind3 = ind2; ind2 = i
        elif s > max3:
            max3 = s
            ind3 = i
    if max2 < f32(0.1) * f32(max1):
        ind2 = -1; ind3 = -1
    elif max3 < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(a1, a2):
    factor = f32(1.0) / f32(HISTO_LENGTH)
    rot = f32(a1) - f32(a2)
    if rot < 0.0:
        rot = rot + f32(360.0)
    b = S._round_half_away(f32(rot * factor))
    if b == HISTO_LENGTH:
        b = 0
    assert 0 <= b < HISTO_LENGTH
    return b


def project(cam, pose12, X, th):
    """:1477-1479, :1498-1527 for one point: dict(u, v, dist3D, level, radius, reason); reason MATCHED = it reaches GetFeaturesInArea."""
    P, X = np.asarray(pose12, f32), np.asarray(X, f32)
    Rcw, tcw = P[:9].reshape(3, 3), P[9:12]
    r = dict(u=f32(0), v=f32(0), dist3D=f32(0), level=0, radius=f32(0), reason=MATCHED)
    with np.errstate(all="ignore"):
        Ow = -S._mul3(Rcw.T, tcw)
        x3Dc = S._mul3(Rcw, X[:3]) + tcw
        xc, yc = x3Dc[0], x3Dc[1]
        invzc = f32(1.0 / f64(x3Dc[2]))
        u = f32(f32(cam.fx * xc) * invzc) + cam.cx
        v = f32(f32(cam.fy * yc) * invzc) + cam.cy
    r["u"], r["v"] = u, v
    if u < cam.minX or u > cam.maxX:
        r["reason"] = OUT_OF_IMAGE
        return r
    if v < cam.minY or v > cam.maxY:
        r["reason"] = OUT_OF_IMAGE
        return r
    PO = X[:3] - Ow
    dist3D = S._norm3(PO)
    r["dist3D"] = dist3D
    maxDistance, minDistance = f32(1.2) * X[7], f32(0.8) * X[6]
    if dist3D < minDistance or dist3D > maxDistance:
        r["reason"] = OUT_OF_RANGE
        return r
    r["level"] = S.predict_scale(X[7], dist3D, cam)
    r["radius"] = f32(th) * cam.sf[r["level"]]
    return r


def search_by_projection(frame, pose12, kf_angle, kf_valid, sAlreadyFound, pts_f, pts_desc, mvpMapPoints, th, orb_dist, check_orientation=True,
                         ordered=True):
    """The function, literally. frame: the lost frame; the candidate key frame is the arrays indexed by its feature i (vpMPs[i] exists and
    is good where kf_valid[i]); sAlreadyFound: a set of i; mvpMapPoints: the frame's list (None or i), WRITTEN as the reference writes it.
    dict(best_idx [npts], nmatches, reason [npts]). ordered=False is NOT the reference: it looks at the entry state only, for the tests
    that show the fixtures contend."""
    cam = frame.cam
    npts = len(pts_f)
    nmatches = 0
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    who = {}                                                    # frame feature -> the point that holds it (for best_idx)
    best_idx, reason = np.full(npts, -1, np.int32), np.full(npts, NOT_CANDIDATE, np.int32)
    entry = list(mvpMapPoints)
    for i in range(npts):
        if not kf_valid[i] or i in sAlreadyFound:
            continue
        g = project(cam, pose12, pts_f[i], th)
        if g["reason"] != MATCHED:
            reason[i] = g["reason"]
            continue
        lvl = g["level"]
        vIndices2 = get_features_in_area(frame, g["u"], g["v"], g["radius"], lvl - 1, lvl + 1)
        if not vIndices2:
            reason[i] = NO_FEATURE_IN_WINDOW
            continue
        bestDist, bestIdx2 = 256, -1
        for i2 in vIndices2:
            if (mvpMapPoints if ordered else entry)[i2] is not None:
                continue
            dist = hamming(pts_desc[i], frame.desc[i2])
            if dist < bestDist:
                bestDist, bestIdx2 = dist, i2
        reason[i] = ABOVE_THRESHOLD
        if bestDist <= orb_dist:
            mvpMapPoints[bestIdx2] = i
            who[i] = bestIdx2
            best_idx[i], reason[i] = bestIdx2, MATCHED
            nmatches += 1
            if check_orientation:
                rotHist[rot_bin(kf_angle[i], frame.kps["angle"][bestIdx2])].append((bestIdx2, i))
    if check_orientation:
        ind1, ind2, ind3 = compute_three_maxima(rotHist, HISTO_LENGTH)
        for b in range(HISTO_LENGTH):
            if b != ind1 and b != ind2 and b != ind3:
                for i2, i in rotHist[b]:
                    mvpMapPoints[i2] = None
                    best_idx[i], reason[i] = -1, ROTATION
                    nmatches -= 1
    return dict(best_idx=best_idx, nmatches=nmatches, reason=reason)


def match_lists(cands, taken_in, angle_kf, angle_f, orb_dist, check_orientation=True):
    """The loop of :1536-1597 over given candidate lists cands[p] = [(distance, feature), ...] in visiting order: (best_idx, removed,
    nmatches)."""
    taken = np.array(taken_in, bool).copy()
    best = np.full(len(cands), -1, np.int32)
    removed = np.zeros(len(cands), np.uint8)
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    n = 0
    for p, lst in enumerate(cands):
        bestDist, bestIdx2 = 256, -1
        for d, idx in lst:
            if taken[idx]:
                continue
            if d < bestDist:
                bestDist, bestIdx2 = d, idx
        if bestDist <= orb_dist:
            taken[bestIdx2] = True
            best[p] = bestIdx2
            n += 1
            if check_orientation:
                rotHist[rot_bin(angle_kf[p], angle_f[bestIdx2])].append(p)
    if check_orientation:
        ind = compute_three_maxima(rotHist, HISTO_LENGTH)
        for b in range(HISTO_LENGTH):
            if b not in ind:
                for p in rotHist[b]:
                    best[p], removed[p] = -1, 1
                    n -= 1
    return best, removed, n


# ---- the cascade --------------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(min_good=10, accept=50, narrow_above=30, th_coarse=10.0, orb_dist_coarse=100, th_narrow=3.0, orb_dist_narrow=64, check_orientation=True)


def pose_optimization(frame, F, solver):
    """Optimizer::PoseOptimization(Frame*) on the state F = dict(mTcw, mvpMapPoints, mvbOutlier, ...): the edges in key-point order
    (src/Optimizer.cc:3792-3870), the solve, SetPose. Returns nInitialCorrespondences - nBad."""
    idx = [i for i in range(frame.N) if F["mvpMapPoints"][i] is not None]
    obs = np.zeros((len(idx), 7))
    for k, i in enumerate(idx):
        F["mvbOutlier"][i] = False
        X = F["pts_f"][F["mvpMapPoints"][i]]
        ur = -1.0 if F["uright"] is None else f64(F["uright"][i])
        obs[k] = [X[0], X[1], X[2], frame.x[i], frame.y[i], ur, F["inv_sigma2"][frame.octave[i]]]
    if len(idx) < 3:
        F["chi2"] = 0.0
        return 0
    r = solver(F["mTcw"], F["intr5"], obs)
    for k, i in enumerate(idx):
        F["mvbOutlier"][i] = bool(r["outlier"][k])
    F["mTcw"] = np.asarray(r["pose12"], f32).copy()
    if F["perturb"] is not None:
        F["mTcw"] = F["perturb"](F["mTcw"])
    F["chi2"] = r["final_chi2"]
    return r["n_inliers"]


def refine(frame, intr5, uright, inv_sigma2, hyp, solver, cfg=None, perturb=None):
    """src/Tracking.cc:2209-2273 for one hypothesis hyp = dict(pose12, kf_angle, kf_valid, pts_f, pts_desc, bow_match [N], inlier [N]).
    perturb: applied to every pose a solve hands on (the fixture-robustness condition). dict(accepted, n_good, stage, counts [8], pose12,
    chi2, frame_match [N], outlier [N])."""
    c = dict(DEFAULTS, **(cfg or {}))
    N = frame.N
    F = dict(mTcw=np.asarray(hyp["pose12"], f32).copy(), mvpMapPoints=[None] * N, mvbOutlier=[False] * N, pts_f=np.asarray(hyp["pts_f"], f32),
             uright=uright, inv_sigma2=np.asarray(inv_sigma2, f32), intr5=np.asarray(intr5, f64), perturb=perturb, chi2=0.0)
    counts = np.array([-1, -1, -1, -1, -1, 0, 0, 0], np.int32)
    search = lambda sFound, th, od: search_by_projection(frame, F["mTcw"], hyp["kf_angle"], hyp["kf_valid"], sFound, hyp["pts_f"], hyp["pts_desc"],
                                                         F["mvpMapPoints"], th, od, c["check_orientation"])["nmatches"]
    sFound = set()
    for j in range(N):
        if hyp["inlier"][j]:
            F["mvpMapPoints"][j] = int(hyp["bow_match"][j]) if hyp["bow_match"][j] >= 0 else None
            if hyp["bow_match"][j] >= 0:
                sFound.add(int(hyp["bow_match"][j]))
        else:
            F["mvpMapPoints"][j] = None
    stage = None
    nGood = pose_optimization(frame, F, solver)
    counts[0] = nGood
    if nGood < c["min_good"]:
        stage = FEW_INLIERS                                     # `continue`: nothing nulled
    else:
        for io in range(N):
            if F["mvbOutlier"][io]:
                F["mvpMapPoints"][io] = None
        if nGood < c["accept"]:
            nadditional = search(sFound, c["th_coarse"], c["orb_dist_coarse"])
            counts[1] = nadditional
            if nadditional + nGood >= c["accept"]:
                nGood = pose_optimization(frame, F, solver)
                counts[2] = nGood
                if nGood > c["narrow_above"] and nGood < c["accept"]:
                    sFound = set()
                    for ip in range(N):
                        if F["mvpMapPoints"][ip] is not None:
                            sFound.add(F["mvpMapPoints"][ip])
                    nadditional = search(sFound, c["th_narrow"], c["orb_dist_narrow"])
                    counts[3] = nadditional
                    if nGood + nadditional >= c["accept"]:
                        nGood = pose_optimization(frame, F, solver)
                        counts[4] = nGood
                        for io in range(N):
                            if F["mvbOutlier"][io]:
                                F["mvpMapPoints"][io] = None
                        stage = ACCEPTED_THIRD if nGood >= c["accept"] else THIRD_REJECTED
                    else:
                        stage = NARROW_SHORT
                else:
                    stage = ACCEPTED_SECOND if nGood >= c["accept"] else SECOND_WEAK
            else:
                stage = COARSE_SHORT
        else:
            stage = ACCEPTED_FIRST
    return dict(accepted=int(nGood >= c["accept"]), n_good=int(nGood), stage=stage, counts=counts, pose12=F["mTcw"], chi2=F["chi2"],
                frame_match=np.array([-1 if m is None else m for m in F["mvpMapPoints"]], np.int32), outlier=np.array(F["mvbOutlier"], np.uint8))
