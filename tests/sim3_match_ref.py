"""numpy restatement (float32, with the reference's casts) of the three projection matchers that take a similarity, as literal point-order
loops written from the reference's text (src/ORBmatcher.cc:290-403, :977-1100, :1102-1326, src/KeyFrame.cc:906-950, src/Frame.cc:562-572,
src/MapPoint.cc:392-407). The checker of tests/test_sim3_match_ref.py and tests/test_gpu_sim3_match.py; product code never imports it.

Casts: Mat::dot, cv::norm and sqrt(double) work in double and are stored to float; `Mat / float` and `float * Mat` are MatExpr scalings
by a double alpha, rounded per element; a 3 x 3 product is the small-matrix gemm (m0 x0 + m1 x1) + m2 x2 in float; every `cv::Mat = A*x + b`
is rounded to float; PredictScale's logarithm is (float)log((double)ratio) as in the library's other matchers, and a quotient no int holds
converts as x86 converts it (INT_MIN), which clamps to level 0."""
import numpy as np

f32, f64 = np.float32, np.float64
MATCHED, NOT_CANDIDATE, BEHIND, OUT_OF_IMAGE, OUT_OF_RANGE, VIEW_ANGLE, NO_FEATURE_IN_WINDOW, ABOVE_THRESHOLD, NOT_MUTUAL = range(9)
REASON_NAMES = ("MATCHED", "NOT_CANDIDATE", "BEHIND", "OUT_OF_IMAGE", "OUT_OF_RANGE", "VIEW_ANGLE", "NO_FEATURE_IN_WINDOW", "ABOVE_THRESHOLD", "NOT_MUTUAL")
TH_LOW, TH_HIGH = 50, 100
COLS, ROWS = 64, 48
SEARCH_BY_SIM3, SEARCH_BY_PROJECTION, FUSE = 0, 1, 2
INT_MIN = -2 ** 31
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def _mul3(R, X):
    """(R[r,0] X0 + R[r,1] X1) + R[r,2] X2 in float32."""
    R, X = np.asarray(R, f32).reshape(3, 3), np.asarray(X, f32)
    return (R[:, 0] * X[0] + R[:, 1] * X[1]) + R[:, 2] * X[2]


def _norm3(v):
    v = np.asarray(v, f32).astype(f64)
    return f32(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


class Camera:
    """fx fy cx cy, the image bounds, the scale table: what the three functions read of a key frame beside its features."""

    def __init__(self, intr4, bounds4, scale_factors, nlevels=None):
        self.fx, self.fy, self.cx, self.cy = [f32(v) for v in intr4]
        self.minX, self.maxX, self.minY, self.maxY = [f32(v) for v in bounds4]
        self.wInv = f32(COLS) / f32(self.maxX - self.minX)
        self.hInv = f32(ROWS) / f32(self.maxY - self.minY)
        self.nlevels = len(scale_factors) if nlevels is None else int(nlevels)
        self.sf = np.asarray(scale_factors, f32)[:self.nlevels]
        with np.errstate(all="ignore"):
            self.log_sf = f32(np.log(f64(self.sf[1 if self.nlevels > 1 else 0])))


def _round_half_away(x):
    x = f64(x)
    return int(np.sign(x) * np.floor(np.abs(x) + 0.5))


def cell_rect(c, u, v, r):
    """The cell rectangle of GetFeaturesInArea (src/KeyFrame.cc:911-925), or None where it returns early."""
    x0 = max(0, int(np.floor((u - c.minX - r) * c.wInv)))
    if x0 >= COLS:
        return None
    x1 = min(COLS - 1, int(np.ceil((u - c.minX + r) * c.wInv)))
    if x1 < 0:
        return None
    y0 = max(0, int(np.floor((v - c.minY - r) * c.hInv)))
    if y0 >= ROWS:
        return None
    y1 = min(ROWS - 1, int(np.ceil((v - c.minY + r) * c.hInv)))
    if y1 < 0:
        return None
    return x0, x1, y0, y1


class KeyFrame:
    """mvKeysUn, mDescriptors and mGrid (Frame::AssignFeaturesToGrid: push_back in key-point order)."""

    def __init__(self, cam, kps, desc):
        self.cam, self.kps, self.desc, self.N = cam, kps, np.asarray(desc, np.uint8).reshape(-1, 32), len(kps)
        self.x, self.y, self.octave = np.asarray(kps["x"], f32), np.asarray(kps["y"], f32), np.asarray(kps["octave"], np.int64)
        self.grid = [[[] for _ in range(ROWS)] for _ in range(COLS)]
        for i in range(self.N):
            px = _round_half_away((self.x[i] - cam.minX) * cam.wInv)
            py = _round_half_away((self.y[i] - cam.minY) * cam.hInv)
            if px < 0 or px >= COLS or py < 0 or py >= ROWS:
                continue
            self.grid[px][py].append(i)

    def csr(self):
        """cell_start [64*48+1], cell_idx [N in grid] in storage order ix*48 + iy."""
        start, idx = [0], []
        for ix in range(COLS):
            for iy in range(ROWS):
                idx += self.grid[ix][iy]
                start.append(len(idx))
        return np.array(start, np.int32), np.array(idx, np.int32)

    def features_in_area(self, u, v, r):
        rect = cell_rect(self.cam, u, v, r)
        out = []
        if rect is None:
            return out
        x0, x1, y0, y1 = rect
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for j in self.grid[ix][iy]:
                    if abs(self.x[j] - u) < r and abs(self.y[j] - v) < r:
                        out.append(j)
        return out


def decompose(Scw):
    """scw, Rcw [3,3], tcw [3], Ow [3] of Scw [12] (:298-303)."""
    S = np.asarray(Scw, f32).reshape(3, 4)
    row0 = S[0, :3].astype(f64)
    scw = f32(np.sqrt((row0[0] * row0[0] + row0[1] * row0[1]) + row0[2] * row0[2]))
    alpha = 1.0 / f64(scw)
    Rcw = (S[:, :3].astype(f64) * alpha).astype(f32)
    tcw = (S[:, 3].astype(f64) * alpha).astype(f32)
    Ow = -_mul3(Rcw.T, tcw)
    return scw, Rcw, tcw, Ow


def pair(R12, t12, s12):
    """sR12, sR21 [3,3], t21 [3] (:1119-1121)."""
    R12, t12 = np.asarray(R12, f32).reshape(3, 3), np.asarray(t12, f32)
    with np.errstate(all="ignore"):
        sR12 = (R12.astype(f64) * f64(f32(s12))).astype(f32)
        sR21 = (R12.T.astype(f64) * (1.0 / f64(f32(s12)))).astype(f32)
    return sR12, sR21, -_mul3(sR21, t12)


def predict_scale(max_distance, dist, cam):
    with np.errstate(all="ignore"):
        ratio = f32(max_distance) / f32(dist)
        q = np.ceil(f32(np.log(f64(ratio))) / cam.log_sf)
    n = int(q) if np.isfinite(q) and -2.0 ** 31 < q < 2.0 ** 31 else INT_MIN
    return 0 if n < 0 else (cam.nlevels - 1 if n >= cam.nlevels else n)


def gates(cam, pc, dist3D, X, PO, th):
    """From the point in the camera frame to the window. dict(u, v, dist3D, level, radius, rect, reason): reason is the `continue` that
    ended the point, or MATCHED when it reaches GetFeaturesInArea with a cell rectangle."""
    r = dict(u=f32(0), v=f32(0), dist3D=f32(dist3D), level=0, radius=f32(0), rect=(0, -1, 0, -1), reason=MATCHED)
    if pc[2] < 0.0:
        r["reason"] = BEHIND
        return r
    with np.errstate(all="ignore"):
        invz = f32(1.0 / f64(pc[2]))
        x, y = pc[0] * invz, pc[1] * invz
        u, v = cam.fx * x + cam.cx, cam.fy * y + cam.cy
    r["u"], r["v"] = u, v
    if not (u >= cam.minX and u < cam.maxX and v >= cam.minY and v < cam.maxY):
        r["reason"] = OUT_OF_IMAGE
        return r
    maxD, minD = f32(1.2) * X[7], f32(0.8) * X[6]
    if dist3D < minD or dist3D > maxD:
        r["reason"] = OUT_OF_RANGE
        return r
    if PO is not None:
        dot = (f64(PO[0]) * f64(X[3]) + f64(PO[1]) * f64(X[4])) + f64(PO[2]) * f64(X[5])
        if dot < 0.5 * f64(dist3D):
            r["reason"] = VIEW_ANGLE
            return r
    lvl = predict_scale(X[7], dist3D, cam)
    radius = f32(th) * cam.sf[lvl]
    r["level"], r["radius"] = lvl, radius
    rect = cell_rect(cam, u, v, radius)
    if rect is None:
        r["reason"] = NO_FEATURE_IN_WINDOW
    else:
        r["rect"] = rect
    return r


def project_scw(cam, dec, X, th):
    scw, Rcw, tcw, Ow = dec
    X = np.asarray(X, f32)
    pc = _mul3(Rcw, X[:3]) + tcw
    PO = X[:3] - Ow
    return gates(cam, pc, _norm3(PO), X, PO, th)


def project_pair(cam, pose12_own, sR, t, X, th):
    X, P = np.asarray(X, f32), np.asarray(pose12_own, f32)
    with np.errstate(all="ignore"):
        pa = _mul3(P[:9], X[:3]) + P[9:12]
        pb = _mul3(sR, pa) + np.asarray(t, f32)
        d = _norm3(pb)
    return gates(cam, pb, d, X, None, th)


def _best_in_window(kf, g, desc, th_desc, taken=None):
    """The inner loop of the three functions: (bestIdx or -1, reason)."""
    idxs = kf.features_in_area(g["u"], g["v"], g["radius"])
    if not idxs:
        return -1, NO_FEATURE_IN_WINDOW
    best_dist, best = 256 if th_desc == TH_LOW else 2 ** 31 - 1, -1
    lvl = g["level"]
    for idx in idxs:
        if taken is not None and taken[idx]:
            continue
        if kf.octave[idx] < lvl - 1 or kf.octave[idx] > lvl:
            continue
        d = hamming(desc, kf.desc[idx])
        if d < best_dist:
            best_dist, best = d, idx
    if best_dist <= th_desc:
        return best, MATCHED
    return -1, ABOVE_THRESHOLD


def search_by_sim3(kf1, pose1, has1, pts_f1, pts_desc1, already1, kf2, pose2, has2, pts_f2, pts_desc2, already2, R12, t12, s12, th):
    """dict(match12 [N1], nfound, match1 [N1], match2 [N2], reason1 [N1], reason2 [N2])."""
    cam = kf1.cam
    sR12, sR21, t21 = pair(R12, t12, s12)
    t12 = np.asarray(t12, f32)

    def one_way(kf_own, kf_oth, pose, has, pts_f, pts_desc, already, sR, t):
        match, reason = np.full(kf_own.N, -1, np.int32), np.full(kf_own.N, NOT_CANDIDATE, np.int32)
        for i in range(kf_own.N):
            if not has[i] or already[i]:
                continue
            g = project_pair(cam, pose, sR, t, pts_f[i], th)
            if g["reason"] != MATCHED:
                reason[i] = g["reason"]
                continue
            match[i], reason[i] = _best_in_window(kf_oth, g, pts_desc[i], TH_HIGH)
        return match, reason
    m1, r1 = one_way(kf1, kf2, pose1, has1, pts_f1, pts_desc1, already1, sR21, t21)
    m2, r2 = one_way(kf2, kf1, pose2, has2, pts_f2, pts_desc2, already2, sR12, t12)
    m12, nfound = np.full(kf1.N, -1, np.int32), 0
    for i1 in range(kf1.N):
        idx2 = m1[i1]
        if idx2 >= 0:
            if m2[idx2] == i1:
                m12[i1] = idx2
                nfound += 1
            else:
                r1[i1] = NOT_MUTUAL
    for i2 in range(kf2.N):
        if m2[i2] >= 0 and m1[m2[i2]] != i2:
            r2[i2] = NOT_MUTUAL
    return dict(match12=m12, nfound=nfound, match1=m1, match2=m2, reason1=r1, reason2=r2)


def search_by_projection(kf, Scw, pts_f, pts_desc, pts_valid, feat_taken, th, ordered=True):
    """dict(best_idx [npts], nmatches, reason [npts]). ordered=False is NOT the reference: it is the variant that looks at the entry
    bitmap only, for the tests that show the fixtures contend."""
    dec = decompose(Scw)
    taken = np.array(feat_taken, bool).copy()
    npts = len(pts_f)
    best_idx, reason, n = np.full(npts, -1, np.int32), np.full(npts, NOT_CANDIDATE, np.int32), 0
    for p in range(npts):
        if not pts_valid[p]:
            continue
        g = project_scw(kf.cam, dec, pts_f[p], th)
        if g["reason"] != MATCHED:
            reason[p] = g["reason"]
            continue
        best_idx[p], reason[p] = _best_in_window(kf, g, pts_desc[p], TH_LOW, taken)
        if best_idx[p] >= 0:
            if ordered:
                taken[best_idx[p]] = True
            n += 1
    return dict(best_idx=best_idx, nmatches=n, reason=reason)


def fuse(kf, Scw, pts_f, pts_desc, pts_valid, th):
    """dict(best_idx [npts], nfused, reason [npts])."""
    dec = decompose(Scw)
    npts = len(pts_f)
    best_idx, reason, n = np.full(npts, -1, np.int32), np.full(npts, NOT_CANDIDATE, np.int32), 0
    for p in range(npts):
        if not pts_valid[p]:
            continue
        g = project_scw(kf.cam, dec, pts_f[p], th)
        if g["reason"] != MATCHED:
            reason[p] = g["reason"]
            continue
        best_idx[p], reason[p] = _best_in_window(kf, g, pts_desc[p], TH_LOW)
        n += best_idx[p] >= 0
    return dict(best_idx=best_idx, nfused=int(n), reason=reason)


def claim_in_order(cands, taken_in):
    """The loop of :370-398 over given candidate lists: cands[p] = [(distance, feature), ...] in visiting order. best_idx [npts]."""
    taken = np.array(taken_in, bool).copy()
    out = np.full(len(cands), -1, np.int32)
    for p, lst in enumerate(cands):
        best_dist, best = 256, -1
        for d, idx in lst:
            if taken[idx]:
                continue
            if d < best_dist:
                best_dist, best = d, idx
        if best_dist <= TH_LOW:
            taken[best] = True
            out[p] = best
    return out
