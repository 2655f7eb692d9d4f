"""numpy restatement (float32, with the reference's casts) of ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520),
Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea (src/Frame.cc:410-425, 562-572, 507-560), ORBmatcher::ComputeThreeMaxima
(:1602-1643) and KeyFrame::ComputeSceneMedianDepth (src/KeyFrame.cc:970-1000), as literal loops written from the reference's text. The
checker of tests/test_search_init_ref.py and tests/test_gpu_search_init.py; product code never imports it.

Casts: the cell rectangle is float arithmetic with floor / ceil (a value no int holds converts as x86 converts it, to INT_MIN); PosInGrid
is C round (half away from zero); the ratio test is the float product (float)bestDist2 * mfNNratio compared with (float)bestDist; the bin
is round(rot * (1.0f / 30)) of a float product; a depth is Mat::dot in double plus zcw, stored to float."""
import numpy as np

f32, f64 = np.float32, np.float64
MATCHED, NOT_CANDIDATE, NO_FEATURE_IN_WINDOW, ABOVE_THRESHOLD, RATIO, DISPLACED, ROTATION = range(7)
REASON_NAMES = ("MATCHED", "NOT_CANDIDATE", "NO_FEATURE_IN_WINDOW", "ABOVE_THRESHOLD", "RATIO", "DISPLACED", "ROTATION")
TH_LOW, HISTO_LENGTH = 50, 30
COLS, ROWS = 64, 48
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def _round_half_away(x):
    x = f64(x)
    return int(np.sign(x) * np.floor(np.abs(x) + 0.5))


def _to_int(q):
    """(int) of a float as x86 converts it."""
    q = f64(q)
    return int(q) if -2147483648.0 < q < 2147483648.0 else INT_MIN


class Frame:
    """mvKeysUn, mDescriptors, the image bounds and mGrid (AssignFeaturesToGrid: push_back in key-point order)."""

    def __init__(self, kps, desc, bounds4):
        self.kps, self.desc, self.N = kps, np.asarray(desc, np.uint8).reshape(-1, 32), len(kps)
        self.minX, self.maxX, self.minY, self.maxY = [f32(v) for v in bounds4]
        self.wInv = f32(COLS) / f32(self.maxX - self.minX)
        self.hInv = f32(ROWS) / f32(self.maxY - self.minY)
        self.x, self.y = np.asarray(kps["x"], f32), np.asarray(kps["y"], f32)
        self.octave, self.angle = np.asarray(kps["octave"], np.int64), np.asarray(kps["angle"], f32)
        self.grid = [[[] for _ in range(ROWS)] for _ in range(COLS)]
        for i in range(self.N):
            px = _round_half_away((self.x[i] - self.minX) * self.wInv)           # PosInGrid :564-565
            py = _round_half_away((self.y[i] - self.minY) * self.hInv)
            if px < 0 or px >= COLS or py < 0 or py >= ROWS:
                continue
            self.grid[px][py].append(i)

    def csr(self):
        """cell_start [64*48+1], cell_idx [features inside the grid] in storage order ix*48 + iy."""
        start, idx = [0], []
        for ix in range(COLS):
            for iy in range(ROWS):
                idx += self.grid[ix][iy]
                start.append(len(idx))
        return np.array(start, np.int32), np.array(idx, np.int32)

    def cell_rect(self, x, y, r):
        """(nMinCellX, nMaxCellX, nMinCellY, nMaxCellY) as far as :512-526 computes them (-1 / 0 placeholders), and whether it returned early."""
        x, y, r = f32(x), f32(y), f32(r)
        with np.errstate(all="ignore"):
            x0 = max(0, _to_int(np.floor((x - self.minX - r) * self.wInv)))
            if x0 >= COLS:
                return (x0, -1, 0, -1), True
            x1 = min(COLS - 1, _to_int(np.ceil((x - self.minX + r) * self.wInv)))
            if x1 < 0:
                return (x0, x1, 0, -1), True
            y0 = max(0, _to_int(np.floor((y - self.minY - r) * self.hInv)))
            if y0 >= ROWS:
                return (x0, x1, y0, -1), True
            y1 = min(ROWS - 1, _to_int(np.ceil((y - self.minY + r) * self.hInv)))
            if y1 < 0:
                return (x0, x1, y0, y1), True
        return (x0, x1, y0, y1), False

    def features_in_area(self, x, y, r, min_level=-1, max_level=-1):
        """GetFeaturesInArea :507-560."""
        x, y, r = f32(x), f32(y), f32(r)
        (x0, x1, y0, y1), early = self.cell_rect(x, y, r)
        out = []
        if early:
            return out
        check_levels = (min_level > 0) or (max_level >= 0)
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for j in self.grid[ix][iy]:
                    if check_levels:
                        if self.octave[j] < min_level:
                            continue
                        if max_level >= 0 and self.octave[j] > max_level:
                            continue
                    if abs(f32(self.x[j] - x)) < r and abs(f32(self.y[j] - y)) < r:
                        out.append(j)
        return out


def rot_bin(a1, a2):
    """:475-480."""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = _round_half_away(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))
    if b == HISTO_LENGTH:
        b = 0
    assert 0 <= b < HISTO_LENGTH
    return b


def three_maxima(sizes):
    """ComputeThreeMaxima :1602-1643 over the bins' sizes: (ind1, ind2, ind3)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif max3 < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def candidate_lists(F1, F2, prev_matched, window_size):
    """Per point of frame 1: None where :422 skips it, else [(distance, feature), ...] in GetFeaturesInArea order."""
    pm = np.asarray(prev_matched, f32).reshape(-1, 2)
    out = []
    for i1 in range(F1.N):
        level1 = int(F1.octave[i1])
        if level1 > 0:
            out.append(None)
            continue
        out.append([(hamming(F1.desc[i1], F2.desc[i2]), i2) for i2 in F2.features_in_area(pm[i1, 0], pm[i1, 1], f32(window_size), level1, level1)])
    return out


def search_for_initialization(F1, F2, prev_matched, window_size=100, nnratio=0.9, check_orientation=True, skip_rule=True, lists=None):
    """:405-520. skip_rule=False is the same loop without :444 (the order-free result the fixture is measured against). `lists`: the
    candidate lists, when the caller has them. dict(matches12, nmatches, prev_matched, matches21, matched_distance, rot_hist, reason,
    ties): ties = points whose loop met a candidate at exactly the best distance so far."""
    nnratio = f32(nnratio)
    pm = np.array(prev_matched, f32, copy=True).reshape(-1, 2)
    matches12 = np.full(F1.N, -1, np.int32)
    nmatches = 0
    rot = [[] for _ in range(HISTO_LENGTH)]
    dist21 = np.full(F2.N, INT_MAX, np.int32)
    matches21 = np.full(F2.N, -1, np.int32)
    reason = np.full(F1.N, NOT_CANDIDATE, np.int32)
    lists = candidate_lists(F1, F2, pm, window_size) if lists is None else lists
    ties = 0
    for i1 in range(F1.N):
        if lists[i1] is None:
            continue
        if not lists[i1]:
            reason[i1] = NO_FEATURE_IN_WINDOW
            continue
        best, best2, idx2, tie = INT_MAX, INT_MAX, -1, False
        for dist, i2 in lists[i1]:
            if skip_rule and dist21[i2] <= dist:
                continue
            if dist < best:
                best2, best, idx2 = best, dist, i2
            else:
                tie |= dist == best
                if dist < best2:
                    best2 = dist
        ties += tie
        if not best <= TH_LOW:
            reason[i1] = ABOVE_THRESHOLD
            continue
        if not f32(best) < f32(f32(best2) * nnratio):
            reason[i1] = RATIO
            continue
        if matches21[idx2] >= 0:
            matches12[matches21[idx2]] = -1
            reason[matches21[idx2]] = DISPLACED
            nmatches -= 1
        matches12[i1] = idx2
        matches21[idx2] = i1
        dist21[idx2] = best
        nmatches += 1
        reason[i1] = MATCHED
        if check_orientation:
            rot[rot_bin(F1.angle[i1], F2.angle[idx2])].append(i1)
    rot_hist = np.array([len(b) for b in rot], np.int32)
    if check_orientation:
        keep = three_maxima(rot_hist)
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for i1 in rot[i]:
                if matches12[i1] >= 0:
                    matches12[i1] = -1
                    reason[i1] = ROTATION
                    nmatches -= 1
    for i1 in range(F1.N):
        if matches12[i1] >= 0:
            pm[i1] = (F2.x[matches12[i1]], F2.y[matches12[i1]])
    return dict(matches12=matches12, nmatches=nmatches, prev_matched=pm, matches21=matches21, matched_distance=dist21, rot_hist=rot_hist, reason=reason,
                ties=ties)


def chain_bound(lists):
    """The ordered phase's sweep bound: 1 + the longest chain p_1 < p_2 < ... in which consecutive points share a candidate feature."""
    depth_of_feature, longest = {}, 0
    for lst in lists:
        if not lst:
            continue
        fs = set(f for _, f in lst)
        d = 1 + max([depth_of_feature.get(f, 0) for f in fs])
        for f in fs:
            depth_of_feature[f] = d
        longest = max(longest, d)
    return longest + 1


def scene_depth(pose12, X):
    """:992: Rcw2.dot(x3Dw) + zcw in double, stored to float."""
    p, X = np.asarray(pose12, f32).astype(f64), np.asarray(X, f32).astype(f64)
    return f32(((p[6] * X[0] + p[7] * X[1]) + p[8] * X[2]) + p[11])


def scene_median_depth(pose12, points, has_point, q=2):
    """:970-1000: (vDepths[(size - 1) / q] after the sort, size); (-1, 0) where the reference indexes an empty vector."""
    d = sorted(scene_depth(pose12, X) for X, h in zip(np.asarray(points, f32).reshape(-1, 3), has_point) if h)
    if not d:
        return f32(-1.0), 0
    return f32(d[(len(d) - 1) // q]), len(d)
