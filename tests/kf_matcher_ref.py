"""Literal pure-Python restatements of ORBmatcher::SearchForTriangulation and ORBmatcher::Fuse(KeyFrame, points), float32 arithmetic spelled
out, shared by tests/test_oracle_kf_matcher.py, tests/test_kf_matcher_cases.py and the hand-built cases of tests/kf_matcher_cases.py.

Every literal takes rule=None (the reference behaviour) or the name of ONE deliberately altered decision rule. The altered variants exist
only to prove on the CPU that a hand-built case decides that rule (the output must change); nothing is ever compared against them."""
import numpy as np

POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
f32 = np.float32
TH_LOW, HISTO_LENGTH = 50, 30

TRIANGULATION_RULES = ("tie_first", "th_low_exclusive", "no_epipole_gate", "epipole_gate_always", "epipole_le", "sigma_of_kp1", "ignore_hp2",
                       "only_stereo_one_sided", "maxima_ge", "maxima_ratio_le")
FUSE_RULES = ("tie_last", "th_low_exclusive", "level_window_up", "chi_swapped", "no_behind_gate", "in_image_le", "no_min_offset", "no_distance_margin",
              "view_cos_0", "radius_le", "no_level_clamp")


def ham(a, b):
    return int(POP[np.bitwise_xor(a, b)].sum())


def three_maxima(cnt, rule=None):
    """ORBmatcher::ComputeThreeMaxima over the bin counts: the indices of the bins that are kept. Strict '>' lets the earlier of two equal
    bins stand; the one-tenth test is float32 (0.1f * (float)max1) and strict."""
    ge, ratio_le = rule == "maxima_ge", rule == "maxima_ratio_le"
    m1 = m2 = m3 = 0; i1 = i2 = i3 = -1
    over = (lambda s, m: s >= m) if ge else (lambda s, m: s > m)
    for i, s in enumerate(cnt):
        if over(s, m1):
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif over(s, m2):
            m3, m2, i3, i2 = m2, s, i2, i
        elif over(s, m3):
            m3, i3 = s, i
    tenth = f32(f32(0.1) * f32(m1))
    below = (lambda m: f32(m) <= tenth) if ratio_le else (lambda m: f32(m) < tenth)
    if below(m2):
        i2 = i3 = -1
    elif below(m3):
        i3 = -1
    return [i for i in (i1, i2, i3) if i >= 0]


def rotation_bin(a1, a2):
    rot = f32(f32(a1) - f32(a2))
    if rot < 0:
        rot = f32(rot + f32(360))
    bn = int(np.floor(float(f32(rot * f32(1.0 / HISTO_LENGTH))) + 0.5))
    return 0 if bn == HISTO_LENGTH else bn


def epipole(p):
    """The epipole of key frame 1's centre in key frame 2's image, in the float32 arithmetic of SearchForTriangulation."""
    R2, t2 = p["pose2"][:9].reshape(3, 3), p["pose2"][9:]
    C2 = np.array([f32(f32(f32(R2[r, 0] * p["Cw1"][0]) + f32(R2[r, 1] * p["Cw1"][1])) + f32(R2[r, 2] * p["Cw1"][2])) for r in range(3)], f32)
    C2 = (C2.astype(np.float64) + t2.astype(np.float64)).astype(f32)
    fx, fy, cx, cy = p["intr4"]
    with np.errstate(divide="ignore", invalid="ignore"):
        invz = f32(1.0) / C2[2]
        return f32(f32(f32(fx * C2[0]) * invz) + cx), f32(f32(f32(fy * C2[1]) * invz) + cy)


def epipolar_line(p, x1, y1):
    F = p["F12"].reshape(3, 3)
    a = f32(f32(f32(x1 * F[0, 0]) + f32(y1 * F[1, 0])) + F[2, 0]); b = f32(f32(f32(x1 * F[0, 1]) + f32(y1 * F[1, 1])) + F[2, 1])
    c = f32(f32(f32(x1 * F[0, 2]) + f32(y1 * F[1, 2])) + F[2, 2])
    return a, b, c


def epipole_dist2(ex, ey, x2, y2):
    dx, dy = f32(ex - x2), f32(ey - y2)
    return f32(f32(dx * dx) + f32(dy * dy))


def literal_triangulation(p, only_stereo, ori, rule=None):
    assert rule is None or rule in TRIANGULATION_RULES, rule
    k1, k2 = p["k1"], p["k2"]
    ex, ey = epipole(p)
    m12 = np.full(len(k1), -1, np.int64); hist = [[] for _ in range(HISTO_LENGTH)]; nm = 0
    for nd in sorted(set(int(x) for x in p["node1"] if x >= 0) & set(int(x) for x in p["node2"] if x >= 0)):
        for i1 in np.nonzero(p["node1"] == nd)[0]:
            if p["hp1"][i1]:
                continue
            s1 = p["ur1"][i1] >= 0
            if only_stereo and not s1:
                continue
            x1, y1 = k1["x"][i1], k1["y"][i1]
            a, b, c = epipolar_line(p, x1, y1)
            best, bi = TH_LOW, -1
            for i2 in np.nonzero(p["node2"] == nd)[0]:
                if p["hp2"][i2] and rule != "ignore_hp2":
                    continue
                s2 = p["ur2"][i2] >= 0
                if only_stereo and not s2 and rule != "only_stereo_one_sided":
                    continue
                d = ham(p["d1"][i1], p["d2"][i2])
                if rule == "th_low_exclusive" and d >= TH_LOW:
                    continue
                if d > TH_LOW or d > best or (rule == "tie_first" and d == best and bi >= 0):
                    continue
                x2, y2, o2 = k2["x"][i2], k2["y"][i2], k2["octave"][i2]
                if ((not s1 and not s2) or rule == "epipole_gate_always") and rule != "no_epipole_gate":
                    e2, lim = epipole_dist2(ex, ey, x2, y2), f32(f32(100) * p["sf"][o2])
                    if e2 < lim or (rule == "epipole_le" and e2 == lim):
                        continue
                num = f32(f32(f32(a * x2) + f32(b * y2)) + c); den = f32(f32(a * a) + f32(b * b))
                if den == 0:
                    continue
                osig = k1["octave"][i1] if rule == "sigma_of_kp1" else o2
                if float(f32(f32(num * num) / den)) < 3.84 * float(p["level_sigma2"][osig]):
                    bi, best = int(i2), d
            if bi >= 0:
                m12[i1] = bi; nm += 1
                if ori:
                    hist[rotation_bin(k1["angle"][i1], k2["angle"][bi])].append(int(i1))
    if ori:
        keep = three_maxima([len(hh) for hh in hist], rule)
        for bn in range(HISTO_LENGTH):
            if bn not in keep:
                for j in hist[bn]:
                    m12[j] = -1; nm -= 1
    return nm, m12


def fuse_geometry(p, X, intr5):
    """Projection of one world point into key frame 2 in Fuse's float32 arithmetic: pc[3], u, v, ur, PO[3], dist3D."""
    R, t = p["pose2"][:9].reshape(3, 3), p["pose2"][9:]
    fx, fy, cx, cy, bf = [f32(v) for v in intr5]
    X = np.asarray(X, f32)
    Ow = np.array([-f32(f32(f32(R[0, r] * t[0]) + f32(R[1, r] * t[1])) + f32(R[2, r] * t[2])) for r in range(3)], f32)
    pc = [f32((np.float64(f32(f32(f32(R[r, 0] * X[0]) + f32(R[r, 1] * X[1])) + f32(R[r, 2] * X[2]))) + np.float64(t[r]))) for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        invz = f32(1) / pc[2]
        u = f32(f32(fx * f32(pc[0] * invz)) + cx); v = f32(f32(fy * f32(pc[1] * invz)) + cy)
        ur = f32(u - f32(bf * invz))
    PO = (X - Ow).astype(f32)
    dist = f32(np.sqrt(np.float64(PO[0]) ** 2 + np.float64(PO[1]) ** 2 + np.float64(PO[2]) ** 2))
    return pc, u, v, ur, PO, dist


def predicted_level(maxd, dist, log_sf):
    return int(np.ceil(f32(f32(np.log(np.float64(f32(f32(maxd) / f32(dist))))) / f32(log_sf))))


def literal_fuse(p, pts_f, valid, desc, intr5, th, bounds4=(0.0, 752.0, 0.0, 480.0), nlevels=8, rule=None):
    """Pure-Python restatement of ORBmatcher::Fuse (float32 arithmetic spelled out; candidates in KeyFrame::GetFeaturesInArea order)."""
    assert rule is None or rule in FUSE_RULES, rule
    k2 = p["k2"]; n = len(k2)
    minX, maxX, minY, maxY = [f32(v) for v in bounds4]
    wInv, hInv = f32(64) / f32(maxX - minX), f32(48) / f32(maxY - minY)
    sf = np.concatenate([p["sf"][:nlevels], np.full(16 - nlevels, p["sf"][nlevels - 1], f32)]).astype(f32)       # the C ABI's 16-entry table
    # grid (Frame::AssignFeaturesToGrid: round() to cell, insertion order)
    grid = [[[] for _ in range(48)] for _ in range(64)]
    for i in range(n):
        gx = int(np.floor(float(f32(f32(k2["x"][i] - minX) * wInv)) + 0.5)); gy = int(np.floor(float(f32(f32(k2["y"][i] - minY) * hInv)) + 0.5))
        if 0 <= gx < 64 and 0 <= gy < 48:
            grid[gx][gy].append(i)
    log_sf = f32(np.log(np.float64(p["sf"][1])))
    out = np.full(len(pts_f), -1, np.int64)
    for i in range(len(pts_f)):
        if not valid[i]:
            continue
        X = pts_f[i, :3]; nrm = pts_f[i, 3:6]; mind, maxd = pts_f[i, 6], pts_f[i, 7]
        pc, u, v, ur, PO, dist = fuse_geometry(p, X, intr5)
        if pc[2] < 0 and rule != "no_behind_gate":
            continue
        if not (u >= minX and (u <= maxX if rule == "in_image_le" else u < maxX) and v >= minY and v < maxY):
            continue
        lo, hi = (f32(1.0), f32(1.0)) if rule == "no_distance_margin" else (f32(0.8), f32(1.2))
        if dist < f32(lo * mind) or dist > f32(hi * maxd):
            continue
        cos_lim = 0.0 if rule == "view_cos_0" else 0.5
        if float(np.float64(PO[0]) * nrm[0] + np.float64(PO[1]) * nrm[1] + np.float64(PO[2]) * nrm[2]) < cos_lim * float(dist):
            continue
        lvl = predicted_level(maxd, dist, log_sf)
        if rule != "no_level_clamp":
            lvl = 0 if lvl < 0 else (nlevels - 1 if lvl >= nlevels else lvl)
        r = f32(f32(th) * sf[min(max(lvl, 0), 15)])
        ou, ov = (u, v) if rule == "no_min_offset" else (f32(u - minX), f32(v - minY))
        x0 = max(0, int(np.floor(f32(f32(ou - r) * wInv)))); x1 = min(63, int(np.ceil(f32(f32(ou + r) * wInv))))
        y0 = max(0, int(np.floor(f32(f32(ov - r) * hInv)))); y1 = min(47, int(np.ceil(f32(f32(ov + r) * hInv))))
        if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
            continue
        best, bi = 256, -1
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for idx in grid[ix][iy]:
                    kx, ky, kl = k2["x"][idx], k2["y"][idx], int(k2["octave"][idx])
                    ax, ay = abs(f32(kx - u)), abs(f32(ky - v))
                    if not ((ax <= r and ay <= r) if rule == "radius_le" else (ax < r and ay < r)):
                        continue
                    if (kl < lvl or kl > lvl + 1) if rule == "level_window_up" else (kl < lvl - 1 or kl > lvl):
                        continue
                    ex, ey = f32(u - kx), f32(v - ky)
                    chi_stereo, chi_mono = (5.99, 7.8) if rule == "chi_swapped" else (7.8, 5.99)
                    if p["ur2"][idx] >= 0:
                        er = f32(ur - p["ur2"][idx])
                        e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                        if float(f32(e2 * p["inv_level_sigma2"][kl])) > chi_stereo:
                            continue
                    else:
                        e2 = f32(f32(ex * ex) + f32(ey * ey))
                        if float(f32(e2 * p["inv_level_sigma2"][kl])) > chi_mono:
                            continue
                    d = ham(desc[i], p["d2"][idx])
                    if d < best or (rule == "tie_last" and d == best):
                        best, bi = d, idx
        if best < TH_LOW or (best == TH_LOW and rule != "th_low_exclusive"):
            out[i] = bi
    return int((out >= 0).sum()), out
