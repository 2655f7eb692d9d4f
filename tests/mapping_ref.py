"""numpy restatement of map-point creation, the checker of tests/test_mapping_ref.py and tests/test_gpu_mapping*.py (never imported
by product code). Reference: LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1227-1483), KeyFrame::UnprojectStereo
(src/KeyFrame.cc:952-968), MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:249-314), MapPoint::UpdateNormalAndDepth (:337-378).

Two forms of the per-pair loop, vectorised over the pairs:
  mode "f32": op for op in the reference's float / double placement ("map-point creation" audit): every array is
              float32 except where cv::norm, Mat::dot, addWeighted, `1.0 / z` and cos(2 atan2) put a double. The SVD is LAPACK's
              float32 one (numpy.linalg.svd on a float32 array): a different algorithm from the library's Jacobi, so positions are
              compared with a tolerance, integer and decision outputs exactly outside the decision band.
  mode "f64": the definitional check: numpy.linalg.svd in double on the SAME float32 matrix A, everything else in double.

Every gate quantity is computed for every pair (no early exit), the reason code is derived afterwards in the reference's order. That
gives, per pair and per gate family (parallax cosine, depth, squared reprojection error, distance ratio), `margins`: the smallest
relative distance of a gate quantity from its threshold over the gates the pair actually reaches, |q - thr| / max(|q|, |thr|) (depth against 0: |z| / |Pw - Ow|; parallax cosine against 0: |cos|). A pair with a margin below
its family's band may flip between two correct float32 implementations."""
import numpy as np

ACCEPT, NO_POINT, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, SCALE, NO_PAIR = 0, 1, 2, 3, 4, 5, 6, 255

# Measured by tests/test_mapping_ref.py::test_float32_restatement_against_float64 over its parameter sets of make_mapping_problem
# (float32 restatement with LAPACK sgesdd against the float64 definitional check), rounded up; that test asserts that a fresh
# measurement does not exceed them and is not more than ten times below them.
#   POS_DEV_F32: largest |Pw_f32 - Pw_f64| / |Pw_f64| over the pairs both forms triangulate and accept.
#   GATE_DEV_F32[g]: largest relative deviation of gate quantity g between the two forms, relative to max(|q|, |threshold|) as in
#                    `margin` (depth: relative to the distance to the camera). One figure per quantity and not one for all four:
#                    the parallax cosine lives within 2e-4 of its 0.9998 threshold for every pair under 1.1 degrees of parallax,
#                    so the reprojection error's deviation (a thousand times the cosine's) used as the cosine's band would leave
#                    out most pairs of any test case.
POS_DEV_F32 = 1.6e-7
GATE_DEV_F32 = dict(cos=1.5e-7, depth=2.5e-5, reproj=3.0e-4, ratio=6.5e-7)
POS_TOL_GPU = 4 * POS_DEV_F32          # a different float32-output SVD: same order of backward error, other constants
DECISION_BAND = {g: 10 * v for g, v in GATE_DEV_F32.items()}
MAX_BAND_SHARE = 0.02                  # at most this share of the pairs of any test case may lie inside the band
GATES = ("cos", "depth", "reproj", "ratio")

# The parameter sets of make_mapping_problem the CPU and GPU tests share: (seed, J, key points per frame, stereo fraction).
PARAM_SETS = [(0, 20, 1000, 0.0), (0, 20, 1000, 0.4), (1, 20, 1000, 1.0), (0, 6, 2000, 0.0), (0, 6, 2000, 0.4), (0, 6, 2000, 1.0)]


def _rel(q, thr):
    q = np.asarray(q, np.float64); thr = np.asarray(thr, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(q - thr) / np.maximum(np.maximum(np.abs(q), np.abs(thr)), 1e-300)
    return np.where(np.isfinite(r), r, 0.0)


def _A_f32(T1, T2, xn1, xn2):
    """A.row(0) = xn1(0) * Tcw1.row(2) - Tcw1.row(0) ...: cv::addWeighted, (float)((double)a * alpha - (double)b)."""
    d = lambda a: np.asarray(a, np.float64)
    def Tcw(T):
        return np.concatenate([T[:9].reshape(3, 3), T[9:12].reshape(3, 1)], 1)          # [3][4]
    M1, M2 = d(Tcw(T1)), d(Tcw(T2))
    A = np.empty((len(xn1[0]), 4, 4), np.float32)
    A[:, 0, :] = (M1[2][None, :] * d(xn1[0])[:, None] - M1[0][None, :]).astype(np.float32)
    A[:, 1, :] = (M1[2][None, :] * d(xn1[1])[:, None] - M1[1][None, :]).astype(np.float32)
    A[:, 2, :] = (M2[2][None, :] * d(xn2[0])[:, None] - M2[0][None, :]).astype(np.float32)
    A[:, 3, :] = (M2[2][None, :] * d(xn2[1])[:, None] - M2[1][None, :]).astype(np.float32)
    return A


def triangulate_pairs(cam, kf1, kf2, match12, mode="f32"):
    """The per-pair loop for every i1 with match12[i1] >= 0. Returns dict(accept u8 [n1], reason u8 [n1], Pw [n1,3] float32 (f32) or
    float64 (f64), margins {gate family: [pairs]}, branch [n1] (0 none, 1 triangulated, 2 / 3 UnprojectStereo of key frame 1 / 2), q = dict of the gate
    quantities with their thresholds, as float64 arrays over the pairs, and idx1 = their i1)."""
    FT = np.float32 if mode == "f32" else np.float64
    f = lambda a: np.asarray(a, FT)
    d = lambda a: np.asarray(a, np.float64)
    f32 = lambda a: np.asarray(a, np.float32)
    n1 = len(kf1["kps"])
    match12 = np.asarray(match12)
    i1 = np.nonzero(match12 >= 0)[0]; i2 = match12[i1].astype(np.int64)
    out = dict(accept=np.zeros(n1, np.uint8), reason=np.full(n1, NO_PAIR, np.uint8), Pw=np.zeros((n1, 3), FT), margins={g: np.zeros(0) for g in GATES},
               branch=np.zeros(n1, np.uint8), idx1=i1, q={})
    if len(i1) == 0:
        return out
    fx, fy, cx, cy = [f(f32(v)) for v in cam["intr4"]]
    invfx, invfy = f(1) / fx, f(1) / fy
    if mode == "f32":
        invfx, invfy = f32(1) / f32(cam["intr4"][0]), f32(1) / f32(cam["intr4"][1])
    mb, mbf = f(f32(cam["mb"])), f(f32(cam["mbf"]))
    sf, sg2 = f32(cam["sf"]), f32(cam["level_sigma2"])
    T1f, T2f = f32(kf1["pose12"]), f32(kf2["pose12"])
    T1, T2, O1, O2 = f(T1f), f(T2f), f(f32(kf1["Ow"])), f(f32(kf2["Ow"]))
    u1, v1, o1 = f(kf1["kps"]["x"][i1]), f(kf1["kps"]["y"][i1]), kf1["kps"]["octave"][i1]
    u2, v2, o2 = f(kf2["kps"]["x"][i2]), f(kf2["kps"]["y"][i2]), kf2["kps"]["octave"][i2]
    ur1, ur2, z1s, z2s = f(kf1["ur"][i1]), f(kf2["ur"][i2]), f(kf1["depth"][i1]), f(kf2["depth"][i2])
    st1, st2 = ur1 >= 0, ur2 >= 0
    one = np.ones(len(i1), FT)
    xn1 = [(u1 - cx) * invfx, (v1 - cy) * invfy, one]
    xn2 = [(u2 - cx) * invfx, (v2 - cy) * invfy, one]
    ray = lambda T, xn: [T[r] * xn[0] + T[3 + r] * xn[1] + T[6 + r] * xn[2] for r in range(3)]       # Rwc * xn: float products, float sums
    dot3 = lambda a, b: (d(a[0]) * d(b[0]) + d(a[1]) * d(b[1])) + d(a[2]) * d(b[2])
    r1, r2 = ray(T1, xn1), ray(T2, xn2)
    with np.errstate(all="ignore"):
        cosr = f(dot3(r1, r2) / (np.sqrt(dot3(r1, r1)) * np.sqrt(dot3(r2, r2))))
        cs1 = cosr + f(1); cs2 = cs1.copy()
        half = mb / f(2)
        c1 = f(np.cos(2.0 * np.arctan2(d(half), d(z1s)))); c2 = f(np.cos(2.0 * np.arctan2(d(half), d(z2s))))
        cs1 = np.where(st1, c1, cs1); cs2 = np.where(~st1 & st2, c2, cs2)
        cs = np.minimum(cs1, cs2)
        tri = (cosr < cs) & (cosr > 0) & (st1 | st2 | (d(cosr) < 0.9998))
        us1 = ~tri & st1 & (cs1 < cs2)
        us2 = ~tri & ~us1 & st2 & (cs2 < cs1)
        # linear triangulation: the float32 A of the op-for-op form in both modes
        xa = [(f32(kf1["kps"]["x"][i1]) - f32(cam["intr4"][2])) * (f32(1) / f32(cam["intr4"][0])), (f32(kf1["kps"]["y"][i1]) - f32(cam["intr4"][3])) * (f32(1) / f32(cam["intr4"][1]))]
        xb = [(f32(kf2["kps"]["x"][i2]) - f32(cam["intr4"][2])) * (f32(1) / f32(cam["intr4"][0])), (f32(kf2["kps"]["y"][i2]) - f32(cam["intr4"][3])) * (f32(1) / f32(cam["intr4"][1]))]
        A = _A_f32(T1f, T2f, xa, xb)
        vt = np.linalg.svd(A.astype(FT))[2]
        x = vt[:, 3, :]
        w0 = x[:, 3] == 0
        Xt = f(d(x[:, :3]) / d(x[:, 3:4]))
        def unproject(T, O, ud, vd, z):
            xx = (ud - cx) * z * invfx; yy = (vd - cy) * z * invfy
            return np.stack([f(d(T[r] * xx + T[3 + r] * yy + T[6 + r] * z) + d(O[r])) for r in range(3)], 1)
        X1 = unproject(T1, O1, f(kf1["xy_dist"][i1, 0]), f(kf1["xy_dist"][i1, 1]), z1s)
        X2 = unproject(T2, O2, f(kf2["xy_dist"][i2, 0]), f(kf2["xy_dist"][i2, 1]), z2s)
        nopoint = (tri & w0) | (us1 & ~(z1s > 0)) | (us2 & ~(z2s > 0)) | ~(tri | us1 | us2)
        X = np.where(tri[:, None], Xt, np.where(us1[:, None], X1, X2))
        X = np.where(nopoint[:, None], f(0), X)
        Xc = [X[:, 0], X[:, 1], X[:, 2]]
        camc = lambda T, r: f(dot3([T[3 * r] * one, T[3 * r + 1] * one, T[3 * r + 2] * one], Xc) + d(T[9 + r]))
        def view(T, u, v, ur, st, o, z):
            xx, yy = camc(T, 0), camc(T, 1)
            invz = f(1.0 / d(z))
            uu = fx * xx * invz + cx; vv = fy * yy * invz + cy
            ex, ey = uu - u, vv - v
            er = (uu - mbf * invz) - ur
            e = np.where(st, ex * ex + ey * ey + er * er, ex * ex + ey * ey)
            thr = np.where(st, 7.8, 5.991) * d(sg2[np.clip(o, 0, 15 if len(sg2) > 15 else len(sg2) - 1)])
            return e, thr
        zc1, zc2 = camc(T1, 2), camc(T2, 2)
        e1, thr1 = view(T1, u1, v1, ur1, st1, o1, zc1)
        e2, thr2 = view(T2, u2, v2, ur2, st2, o2, zc2)
        nrm = lambda O: f(np.sqrt(dot3([Xc[k] - O[k] for k in range(3)], [Xc[k] - O[k] for k in range(3)])))
        dist1, dist2 = nrm(O1), nrm(O2)
        ratio_d = dist2 / dist1
        lv = len(sf) - 1
        ratio_o = f(sf[np.clip(o1, 0, lv)] / sf[np.clip(o2, 0, lv)])
        rf = f(f32(1.5) * f32(cam["scale_factor"]))
        sc_lo, sc_hi = ratio_d * rf, ratio_o * rf
        bad_scale = (dist1 == 0) | (dist2 == 0) | (sc_lo < ratio_o) | (ratio_d > sc_hi)
        reason = np.full(len(i1), ACCEPT, np.uint8)
        for code, cond in ((SCALE, bad_scale), (REPROJ_2, d(e2) > thr2), (REPROJ_1, d(e1) > thr1), (BEHIND_2, ~(zc2 > 0)), (BEHIND_1, ~(zc1 > 0)),
                           (NO_POINT, nopoint)):
            reason = np.where(cond, code, reason).astype(np.uint8)
        # margins: per gate family, over the gates the pair reaches (inf where it does not reach them)
        mono = ~(st1 | st2)
        m_par = np.minimum(_rel(cosr, cs), np.abs(d(cosr)))
        m_par = np.where(mono, np.minimum(m_par, _rel(cosr, 0.9998)), np.minimum(m_par, _rel(cs1, cs2)))
        m_z1 = np.abs(d(zc1)) / np.maximum(d(dist1), 1e-300); m_z2 = np.abs(d(zc2)) / np.maximum(d(dist2), 1e-300)
        m_e1, m_e2 = _rel(e1, thr1), _rel(e2, thr2)
        m_sc = np.minimum(_rel(sc_lo, ratio_o), _rel(ratio_d, sc_hi))
        reach = lambda code: (reason == ACCEPT) | (reason >= code)
        fin = lambda m: np.where(np.isfinite(m), m, 0.0)
        inf = np.inf
        margins = dict(cos=fin(m_par),
                       depth=np.minimum(np.where(reach(BEHIND_1), fin(m_z1), inf), np.where(reach(BEHIND_2), fin(m_z2), inf)),
                       reproj=np.minimum(np.where(reach(REPROJ_1), fin(m_e1), inf), np.where(reach(REPROJ_2), fin(m_e2), inf)),
                       ratio=np.where(reach(SCALE), fin(m_sc), inf))
    out["reason"][i1] = reason; out["accept"][i1] = reason == ACCEPT
    out["Pw"][i1] = X; out["margins"] = margins
    out["branch"][i1] = np.where(nopoint, 0, np.where(tri, 1, np.where(us1, 2, 3)))
    out["q"] = dict(cos=(d(cosr), d(cs)), z1=(d(zc1), d(dist1)), z2=(d(zc2), d(dist2)), e1=(d(e1), thr1), e2=(d(e2), thr2),
                    sc_lo=(d(sc_lo), d(ratio_o)), sc_hi=(d(ratio_d), d(sc_hi)))
    return out


def in_band(r, band=None):
    """[n1] bool: the pair of i1 has a reached gate quantity within the decision band of its threshold."""
    band = DECISION_BAND if band is None else band
    out = np.zeros(len(r["reason"]), bool)
    hit = np.zeros(len(r["idx1"]), bool)
    for g in GATES:
        if len(r["margins"][g]):
            hit |= r["margins"][g] < band[g]
    out[r["idx1"]] = hit
    return out


def gate_deviation(r32, r64):
    """({gate family: largest relative deviation of its quantities between two results over the same pairs}, [relative position
    deviations of the pairs both accept]). Only pairs that take the same branch in both and reach the gate in r64 count."""
    i1 = r32["idx1"]
    same = (r32["branch"][i1] == r64["branch"][i1]) & (r64["branch"][i1] > 0)
    rs = r64["reason"][i1]
    worst = {g: 0.0 for g in GATES}
    order = dict(cos=(NO_POINT, "cos"), z1=(BEHIND_1, "depth"), z2=(BEHIND_2, "depth"), e1=(REPROJ_1, "reproj"), e2=(REPROJ_2, "reproj"),
                 sc_lo=(SCALE, "ratio"), sc_hi=(SCALE, "ratio"))
    for name, (code, fam) in order.items():
        qa, ta = r32["q"][name]; qb, tb = r64["q"][name]
        reached = same & ((rs == ACCEPT) | (rs >= code))
        with np.errstate(all="ignore"):
            if fam == "depth":
                dev = np.abs(qa - qb) / np.maximum(tb, 1e-300)
            else:
                dev = np.abs(qa - qb) / np.maximum(np.maximum(np.abs(qb), np.abs(tb)), 1e-300)
        dev = np.where(reached & np.isfinite(dev), dev, 0.0)
        worst[fam] = max(worst[fam], float(dev.max(initial=0.0)))
    both = (r32["accept"][i1] == 1) & (r64["accept"][i1] == 1) & same
    P32, P64 = r32["Pw"][i1][both].astype(np.float64), r64["Pw"][i1][both].astype(np.float64)
    pos = np.linalg.norm(P32 - P64, axis=1) / np.linalg.norm(P64, axis=1) if both.any() else np.zeros(0)
    return worst, pos


def hamming_matrix(D):
    D = np.ascontiguousarray(D, np.uint8)
    x = D[:, None, :] ^ D[None, :, :]
    return np.unpackbits(x, axis=2).sum(2).astype(np.int32)


def map_point_update(obs_kf, obs_feat, ref_obs, Pw, kf_desc, kf_octave, kf_Ow, sf):
    """One point: observations (key frame, feature) in map order. kf_desc[k] [n,32], kf_octave[k] [n], kf_Ow[k] [3].
    Returns (descriptor [32], best_obs, pts_f [8] float32) by the literal sort-and-take rule of MapPoint.cc:295-308."""
    f32 = np.float32
    N = len(obs_kf)
    Pw = np.asarray(Pw, f32)
    if N == 0:
        return np.zeros(32, np.uint8), -1, np.concatenate([Pw, np.zeros(5, f32)])
    D = np.stack([kf_desc[k][i] for k, i in zip(obs_kf, obs_feat)])
    H = hamming_matrix(D)
    best, best_median = 0, 2 ** 31 - 1
    for i in range(N):
        median = int(np.sort(H[i])[int(0.5 * (N - 1))])
        if median < best_median:
            best_median, best = median, i
    normal = np.zeros(3, f32)
    for k in obs_kf:
        dlt = Pw - np.asarray(kf_Ow[k], f32)
        nrm = np.sqrt((dlt.astype(np.float64) ** 2)[0] + (dlt.astype(np.float64) ** 2)[1] + (dlt.astype(np.float64) ** 2)[2])
        normal = normal + (dlt.astype(np.float64) / nrm).astype(f32)
    kr, ir = obs_kf[ref_obs], obs_feat[ref_obs]
    dlt = (Pw - np.asarray(kf_Ow[kr], f32)).astype(np.float64)
    dist = f32(np.sqrt(dlt[0] * dlt[0] + dlt[1] * dlt[1] + dlt[2] * dlt[2]))
    sf = np.asarray(sf, f32)
    maxd = f32(dist * sf[int(kf_octave[kr][ir])]); mind = f32(maxd / sf[len(sf) - 1])
    nv = (normal.astype(np.float64) / float(N)).astype(f32)
    return D[best].copy(), best, np.array([Pw[0], Pw[1], Pw[2], nv[0], nv[1], nv[2], mind, maxd], f32)


def baseline_skips(cam, kf1, kf2, monocular):
    """src/LocalMapping.cc:1272-1289."""
    f32 = np.float32
    dlt = (np.asarray(kf2["Ow"], f32) - np.asarray(kf1["Ow"], f32)).astype(np.float64)
    baseline = f32(np.sqrt(dlt[0] * dlt[0] + dlt[1] * dlt[1] + dlt[2] * dlt[2]))
    if not monocular:
        return bool(baseline < f32(cam["mb"]))
    return bool(np.float64(f32(baseline / f32(kf2["median_depth"]))) < 0.01)


def create_new_map_points(problem, search, monocular, j_list=None, has_point1=None, band=None, mode="f32"):
    """The reference's sequential loop over the neighbours. `search(kf1, hp1, kf2)` -> match12 is the SearchForTriangulation to use
    (the CPU oracle's in the tests). Returns dict(new_idx [n,3], pts_f [n,8], desc [n,32], has_point1, uncertain_i1 = the set of i1
    whose pair lay inside the decision band for some neighbour (their later history may legitimately differ), Pw64 = the float64 definitional position of every created point, per_neighbour)."""
    cam, kf1 = problem["cam"], problem["kf1"]
    hp1 = np.array(problem["kf1"]["hp"] if has_point1 is None else has_point1, np.uint8)
    idx, pts, desc, unc, per, P64 = [], [], [], set(), [], []
    for j in (range(len(problem["neigh"])) if j_list is None else j_list):
        kf2 = problem["neigh"][j]
        if baseline_skips(cam, kf1, kf2, monocular):
            per.append(None); continue
        m12 = search(kf1, hp1, kf2)
        r = triangulate_pairs(cam, kf1, kf2, m12, mode)
        per.append((m12, r))
        r64 = triangulate_pairs(cam, kf1, kf2, m12, "f64")
        if band is not False:
            unc.update(int(i) for i in np.nonzero(in_band(r, band))[0])
        for i1 in np.nonzero(r["accept"])[0]:
            i2 = int(m12[i1])
            first, second = ((kf2, i2), (kf1, i1)) if kf2["kf2_first"] else ((kf1, i1), (kf2, i2))
            P = r["Pw"][i1].astype(np.float32)
            dsc, _, pf = map_point_update([0, 1], [first[1], second[1]], 1 if kf2["kf2_first"] else 0, P, [first[0]["desc"], second[0]["desc"]],
                                          [first[0]["kps"]["octave"], second[0]["kps"]["octave"]], [first[0]["Ow"], second[0]["Ow"]], cam["sf"])
            idx.append((int(i1), j, i2)); pts.append(pf); desc.append(dsc); P64.append(r64["Pw"][i1])
            hp1[i1] = 1
    return dict(new_idx=np.array(idx, np.int32).reshape(-1, 3), pts_f=np.array(pts, np.float32).reshape(-1, 8), desc=np.array(desc, np.uint8).reshape(-1, 32),
                has_point1=hp1, uncertain_i1=unc, per_neighbour=per, Pw64=np.array(P64, np.float64).reshape(-1, 3))
