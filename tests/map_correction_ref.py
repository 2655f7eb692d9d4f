"""Numpy checker of the map correction of loop closing, written as the literal ordered loops of the reference: the propagation of
LoopClosing::CorrectLoop (src/LoopClosing.cc:460-542) with KeyFrame::SetPose (src/KeyFrame.cc:361-375), MapPoint::UpdateNormalAndDepth
(src/MapPoint.cc:337-378), g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) and Converter::toCvMat(g2o::Sim3) (src/Converter.cc:93-99).

Every statement is a scalar one in the reference's type and order: np.float32 scalars where the reference holds a CV_32F matrix, Python
floats (IEEE double) where it holds Eigen doubles; no vectorised sums. The state the loops change (the key frames' centres, the points) is
changed in place, in the order the loops change it, so that UpdateNormalAndDepth of a point sees exactly the key frames that SetPose has
reached. std::map<KeyFrame*, ...> is walked in ascending key: the position of a slot in kf_by_key. A scene is what
viorb_amd.map_correction.scene_from_lists returns; the result has the fields of viorb_correct_loop_result for that stream."""
import math
import numpy as np

f32 = np.float32
OK, INVALID = 0, -1
FIELDS = ("n_member", "member_kf", "Scw_f12", "Scw_out", "Smeas_out", "pose12_out", "Ow_out", "pts_f_out", "pt_corrected_by_out", "pt_corrected_ref_out", "pt_touched")
# the situations a random set must hold (tests/test_map_correction_ref.py counts them)
EVENTS = ("two-members", "twice-in-member", "already-corrected", "bad-point", "null-keypoint", "no-observations", "observer-below", "observer-equal",
          "observer-above", "observer-not-member", "ref-below", "ref-not-below", "scale-not-1", "mat2q-trace", "mat2q-x", "mat2q-y", "mat2q-z", "empty-list", "no-points")


# ---- Eigen / g2o in double -------------------------------------------------------------------------------------------------------------------
def mat2q(m, events=None):
    """Eigen::Quaterniond(Matrix3d) (x, y, z, w), its four branches."""
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        s = math.sqrt(t + 1.0); r = 0.5 / s
        _count(events, "mat2q-trace")
        return ((m[2][1] - m[1][2]) * r, (m[0][2] - m[2][0]) * r, (m[1][0] - m[0][1]) * r, 0.5 * s)
    if m[0][0] >= m[1][1] and m[0][0] >= m[2][2]:
        s = math.sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0); r = 0.5 / s
        _count(events, "mat2q-x")
        return (0.5 * s, (m[1][0] + m[0][1]) * r, (m[2][0] + m[0][2]) * r, (m[2][1] - m[1][2]) * r)
    if m[1][1] > m[0][0] and m[1][1] >= m[2][2]:
        s = math.sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0); r = 0.5 / s
        _count(events, "mat2q-y")
        return ((m[1][0] + m[0][1]) * r, 0.5 * s, (m[2][1] + m[1][2]) * r, (m[0][2] - m[2][0]) * r)
    s = math.sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0); r = 0.5 / s
    _count(events, "mat2q-z")
    return ((m[0][2] + m[2][0]) * r, (m[2][1] + m[1][2]) * r, 0.5 * s, (m[1][0] - m[0][1]) * r)


def qmat(q):
    """Quaterniond::toRotationMatrix (no normalisation)."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def qmul(a, b):
    return (a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2])


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def qrot(q, v):
    """Quaterniond * Vector3d: v + w * (2 qv x v) + qv x (2 qv x v)."""
    qv = q[:3]
    uv = cross(qv, v)
    uv = (uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2])
    c = cross(qv, uv)
    return (v[0] + uv[0] * q[3] + c[0], v[1] + uv[1] * q[3] + c[1], v[2] + uv[2] * q[3] + c[2])


def sim3_mul(a, b):
    """Sim3::operator*: r = ra rb, t = sa (ra tb) + ta, s = sa sb. A Sim3 is (r, t, s)."""
    ra, ta, sa = a; rb, tb, sb = b
    x = qrot(ra, tb)
    return (qmul(ra, rb), (x[0] * sa + ta[0], x[1] * sa + ta[1], x[2] * sa + ta[2]), sa * sb)


def sim3_inv(a):
    r, t, s = a
    rc = (-r[0], -r[1], -r[2], r[3])
    k = -1. / s
    return (rc, qrot(rc, (t[0] * k, t[1] * k, t[2] * k)), 1. / s)


def sim3_map(a, p):
    r, t, s = a
    x = qrot(r, p)
    return (x[0] * s + t[0], x[1] * s + t[1], x[2] * s + t[2])


def sim3_row(a):
    return [a[0][0], a[0][1], a[0][2], a[0][3], a[1][0], a[1][1], a[1][2], a[2]]


# ---- OpenCV in float -------------------------------------------------------------------------------------------------------------------------
def camera_centre(T):
    """SetPose: Rwc = Rcw.t(), Ow = -Rwc * tcw: three float products summed left to right."""
    return [((-T[r]) * T[9] + (-T[3 + r]) * T[10]) + (-T[6 + r]) * T[11] for r in range(3)]


def norm3(d):
    """cv::norm of a CV_32F 3-vector: the squares accumulate in double."""
    return math.sqrt((float(d[0]) * float(d[0]) + float(d[1]) * float(d[1])) + float(d[2]) * float(d[2]))


def sim3_of_pose(R9, t3, events=None):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0)."""
    return (mat2q([[float(R9[3 * r + c]) for c in range(3)] for r in range(3)], events), (float(t3[0]), float(t3[1]), float(t3[2])), 1.0)


def _count(events, what, n=1):
    if events is not None:
        events[what] = events.get(what, 0) + n


def update_normal_and_depth(s, rank, P8, Ow, p, sf, nlevels, claimer=None, members=(), events=None):
    """MapPoint::UpdateNormalAndDepth of point p on the state as it stands (Ow: the key frames' centres now). claimer / members only
    count the situations."""
    words = [int(w) for w in s["obs"][s["obs_start"][p]:s["obs_start"][p + 1]]]
    if not words:                                                       # :352
        _count(events, "no-observations")
        return
    observations = sorted(words, key=lambda w: rank[w & 0xffff])        # std::map<KeyFrame*, size_t>: ascending key (stable where a slot repeats)
    Pos = P8[p][0:3]
    normal = [f32(0), f32(0), f32(0)]
    n = 0
    for w in observations:
        k = w & 0xffff
        Owi = Ow[k]
        normali = [Pos[i] - Owi[i] for i in range(3)]
        nrm = norm3(normali)
        normal = [normal[i] + f32(float(normali[i]) / nrm) for i in range(3)]
        n += 1
        if claimer is not None:
            _count(events, "observer-not-member" if k not in members else "observer-below" if rank[k] < rank[claimer] else "observer-equal" if k == claimer else "observer-above")
    ref = int(s["pt_ref"][p])
    if claimer is not None:
        _count(events, "ref-below" if ref in members and rank[ref] < rank[claimer] else "ref-not-below")
    PC = [Pos[i] - Ow[ref][i] for i in range(3)]
    dist = f32(norm3(PC))
    level = next((w >> 16) & 0xff for w in words if (w & 0xffff) == ref)     # mvKeysUn[observations[pRefKF]].octave
    mfMaxDistance = dist * sf[min(level, 15)]
    mfMinDistance = mfMaxDistance / sf[nlevels - 1]
    P8[p][7], P8[p][6] = mfMaxDistance, mfMinDistance
    for i in range(3):
        P8[p][3 + i] = f32(float(normal[i]) / float(n))


def correct_loop(s, sf=None, nlevels=8, events=None):
    """LoopClosing.cc:460-542 on one scene. sf: mvScaleFactors float32 [16] (default 1.2^i in float32)."""
    if sf is None:
        sf = [f32(1.0)]
        for _ in range(15):
            sf.append(f32(sf[-1] * f32(1.2)))
    sf = [f32(v) for v in sf]
    nk, np_ = len(s["kf_by_key"]), len(s["pt_bad"])
    rank = {int(k): j for j, k in enumerate(s["kf_by_key"])}
    cur, cur_id = int(s["cur_kf"]), int(s["cur_id"])
    Tcw = [[f32(v) for v in s["pose12"][k]] for k in range(nk)]
    Ow = [camera_centre(T) for T in Tcw]                                # every key frame's SetPose so far
    P8 = [[f32(v) for v in row] for row in s["pts_f"]]
    by = [int(v) for v in s["pt_corrected_by"]]
    cref, touched = [-1] * np_, [0] * np_
    Scw = (tuple(float(v) for v in s["Scw8"][0:4]), tuple(float(v) for v in s["Scw8"][4:7]), float(s["Scw8"][7]))
    _count(events, "scale-not-1", int(Scw[2] != 1.0))
    connected = [int(k) for k in s["conn"]] + [cur]                     # :461-462
    _count(events, "empty-list", int(len(connected) == 1))
    _count(events, "no-points", int(np_ == 0))
    Corrected, NonCorrected = {cur: Scw}, {}                           # :464-465
    Twc_R = [[Tcw[cur][3 * c + k] for c in range(3)] for k in range(3)]         # GetPoseInverse (:466): Rwc[k][c] = Rcw[c][k]
    Twc_t = Ow[cur]
    zero, one = f32(0), f32(1)
    for i in connected:                                                 # :473-495
        T = Tcw[i]
        if i != cur:
            # Tic = Tiw * Twc: 4 x 4 float, four products per entry summed left to right; Twc's last row is 0 0 0 1
            Ric = [((T[3 * r] * Twc_R[0][c] + T[3 * r + 1] * Twc_R[1][c]) + T[3 * r + 2] * Twc_R[2][c]) + T[9 + r] * zero for r in range(3) for c in range(3)]
            tic = [((T[3 * r] * Twc_t[0] + T[3 * r + 1] * Twc_t[1]) + T[3 * r + 2] * Twc_t[2]) + T[9 + r] * one for r in range(3)]
            Corrected[i] = sim3_mul(sim3_of_pose(Ric, tic, events), Scw)
        NonCorrected[i] = sim3_of_pose(T[0:9], T[9:12], events)
    order = sorted(Corrected, key=lambda k: rank[k])                    # the iteration of std::map<KeyFrame*, g2o::Sim3>
    pose_out = [list(T) for T in Tcw]
    seen_in_member = {}
    for i in order:                                                     # :498-542
        Siw_c = Corrected[i]
        Swi_c = sim3_inv(Siw_c)
        Siw = NonCorrected[i]
        here = set()
        for p in (int(v) for v in s["kp_point"][s["kp_start"][i]:s["kp_start"][i + 1]]):
            if p < 0:
                _count(events, "null-keypoint")
                continue
            if s["pt_bad"][p]:
                _count(events, "bad-point")
                continue
            if p in here:
                _count(events, "twice-in-member")
            here.add(p)
            if by[p] == cur_id:
                if touched[p] and seen_in_member.get(p) != i:
                    _count(events, "two-members")
                elif not touched[p]:
                    _count(events, "already-corrected")
                continue
            seen_in_member[p] = i
            q = sim3_map(Swi_c, sim3_map(Siw, (float(P8[p][0]), float(P8[p][1]), float(P8[p][2]))))
            P8[p][0], P8[p][1], P8[p][2] = f32(q[0]), f32(q[1]), f32(q[2])
            by[p], cref[p], touched[p] = cur_id, i, 1
            update_normal_and_depth(s, rank, P8, Ow, p, sf, nlevels, claimer=i, members=Corrected, events=events)
        R = qmat(Siw_c[0])                                              # :530-538
        k = 1. / Siw_c[2]
        t = (Siw_c[1][0] * k, Siw_c[1][1] * k, Siw_c[1][2] * k)
        pose_out[i] = [f32(R[r][c]) for r in range(3) for c in range(3)] + [f32(t[0]), f32(t[1]), f32(t[2])]
        Ow[i] = camera_centre(pose_out[i])                              # SetPose
    res = dict(status=OK, n_member=len(order), member_kf=np.array(order, np.int32))
    f12 = []
    for i in order:                                                     # Converter::toCvMat(Sim3): the top three rows of [s * R | t]
        R, sc = qmat(Corrected[i][0]), Corrected[i][2]
        f12.append([f32(R[r][c] * sc) if c < 3 else f32(Corrected[i][1][r]) for r in range(3) for c in range(4)])
    res["Scw_f12"] = np.array(f12, np.float32).reshape(len(order), 12)
    Sm = [NonCorrected[k] if k in NonCorrected else sim3_of_pose(Tcw[k][0:9], Tcw[k][9:12]) for k in range(nk)]
    res["Smeas_out"] = np.array([sim3_row(a) for a in Sm], np.float64).reshape(nk, 8)
    res["Scw_out"] = np.array([sim3_row(Corrected[k] if k in Corrected else Sm[k]) for k in range(nk)], np.float64).reshape(nk, 8)
    res["pose12_out"] = np.array(pose_out, np.float32).reshape(nk, 12)
    res["Ow_out"] = np.array(Ow, np.float32).reshape(nk, 3)
    res["pts_f_out"] = np.array(P8, np.float32).reshape(np_, 8)
    res["pt_corrected_by_out"], res["pt_corrected_ref_out"], res["pt_touched"] = np.array(by, np.int32), np.array(cref, np.int32), np.array(touched, np.uint8)
    return res


def differences(got, want, fields=FIELDS):
    """The fields in which result `got` does not have the bits of `want` (status first): every element of every array is compared, floats
    and doubles as their bit patterns."""
    if got["status"] != want["status"]:
        return [("status", got["status"], want["status"])]
    bad = []
    for f in fields:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append((f, "shape", a.shape, b.shape, a.dtype, b.dtype))
            continue
        if a.dtype.kind == "f":
            a, b = a.view("u%d" % a.dtype.itemsize), b.view("u%d" % b.dtype.itemsize)
        if not np.array_equal(a, b):
            bad.append((f, np.argwhere(a != b)[:4].tolist()))
    return bad


# ==== the map update after a global bundle adjustment (src/LoopClosing.cc:712-803 = src/LocalMapping.cc:824-916) ============================
AG_FIELDS = ("pose12_out", "ns22_out", "TcwBef_out", "nsBef_out", "TcwGBA_out", "nsGBA_out", "kf_in_gba_out", "kf_reached", "Pw_out", "pt_code")
AG_BAD, AG_POS_GBA, AG_BY_REF, AG_UNTOUCHED, AG_REF_UNREACHED = 0, 1, 2, 3, 4
AG_EVENTS = ("chain-of-three-outside", "root-outside", "siblings", "code-0", "code-1", "code-2", "code-3", "code-4", "two-origins", "set-rot-normalises", "unreached-kf")


def mul44(A, B):
    """cv::Mat A * B of two poses [R | t] as 4 x 4 float: four products per entry summed left to right, B's last row 0 0 0 1."""
    zero, one = f32(0), f32(1)
    R = [((A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c]) + A[9 + r] * zero for r in range(3) for c in range(3)]
    t = [((A[3 * r] * B[9] + A[3 * r + 1] * B[10]) + A[3 * r + 2] * B[11]) + A[9 + r] * one for r in range(3)]
    return R + t


def pose_inverse(T):
    """GetPoseInverse / toCvMatInverse as a pose [Rwc | Ow]."""
    return [T[3 * c + r] for r in range(3) for c in range(3)] + camera_centre(T)


def pose_from_ns(ns, Tbc):
    """KeyFrame::UpdatePoseFromNS (src/KeyFrame.cc:102-119): Rwb, Pwb to float; Rcw = (Rwb Rbc)^T; Pwc = Rwb Pbc + Pwb; Pcw = -Rcw Pwc."""
    Rd = qmat((float(ns[6]), float(ns[7]), float(ns[8]), float(ns[9])))
    Rwb = [f32(Rd[r][c]) for r in range(3) for c in range(3)]
    Pwb = [f32(ns[0]), f32(ns[1]), f32(ns[2])]
    Rwc = [Rwb[3 * r] * Tbc[c] + Rwb[3 * r + 1] * Tbc[3 + c] + Rwb[3 * r + 2] * Tbc[6 + c] for r in range(3) for c in range(3)]
    Pwc = [(Rwb[3 * r] * Tbc[9] + Rwb[3 * r + 1] * Tbc[10] + Rwb[3 * r + 2] * Tbc[11]) + Pwb[r] for r in range(3)]
    return [Rwc[3 * c + r] for r in range(3) for c in range(3)] + [(-Rwc[r]) * Pwc[0] + (-Rwc[3 + r]) * Pwc[1] + (-Rwc[6 + r]) * Pwc[2] for r in range(3)]


def apply_global_ba(s, Tbc12, events=None):
    """The literal walk and point loop on one scene."""
    Tbc = [f32(v) for v in np.asarray(Tbc12).reshape(12)]
    nk, np_ = len(s["kf_in_gba"]), len(s["pt_bad"])
    children = [[int(c) for c in s["child_kf"][s["child_start"][k]:s["child_start"][k + 1]]] for k in range(nk)]
    flag = [int(v) for v in s["kf_in_gba"]]
    Tcw = [[f32(v) for v in row] for row in s["pose12"]]
    TcwGBA = [[f32(v) for v in row] for row in s["TcwGBA12"]]
    ns = [[float(v) for v in row] for row in s["ns22"]]
    nsGBA = [[float(v) for v in row] for row in s["nsGBA22"]]
    TcwBef, nsBef, reached = [list(T) for T in Tcw], [list(n) for n in ns], [0] * nk
    outside_depth = [0] * nk
    queue = [int(o) for o in s["origins"]]                              # lpKFtoCheck
    _count(events, "two-origins", int(len(queue) >= 2))
    while queue:
        k = queue[0]
        Twc = pose_inverse(Tcw[k])                                      # before its own update
        if not flag[k]:
            _count(events, "root-outside")
        n_out = 0
        for c in children[k]:
            if not flag[c]:
                Tchildc = mul44(Tcw[c], Twc)
                TcwGBA[c] = mul44(Tchildc, TcwGBA[k])
                flag[c] = 1
                outside_depth[c] = outside_depth[k] + 1
                n_out += 1
                _count(events, "chain-of-three-outside", int(outside_depth[c] == 3))
                g = list(ns[c])                                         # mNavStateGBA = GetNavState()
                Twb = pose_inverse(mul44(Tbc, TcwGBA[c]))
                Rwb = [[float(Twb[3 * r + cc]) for cc in range(3)] for r in range(3)]
                Pwb = [float(Twb[9]), float(Twb[10]), float(Twb[11])]
                Rw1 = qmat((g[6], g[7], g[8], g[9]))
                M = [[Rwb[r][0] * Rw1[cc][0] + Rwb[r][1] * Rw1[cc][1] + Rwb[r][2] * Rw1[cc][2] for cc in range(3)] for r in range(3)]      # RwbGBA * Rw1^T
                V2 = [M[r][0] * g[3] + M[r][1] * g[4] + M[r][2] * g[5] for r in range(3)]
                q = mat2q(Rwb)                                          # Set_Rot: Sophus::SO3(Matrix3d) normalises
                n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
                _count(events, "set-rot-normalises", int(n != 1.0))
                g[0:3], g[3:6], g[6:10] = Pwb, V2, [q[0] / n, q[1] / n, q[2] / n, q[3] / n]
                nsGBA[c] = g
            queue.append(c)
        _count(events, "siblings", int(n_out >= 2))
        TcwBef[k], nsBef[k] = list(Tcw[k]), list(ns[k])
        ns[k] = list(nsGBA[k])
        Tcw[k] = pose_from_ns(ns[k], Tbc)
        reached[k] = 1
        queue.pop(0)
    _count(events, "unreached-kf", int(sum(reached) < nk))
    Pw = [[f32(v) for v in row] for row in s["Pw"]]
    code = [AG_BAD] * np_
    for p in range(np_):
        if s["pt_bad"][p]:
            pass
        elif s["pt_in_gba"][p]:
            Pw[p], code[p] = [f32(v) for v in s["PosGBA"][p]], AG_POS_GBA
        else:
            r = int(s["pt_ref"][p])
            if not flag[r]:
                code[p] = AG_UNTOUCHED
            elif not reached[r]:
                code[p] = AG_REF_UNREACHED                              # the departure: mTcwBefGBA was never set
            else:
                Tb, P = TcwBef[r], Pw[p]
                Xc = [f32(float((Tb[3 * i] * P[0] + Tb[3 * i + 1] * P[1]) + Tb[3 * i + 2] * P[2]) + float(Tb[9 + i])) for i in range(3)]
                Twc = pose_inverse(Tcw[r])
                Pw[p] = [f32(float((Twc[3 * i] * Xc[0] + Twc[3 * i + 1] * Xc[1]) + Twc[3 * i + 2] * Xc[2]) + float(Twc[9 + i])) for i in range(3)]
                code[p] = AG_BY_REF
        _count(events, "code-%d" % code[p])
    return dict(status=OK, pose12_out=np.array(Tcw, np.float32).reshape(nk, 12), ns22_out=np.array(ns, np.float64).reshape(nk, 22),
                TcwBef_out=np.array(TcwBef, np.float32).reshape(nk, 12), nsBef_out=np.array(nsBef, np.float64).reshape(nk, 22),
                TcwGBA_out=np.array(TcwGBA, np.float32).reshape(nk, 12), nsGBA_out=np.array(nsGBA, np.float64).reshape(nk, 22),
                kf_in_gba_out=np.array(flag, np.uint8), kf_reached=np.array(reached, np.uint8), Pw_out=np.array(Pw, np.float32).reshape(np_, 3),
                pt_code=np.array(code, np.uint8))
