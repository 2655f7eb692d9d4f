"""Hand-built cases for SearchForTriangulation, Fuse(KeyFrame, points) and SearchByBoW, shared by tests/test_kf_matcher_cases.py (CPU) and the
GPU parity tests: small planted structures inside an ordinary synthetic background problem, each placed so that ONE decision rule of the
reference changes the output (ties between equal distances, a partner exactly at TH_LOW, a feature exactly on a gate). A case names the
rules it decides (tests/kf_matcher_ref.py, tests/bow_ref.py list them); the CPU test proves each claim with the altered literal.

Triangulation cases are dicts(p=<layout of synth.make_two_view_problem>, only_stereo, ori, rules); Fuse cases dicts(p, pts_f, valid, desc,
intr5, th, bounds4, nlevels, rules); BoW cases dicts(args=<the 7-tuple of test_gpu_bow._pair>, ratio, ori, rules)."""
import functools
import numpy as np
from viorb_amd.synth import make_two_view_problem, local_points_f32, KP_NP
import kf_matcher_ref as T

f32 = np.float32


# ---- descriptors ------------------------------------------------------------------------------------------------------------------------------
def far(k):
    """Descriptors about 96 bits from each other: random upper 24 bytes, the low 64 bits (where flip() works) zero."""
    d = np.random.default_rng(7000 + k).integers(0, 256, 32).astype(np.uint8)
    d[:8] = 0
    return d


def flip(base, n, start=0):
    """`base` with bits start .. start+n-1 flipped: Hamming distance n from base; two disjoint ranges of n bits are 2n apart."""
    d = np.array(base, np.uint8, copy=True)
    for b in range(start, start + n):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


class _Ids:
    def __init__(self):
        self.node, self.desc = 100, 0

    def new_node(self):
        self.node += 1
        return self.node

    def new_desc(self):
        self.desc += 1
        return far(self.desc)


def _extend(rng, arrays, fills, spare):
    """Append `spare` inert rows to parallel arrays, shuffle all rows, return (arrays, perm, free slots in shuffled order)."""
    n = len(arrays[0]); tot = n + spare
    perm = rng.permutation(tot)                                         # new row j holds old row perm[j]
    out = []
    for a, fill in zip(arrays, fills):
        b = np.zeros((tot,) + a.shape[1:], a.dtype); b[:n] = a
        b[n:] = fill(spare) if callable(fill) else fill
        out.append(b[perm])
    free = np.nonzero(perm >= n)[0]
    return out, perm, [int(v) for v in rng.permutation(free)]


def _take(free, k, ordered=False):
    idx = [free.pop() for _ in range(k)]
    return sorted(idx) if ordered else idx


def _blank_kps(x=5.0, y=5.0):
    k = np.zeros(1, KP_NP); k["x"], k["y"], k["size"], k["class_id"] = x, y, 31, -1
    return k[0]


# ================================================================================================================================================
# SearchForTriangulation
# ================================================================================================================================================
class _Tri:
    """A make_two_view_problem background with spare inert features (no node, has a map point) at shuffled indices of both frames, to be
    overwritten by planted ones. n2 < n1 and neither is a power of two, so the kernel's padded sort keys and its N2 bound both matter."""

    def __init__(self, seed, n1=330, n2=290, nc=200, stereo_frac=0.0, spare1=40, spare2=70):
        self.rng = rng = np.random.default_rng(900 + seed)
        p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in make_two_view_problem(seed, n1, n2, nc, stereo_frac=stereo_frac).items()}
        self.free, perms = {}, {}
        for s, spare in (("1", spare1), ("2", spare2)):
            keys = ["k" + s, "d" + s, "node" + s, "hp" + s, "ur" + s]
            arrs, perm, free = _extend(rng, [p[k] for k in keys], [_blank_kps(), lambda m: rng.integers(0, 256, (m, 32), dtype=np.uint8), -1, 1, -1.0], spare)
            for k, a in zip(keys, arrs):
                p[k] = a
            self.free[s], perms[s] = free, perm
        inv2 = np.empty(len(perms["2"]), np.int64); inv2[perms["2"]] = np.arange(len(perms["2"]))
        old = np.concatenate([p["truth12"], np.full(spare1, -1, np.int64)])[perms["1"]]
        p["truth12"] = np.where(old >= 0, inv2[np.maximum(old, 0)], -1)
        self.p, self.ids = p, _Ids()

    def take(self, s, k, ordered=False):
        return _take(self.free[s], k, ordered)

    def put(self, s, i, xy, desc, node, octave=0, angle=10.0, hp=0, ur=-1.0):
        p = self.p
        k = p["k" + s]
        k["x"][i], k["y"][i], k["octave"][i], k["angle"][i] = xy[0], xy[1], octave, angle
        k["size"][i] = 31 * p["sf"][octave]
        p["d" + s][i], p["node" + s][i], p["hp" + s][i], p["ur" + s][i] = desc, node, hp, ur

    def on_line(self, xy1, near, off=0.0):
        """The point of key-point xy1's epipolar line in image 2 nearest to `near`, moved `off` pixels along the line's normal."""
        a, b, c = [float(v) for v in T.epipolar_line(self.p, f32(xy1[0]), f32(xy1[1]))]
        nrm = np.hypot(a, b)
        s = (a * near[0] + b * near[1] + c) / nrm
        return (near[0] - (s - off) * a / nrm, near[1] - (s - off) * b / nrm)

    def group(self, xy1, cands, desc1=None, node=None, octave1=0, ur1=-1.0, ordered=True):
        """One frame-1 feature in a node of its own and its frame-2 candidates, each a dict(dx=<pixels along x from xy1>, off, bits | desc, octave, hp,
        ur, xy). Candidates take ascending frame-2 indices in the order given. Returns (i1, [i2...])."""
        node = self.ids.new_node() if node is None else node
        base = self.ids.new_desc() if desc1 is None else desc1
        i1 = self.take("1", 1)[0]
        self.put("1", i1, xy1, base, node, octave=octave1, ur=ur1)
        i2s = self.take("2", len(cands), ordered)
        for i2, c in zip(i2s, cands):
            xy = c["xy"] if "xy" in c else self.on_line(xy1, (xy1[0] + c.get("dx", 30.0), xy1[1]), c.get("off", 0.0))
            desc = c["desc"] if "desc" in c else flip(base, c.get("bits", 10), c.get("start", 0))
            self.put("2", i2, xy, desc, c.get("node", node), octave=c.get("octave", 0), hp=c.get("hp", 0), ur=c.get("ur", -1.0))
        return i1, i2s


def _plant_sideways(B):
    """The planted groups that need no special geometry (the background's sideways baseline: the epipole is thousands of pixels away)."""
    count = iter(range(1000))
    def spot():
        k = next(count)
        return (70.0 + 45.0 * (k % 8), 60.0 + 50.0 * (k // 8))
    # equal distances: the LAST candidate in index order on the line wins (dist > bestDist -> continue)
    B.group(spot(), [dict(bits=20, dx=20), dict(bits=20, dx=40), dict(bits=20, dx=60)])                           # the same descriptor three times
    B.group(spot(), [dict(bits=20, dx=20), dict(bits=20, start=20, dx=40), dict(bits=20, start=40, dx=60)])        # equal distance, different bits
    B.group(spot(), [dict(bits=20, dx=20), dict(bits=20, start=20, dx=40, off=30.0)])                              # the later one is off the line: the first stands
    B.group(spot(), [dict(bits=20, dx=20, off=30.0), dict(bits=20, start=20, dx=40)])
    B.group(spot(), [dict(bits=50, dx=20), dict(bits=50, start=50, dx=40)])                                        # a tie at TH_LOW itself (bestDist starts at TH_LOW)
    # TH_LOW boundary
    for bits in (49, 50, 51):
        B.group(spot(), [dict(bits=bits)])
    # frame 2's map-point flag: the best candidate has a map point, the runner-up has none
    B.group(spot(), [dict(bits=10, hp=1, dx=20), dict(bits=30, dx=40)])
    B.group(spot(), [dict(bits=30, dx=20), dict(bits=10, hp=1, dx=40)])
    # 3.84 gate reads key frame 2's octave: 3.84 * sigma2 = 3.84 at octave 0 and 49.3 at octave 7; 3 and 5 pixels off the line
    B.group(spot(), [dict(bits=10, octave=7, off=3.0)], octave1=0)
    B.group(spot(), [dict(bits=10, octave=7, off=-5.0)], octave1=0)
    B.group(spot(), [dict(bits=10, octave=0, off=3.0)], octave1=7)
    B.group(spot(), [dict(bits=10, octave=0, off=-5.0), dict(bits=30, octave=7, off=6.0, dx=50)], octave1=7)
    # node edges: absent on both sides, present in one frame only, the largest id (the smallest, 0, is in the background)
    B.group(spot(), [dict(bits=0, node=-1)], node=-1)
    B.group(spot(), [dict(bits=0, node=-1)])
    B.group(spot(), [dict(bits=0, node=B.ids.new_node())])
    B.group(spot(), [dict(bits=5)], node=2 ** 31 - 2)


@functools.lru_cache(maxsize=None)
def tri_ties_thresholds():
    """Sideways baseline, all mono. Decides: which of equal-distance candidates wins, TH_LOW inclusive, frame 2's map-point flag, the octave
    the 3.84 gate reads. Also node -1 / one-sided nodes / the largest node id, and n2 < n1 with neither a power of two."""
    B = _Tri(1)
    _plant_sideways(B)
    return dict(p=B.p, only_stereo=False, ori=False, rules=("tie_first", "th_low_exclusive", "ignore_hp2", "sigma_of_kp1"))


@functools.lru_cache(maxsize=None)
def tri_f_zero():
    """F12 = 0: den == 0 for every pair, so nothing matches and no NaN reaches the output. Decides none of the listed rules (it pins the
    den == 0 exit, which has no altered variant)."""
    p = dict(tri_ties_thresholds()["p"])
    p["F12"] = np.zeros((3, 3), f32)
    return dict(p=p, only_stereo=False, ori=True, rules=())


def _forward_geometry(p, rng):
    """R2 = R1 and camera 2 moved 0.5 along the optical axis: the epipole is at (cx, cy) up to rounding. The planted correspondences of the
    background are re-projected (a depth per pair) so that they still lie on their epipolar lines."""
    R1, t1 = p["pose1"][:9].reshape(3, 3).astype(np.float64), p["pose1"][9:].astype(np.float64)
    fx, fy, cx, cy = [float(v) for v in p["intr4"]]
    R2, t2 = R1.copy(), t1 - np.array([0.0, 0.0, 0.5])
    for i1 in np.nonzero(p["truth12"] >= 0)[0]:
        i2 = p["truth12"][i1]; z = rng.uniform(3, 12)
        Pc1 = np.array([(p["k1"]["x"][i1] - cx) / fx * z, (p["k1"]["y"][i1] - cy) / fy * z, z])
        Pc2 = R2 @ (R1.T @ (Pc1 - t1)) + t2
        p["k2"]["x"][i2] = fx * Pc2[0] / Pc2[2] + cx + rng.normal(0, 0.3); p["k2"]["y"][i2] = fy * Pc2[1] / Pc2[2] + cy + rng.normal(0, 0.3)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    R12 = R1 @ R2.T; t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    p["F12"] = (np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)).astype(f32)
    p["pose2"] = np.concatenate([R2.ravel(), t2]).astype(f32)


def gate_points(ex, ey, lim, dx, sign=1.0):
    """Frame-2 positions (float32) whose squared distance to the epipole, in the kernel's float32 arithmetic, is the largest value below `lim`,
    exactly `lim` (None when no float32 y gives it) and the smallest value above it; x is ex - dx, y is searched one ulp at a time."""
    x2 = f32(ex - f32(dx)); rx = float(f32(ex - x2))
    y2 = f32(ey - sign * np.sqrt(float(lim) - rx * rx))
    away = f32(ey - sign * 1e6)
    for _ in range(200):                                                 # walk inside the gate first
        if T.epipole_dist2(ex, ey, x2, y2) < lim:
            break
        y2 = np.nextafter(y2, ey)
    out = dict(below=None, at=None, above=None)
    for _ in range(400):
        d2 = T.epipole_dist2(ex, ey, x2, y2)
        if d2 < lim:
            out["below"] = (x2, y2)
        elif d2 == lim:
            out["at"] = out["at"] or (x2, y2)
        else:
            out["above"] = (x2, y2)
            break
        y2 = np.nextafter(y2, away)
    assert out["below"] and out["above"]
    return out


def _plant_epipole(B):
    """For octaves 0 and 5: a best-descriptor candidate just inside / exactly on / just outside the 100 * sf[octave] circle round the epipole,
    with a worse candidate far out on the same epipolar line. Octave 0 has an exact point (6, 8, 10); for octave 5 the list says which exist."""
    p = B.p
    ex, ey = T.epipole(p)
    found = {}
    for octave, dx, sign in ((0, 6.0, 1.0), (5, 9.5, -1.0)):
        lim = f32(f32(100) * p["sf"][octave])
        g = gate_points(ex, ey, lim, dx, sign)
        found[octave] = sorted(k for k in g if g[k])
        for where in found[octave]:
            for ur1, ur2 in ((-1.0, -1.0), (50.0, -1.0), (-1.0, 50.0)):                  # mono/mono is gated; a stereo side switches the gate off
                x2, y2 = [float(v) for v in g[where]]
                vx, vy = x2 - float(ex), y2 - float(ey); r = np.hypot(vx, vy)
                xy1 = (float(ex) + 0.5 * vx, float(ey) + 0.5 * vy)
                B.group(xy1, [dict(xy=(x2, y2), bits=5, octave=octave, ur=ur2), dict(xy=(float(ex) + 60 * vx / r, float(ey) + 60 * vy / r), bits=30, octave=octave)],
                        ur1=ur1, ordered=False)
    return found


@functools.lru_cache(maxsize=None)
def tri_epipole():
    """Forward motion (epipole at the image centre), 30 % stereo features. Decides the mono epipole gate: present, strict, and off when either
    side is stereo. Exact equality exists for octave 0 (dx, dy = 6, 8: 36 + 64 = 100). For octave 5 (100 * sf = 248.83, dx = 9.5) no float32 y
    gives it, so there the two positions one ulp either side of the circle stand in; `exact` records which positions were found."""
    B = _Tri(2, stereo_frac=0.3)
    _forward_geometry(B.p, B.rng)
    exact = _plant_epipole(B)
    assert "at" in exact[0]
    return dict(p=B.p, only_stereo=False, ori=False, rules=("no_epipole_gate", "epipole_gate_always", "epipole_le"), exact=exact)


@functools.lru_cache(maxsize=None)
def tri_only_stereo():
    """bOnlyStereo with 60 % stereo features: the best candidate of a stereo frame-1 feature is mono and must be skipped for the stereo runner-up;
    a mono frame-1 feature with a stereo partner stays unmatched."""
    B = _Tri(3, stereo_frac=0.6)
    B.group((200.0, 100.0), [dict(bits=5, dx=20), dict(bits=30, dx=40, ur=70.0)], ur1=60.0)
    B.group((260.0, 150.0), [dict(bits=30, dx=20, ur=70.0), dict(bits=5, dx=40)], ur1=60.0)
    B.group((320.0, 200.0), [dict(bits=5, dx=20, ur=70.0)], ur1=-1.0)
    return dict(p=B.p, only_stereo=True, ori=False, rules=("only_stereo_one_sided",))


def _with_rotation_counts(counts):
    """The sideways case with every match's rotation bin chosen: counts = {bin: how many matches}. Matches beyond the total are switched off
    (their frame-1 feature gets a map point). Angles are exact multiples of 30 degrees apart, so bins 0..12 only."""
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tri_ties_thresholds()["p"].items()}
    _, m = T.literal_triangulation(p, False, False)
    matched = [int(i) for i in np.nonzero(m >= 0)[0]]
    bins = [b for b, c in counts.items() for _ in range(c)]
    assert len(matched) >= len(bins), (len(matched), len(bins))
    order = np.random.default_rng(5).permutation(len(matched))
    p["k2"]["angle"][:] = 10.0
    for rank, j in enumerate(order):
        i1 = matched[j]
        if rank < len(bins):
            p["k1"]["angle"][i1] = 10.0 + 30.0 * bins[rank]
        else:
            p["hp1"][i1] = 1
    return p


def _rot_case(counts, rules, doc):
    def make():
        return dict(p=_with_rotation_counts(counts), only_stereo=False, ori=True, rules=rules)
    make.__doc__ = doc
    return functools.lru_cache(maxsize=None)(make)


tri_rot_equal_bins = _rot_case({3: 20, 6: 20, 1: 2, 8: 2}, ("maxima_ge", "maxima_ratio_le"),
                               "Two bins share the highest count and two share the third place, which is exactly 0.1 * max1: the earlier bin of each pair is kept.")
tri_rot_second_tenth = _rot_case({4: 30, 9: 3, 11: 2}, ("maxima_ratio_le",),
                                 "max2 exactly 0.1 * max1 (kept), max3 under it (dropped). 30 and 3: 0.1f * 30.0f is 3.0f, while 0.1 * 30 in double is above 3.")
tri_rot_second_under = _rot_case({4: 30, 9: 2, 11: 2}, (), "max2 just under 0.1 * max1: only the top bin survives. Decides no listed rule; pins the drop.")
tri_rot_third_tenth = _rot_case({2: 20, 5: 7, 12: 2, 0: 1}, ("maxima_ratio_le",), "max3 exactly 0.1 * max1 (kept); the fourth bin goes.")
tri_rot_third_under = _rot_case({2: 20, 5: 7, 12: 1}, (), "max3 just under 0.1 * max1. Decides no listed rule; pins the drop.")

TRI_CASES = dict(tri_ties_thresholds=tri_ties_thresholds, tri_f_zero=tri_f_zero, tri_epipole=tri_epipole, tri_only_stereo=tri_only_stereo,
                 tri_rot_equal_bins=tri_rot_equal_bins, tri_rot_second_tenth=tri_rot_second_tenth, tri_rot_second_under=tri_rot_second_under,
                 tri_rot_third_tenth=tri_rot_third_tenth, tri_rot_third_under=tri_rot_third_under)


def tri_args(c, ori=None):
    p = c["p"]
    return (p["k1"], p["d1"], p["hp1"], p["ur1"], p["node1"], p["k2"], p["d2"], p["hp2"], p["ur2"], p["node2"], p["F12"], p["Cw1"], p["pose2"], p["intr4"],
            p["sf"], p["level_sigma2"], c["only_stereo"], c["ori"] if ori is None else ori)


# ================================================================================================================================================
# Fuse(KeyFrame, points)
# ================================================================================================================================================
STD_BOUNDS = (0.0, 752.0, 0.0, 480.0)
LENS_BOUNDS = (-38.5, 789.2, -31.7, 511.4)


def fuse_background(seed, n1, n2, nc, stereo, n_random=60, noise=8, sf=None):
    """Map points = the common 3-D points of a two-view problem plus random ones; descriptors = the nearest frame-2 key point's with `noise` bits
    flipped (the construction of the older Fuse tests). sf: replace the pyramid (len(sf) levels, octaves folded into it)."""
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in make_two_view_problem(seed, n1, n2, nc, stereo_frac=stereo).items()}
    if sf is not None:
        p["sf"] = np.asarray(sf, f32); p["level_sigma2"] = (p["sf"] * p["sf"]).astype(f32); p["inv_level_sigma2"] = (f32(1) / p["level_sigma2"]).astype(f32)
        for k in ("k1", "k2"):
            p[k]["octave"] %= len(p["sf"])
    rng = np.random.default_rng(seed)
    R2, t2 = p["pose2"][:9].reshape(3, 3).astype(np.float64), p["pose2"][9:].astype(np.float64)
    fx, fy, cx, cy = [float(v) for v in p["intr4"]]
    X = np.concatenate([p["X"], np.stack([rng.uniform(-4, 4, n_random), rng.uniform(-3, 3, n_random), rng.uniform(1, 15, n_random)], 1)])
    uv2 = (R2 @ X.T).T + t2; uv2 = np.stack([fx * uv2[:, 0] / uv2[:, 2] + cx, fy * uv2[:, 1] / uv2[:, 2] + cy], 1)
    k2xy = np.stack([p["k2"]["x"], p["k2"]["y"]], 1).astype(np.float64)
    partner = np.array([int(np.argmin(((k2xy - q) ** 2).sum(1))) for q in uv2])
    pts_f = local_points_f32(p["k2"]["octave"][partner], p["pose1"].astype(np.float64), X.astype(np.float32), p["sf"])
    valid = (rng.random(len(X)) < 0.9).astype(np.uint8)
    desc = p["d2"][partner].copy()
    for _ in range(noise):
        b = rng.integers(0, 256, len(X)); desc[np.arange(len(X)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    intr5 = np.concatenate([p["intr4"], [np.float32(40.0)]]).astype(np.float32)
    return p, pts_f, valid, desc, intr5


class _Fuse:
    """A fuse_background with spare frame-2 features (outside every grid) at shuffled indices and a growing list of planted points."""

    def __init__(self, seed, stereo=0.0, th=3.0, bounds4=STD_BOUNDS, sf=None, n1=300, n2=310, nc=200, spare=80):
        self.rng = rng = np.random.default_rng(300 + seed)
        p, pts_f, valid, desc, self.intr5 = fuse_background(seed, n1, n2, nc, stereo, sf=sf)
        keys = ["k2", "d2", "ur2", "node2", "hp2"]
        arrs, perm, self.free = _extend(rng, [p[k] for k in keys], [_blank_kps(-5000.0, -5000.0), lambda m: rng.integers(0, 256, (m, 32), dtype=np.uint8), -1.0, -1, 1],
                                        spare)
        for k, a in zip(keys, arrs):
            p[k] = a
        p["truth12"] = None
        self.p, self.th, self.bounds4, self.ids = p, th, bounds4, _Ids()
        self.pts, self.valid, self.desc = [r for r in pts_f], list(valid), [d for d in desc]
        self.log_sf = f32(np.log(np.float64(p["sf"][1])))

    def world(self, u, v, z=5.0, behind=False):
        """A world point (float32) that projects to about (u, v) at depth z in key frame 2; behind: mirrored through the camera centre."""
        R, t = self.p["pose2"][:9].reshape(3, 3).astype(np.float64), self.p["pose2"][9:].astype(np.float64)
        fx, fy, cx, cy = [float(x) for x in self.intr5[:4]]
        Pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z]) * (-1.0 if behind else 1.0)
        return (R.T @ (Pc - t)).astype(f32)

    def point(self, X, desc, level=None, maxd=None, mind=None, angle_deg=0.0, ratio=None):
        """Append a map point; level: the level PredictScale gives before the clamp (maxd = dist * sf[1]^(level - 0.5), or dist * ratio);
        angle_deg: angle between its normal and the viewing ray. Returns (index, u, v, ur, dist) in Fuse's float32 arithmetic."""
        _, u, v, ur, PO, dist = T.fuse_geometry(self.p, X, self.intr5)
        s1 = float(self.p["sf"][1])
        if maxd is None:
            maxd = float(dist) * (s1 ** (level - 0.5) if ratio is None else ratio)
        mind = maxd / s1 ** 20 if mind is None else mind
        d = PO.astype(np.float64) / np.linalg.norm(PO.astype(np.float64))
        o = np.cross(d, [0.0, 0.0, 1.0]); o /= np.linalg.norm(o)
        a = np.deg2rad(angle_deg)
        nrm = np.cos(a) * d + np.sin(a) * o
        self.pts.append(np.concatenate([X, nrm, [mind, maxd]]).astype(f32)); self.valid.append(1); self.desc.append(np.asarray(desc, np.uint8))
        return len(self.pts) - 1, u, v, ur, dist

    def feats(self, specs, ordered=True):
        """Planted frame-2 features, dicts(xy, octave, desc, ur); ascending indices in the order given. Returns the indices."""
        idx = _take(self.free, len(specs), ordered)
        for i, c in zip(idx, specs):
            k = self.p["k2"]
            k["x"][i], k["y"][i], k["octave"][i] = c["xy"][0], c["xy"][1], c["octave"]
            k["size"][i] = 31 * self.p["sf"][c["octave"]]
            self.p["d2"][i], self.p["ur2"][i] = c["desc"], c.get("ur", -1.0)
        return idx

    def pair(self, u, v, level, bits=10, octave=None, dxy=(0.5, 0.0), z=5.0, **kw):
        """A point predicted at `level` that projects to about (u, v) and one feature dxy away from the projection."""
        base = self.ids.new_desc()
        i, pu, pv, ur, dist = self.point(self.world(u, v, z, behind=kw.pop("behind", False)), base, level, **kw)
        j = self.feats([dict(xy=(f32(pu + f32(dxy[0])), f32(pv + f32(dxy[1]))), octave=min(max(level, 0), len(self.p["sf"]) - 1) if octave is None else octave,
                             desc=flip(base, bits))])[0]
        return i, j

    def case(self, rules, **extra):
        return dict(p=self.p, pts_f=np.stack(self.pts).astype(f32), valid=np.array(self.valid, np.uint8), desc=np.stack(self.desc).astype(np.uint8), intr5=self.intr5,
                    th=self.th, bounds4=self.bounds4, nlevels=len(self.p["sf"]), rules=rules, **extra)


def exact_u(B, target, v, z=5.0):
    """A world point whose projection's u is exactly the float32 `target` in Fuse's arithmetic (X[0] moved one ulp at a time)."""
    for depth in np.arange(z, z + 4.0, 0.173):                           # not every float32 u is reachable at one depth: the roundings skip some
        X = B.world(float(target), v, depth)
        turns, last = 0, 0
        for _ in range(2000):
            u = T.fuse_geometry(B.p, X, B.intr5)[1]
            if u == f32(target):
                return X
            step = 1 if u < f32(target) else -1
            turns += step == -last
            if turns > 2:
                break
            last = step
            X[0] = np.nextafter(X[0], f32(np.inf * step))
    raise AssertionError("no float32 point projects to u = %r" % target)


@functools.lru_cache(maxsize=None)
def fuse_rules():
    """Standard bounds, th = 3, 8 levels, 30 % stereo features. Grid cells are 11.75 x 10 pixels; cell = round(x / 11.75)."""
    B = _Fuse(21, stereo=0.3)
    cw, ch = 11.75, 10.0
    # equal distances: the FIRST candidate in GetFeaturesInArea order wins (columns, then rows, then insertion = index order inside a cell)
    base = B.ids.new_desc()
    _, u, v, _, _ = B.point(B.world(cw * 10, ch * 10), base, 2)
    B.feats([dict(xy=(u + 1.0, v), octave=2, desc=flip(base, 20)), dict(xy=(u - 1.0, v + 1.0), octave=2, desc=flip(base, 20, 20))])               # one cell
    base = B.ids.new_desc()
    _, u, v, _, _ = B.point(B.world(cw * 20.5, ch * 10), base, 2)
    B.feats([dict(xy=(u + 1.5, v), octave=2, desc=flip(base, 20)), dict(xy=(u - 1.5, v), octave=2, desc=flip(base, 20, 20))])                     # lower index in the LATER column
    base = B.ids.new_desc()
    _, u, v, _, _ = B.point(B.world(cw * 30, ch * 20.5), base, 2)
    B.feats([dict(xy=(u, v + 1.5), octave=2, desc=flip(base, 20)), dict(xy=(u, v - 1.5), octave=2, desc=flip(base, 20, 20))])                     # lower index in the LATER row
    # TH_LOW boundary
    for k, bits in enumerate((49, 50, 51)):
        B.pair(100.0 + 40 * k, 200.0, 1, bits=bits)
    # level window [l-1, l]: partners at l-2 .. l+1
    for k, octave in enumerate((1, 2, 3, 4)):
        B.pair(100.0 + 40 * k, 250.0, 3, octave=octave)
    # chi-square gates: e2 * invSigma2 = 6.5 for a mono and for a stereo feature (5.99 mono, 7.8 stereo)
    B.pair(300.0, 250.0, 0, dxy=(2.5, 0.5))
    base = B.ids.new_desc()
    _, u, v, ur, _ = B.point(B.world(340.0, 250.0), base, 0)
    B.feats([dict(xy=(f32(u + f32(2.4)), f32(v + f32(0.7))), octave=0, desc=flip(base, 10), ur=f32(ur - f32(0.5)))])
    # behind the camera, projecting inside the image
    B.pair(400.0, 300.0, 2, behind=True)
    # u exactly maxX (the only feature that is still inside a grid cell is 5.9 pixels away: level 7)
    base = B.ids.new_desc()
    _, u, v, _, _ = B.point(exact_u(B, 752.0, 300.0), base, 7)
    assert u == f32(752.0)
    B.feats([dict(xy=(746.1, v), octave=7, desc=flip(base, 10))])
    # distance gates: dist3D half a percent inside / outside 0.8 * min and 1.2 * max
    for k, q in enumerate((0.995, 1.005)):
        base = B.ids.new_desc(); X = B.world(100.0 + 40 * k, 330.0)
        dist = float(T.fuse_geometry(B.p, X, B.intr5)[5])
        _, u, v, _, _ = B.point(X, base, 2, mind=dist / (0.8 * q))
        B.feats([dict(xy=(u + 0.5, v), octave=2, desc=flip(base, 10))])
        base = B.ids.new_desc(); X = B.world(200.0 + 40 * k, 330.0)
        dist = float(T.fuse_geometry(B.p, X, B.intr5)[5])
        _, u, v, _, _ = B.point(X, base, maxd=dist / (1.2 * q), mind=0.01)
        B.feats([dict(xy=(u + 0.5, v), octave=0, desc=flip(base, 10))])
    # viewing angle: cos 55, 58 pass 0.5; cos 62, 65 do not
    for k, a in enumerate((55.0, 58.0, 62.0, 65.0)):
        B.pair(100.0 + 40 * k, 380.0, 1, angle_deg=a)
    return B.case(("tie_last", "th_low_exclusive", "level_window_up", "chi_swapped", "no_behind_gate", "in_image_le", "no_distance_margin", "view_cos_0"))


@functools.lru_cache(maxsize=None)
def fuse_lens_bounds():
    """Lens bounds with negative minX / minY, th = 2. Cells are 12.93 x 11.31 pixels; u - minX enters the cell window. Points and features in the
    first and the last grid column and row, u exactly maxX, and a feature exactly `radius` away in x (level 0: radius = 2, chi-square 4)."""
    B = _Fuse(22, stereo=0.0, th=2.0, bounds4=LENS_BOUNDS)
    B.pair(-35.0, -28.0, 1)                                   # cell (0, 0)
    B.pair(776.0, 500.0, 1)                                   # cell (63, 47)
    B.pair(-35.0, 500.0, 1); B.pair(776.0, -28.0, 1)
    B.pair(785.5, 100.0, 1)                                   # its only feature is past the last column: in no cell
    base = B.ids.new_desc()
    maxX = f32(LENS_BOUNDS[1])
    _, u, v, _, _ = B.point(exact_u(B, maxX, 200.0), base, 7)
    assert u == maxX
    B.feats([dict(xy=(f32(maxX - f32(6.9)), v), octave=7, desc=flip(base, 10))])
    for k, d in enumerate((2.0, -2.0)):                        # exactly `radius` away in x
        base = B.ids.new_desc()
        _, u, v, _, _ = B.point(B.world(300.0 + 40 * k, 240.0), base, 0)
        kx = f32(u + f32(d))
        assert abs(f32(kx - u)) == f32(2.0)
        B.feats([dict(xy=(kx, v), octave=0, desc=flip(base, 10))])
    return B.case(("no_min_offset", "in_image_le", "radius_le"))


@functools.lru_cache(maxsize=None)
def fuse_four_levels():
    """nlevels = 4 with scale factors 1.5^i: predicted levels 0, 3, 4 and 5 before the clamp, partners on levels 2 and 3.
    A predicted level of -1 needs max_dist / dist3D <= 1 / 1.5 while the distance gate needs it >= 1 / 1.2, so the lower clamp cannot be
    reached past that gate (nor with any scale factor of 1.2 or more, short of exact equality); the point planted for it is rejected by the gate under every rule, and
    `no_level_clamp` is decided by the upper clamp alone."""
    B = _Fuse(23, stereo=0.2, sf=[1.5 ** i for i in range(4)])
    B.pair(100.0, 100.0, -1, octave=0)
    B.pair(140.0, 100.0, 0, ratio=0.9)                        # level 0 past the gate: 1 / 1.2 <= max_dist / dist3D <= 1
    B.pair(180.0, 100.0, 3)
    B.pair(220.0, 100.0, 4, octave=3)
    B.pair(260.0, 100.0, 5, octave=3)
    B.pair(300.0, 100.0, 5, octave=2)
    B.pair(340.0, 100.0, 5, octave=1)
    return B.case(("no_level_clamp",))


FUSE_CASES = dict(fuse_rules=fuse_rules, fuse_lens_bounds=fuse_lens_bounds, fuse_four_levels=fuse_four_levels)


def fuse_oracle(oracle, c):
    p = c["p"]
    log_sf = np.float32(np.log(np.float64(p["sf"][1])))
    return oracle.fuse(p["k2"], p["d2"], p["ur2"], c["bounds4"], p["pose2"], c["intr5"], p["sf"], p["inv_level_sigma2"], log_sf, c["pts_f"], c["valid"], c["desc"], c["th"])


def fuse_literal(c, rule=None):
    return T.literal_fuse(c["p"], c["pts_f"], c["valid"], c["desc"], c["intr5"], c["th"], c["bounds4"], c["nlevels"], rule)


# ================================================================================================================================================
# SearchByBoW
# ================================================================================================================================================
class _Bow:
    """A background of noisy copies sharing a node (as test_gpu_bow._pair builds, with node ids drawn directly) and spare inert features at
    shuffled indices of both sides. Planted features turn by 355 degrees (bin 12), like three quarters of the background."""

    def __init__(self, seed, nK=260, nF=280, nc=180, spareK=30, spareF=110):
        self.rng = rng = np.random.default_rng(500 + seed)
        kd = rng.integers(0, 256, (nK, 32), dtype=np.uint8)
        src = rng.permutation(nK)[:nc]
        fd = kd[src].copy()
        for _ in range(10):
            b = rng.integers(0, 256, nc); fd[np.arange(nc), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
        fd = np.concatenate([fd, rng.integers(0, 256, (nF - nc, 32), dtype=np.uint8)])
        kn = rng.integers(0, 40, nK).astype(np.int32); fn = np.concatenate([kn[src], rng.integers(0, 40, nF - nc).astype(np.int32)])
        ka = rng.uniform(0, 360, nK).astype(f32)
        fa = (np.concatenate([ka[src] + rng.choice([5.0, 5.0, 5.0, 130.0], nc) + rng.normal(0, 3, nc), rng.uniform(0, 360, nF - nc)]).astype(f32) % f32(360))
        kn[rng.random(nK) < 0.02] = -1; fn[rng.random(nF) < 0.02] = -1
        kh = (rng.random(nK) < 0.8).astype(np.uint8)
        rnd = lambda m: rng.integers(0, 256, (m, 32), dtype=np.uint8)
        (self.kd, self.ka, self.kn, self.kh), _, self.freeK = _extend(rng, [kd, ka, kn, kh], [rnd, 0.0, -1, 0], spareK)
        (self.fd, self.fa, self.fn), _, self.freeF = _extend(rng, [fd, fa, fn], [rnd, 0.0, -1], spareF)
        self.ids = _Ids()

    def group(self, kfs, frs, node=None):
        """Key-frame features (dicts desc, hp) and frame features (dicts desc) of one node, each side at ascending indices in the order given."""
        node = self.ids.new_node() if node is None else node
        ik, jf = _take(self.freeK, len(kfs), True), _take(self.freeF, len(frs), True)
        for i, c in zip(ik, kfs):
            self.kd[i], self.kn[i], self.kh[i], self.ka[i] = c["desc"], node, c.get("hp", 1), 100.0
        for j, c in zip(jf, frs):
            self.fd[j], self.fn[j], self.fa[j] = c["desc"], node, 105.0
        return ik, jf

    def args(self):
        return (self.kd, self.ka, self.kn, self.kh, self.fd, self.fa, self.fn)


def _plant_bow(B, with_threshold=True):
    d = B.ids.new_desc
    b = d(); B.group([dict(desc=b)], [dict(desc=flip(b, 20)), dict(desc=flip(b, 20, 20))])                       # two frame features at the same best distance
    b = d(); B.group([dict(desc=b)], [dict(desc=flip(b, 20)), dict(desc=flip(b, 20)), dict(desc=d())])           # ... with the same descriptor
    b = d(); B.group([dict(desc=b)], [dict(desc=flip(b, 50, 50)), dict(desc=flip(b, 35))])                       # 35 against 0.7 * 50
    b = d(); B.group([dict(desc=b)], [dict(desc=flip(b, 34)), dict(desc=flip(b, 50, 50))])                       # 34 against 0.7 * 50 passes
    if with_threshold:
        for bits in (49, 50, 51):
            b = d(); B.group([dict(desc=b)], [dict(desc=flip(b, bits)), dict(desc=d())])
    # two key-frame features want the same frame feature: the earlier index takes it, the later settles for its runner-up / for nothing
    b = d(); B.group([dict(desc=flip(b, 10)), dict(desc=flip(b, 5))], [dict(desc=flip(b, 35, 10)), dict(desc=b)])
    b = d(); B.group([dict(desc=flip(b, 10)), dict(desc=flip(b, 5))], [dict(desc=b), dict(desc=d())])
    # a key-frame feature without a map point that would otherwise win
    b = d(); B.group([dict(desc=flip(b, 5), hp=0), dict(desc=flip(b, 15))], [dict(desc=b), dict(desc=d())])
    # a node with 70 frame features: the 64-lane scan takes a second pass. Best in the second pass; a tie across the pass boundary.
    b, c = d(), d()
    frs = [dict(desc=d()) for _ in range(70)]
    frs[66] = dict(desc=flip(b, 8)); frs[5] = dict(desc=flip(b, 30)); frs[10] = dict(desc=flip(c, 12)); frs[69] = dict(desc=flip(c, 12, 12))
    B.group([dict(desc=b), dict(desc=c)], frs)


@functools.lru_cache(maxsize=None)
def bow_rules():
    """nnratio 0.7. With a ratio below 1 two candidates at the same best distance always fail the ratio test, so which of them is `best`
    cannot show: `tie_last` is decided by bow_loose_ratio instead."""
    B = _Bow(1)
    _plant_bow(B)
    return dict(args=B.args(), ratio=0.7, ori=True, rules=("th_low_exclusive", "ratio_le", "second_ignores_equal", "ignore_has_point", "not_exclusive"))


@functools.lru_cache(maxsize=None)
def bow_loose_ratio():
    """nnratio 1.2 (the ratio is an argument of the matcher): candidates at the same best distance pass the ratio test and the FIRST one in
    index order must win, also when the two lie in different passes of the 64-lane scan."""
    B = _Bow(2)
    _plant_bow(B, with_threshold=False)
    return dict(args=B.args(), ratio=1.2, ori=False, rules=("tie_last",))


BOW_CASES = dict(bow_rules=bow_rules, bow_loose_ratio=bow_loose_ratio)
