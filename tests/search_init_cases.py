"""Fixtures shared by tests/test_search_init_ref.py (CPU) and tests/test_gpu_search_init.py: the synthetic frames of
synth.make_search_init_problem, hand-built edge cases, and the checker's (tests/search_init_ref.py) results on them, computed once."""
import functools
import numpy as np
from viorb_amd import capi
from viorb_amd.synth import make_search_init_problem
import search_init_ref as T

f32 = np.float32
BOUNDS = np.array([0, 752, 0, 480], f32)
SEEDS = (0, 1, 2)
OUTPUTS = ("matches12", "nmatches", "prev_matched", "matches21", "matched_distance", "rot_hist", "reason")


@functools.lru_cache(maxsize=None)
def problem(seed=0, geometry=False):
    return make_search_init_problem(seed, geometry=geometry)


def frames(P):
    return T.Frame(P["kps1"], P["desc1"], P["bounds4"]), T.Frame(P["kps2"], P["desc2"], P["bounds4"])


@functools.lru_cache(maxsize=None)
def lists(seed=0, geometry=False):
    P = problem(seed, geometry)
    F1, F2 = frames(P)
    return T.candidate_lists(F1, F2, P["prev_matched"], P["window_size"])


@functools.lru_cache(maxsize=None)
def expected(seed=0, geometry=False, check_orientation=True, skip_rule=True):
    P = problem(seed, geometry)
    F1, F2 = frames(P)
    return T.search_for_initialization(F1, F2, P["prev_matched"], P["window_size"], P["nnratio"], check_orientation, skip_rule, lists(seed, geometry))


def run_ref(c, prev_matched=None, **kw):
    """The checker on a hand-built case (a dict of make_case)."""
    F1, F2 = T.Frame(c["kps1"], c["desc1"], c["bounds4"]), T.Frame(c["kps2"], c["desc2"], c["bounds4"])
    a = dict(window_size=c["window_size"], nnratio=c["nnratio"], check_orientation=c["check_orientation"])
    a.update(kw)
    return T.search_for_initialization(F1, F2, c["prev_matched"] if prev_matched is None else prev_matched, **a)


def same(got, want, keys=OUTPUTS):
    """np.array_equal over the named entries, with the entry that differs in the message."""
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (k, np.asarray(got[k]), np.asarray(want[k]))


# ---- hand-built cases ---------------------------------------------------------------------------------------------------------------------
def kps(xy, octave=None, angle=None):
    xy = np.asarray(xy, f32).reshape(-1, 2)
    k = np.zeros(len(xy), capi.KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["octave"] = 0 if octave is None else octave
    k["angle"] = 0 if angle is None else angle
    k["size"], k["class_id"] = 31, -1
    return k


def bits(n_set, base=None):
    """A descriptor at Hamming distance n_set from `base` (default: all zero): its first n_set bits flipped."""
    d = np.zeros(32, np.uint8) if base is None else np.array(base, np.uint8, copy=True)
    for b in range(n_set):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def far(k):
    """Descriptors far (> 100 bits) from each other and from the low-bit patterns of bits(): byte pattern k in the upper 24 bytes."""
    rng = np.random.default_rng(1000 + k)
    d = rng.integers(0, 256, 32).astype(np.uint8)
    d[:8] = 0
    return d


def make_case(xy1, desc1, xy2, desc2, prev_matched=None, octave1=None, octave2=None, angle1=None, angle2=None, window_size=100, nnratio=0.9,
              check_orientation=True, bounds4=BOUNDS):
    k1, k2 = kps(xy1, octave1, angle1), kps(xy2, octave2, angle2)
    pm = np.stack([k1["x"], k1["y"]], 1).astype(f32) if prev_matched is None else np.asarray(prev_matched, f32).reshape(-1, 2)
    return dict(kps1=k1, desc1=np.asarray(desc1, np.uint8).reshape(-1, 32), kps2=k2, desc2=np.asarray(desc2, np.uint8).reshape(-1, 32), prev_matched=pm,
                window_size=window_size, nnratio=nnratio, check_orientation=check_orientation, bounds4=np.asarray(bounds4, f32))


def descending_staircase(n=70):
    """n level-0 points of frame 1 that all prefer feature 0, at distances n-1, n-2, ..., 0 (falling by one bit each). Acceptance needs a
    distance <= TH_LOW, so the first n - 51 points end above the threshold and each of the last 51 takes the feature from the one before:
    50 displacements in a row. A second feature far away keeps the list honest."""
    base = far(0)
    xy1 = [(100 + 2 * (k % 10), 100 + 2 * (k // 10)) for k in range(n)]
    d1 = [bits(n - 1 - k, base) for k in range(n)]
    return make_case(xy1, d1, [(110, 106), (600, 400)], [base, far(1)], window_size=100, check_orientation=False)


def ascending_staircase(n=70, d=20):
    """Point k sees features k and k+1 (8 pixels apart, window 10), both at distance d; feature 0 is above level 0, so point 0 sees feature
    1 only. In order: point k finds feature k taken at distance d (the skip rule hides it, also as second best) and takes feature k+1, so
    every point depends on the one before through a different feature: a chain of n. Without its predecessor's state a point fails the
    ratio test (d against d). Features alternate between two descriptors 2d bits apart; every point is d bits from either."""
    base = far(0)
    xy2 = [(40 + 8 * j, 200) for j in range(n + 1)]
    xy1 = [(40 + 8 * k + 4, 200) for k in range(n)]
    d2 = [base if j % 2 == 0 else bits(2 * d, base) for j in range(n + 1)]
    d1 = [bits(d, base) for _ in range(n)]
    c = make_case(xy1, d1, xy2, d2, window_size=10, check_orientation=False)
    c["kps2"]["octave"][0] = 1
    return c


def overfull(list_cap):
    """One window with list_cap + 9 level-0 features whose distances to the points are all <= TH_LOW (so none is left out of a list), the
    best one last. Point 0 takes it at distance 3, point 1 takes it away at distance 2, point 3 finds it hidden and fails the ratio test
    among the rest; point 2 is elsewhere."""
    n = list_cap + 9
    base = far(3)
    xy2 = [(300 + 3 * (j % 8), 240 + 3 * (j // 8)) for j in range(n)]
    d2 = [bits(40 - (j % 7), base) for j in range(n)]
    d2[n - 1] = bits(3, base)
    xy1 = [(310, 245), (312, 246), (500, 100), (311, 247)]
    d1 = [base, bits(1, base), far(4), base]
    return make_case(xy1, d1, xy2, d2, check_orientation=True)
