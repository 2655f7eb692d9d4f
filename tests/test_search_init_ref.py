"""CPU tests of the monocular matcher (no GPU): the exported symbols, hand-worked pins of the numpy checker tests/search_init_ref.py for
every rule of ORBmatcher::SearchForInitialization that is easy to get wrong, the conditions the fixtures of the GPU tests have to meet
(asserted on the checker alone), the host hooks viorb_debug_search_init_ordered / _window / viorb_debug_scene_depth (search_init_core.h
compiled for the host) against the checker bit for bit, and the argument checks."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import search_init as M
import search_init_ref as T
import search_init_cases as K

f32 = np.float32
INT_MAX = 2 ** 31 - 1


def test_symbols_struct_sizes_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    assert C.sizeof(capi.SearchInitOutputs) == 7 * C.sizeof(C.c_void_p)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_search_init.h"' in open(os.path.join(inc, "viorb.h")).read()
    text = open(os.path.join(inc, "viorb_search_init.h")).read()
    assert '#error "include viorb.h"' in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_SEARCH_INIT)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_SEARCH_INIT[name][1]) == n, name
    for code, name in enumerate(T.REASON_NAMES):
        assert re.search(r"#define VIORB_SI_%s\s+%d\b" % (name, code), text), name
        assert getattr(M, name) == getattr(T, name) == code
    fields = re.search(r"typedef struct viorb_search_init_outputs \{(.*?)\}", text, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == capi.SEARCH_INIT_OUTPUT_FIELDS
    for name in ("SearchInitBatch", "search_for_initialization", "scene_median_depth", "scene_median_depth_batch"):
        assert hasattr(viorb_amd, name)
    pts, wave, lst, thr = M.shape()
    assert wave == 64 and pts >= 1 and lst >= 1 and thr % 64 == 0


# ---- checker pins: hand-worked cases, the expected arrays written out -------------------------------------------------------------------
def test_pin_which_points_and_features_take_part():
    # point 1 is at octave 1 (:422); feature 2 is at octave 2, so point 2's window holds no level-0 feature (Frame.cc:541-548)
    c = K.make_case([(100, 100), (400, 100), (100, 350)], [K.bits(4, K.far(0)), K.far(1), K.far(2)], [(104, 98), (400, 100), (100, 350)],
                    [K.far(0), K.far(1), K.far(2)], octave1=[0, 1, 0], octave2=[0, 0, 2], check_orientation=False)
    e = K.run_ref(c)
    assert e["matches12"].tolist() == [0, -1, -1] and e["nmatches"] == 1
    assert e["reason"].tolist() == [T.MATCHED, T.NOT_CANDIDATE, T.NO_FEATURE_IN_WINDOW]
    assert e["matches21"].tolist() == [0, -1, -1] and e["matched_distance"].tolist() == [4, INT_MAX, INT_MAX]
    assert e["prev_matched"].tolist() == [[104, 98], [400, 100], [100, 350]]


def test_pin_cell_rectangle_early_returns():
    # prev_matched left of the image: x + r = -50 -> nMaxCellX < 0; right of it: x - r = 800 -> nMinCellX = 68 >= 64; both windows are empty
    # although a feature with the very descriptor lies within r of the image border
    c = K.make_case([(10, 100), (740, 100), (300, 300)], [K.far(0), K.far(1), K.far(2)], [(5, 100), (745, 100), (305, 300)], [K.far(0), K.far(1), K.far(2)],
                    prev_matched=[(-150, 100), (900, 100), (300, 300)], check_orientation=False)
    F2 = T.Frame(c["kps2"], c["desc2"], c["bounds4"])
    assert F2.cell_rect(-150, 100, 100) == ((0, -4, 0, -1), True) and F2.cell_rect(900, 100, 100) == ((68, -1, 0, -1), True)
    assert F2.cell_rect(300, 300, 100) == ((17, 35, 20, 40), False)
    assert F2.cell_rect(300, -150, 100) == ((17, 35, 0, -5), True) and F2.cell_rect(300, 1000, 100) == ((17, 35, 90, -1), True)
    e = K.run_ref(c)
    assert e["matches12"].tolist() == [-1, -1, 2]
    assert e["reason"].tolist() == [T.NO_FEATURE_IN_WINDOW, T.NO_FEATURE_IN_WINDOW, T.MATCHED]
    assert e["prev_matched"].tolist() == [[-150, 100], [900, 100], [305, 300]]


def test_pin_feature_outside_the_grid_and_round_half_away():
    # 751.9 * 64 / 752 rounds to column 64: PosInGrid refuses the feature, it is in no cell
    c = K.make_case([(740, 100)], [K.far(0)], [(751.9, 100)], [K.far(0)], check_orientation=False)
    F2 = T.Frame(c["kps2"], c["desc2"], c["bounds4"])
    assert sum(len(cell) for col in F2.grid for cell in col) == 0
    e = K.run_ref(c)
    assert e["matches12"].tolist() == [-1] and e["reason"].tolist() == [T.NO_FEATURE_IN_WINDOW]
    # bounds 512 x 384: 1 / 8 of a cell per pixel, exactly. Feature 0 at x = 4 is at 0.5 -> column 1 (np.round would say 0), feature 1 at
    # x = 3 is in column 0 and is visited first; both are 10 bits from the point, and with nnratio 1.2 the first visited wins
    b = [0, 512, 0, 384]
    c = K.make_case([(4, 150)], [K.far(0)], [(4, 100), (3, 200)], [K.bits(10, K.far(0)), K.bits(10, K.far(0))], window_size=150, nnratio=1.2,
                    check_orientation=False, bounds4=b)
    F2 = T.Frame(c["kps2"], c["desc2"], c["bounds4"])
    assert F2.grid[1][13] == [0] and F2.grid[0][25] == [1]            # 100 / 8 = 12.5 -> row 13 as well
    assert F2.features_in_area(4, 150, 150, 0, 0) == [1, 0]
    assert K.run_ref(c)["matches12"].tolist() == [1]


def _skip_case():
    # F = feature 0, G = feature 1 = F with 23 bits flipped. Point 0 is 10 from F (13 from G), point 1 is 11 from F and 12 from G, point 2
    # is 5 from F (18 from G)
    base = K.far(0)
    return K.make_case([(200, 200), (201, 200), (202, 200)], [K.bits(10, base), K.bits(11, base), K.bits(5, base)], [(200, 204), (204, 200)],
                       [base, K.bits(23, base)], check_orientation=False)


def test_pin_skip_rule_and_displacement():
    c = _skip_case()
    e = K.run_ref(c)
    # point 0 takes F at 10. Point 1: F is hidden (10 <= 11) for best AND second best, so G at 12 stands alone and is accepted; without
    # :444 F at 11 would be best, G at 12 second, and 11 < 12 * 0.9 fails. Point 2: G is hidden (12 <= 18), F at 5 < 10 is taken from point 0
    assert e["matches12"].tolist() == [-1, 1, 0] and e["nmatches"] == 2
    assert e["matches21"].tolist() == [2, 1] and e["matched_distance"].tolist() == [5, 12]
    assert e["reason"].tolist() == [T.DISPLACED, T.MATCHED, T.MATCHED]
    assert e["prev_matched"].tolist() == [[200, 200], [204, 200], [200, 204]]
    f = K.run_ref(c, skip_rule=False)
    assert f["matches12"].tolist() == [-1, -1, 0] and f["reason"].tolist() == [T.DISPLACED, T.RATIO, T.MATCHED]


def test_pin_ties_first_in_visiting_order():
    # both features are 10 bits from the point; feature 1 lies in a lower column and is visited first
    base = K.far(0)
    c = K.make_case([(200, 100)], [base], [(280, 100), (120, 100)], [K.bits(10, base), K.bits(10, base)], nnratio=1.2, check_orientation=False)
    e = K.run_ref(c)
    assert e["matches12"].tolist() == [1] and e["ties"] == 1 and e["matched_distance"].tolist() == [INT_MAX, 10]
    e = K.run_ref(c, nnratio=0.9)                # the equal distance is bestDist2 (:453): 10 < 9 fails
    assert e["matches12"].tolist() == [-1] and e["reason"].tolist() == [T.RATIO]


def test_pin_ratio_test_is_a_float_product_and_int_max_passes():
    base = K.far(0)
    # 0.6f * 5.0f rounds to 3.0f: 3 < 3.0f fails, where the double product 3.0000001 would let it pass
    c = K.make_case([(200, 100)], [base], [(210, 100), (190, 100)], [K.bits(3, base), K.bits(5, base)], nnratio=0.6, check_orientation=False)
    assert f32(5) * f32(0.6) == f32(3) and 5 * float(f32(0.6)) > 3
    e = K.run_ref(c)
    assert e["matches12"].tolist() == [-1] and e["reason"].tolist() == [T.RATIO]
    # a single candidate: bestDist2 = INT_MAX; 50 is accepted, 51 is above TH_LOW
    for d, m, r in ((50, 0, T.MATCHED), (51, -1, T.ABOVE_THRESHOLD)):
        c = K.make_case([(200, 100)], [base], [(210, 100)], [K.bits(d, base)], check_orientation=False)
        e = K.run_ref(c)
        assert e["matches12"].tolist() == [m] and e["reason"].tolist() == [r]


def test_pin_histogram_keeps_displaced_entries_and_prev_matched_only_for_matches():
    # four features far apart, all at angle 0. Points 0..3 match features 0..3 at angles 150, 30, 60, 90 (bins 5, 1, 2, 3); point 4 (angle
    # 150) takes feature 0 from point 0. rotHist[5] holds both, so the three maxima are bins 5, 1, 2 and bin 3 goes: point 3 is removed.
    # Were the displaced entry dropped, the maxima would be bins 1, 2, 3 and point 4 would go instead.
    xy2 = [(100, 100), (400, 100), (100, 350), (400, 350)]
    d2 = [K.far(j) for j in range(4)]
    xy1 = [(102, 100), (402, 100), (102, 350), (402, 350), (101, 101)]
    d1 = [K.bits(10, K.far(j)) for j in range(4)] + [K.bits(5, K.far(0))]
    c = K.make_case(xy1, d1, xy2, d2, angle1=[150, 30, 60, 90, 150])
    e = K.run_ref(c)
    hist = np.zeros(30, np.int32)
    hist[[1, 2, 3, 5]] = [1, 1, 1, 2]
    assert e["rot_hist"].tolist() == hist.tolist()
    assert e["matches12"].tolist() == [-1, 1, 2, -1, 0] and e["nmatches"] == 3
    assert e["reason"].tolist() == [T.DISPLACED, T.MATCHED, T.MATCHED, T.ROTATION, T.MATCHED]
    assert e["matches21"].tolist() == [4, 1, 2, 3] and e["matched_distance"].tolist() == [5, 10, 10, 10]       # not cleared by the rotation step
    assert e["prev_matched"].tolist() == [[102, 100], [400, 100], [100, 350], [402, 350], [100, 100]]
    assert K.run_ref(c, check_orientation=False)["matches12"].tolist() == [-1, 1, 2, 3, 0]


def test_pin_bin_arithmetic():
    assert T.rot_bin(10, 350) == 1            # -340 + 360 = 20 -> 0.67
    assert T.rot_bin(350, 5) == 12            # 345 / 30 = 11.5 -> 12, the highest bin in use
    assert T.rot_bin(15, 0) == 1              # 15 * (1.0f / 30) is 0.5f: half away from zero (np.round gives 0)
    assert T.rot_bin(359.9, 0) == 12 and T.rot_bin(0, 0) == 0 and T.rot_bin(0, 359.9) == 0
    assert max(T.rot_bin(a, b) for a in np.arange(0, 360, 7.3) for b in np.arange(0, 360, 11.1)) == 12
    assert T.three_maxima([0] * 30) == (-1, -1, -1) and T.three_maxima([20, 1, 3] + [0] * 27) == (0, 2, -1)
    assert T.three_maxima([5, 5, 5, 5] + [0] * 26) == (0, 1, 2)


# ---- the fixtures' conditions, on the checker alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", K.SEEDS)
def test_fixture_conditions(seed):
    P, e, free = K.problem(seed), K.expected(seed), K.expected(seed, False, True, False)
    n1, n2 = len(P["kps1"]), len(P["kps2"])
    assert 340 <= n1 <= 380 and 410 <= n2 <= 450 and n1 % 64 and n2 % 64
    r = np.bincount(e["reason"], minlength=7)
    print(seed, n1, n2, r, e["ties"], int((e["matches12"] != free["matches12"]).sum()), e["nmatches"])
    assert r[T.DISPLACED] >= 3 and r[T.RATIO] >= 3 and r[T.ABOVE_THRESHOLD] >= 10 and r[T.ROTATION] >= 10 and r[T.NOT_CANDIDATE] >= 10
    assert e["ties"] >= 20
    assert (e["matches12"] != free["matches12"]).sum() >= 10
    assert e["nmatches"] == (e["matches12"] >= 0).sum() >= 100
    hit = e["matches12"] >= 0
    assert (e["matches12"][hit] == P["truth12"][hit]).mean() > 0.9
    assert (e["prev_matched"][hit] != P["prev_matched"][hit]).any() and np.array_equal(e["prev_matched"][~hit], P["prev_matched"][~hit])
    # bins 0..12 only
    assert e["rot_hist"][13:].sum() == 0 and e["rot_hist"].sum() == r[T.MATCHED] + r[T.DISPLACED] + r[T.ROTATION]


def test_geometry_fixture_has_enough_true_matches():
    P, e = K.problem(0, True), K.expected(0, True)
    hit = e["matches12"] >= 0
    assert hit.sum() >= 150 and (e["matches12"][hit] == P["truth12"][hit]).mean() > 0.9 and "K4" in P


# ---- the host hooks against the checker, bit for bit ------------------------------------------------------------------------------------
def _hook_equals_loop(lists, nfeat, want, nnratio):
    h = M.debug_ordered(lists, nfeat, nnratio)
    K.same(h, want, ("matches12", "matches21", "matched_distance", "nmatches"))
    acc = h["state"] != M.NONE
    assert np.array_equal(acc, np.isin(want["reason"], (T.MATCHED, T.DISPLACED)))
    rest = ~acc & np.array([bool(l) for l in lists])
    assert np.array_equal(h["why"][rest], want["reason"][rest])
    assert 1 <= h["sweeps"] <= T.chain_bound(lists)
    return h


@pytest.mark.parametrize("seed", K.SEEDS)
def test_ordered_hook_equals_the_loop_on_the_fixture(seed):
    P = K.problem(seed)
    h = _hook_equals_loop(K.lists(seed), len(P["kps2"]), K.expected(seed, False, False), P["nnratio"])
    assert h["sweeps"] >= 2


def _case_lists(c):
    F1, F2 = T.Frame(c["kps1"], c["desc1"], c["bounds4"]), T.Frame(c["kps2"], c["desc2"], c["bounds4"])
    return T.candidate_lists(F1, F2, c["prev_matched"], c["window_size"]), F2.N


def test_ordered_hook_on_both_staircases_and_the_pins():
    c = K.descending_staircase(70)
    e = K.run_ref(c)
    assert np.bincount(e["reason"], minlength=7).tolist() == [1, 0, 0, 19, 0, 50, 0] and e["matches12"][69] == 0 and e["matched_distance"][0] == 0
    lists, n2 = _case_lists(c)
    h = _hook_equals_loop(lists, n2, e, c["nnratio"])
    assert h["sweeps"] <= 71
    c = K.ascending_staircase(70)
    e = K.run_ref(c)
    assert e["matches12"].tolist() == list(range(1, 71)) and e["nmatches"] == 70
    assert K.run_ref(c, skip_rule=False)["nmatches"] == 1          # every later point fails the ratio test without what came before it
    lists, n2 = _case_lists(c)
    h = _hook_equals_loop(lists, n2, e, c["nnratio"])
    assert h["sweeps"] == 71 == T.chain_bound(lists)                # the chain is as long as the bound allows
    for c in (_skip_case(), K.overfull(16)):
        lists, n2 = _case_lists(c)
        _hook_equals_loop(lists, n2, K.run_ref(c, check_orientation=False), c["nnratio"])
    e = K.run_ref(K.overfull(16))
    assert e["reason"].tolist() == [T.DISPLACED, T.MATCHED, T.NO_FEATURE_IN_WINDOW, T.RATIO] and e["matches12"][1] == 24


def test_window_hook_equals_get_features_in_area():
    P = K.problem(0)
    F2 = T.Frame(P["kps2"], P["desc2"], P["bounds4"])
    cs, ci = F2.csr()
    rng = np.random.default_rng(3)
    border = [(0, 0), (751.9, 479.9), (0, 479), (751, 0), (376, 0), (376, 479.5), (0, 240), (751.5, 240),
              (-100, 240), (-100.5, 240), (852, 240), (376, -100), (376, 580), (-99.9, -99.9), (851.9, 579.9), (1e12, 5), (-1e12, 5), (5, 3e38)]
    pts = border + [(rng.uniform(-120, 880), rng.uniform(-120, 600)) for _ in range(300)]
    some = 0
    for x, y in pts:
        for r in (100, 10):
            rect, idx = M.debug_window(P["kps2"], cs, ci, P["bounds4"], x, y, r, 0)
            want_rect, early = F2.cell_rect(x, y, r)
            want = F2.features_in_area(x, y, r, 0, 0)
            assert idx.tolist() == want, (x, y, r)
            assert early or rect == want_rect, (x, y, r, rect, want_rect)
            some += len(want) > 1
    assert some > 200
    # a negative level (no extractor makes one) switches the level filter off, as bCheckLevels does
    _, idx = M.debug_window(P["kps2"], cs, ci, P["bounds4"], 300, 200, 100, -1)
    assert idx.tolist() == F2.features_in_area(300, 200, 100, -1, -1) and (P["kps2"]["octave"][idx] > 0).any()


def test_depth_hook_and_median_of_the_checker():
    rng = np.random.default_rng(5)
    for _ in range(3000):
        pose, X = rng.normal(0, 1, 12).astype(f32), (rng.normal(0, 30, 3) * 10.0 ** rng.integers(-3, 3)).astype(f32)
        assert M.debug_scene_depth(pose, X).tobytes() == T.scene_depth(pose, X).tobytes()
    # the double accumulation is visible: float products summed in float differ
    pose, X = np.zeros(12, f32), np.array([1, 1, 1], f32)
    pose[6:9], pose[11] = [1e8, 1, -1e8], 0.5
    assert M.debug_scene_depth(pose, X) == f32(1.5) and (f32(1e8) + f32(1)) + f32(-1e8) + f32(0.5) != f32(1.5)
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)
    pts = np.array([[0, 0, z] for z in (5, -1, 3, 3, 9)], f32)
    assert T.scene_median_depth(ident, pts, [1] * 5, 2) == (f32(3), 5) and T.scene_median_depth(ident, pts, [1] * 5, 1) == (f32(9), 5)
    assert T.scene_median_depth(ident, pts, [1, 1, 0, 0, 1], 2) == (f32(5), 3) and T.scene_median_depth(ident, pts, [0] * 5, 2) == (f32(-1), 0)
    assert T.scene_median_depth(ident, pts[:2], [1, 1], 2) == (f32(-1), 2) and T.scene_median_depth(ident, pts, [1] * 5, 3) == (f32(3), 5)


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def _code(fn, *a, **k):
    with pytest.raises(viorb_amd.ViorbError) as e:
        fn(*a, **k)
    return e.value.code


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    P = K.problem(0)
    INV, CAPY = capi.ERR_INVALID_ARG, capi.ERR_CAPACITY
    host = lambda **kw: M.search_for_initialization(P["kps1"], P["desc1"], P["kps2"], P["desc2"], P["prev_matched"], kw.pop("bounds", P["bounds4"]), **kw)
    assert _code(host, window_size=0) == INV and _code(host, window_size=-5) == INV and _code(host, nnratio=0.0) == INV and _code(host, nnratio=-1.0) == INV
    assert _code(host, bounds=[0, 0, 0, 480]) == INV and _code(host, bounds=[0, 752, 480, 480]) == INV
    big = np.zeros(M.MAX_FEATURES + 1, capi.KP_DTYPE)
    assert _code(M.search_for_initialization, big, np.zeros((len(big), 32), np.uint8), P["kps2"], P["desc2"], np.zeros((len(big), 2), f32), P["bounds4"]) == CAPY
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)
    assert _code(M.scene_median_depth, ident, np.zeros((4, 3), f32), np.ones(4, np.uint8), q=0) == INV
    # the device entries: every refusal comes before any GPU call, so it needs no device and no valid pointer
    one = C.c_void_p(256)
    bounds, ws = capi.ptr(np.asarray(P["bounds4"], f32)), C.c_void_p(4096)
    wb = L.viorb_search_init_workspace_bytes(100, 2)
    assert wb > 0 and L.viorb_search_init_workspace_bytes(0, 2) == 0 and L.viorb_search_init_workspace_bytes(100, 0) == 0
    assert L.viorb_search_init_workspace_bytes(100, 65536) == 0 and L.viorb_search_init_workspace_bytes(M.MAX_FEATURES + 1, 1) == 0
    assert L.viorb_search_init_workspace_bytes(M.MAX_FEATURES, 1) > 0
    kf = capi.S3mKeyframes(one, one, one, one, one, 100)

    def dev(kps1=one, k=kf, prev=one, cap=100, batch=2, b=bounds, win=100, ratio=0.9, m12=one, nm=one, w=ws, bytes_=wb):
        return L.viorb_search_for_initialization_device(kps1, one, one, C.byref(k), prev, cap, batch, b, win, ratio, 1, m12, nm, None, w, bytes_, None)
    assert dev(kps1=None) == INV and dev(prev=None) == INV and dev(m12=None) == INV and dev(nm=None) == INV and dev(b=None) == INV
    assert dev(k=capi.S3mKeyframes(one, None, one, one, one, 100)) == INV and dev(k=capi.S3mKeyframes(one, one, one, one, None, 100)) == INV
    assert dev(k=capi.S3mKeyframes(one, one, one, one, one, 99)) == INV
    assert dev(cap=0) == INV and dev(cap=M.MAX_FEATURES + 1) == CAPY and dev(batch=0) == INV and dev(batch=65536) == INV
    assert dev(win=0) == INV and dev(ratio=0.0) == INV and dev(b=capi.ptr(np.array([5, 5, 0, 480], f32))) == INV
    assert dev(w=None) == INV and dev(bytes_=wb - 1) == INV and dev(w=C.c_void_p(4097)) == INV

    def med(pose=one, pts=one, cap=100, batch=2, q=2, out=one):
        return L.viorb_scene_median_depth_device(pose, pts, one, one, cap, batch, q, out, one, None)
    assert med(pose=None) == INV and med(pts=None) == INV and med(out=None) == INV and med(cap=0) == INV and med(batch=0) == INV and med(batch=65536) == INV
    assert med(q=0) == INV and med(q=-1) == INV
    assert L.viorb_search_init_shape(None) == INV
    if L.viorb_device_count() < 1:
        ND = capi.ERR_NO_DEVICE
        assert dev() == ND and med() == ND and _code(host) == ND
        assert _code(M.scene_median_depth, ident, np.zeros((4, 3), f32), np.ones(4, np.uint8)) == ND
