"""CPU tests of the two-view initialiser (no GPU): the numpy checker tests/two_view_ref.py against ground truth, the measurement of
every tolerance the GPU tests use (mode "f32" against mode "f64"), the decision-band and skipped-set conditions, the exported symbols,
viorb_two_view_draw_sets, and the host hooks viorb_debug_two_view_* (two_view_core.h compiled for the host) against the checker."""
import ctypes as C
import functools
import os
import re
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi, two_view as tv
from viorb_amd.synth import make_two_view_init_problem
import two_view_ref as T

f32, f64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def case(i):
    ps = T.PARAM_SETS[i]
    p = make_two_view_init_problem(*ps)
    sets = tv.draw_sets(int((p["matches12"] >= 0).sum()), 200, ps[0])
    return p, sets


@functools.lru_cache(maxsize=None)
def solved(i, mode):
    p, sets = case(i)
    return T.initialise(p, sets, mode)


# ---- the checker against ground truth ----------------------------------------------------------------------------------------------------
def test_noise_free_general_recovers_motion_and_depths():
    p = make_two_view_init_problem(11, "general", 400, 430, 300, 0.0, 0.0)
    r = T.initialise(p, tv.draw_sets(300, 200, 1), "f64")
    assert r["status"] == T.FROM_F and r["reason"] == T.OK
    assert T.rot_angle(r["R21"], p["R21"]) < 1e-4 and T.dir_angle(r["t21"], p["t21"]) < 1e-3
    ok = r["triangulated"] != 0
    assert ok.sum() > 250
    ratio = r["P3D"][ok, 2] / p["depth1"][ok]                 # depths up to the scale |t| = 1
    np.testing.assert_allclose(ratio * p["scale"], 1.0, rtol=5e-3)
    assert (r["P3D"][~(r["triangulated"] != 0) & (p["matches12"] < 0)] == 0).all()


def test_planar_recovers_a_homography_and_the_true_motion():
    p = make_two_view_init_problem(12, "planar", 400, 430, 300, 0.0, 0.0)
    r = T.initialise(p, tv.draw_sets(300, 200, 2), "f64")
    assert r["status"] == T.FROM_H and r["reason"] == T.OK
    pm, _ = T.compact(p)
    x1 = np.concatenate([pm[:, :2].astype(f64), np.ones((len(pm), 1))], 1)
    y = x1 @ np.asarray(r["M"], f64).T
    np.testing.assert_allclose(y[:, :2] / y[:, 2:], pm[:, 2:], atol=2e-2)
    assert T.rot_angle(r["R21"], p["R21"]) < 1e-3 and T.dir_angle(r["t21"], p["t21"]) < 1e-2


def test_fundamental_is_rank_two_and_satisfies_the_epipolar_constraint():
    p = make_two_view_init_problem(13, "general", 300, 310, 200, 0.0, 0.0)
    sets = tv.draw_sets(200, 50, 3)
    hy = T.hypotheses(p, sets, "f64")
    pm, _ = T.compact(p)
    x1 = np.concatenate([pm[:, :2].astype(f64), np.ones((len(pm), 1))], 1); x2 = np.concatenate([pm[:, 2:].astype(f64), np.ones((len(pm), 1))], 1)
    good = hy["gapF"] >= T.GAP_MIN
    assert good.sum() >= 40
    for k in np.nonzero(good)[0]:
        F = hy["F21"][k] / np.linalg.norm(hy["F21"][k])
        w = np.linalg.svd(F, compute_uv=False)
        assert w[2] < 1e-12 * w[0]
        l2 = x1 @ F.T                                              # epipolar distance in pixels
        dist = np.abs((x2 * l2).sum(1)) / np.hypot(l2[:, 0], l2[:, 1])
        assert np.median(dist) < 1e-2


def test_the_eight_h_decompositions_reproduce_A():
    p, _ = case(1)
    r = solved(1, "f64")
    ok, R, t, d, A = T.decompose_h(r["M"], p["K4"], "f64")
    assert ok and len(R) == 8
    U, w, Vt = np.linalg.svd(A)
    for i in range(8):
        assert abs(np.linalg.det(R[i]) - 1) < 1e-9
        # A = d2' (R + t' n^T) with |n| = 1: (A / (+-d2) - R) has rank one and its column space is t
        for sgn in (1, -1):
            D = A / (sgn * d[1]) - R[i]
            ww = np.linalg.svd(D, compute_uv=False)
            if ww[1] < 1e-6 * max(ww[0], 1e-12):
                u = np.linalg.svd(D)[0][:, 0]
                assert min(T.dir_angle(u, t[i]), T.dir_angle(-u, t[i])) < 1e-5
                break
        else:
            raise AssertionError("hypothesis %d does not reproduce A" % i)


# ---- measurement of the tolerances ---------------------------------------------------------------------------------------------------------
def _winners(i):
    """(iteration, model) of the winners of both searches of parameter set i (f32 mode), and the selected model."""
    sel = solved(i, "f32")["select"]
    return [(sel["best_iter"][m - 1], m) for m in (1, 2) if sel["best_iter"][m - 1] >= 0], sel["model"]


def measure():
    dev = dict(HYP=0.0, CHI=0.0, SCORE=0.0, ROT=0.0, DIR=0.0, COS=0.0, REPROJ=0.0, DEPTH=0.0, POS=0.0)
    info = dict(skipped=[], band_chi=[], band_rt=[], flips_outside_band=0)
    for i in range(len(T.PARAM_SETS)):
        p, sets = case(i)
        pm, _ = T.compact(p)
        a, b = solved(i, "f32")["hyp"], solved(i, "f64")["hyp"]
        for key, g in (("H21", "gapH"), ("H12", "gapH"), ("F21", "gapF")):
            keep = b[g] >= T.GAP_MIN
            dist = T.mat_dist(a[key], b[key])
            dev["HYP"] = max(dev["HYP"], float(dist[keep].max()))
            info["gap_c"] = max(info.get("gap_c", 0.0), float((dist * b[g]).max() / np.finfo(f32).eps))
            info["skipped"].append(1 - keep.mean())
        band_share = 0.0
        winners, model = _winners(i)
        for k, m in winners:
            M21, M12 = (a["H21"][k], a["H12"][k]) if m == 1 else (a["F21"][k], None)
            ca, cb = T.chi2(m, M21, M12, pm, 1.0, "f32"), T.chi2(m, M21, M12, pm, 1.0, "f64")
            th = T.chi_threshold(m)
            near = cb <= 2 * th                                   # beyond it neither the flag nor the score depends on the value
            if m == model:                                        # the flags that feed the reconstruction
                dev["CHI"] = max(dev["CHI"], float((np.abs(f64(ca) - cb) / np.maximum(np.abs(cb), th))[near].max()))
            sa, fa, _ = T.score(m, ca, "f32"); sb, fb, _ = T.score(m, cb, "f64")
            if (fa == fb).all() and ((ca > f32(th)) == (cb > th)).all():
                dev["SCORE"] = max(dev["SCORE"], abs(float(sa) - float(sb)) / max(float(sb), T.TH_SCORE))
            if m == model:
                band = T.chi_band(m, cb, T.CHI_DEV_F32)
                info["flips_outside_band"] += int(((fa != fb) & ~band).sum())
                band_share = max(band_share, band.mean())
            # decomposition of the selected model's matrix, the same float32 matrix in both modes
            if m != model:
                continue
            if m == 1:
                oa, Ra, ta, _, _ = T.decompose_h(M21, p["K4"], "f32"); ob, Rb, tb, _, _ = T.decompose_h(M21, p["K4"], "f64")
                if not (oa and ob):
                    continue
            else:
                Ra, ta = T.decompose_f(M21, p["K4"], "f32"); Rb, tb = T.decompose_f(M21, p["K4"], "f64")
            _, ra, da = T.match_hypotheses(Ra, ta, Rb, tb)
            dev["ROT"] = max(dev["ROT"], max(ra)); dev["DIR"] = max(dev["DIR"], max(da))
        info["band_chi"].append(band_share)
        # CheckRT on the winner's motions, the same (R, t) in both modes
        w = solved(i, "f32")
        if not w.get("hyp_R"):
            continue
        rt_share, best_h = 0.0, int(np.argmax(w["n_good"]))      # the band share of the motion whose points would be the output
        for h in range(len(w["hyp_R"])):
            ra = T.check_rt(p["K4"], w["hyp_R"][h], w["hyp_t"][h], pm, w["inliers"], 1.0, "f32")
            rb = T.check_rt(p["K4"], w["hyp_R"][h], w["hyp_t"][h], pm, w["inliers"], 1.0, "f64")
            inl = np.asarray(w["inliers"], bool) & ra["finite"] & rb["finite"]
            qa, qb = ra["q"], rb["q"]
            pos = inl & (f64(qb["cos"]) < T.COS_POS_MAX)
            if pos.any():
                d = lambda a: np.asarray(a, f64)
                dev["COS"] = max(dev["COS"], float(np.abs(d(qa["cos"]) - qb["cos"])[inl].max()))
                th2 = float(rb["th2"])
                for e in ("e1", "e2"):
                    dev["REPROJ"] = max(dev["REPROJ"], float((np.abs(d(qa[e]) - qb[e]) / np.maximum(np.abs(qb[e]), th2))[pos].max()))
                dev["DEPTH"] = max(dev["DEPTH"], float((np.abs(d(qa["z1"]) - qb["z1"]) / qb["dist1"])[pos].max()),
                                   float((np.abs(d(qa["z2"]) - qb["z2"]) / qb["dist2"])[pos].max()))
                dev["POS"] = max(dev["POS"], float((np.linalg.norm(d(ra["X"]) - rb["X"], axis=1) / np.linalg.norm(rb["X"], axis=1))[pos].max()))
            band = T.rt_band(rb)
            info["flips_outside_band"] += int(((ra["code"] != rb["code"]) & ~band).sum())
            if h == best_h:
                rt_share = band.sum() / len(pm)
        info["band_rt"].append(rt_share)
    return dev, info


@functools.lru_cache(maxsize=None)
def measured():
    return measure()


def test_float32_restatement_against_float64():
    """Every tolerance constant of two_view_ref.py is the rounded-up largest deviation of its f32 mode from its f64 mode on PARAM_SETS:
    a fresh measurement must not exceed it and must not be more than ten times below it."""
    dev, info = measured()
    print("measured deviations:", {k: "%.3g" % v for k, v in dev.items()})
    for k, v in dev.items():
        const = getattr(T, k + "_DEV_F32")
        assert v <= const, "%s_DEV_F32 = %g is below the measured %g" % (k, const, v)
        assert v >= const / 10, "%s_DEV_F32 = %g is more than ten times the measured %g" % (k, const, v)


def test_decision_bands_and_skipped_sets_of_the_checker_alone():
    """f32 against f64: every flipped flag / CheckRT verdict lies inside its band, the bands hold at most 0.5 % of the matches, at most
    10 % of the sets are near-degenerate."""
    dev, info = measured()
    print("skipped sets:", ["%.3f" % v for v in info["skipped"]], "chi band:", ["%.4f" % v for v in info["band_chi"]], "rt band:", ["%.4f" % v for v in info["band_rt"]])
    assert info["flips_outside_band"] == 0
    assert max(info["band_chi"]) <= T.MAX_BAND_SHARE_CPU and max(info["band_rt"]) <= T.MAX_BAND_SHARE_CPU
    assert max(info["skipped"]) <= T.MAX_SKIPPED_SETS
    print("deviation x gap / eps32: %.2f" % info["gap_c"])
    assert info["gap_c"] <= T.GAP_C


def test_both_modes_take_the_same_decisions_on_the_parameter_sets():
    for i in range(len(T.PARAM_SETS)):
        a, b = solved(i, "f32"), solved(i, "f64")
        assert a["select"]["model"] == b["select"]["model"]
        assert a["status"] == b["status"], (i, a["reason"], b["reason"])


# ---- the library, without a device ---------------------------------------------------------------------------------------------------------
def test_symbols_struct_size_and_abi_version():
    L = viorb_amd.lib()
    assert L.viorb_abi_version() == 2
    assert C.sizeof(capi.TwoViewConfig) == 32 and C.sizeof(capi.TwoViewOutputs) == 18 * C.sizeof(C.c_void_p)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "viorb_two_view.h"' in open(os.path.join(inc, "viorb.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "viorb_two_view.h")).read(), flags=re.S)
    counts = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
              for m in re.finditer(r"\b(viorb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}
    assert set(counts) == set(capi.SIGNATURES_TWO_VIEW)
    for name, n in counts.items():
        assert hasattr(L, name), name
        assert len(capi.SIGNATURES_TWO_VIEW[name][1]) == n, name
    m = re.search(r"typedef struct viorb_two_view_outputs \{(.*?)\}", hdr, flags=re.S)
    assert tuple(re.findall(r"\*\s*([A-Za-z0-9_]+)\s*;", m.group(1))) == capi.TWO_VIEW_OUTPUT_FIELDS


def test_entry_points_check_their_arguments_and_need_a_device():
    L = viorb_amd.lib()
    p, sets = case(5)
    if L.viorb_device_count() < 1:
        with pytest.raises(viorb_amd.ViorbError) as e:
            tv.TwoViewInit(p, sets)
        assert e.value.code == capi.ERR_NO_DEVICE
    bad = sets.copy(); bad[7, 3] = bad[7, 2]
    with pytest.raises(viorb_amd.ViorbError) as e:
        tv.TwoViewInit(p, bad)
    assert e.value.code == capi.ERR_INVALID_ARG
    bad = sets.copy(); bad[0, 0] = 130
    with pytest.raises(viorb_amd.ViorbError) as e:
        tv.TwoViewInit(p, bad)
    assert e.value.code == capi.ERR_INVALID_ARG
    assert L.viorb_two_view_workspace_bytes(0, 200, 1) == 0 and L.viorb_two_view_workspace_bytes(1000, 200, 4) % 256 == 0


def test_draw_sets():
    s = tv.draw_sets(300, 200, 7)
    assert s.shape == (200, 8) and s.min() >= 0 and s.max() < 300
    assert all(len(set(r)) == 8 for r in s)
    assert (s == tv.draw_sets(300, 200, 7)).all() and (s != tv.draw_sets(300, 200, 8)).any()
    assert len(np.unique(s)) > 250                                 # the draws cover the list
    e = tv.draw_sets(8, 50, 1)
    assert all(sorted(r) == list(range(8)) for r in e) and len({tuple(r) for r in e}) > 40
    with pytest.raises(viorb_amd.ViorbError) as err:
        tv.draw_sets(7, 10, 0)
    assert err.value.code == capi.ERR_INVALID_ARG


# ---- the host hooks against the checker ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 4])
def test_hook_hypotheses_match_the_checker(i):
    p, sets = case(i)
    b = solved(i, "f64")["hyp"]
    n1, n2 = tv.debug_normalise(p["xy1"]), tv.debug_normalise(p["xy2"])
    np.testing.assert_allclose(n1, T.normalise(p["xy1"], "f64"), rtol=2e-7)
    np.testing.assert_allclose(n2, T.normalise(p["xy2"], "f64"), rtol=2e-7)
    pm, _ = T.compact(p)
    skipped = 0
    for k in range(0, len(sets), 3):
        q = pm[sets[k]]
        pn1 = ((q[:, 0:2] - n1[None, 0:2]) * n1[None, 2:4]).astype(f32); pn2 = ((q[:, 2:4] - n2[None, 0:2]) * n2[None, 2:4]).astype(f32)
        Hn, _ = tv.debug_hypothesis(T.FROM_H, pn1, pn2); Fn, _ = tv.debug_hypothesis(T.FROM_F, pn1, pn2)
        H21, H12 = tv.debug_denormalise(T.FROM_H, Hn, n1, n2); F21, _ = tv.debug_denormalise(T.FROM_F, Fn, n1, n2)
        if b["gapH"][k] >= T.GAP_MIN:
            assert T.mat_dist(H21, b["H21"][k]) <= T.GPU_FACTOR * T.HYP_DEV_F32 and T.mat_dist(H12, b["H12"][k]) <= T.GPU_FACTOR * T.HYP_DEV_F32
        if b["gapF"][k] >= T.GAP_MIN:
            assert T.mat_dist(F21, b["F21"][k]) <= T.GPU_FACTOR * T.HYP_DEV_F32
            w = np.linalg.svd(f64(Fn), compute_uv=False)
            assert w[2] <= 1e-6 * w[0]
        skipped += (b["gapH"][k] < T.GAP_MIN) + (b["gapF"][k] < T.GAP_MIN)
    assert skipped <= T.MAX_SKIPPED_SETS * 2 * len(range(0, len(sets), 3))


@pytest.mark.parametrize("i", [0, 1])
def test_hook_chi_squares_match_the_checker(i):
    p, _ = case(i)
    r = solved(i, "f32")
    pm, _ = T.compact(p)
    k = r["select"]["best_iter"]
    for m, (M21, M12) in ((1, (r["hyp"]["H21"][k[0]], r["hyp"]["H12"][k[0]])), (2, (r["hyp"]["F21"][k[1]], None))):
        ref = T.chi2(m, M21, M12, pm, 1.0, "f64")
        band = T.chi_band(m, ref, T.GPU_FACTOR * T.CHI_DEV_F32)
        _, flags, contrib = T.score(m, ref, "f64")
        th = T.chi_threshold(m)
        for j in range(len(pm)):
            inl, chi, s = tv.debug_chi2(m, M21, M12, pm[j])
            near = ref[j] <= 2 * th
            assert (np.abs(f64(chi) - ref[j])[near] <= T.GPU_FACTOR * T.CHI_DEV_F32 * np.maximum(ref[j], th)[near]).all()
            if not band[j]:
                assert inl == bool(flags[j]) and abs(s - contrib[j].sum()) <= T.GPU_FACTOR * T.CHI_DEV_F32 * 2 * th
        assert band.mean() <= T.MAX_BAND_SHARE_GPU


@pytest.mark.parametrize("i", [0, 1, 2, 5])
def test_hook_decompositions_and_check_rt_match_the_checker(i):
    p, _ = case(i)
    r = solved(i, "f32")
    m, M = r["select"]["model"], r["M"]
    pm, _ = T.compact(p)
    n, R, t, d = tv.debug_decompose(m, M, p["K4"])
    if m == T.FROM_H:
        ok, Rb, tb, db, _ = T.decompose_h(M, p["K4"], "f64")
        assert ok and n == 8
        np.testing.assert_allclose(d, db, rtol=1e-5)
    else:
        Rb, tb = T.decompose_f(M, p["K4"], "f64")
        assert n == 4
    idx, ra, da = T.match_hypotheses(R[:n], t[:n], Rb, tb)
    assert sorted(idx) == list(range(n))                           # a bijection: the same set of motions
    assert max(ra) <= T.GPU_FACTOR * T.ROT_DEV_F32 and max(da) <= T.GPU_FACTOR * T.DIR_DEV_F32
    # CheckRT of the device-side arithmetic on ITS motions, against the checker on the same motions
    refs = [T.check_rt(p["K4"], R[h], t[h], pm, r["inliers"], 1.0, "f64") for h in range(n)]
    best_h = int(np.argmax([x["n_good"] for x in refs]))
    for h in range(n):
        ref = T.check_rt(p["K4"], R[h], t[h], pm, r["inliers"], 1.0, "f64")
        band = T.rt_band(ref, (T.GPU_FACTOR * T.COS_DEV_F32, T.GPU_FACTOR * T.REPROJ_DEV_F32, T.GPU_FACTOR * T.DEPTH_DEV_F32))
        cosines, codes = [], []
        for j in np.nonzero(r["inliers"])[0]:
            c, X, q = tv.debug_check_rt(p["K4"], R[h], t[h], pm[j])
            codes.append(c)
            if c:
                cosines.append(q[0])
            if not band[j]:
                assert c == ref["code"][j], (h, j, c, ref["code"][j], q, {k: v[j] for k, v in ref["q"].items()})
            if ref["finite"][j] and ref["q"]["cos"][j] < T.COS_POS_MAX:
                assert abs(f64(q[0]) - ref["q"]["cos"][j]) <= T.GPU_FACTOR * T.COS_DEV_F32
                assert np.linalg.norm(f64(X) - ref["X"][j]) <= T.GPU_FACTOR * T.POS_DEV_F32 * np.linalg.norm(ref["X"][j])
        assert h != best_h or band.sum() <= T.MAX_BAND_SHARE_GPU * len(pm)
        # the radix select equals sort + index
        want = np.degrees(np.arccos(f64(np.sort(f32(cosines))[min(50, len(cosines) - 1)]))) if cosines else 0.0
        assert abs(tv.debug_parallax(cosines) - want) <= 1e-6 * max(want, 1.0)


def test_hook_parallax_select_is_an_exact_order_statistic():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 50, 51, 52, 300, 1000):
        c = np.concatenate([rng.uniform(-1, 1, n // 2), 1 - rng.uniform(0, 1e-4, n - n // 2)]).astype(f32)
        if n > 10:
            c[3] = c[7]                                             # ties
        want = f32(np.degrees(np.arccos(f64(np.sort(c)[min(50, n - 1)])))) if n else f32(0)
        assert f32(tv.debug_parallax(c)) == want, n


def test_hook_accept_rules():
    # H: unique clear winner, >= minParallax, > minTriangulated, > 0.9 N
    assert tv.debug_accept(T.FROM_H, [0, 10, 200, 5, 0, 0, 0, 0], [0, 0, 1.0, 0, 0, 0, 0, 0], 210) == (2, T.OK)
    assert tv.debug_accept(T.FROM_H, [0, 150, 200, 5, 0, 0, 0, 0], [0] * 2 + [2.0] + [0] * 5, 210) == (-1, T.NO_WINNER)
    assert tv.debug_accept(T.FROM_H, [0, 10, 200, 5, 0, 0, 0, 0], [0] * 2 + [2.0] + [0] * 5, 230) == (-1, T.FEW_GOOD)
    assert tv.debug_accept(T.FROM_H, [0, 10, 50, 5, 0, 0, 0, 0], [0] * 2 + [2.0] + [0] * 5, 50) == (-1, T.FEW_GOOD)
    assert tv.debug_accept(T.FROM_H, [0, 10, 200, 5, 0, 0, 0, 0], [0] * 2 + [0.99] + [0] * 5, 210) == (-1, T.PARALLAX)
    # F: parallax strictly greater; nGood > 0.7 maxGood counts the winner itself
    assert tv.debug_accept(T.FROM_F, [200, 10, 0, 0], [2.0, 0, 0, 0], 210) == (0, T.OK)
    assert tv.debug_accept(T.FROM_F, [200, 10, 0, 0], [1.0, 0, 0, 0], 210) == (-1, T.PARALLAX)
    assert tv.debug_accept(T.FROM_F, [200, 141, 0, 0], [2.0, 0, 0, 0], 210) == (-1, T.NO_WINNER)
    assert tv.debug_accept(T.FROM_F, [188, 10, 0, 0], [2.0, 0, 0, 0], 210) == (-1, T.FEW_GOOD)
    assert tv.debug_accept(T.FROM_F, [0, 10, 0, 200], [0, 0, 0, 2.0], 210) == (3, T.OK)
    for ng, par, n in (([0, 10, 200, 5, 0, 0, 0, 0], [0, 0, 1.0, 0, 0, 0, 0, 0], 210), ([3, 3, 3, 3, 0, 0, 0, 0], [1.0] * 8, 3)):
        assert tv.debug_accept(T.FROM_H, ng, par, n) == T.accept_h(ng, par, n)
        assert tv.debug_accept(T.FROM_F, ng, par, n) == T.accept_f(ng, par, n)
