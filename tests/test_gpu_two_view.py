"""GPU tests of the two-view initialiser: chained stage parity against tests/two_view_ref.py (each stage checked on the DEVICE's own
input to that stage, so that a divergence never cascades), the end-to-end entry against the chain of the stage entries bit for bit,
the failure reasons, and the host-buffer entry. All cases run as ONE batch (different n1 / n2 / N per stream), computed once.

Tolerances are GPU_FACTOR (4) x the f32-against-f64 deviations the CPU suite measures; a discrete result is left out of the exact
comparison only inside its decision band (BAND_FACTOR x the deviation of its threshold), and the bands may hold at most 2 % of a
case's matches; at most 10 % of a case's sets may be near-degenerate (skipped in the matrix comparison only)."""
import functools
import itertools
import numpy as np
import pytest
from viorb_amd import two_view as tv
from viorb_amd.synth import make_two_view_init_problem
import two_view_ref as T

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
KINDS = ("general", "planar")
NS = (8, 9, 63, 64, 65, 130, 300)          # one wavefront and its stride boundaries, one and two blocks of CheckRT; 8: every set a permutation
CASES = list(itertools.product(KINDS, NS))
ITER = 200


@functools.lru_cache(maxsize=None)
def problem(kind, n):
    # seeds chosen so that every case meets the band and skipped-set caps below with the checker alone (a case that does not is changed,
    # never the cap); n1 != n2 and both above n, so that unmatched key points take part in Normalize
    p = make_two_view_init_problem(400 + n, kind, n + 40, n + 55, n, 0.1 if n >= 63 else 0.0, 0.5)
    return p, tv.draw_sets(n, ITER, n)


@functools.lru_cache(maxsize=None)
def device():
    """Every device result the tests below look at: the three stage entries chained, and the end-to-end entry, on one batch."""
    probs = [problem(*c)[0] for c in CASES]; sets = [problem(*c)[1] for c in CASES]
    B = tv.TwoViewBatch(probs, sets)
    H21, H12, F21, reason = B.hypotheses()
    scores, flags = B.score(H21, H12, F21, flags=True)
    mats = dict(H21=H21.cpu().numpy(), H12=H12.cpu().numpy(), F21=F21.cpu().numpy())
    sel, models, Ms, inl = [], [], [], []
    for b in range(len(CASES)):
        s = T.select(scores[b])
        sel.append(s); models.append(s["model"])
        k = s["best_iter"][s["model"] - 1] if s["model"] else 0
        Ms.append(mats["H21" if s["model"] == T.FROM_H else "F21"][b, k] if s["model"] else np.zeros((3, 3), f32))
        inl.append(flags[b, k, s["model"] - 1, :B.N[b]] if s["model"] else np.zeros(B.N[b], np.uint8))
    rec = B.reconstruct(models, np.stack(Ms), inl)
    return dict(B=B, mats=mats, reason=reason, scores=scores, flags=flags, sel=sel, M=Ms, inl=inl, rec=rec, e2e=B.init())


def idx(kind, n):
    return CASES.index((kind, n))


@pytest.mark.parametrize("kind,n", CASES)
def test_hypotheses_against_the_checker(kind, n):
    D, b = device(), idx(kind, n)
    p, sets = problem(kind, n)
    assert D["reason"][b] == T.OK
    ref = T.hypotheses(p, sets, "f64")
    worst = 0.0
    for key, g in (("H21", "gapH"), ("H12", "gapH"), ("F21", "gapF")):
        keep = ref[g] >= T.GAP_MIN
        assert 1 - keep.mean() <= T.MAX_SKIPPED_SETS, (key, 1 - keep.mean())
        dist = T.mat_dist(D["mats"][key][b], ref[key])
        worst = max(worst, float(dist[keep].max()))
        assert np.isfinite(D["mats"][key][b]).all()
    print("largest matrix distance %.3g (allowed %.3g)" % (worst, T.GPU_FACTOR * T.HYP_DEV_F32))
    assert worst <= T.GPU_FACTOR * T.HYP_DEV_F32
    # the F hypotheses are rank 2
    w = np.linalg.svd(f64(D["mats"]["F21"][b]), compute_uv=False)
    assert (w[:, 2] <= 1e-5 * w[:, 0]).all()


@pytest.mark.parametrize("kind,n", CASES)
def test_scores_and_flags_against_the_checker_on_the_device_matrices(kind, n):
    D, b = device(), idx(kind, n)
    p, _ = problem(kind, n)
    pm, _ = T.compact(p)
    sel = D["sel"][b]
    worst = 0.0
    for k in range(ITER):
        for m in (1, 2):
            M21, M12 = (D["mats"]["H21"][b, k], D["mats"]["H12"][b, k]) if m == 1 else (D["mats"]["F21"][b, k], None)
            chi = T.chi2(m, M21, M12, pm, 1.0, "f32")               # the reference's own float steps on the device's matrix
            band_dir = np.abs(f64(chi) - T.chi_threshold(m)) <= T.BAND_FACTOR * T.CHI_DEV_F32 * T.chi_threshold(m)
            s, fl, _ = T.score(m, chi, "f32")
            got = float(D["scores"][b, k, m - 1])
            allowed = T.GPU_FACTOR * T.SCORE_DEV_F32 * max(float(s), T.TH_SCORE) + T.TH_SCORE * band_dir.sum()
            worst = max(worst, (abs(got - float(s)) - T.TH_SCORE * band_dir.sum()) / max(float(s), T.TH_SCORE))
            assert abs(got - float(s)) <= allowed, (k, m, got, float(s))
            band = band_dir.any(1)
            dfl = D["flags"][b, k, m - 1]
            assert (dfl[:n][~band] == fl[~band]).all() and (dfl[n:] == 0).all()
            if sel["model"] == m and sel["best_iter"][m - 1] == k:
                assert band.mean() <= T.MAX_BAND_SHARE_GPU
    print("largest relative score difference %.3g (allowed %.3g)" % (worst, T.GPU_FACTOR * T.SCORE_DEV_F32))


@pytest.mark.parametrize("kind,n", CASES)
def test_selection_is_exact_on_the_device_scores(kind, n):
    D, b = device(), idx(kind, n)
    sel, e = D["sel"][b], D["e2e"][b]
    assert list(e["best_iter"]) == sel["best_iter"]
    assert e["scores"][0] == sel["S"][0] and e["scores"][1] == sel["S"][1]
    for m, key in ((0, "H21"), (1, "F21")):
        want = D["mats"][key][b, sel["best_iter"][m]] if sel["best_iter"][m] >= 0 else np.zeros((3, 3), f32)
        assert np.array_equal(e[key], want)
        assert np.array_equal(e["inliers_h" if m == 0 else "inliers_f"], D["flags"][b, max(sel["best_iter"][m], 0), m, :n])
    assert e["n_matches"] == n
    if e["status"] != T.FAILED:
        assert e["status"] == sel["model"]
    assert (kind == "planar") == (sel["model"] == T.FROM_H)


def _robust_accept(model, ng, nb, par, dpar, n_inl):
    """The accept rule on every corner of (n_good +- band members, parallax +- its tolerance): the set of outcomes."""
    accept = T.accept_h if model == T.FROM_H else T.accept_f
    out = set()
    H = len(ng)
    for signs in itertools.product((-1, 1), repeat=H):
        for sp in (-1, 1):
            g = [max(ng[h] + signs[h] * nb[h], 0) for h in range(H)] + [0] * (8 - H)
            q = [f32(par[h] + sp * dpar[h]) for h in range(H)] + [f32(0)] * (8 - H)
            out.add(accept(g, q, n_inl))
    return out


@pytest.mark.parametrize("kind,n", CASES)
def test_reconstruction_against_the_checker_on_the_device_matrix_and_flags(kind, n):
    D, b = device(), idx(kind, n)
    p, _ = problem(kind, n)
    pm, i1 = T.compact(p)
    model, M, inl, got = D["sel"][b]["model"], D["M"][b], D["inl"][b], D["rec"][b]
    ref = T.reconstruct(model, M, inl, p, "f64")
    assert got["n_matches"] == n
    if model == T.FROM_H and abs(min(ref["d"][0] / ref["d"][1], ref["d"][1] / ref["d"][2]) - 1.00001) <= T.BAND_FACTOR * 1.2e-7:
        return                                                    # the singular-value gate itself is inside its band
    H = len(ref["hyp_R"])
    assert got["n_hyp"] == H
    if H == 0:
        assert got["status"] == T.FAILED and got["reason"] == ref["reason"]
        return
    j, ra, da = T.match_hypotheses(got["hyp_R"][:H], got["hyp_t"][:H], ref["hyp_R"], ref["hyp_t"])
    assert max(ra) <= T.GPU_FACTOR * T.ROT_DEV_F32 and max(da) <= T.GPU_FACTOR * T.DIR_DEV_F32, (ra, da)
    assert (got["hyp_n_good"][H:] == 0).all() and (got["hyp_parallax"][H:] == 0).all() and (got["hyp_R"][H:] == 0).all()
    # CheckRT on the device's own motions: counts up to the band members, the parallax between the neighbouring order statistics
    rts = [T.check_rt(p["K4"], got["hyp_R"][h], got["hyp_t"][h], pm, inl, 1.0, "f64") for h in range(H)]
    nb = [int(T.rt_band(r).sum()) for r in rts]
    dpar = []
    for h, r in enumerate(rts):
        ng = int(got["hyp_n_good"][h])
        assert abs(ng - r["n_good"]) <= nb[h], (h, ng, r["n_good"], nb[h])
        cs = r["cosines"]
        if ng == 0 or len(cs) == 0:
            assert nb[h] > 0 or got["hyp_parallax"][h] == 0
            dpar.append(0.0)
            continue
        k = min(50, len(cs) - 1)
        tol = T.GPU_FACTOR * T.COS_DEV_F32 + 2e-7
        c = np.cos(np.radians(f64(got["hyp_parallax"][h])))
        lo, hi = cs[max(k - nb[h], 0)] - tol, cs[min(k + nb[h], len(cs) - 1)] + tol
        assert lo <= c <= hi, (h, c, lo, hi)
        dpar.append(float(np.degrees(tol / max(np.sqrt(max(1 - cs[k] ** 2, 0)), 1e-4))))
    best = int(np.argmax([r["n_good"] for r in rts]))
    assert nb[best] <= T.MAX_BAND_SHARE_GPU * n
    outcomes = _robust_accept(model, [r["n_good"] for r in rts], nb, [float(r["parallax"]) for r in rts], dpar, int(np.asarray(inl, bool).sum()))
    win = got["status"] != T.FAILED
    if len(outcomes) == 1:                                        # no accept gate is inside a band: the decision must be the checker's
        w, reason = next(iter(outcomes))
        assert got["reason"] == reason and win == (w >= 0)
        if win:
            assert np.array_equal(got["R21"], got["hyp_R"][w]) and np.array_equal(got["t21"], got["hyp_t"][w])
    if not win:
        assert not got["R21"].any() and not got["t21"].any() and not got["P3D"].any() and not got["triangulated"].any()
        return
    w = [h for h in range(H) if np.array_equal(got["R21"], got["hyp_R"][h]) and np.array_equal(got["t21"], got["hyp_t"][h])][0]
    r, band = rts[w], T.rt_band(rts[w])
    tri, P = np.zeros(len(p["xy1"]), np.uint8), np.zeros((len(p["xy1"]), 3))
    tri[i1[r["code"] == T.RT_TRIANGULATED]] = 1
    P[i1[r["code"] != T.RT_NONE]] = r["X"][r["code"] != T.RT_NONE]
    free = np.ones(len(p["xy1"]), bool); free[i1[band]] = False
    assert np.array_equal(got["triangulated"][free], tri[free])
    counted = np.zeros(len(p["xy1"]), bool); counted[i1[r["code"] != T.RT_NONE]] = True
    assert not got["P3D"][free & ~counted].any()                   # (0, 0, 0) for a key point without a surviving match
    well = np.zeros(len(p["xy1"]), bool); well[i1[(r["code"] != T.RT_NONE) & (f64(r["q"]["cos"]) < T.COS_POS_MAX)]] = True
    sel = free & well
    err = np.linalg.norm(f64(got["P3D"][sel]) - P[sel], axis=1) / np.linalg.norm(P[sel], axis=1)
    print("largest relative position error %.3g over %d points (allowed %.3g)" % (err.max() if len(err) else 0, sel.sum(), T.GPU_FACTOR * T.POS_DEV_F32))
    assert (err <= T.GPU_FACTOR * T.POS_DEV_F32).all()
    assert got["P3D"][free & counted].any(1).all()


def test_accepted_cases_recover_the_ground_truth():
    D = device()
    for kind, n in (("general", 300), ("general", 130), ("planar", 300), ("planar", 65)):
        p, _ = problem(kind, n)
        e = D["e2e"][idx(kind, n)]
        assert e["status"] == (T.FROM_H if kind == "planar" else T.FROM_F) and e["reason"] == T.OK, (kind, n, e["reason"])
        assert T.rot_angle(e["R21"], p["R21"]) < 0.02 and T.dir_angle(e["t21"], p["t21"]) < 0.25
        ok = (e["triangulated"] != 0) & (p["true12"] != 0)
        assert ok.sum() > 0.8 * n * 0.9
        scale = np.median(e["P3D"][ok, 2] / p["depth1"][ok])
        assert np.median(np.abs(e["P3D"][ok, 2] / p["depth1"][ok] / scale - 1)) < 0.1


def test_end_to_end_equals_the_chain_of_stages_bit_for_bit():
    D = device()
    for b, (kind, n) in enumerate(CASES):
        e, c = D["e2e"][b], D["rec"][b]
        for key in ("status", "reason", "n_matches", "n_hyp"):
            assert e[key] == c[key], (kind, n, key, e[key], c[key])
        for key in ("R21", "t21", "P3D", "triangulated", "hyp_n_good", "hyp_parallax", "hyp_R", "hyp_t"):
            assert e[key].tobytes() == c[key].tobytes(), (kind, n, key)


def test_failure_reasons_and_the_host_entry():
    few = make_two_view_init_problem(1, "general", 60, 70, 8, 0.0, 0.5)
    few["matches12"][np.nonzero(few["matches12"] >= 0)[0][:3]] = -1                # 5 matches
    lowp, ls = make_two_view_init_problem(3, "low_parallax", 400, 430, 300, 0.1, 0.5), tv.draw_sets(300, ITER, 3)
    good, gs = problem("general", 130)
    bad = gs.copy(); bad[17, 5] = bad[17, 1]                                         # a repeated index
    oob = gs.copy(); oob[3, 0] = 130                                                 # one past the list
    B = tv.TwoViewBatch([few, lowp, good, good, good], [np.zeros((ITER, 8), np.int32), ls, bad, oob, gs])
    r = B.init()
    assert (r[0]["status"], r[0]["reason"], r[0]["n_matches"]) == (T.FAILED, T.FEW_MATCHES, 5)
    assert r[1]["status"] == T.FAILED and r[1]["reason"] in (T.NO_WINNER, T.PARALLAX, T.FEW_GOOD, T.H_DEGENERATE)
    assert (r[2]["status"], r[2]["reason"]) == (T.FAILED, T.BAD_SET) and (r[3]["status"], r[3]["reason"]) == (T.FAILED, T.BAD_SET)
    for k in (0, 1, 2, 3):
        assert not r[k]["R21"].any() and not r[k]["t21"].any() and not r[k]["P3D"].any() and not r[k]["triangulated"].any()
    want = device()["e2e"][idx("general", 130)]
    for key in want:                                                                 # the batch a stream sits in does not matter
        assert np.asarray(r[4][key]).tobytes() == np.asarray(want[key]).tobytes(), key
    # the reconstruction stage without a model
    rr = B.reconstruct([0, 7, 0, 0, 0], np.zeros((5, 3, 3), f32), [np.zeros(0, np.uint8)] * 5)
    assert all(x["status"] == T.FAILED for x in rr) and rr[1]["reason"] == T.NO_MODEL and rr[0]["reason"] == T.FEW_MATCHES
    # the host-buffer entry, one stream
    h = tv.TwoViewInit(good, gs)
    for key in want:
        assert np.asarray(h[key]).tobytes() == np.asarray(want[key]).tobytes(), key
