"""GPU tests of the Sim3 RANSAC solver (include/viorb_sim3.h) against the numpy checker tests/sim3_ref.py. Each stage is checked on the
device's own input to it (hypotheses from the sets; counts and flags of the DEVICE's models; the selection of the DEVICE's counts), so
that a divergence never cascades. Tolerances: GPU_FACTOR x the measured f32-against-f64 deviations of sim3_ref.py; a flag may differ
only inside its decision band (BAND_FACTOR x the deviation at the threshold). The caps of tests/test_gpu_two_view.py hold: at most 10 %
of a case's sets skipped as near-degenerate, at most 2 % of a case's decisions inside bands.

Three batches, each computed once: a free scale and a fixed scale at min_inliers = 20 over N = 20 (= min_inliers), 21, 63, 64, 65, 130
and 300 correspondences with 0 and 30 % outliers (plus a pair with too few correspondences, one with a bad set and one with a 0 / 0 set),
and N = 3 at min_inliers = 2, where every set is a permutation of the same three correspondences. 300 sets per pair."""
import functools
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi, sim3
from viorb_amd.synth import make_sim3_problem
import sim3_ref as T

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ITERS = T.ITERATIONS
SIZES = (20, 21, 63, 64, 65, 130, 300)
# With 20 or 21 correspondences 300 sets repeat a few hundred triples, and the share of near-degenerate ones varies a lot from scene to
# scene: these scenes had 7 to 11 % and were replaced (the cap is MAX_SKIPPED_SETS = 10 %; every scene used has 6 % at most on the CPU).
SEED_MOVED = {1: 4001, 3: 1003, 101: 12101, 102: 1102, 103: 7103}


@functools.lru_cache(maxsize=None)
def cases(name):
    """(problems, sets, min_inliers, fix_scale, special) of a batch; special maps a role to its pair index."""
    if name == "three":
        # seeds whose triangle is well-conditioned: every set of such a pair is the same triangle, so one near-degenerate one skips them all
        probs = [make_sim3_problem(seed, kind, 3, 0.0, 0.3, 0.001) for seed, kind in ((40, "general"), (45, "general"), (46, "small_rotation"))]
        return probs, [sim3.draw_sets(3, ITERS, 7 + k) for k in range(3)], 2, False, {}
    fix = name == "fixed"
    kind = "fix_scale" if fix else "general"
    probs, sets = [], []
    for j, n in enumerate(SIZES):
        for o in (0.0, 0.3):
            seed = 100 * fix + 2 * j + (o > 0)
            probs.append(make_sim3_problem(SEED_MOVED.get(seed, seed), kind, n, o, 0.5, 0.002))
            sets.append(sim3.draw_sets(n, ITERS, 1000 + len(sets)))
    special = {}
    special["few"] = len(probs); probs.append(make_sim3_problem(90, kind, 10, 0.0, 0.5, 0.002)); sets.append(sim3.draw_sets(10, ITERS, 5))
    special["bad"] = len(probs); probs.append(make_sim3_problem(91, kind, 64, 0.0, 0.5, 0.002))
    s = sim3.draw_sets(64, ITERS, 6).copy(); s[2, 1] = s[2, 0]; s[3, 2] = 64; s[4, 0] = -1
    sets.append(s)
    special["zero"] = len(probs)
    p = make_sim3_problem(92, kind, 65, 0.0, 0.5, 0.002); p["X2c"] = p["X2c"].copy(); p["X2c"][:3] = p["X1c"][:3]
    s = sim3.draw_sets(65, ITERS, 8).copy(); s[1] = (2, 0, 1)
    probs.append(p); sets.append(s)
    return probs, sets, 20, fix, special


@functools.lru_cache(maxsize=None)
def batch(name):
    probs, sets, mi, fix, _ = cases(name)
    return sim3.Sim3Batch(probs, sets, min_inliers=mi, fix_scale=fix)


@functools.lru_cache(maxsize=None)
def stage(name):
    """The stage entries, each on the device's own input: hypotheses, then counts and flags of those models."""
    B = batch(name)
    R, t, s, reason = B.hypotheses()
    counts, flags = B.inliers(R, t, s, flags=True)
    return dict(R=R, t=t, s=s, reason=reason, counts=counts, flags=flags, hR=R.cpu().numpy(), ht=t.cpu().numpy(), hs=s.cpu().numpy())


NAMES = ("free", "fixed", "three")


@pytest.mark.parametrize("name", NAMES)
def test_hypotheses_against_the_checker(name):
    probs, sets, mi, fix, special = cases(name)
    g = stage(name)
    for b, (p, st) in enumerate(zip(probs, sets)):
        if b in (special.get("few"), special.get("bad")):
            continue
        ref = T.hypotheses(p, st, fix, "f64")
        ok = g["reason"][b] == T.SET_OK
        if b == special.get("zero"):
            assert g["reason"][b][1] == T.SET_ZERO_ROTATION and ok.sum() == ITERS - 1
        else:
            assert ok.all()
        keep = (ref["gap"] >= T.GAP_MIN) & ok
        assert 1 - keep.mean() <= T.MAX_SKIPPED_SETS, (name, b, 1 - keep.mean())
        dR = np.abs(g["hR"][b].astype(f64) - ref["R"]).max((1, 2))
        dT = np.linalg.norm(g["ht"][b].astype(f64) - ref["t"], axis=1) / ref["O1n"]
        dS = np.abs(g["hs"][b].astype(f64) - ref["s"]) / np.where(ref["s"] != 0, ref["s"], 1)
        print(name, b, len(p["X1c"]), "skipped %.3f dR %.2e dT %.2e dS %.2e" % (1 - keep.mean(), dR[keep].max(), dT[keep].max(), dS[keep].max()))
        assert dR[keep].max() <= T.GPU_FACTOR * T.R_DEV_F32
        assert dT[keep].max() <= T.GPU_FACTOR * T.T_DEV_F32
        assert dS[keep].max() <= T.GPU_FACTOR * T.S_DEV_F32
        if fix:
            assert (g["hs"][b][ok] == 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_counts_and_flags_of_the_device_models(name):
    probs, sets, mi, fix, special = cases(name)
    g = stage(name)
    for b, p in enumerate(probs):
        n = len(p["X1c"])
        fl = g["flags"][b][:, :n] != 0
        assert (g["flags"][b][:, n:] == 0).all() and (fl.sum(1) == g["counts"][b]).all()
        bad = g["reason"][b] != T.SET_OK
        assert (g["counts"][b][bad] == 0).all()                          # zero models count nothing
        e1, e2 = T.errors(g["hR"][b], g["ht"][b], g["hs"][b], p, "f64")
        ref, band = T.flags_of(e1, e2, p), T.err_band(e1, e2, p, T.GPU_FACTOR * T.ERR_DEV_F32)
        assert band.mean() <= T.MAX_BAND_SHARE_GPU, (name, b, band.mean())
        assert (fl == ref)[~band].all(), (name, b, np.argwhere((fl != ref) & ~band)[:5])
    if "few" in special:
        assert (g["reason"][special["few"]] == T.SET_FEW).all() and (g["hR"][special["few"]] == 0).all()
        r = g["reason"][special["bad"]]
        assert (r[2:5] == T.SET_BAD).all() and (np.delete(r, [2, 3, 4]) == T.SET_OK).all()
        assert (g["hR"][special["bad"]][2:5] == 0).all() and (g["hs"][special["bad"]][2:5] == 0).all()
        z = special["zero"]
        assert g["reason"][z][1] == T.SET_ZERO_ROTATION and (g["hR"][z][1] == 0).all() and g["counts"][z][1] == 0


STATES = [dict(), dict(per=ITERS), dict(first=1, best=0, per=ITERS), dict(first=7, best=18, per=5), dict(first=60, best=25, per=70),
          dict(first=0, best=10 ** 6, per=ITERS), dict(first=290, best=0, per=64), dict(first=ITERS, best=0, per=5), dict(max_its=37, per=ITERS),
          dict(max_its=ITERS + 50, first=250, best=10 ** 6, per=ITERS)]


@pytest.mark.parametrize("name", NAMES)
def test_selection_is_the_literal_rule_on_the_device_counts(name):
    probs, sets, mi, fix, _ = cases(name)
    B, g = batch(name), stage(name)
    for st in STATES:
        mx, first, best, per = st.get("max_its", ITERS), st.get("first", 0), st.get("best", 0), st.get("per", 5)
        d = B.select(g["counts"], max_its=mx, first_iteration=first, best_inliers_in=best, iterations_per_call=per)
        for b, p in enumerate(probs):
            want = T.select(g["counts"][b], len(p["X1c"]), mi, mx, first, best, per)
            got = tuple(int(d[k][b]) for k in ("status", "iterations_done", "best_inliers", "best_iter"))
            assert got == want, (name, st, b, got, want)


def _expect(B, g, probs, mi, b, first, best, per, mx=ITERS):
    """The end-to-end outputs of pair b that the chain of stage entries gives."""
    n = len(probs[b]["X1c"])
    st, done, bi, it = T.select(g["counts"][b], n, mi, mx, first, best, per)
    e = dict(status=st, iterations_done=done, best_inliers=bi, best_iter=it, n_inliers=0, inliers=np.zeros(n, np.uint8), R12=np.zeros((3, 3), f32),
             t12=np.zeros(3, f32), s12=f32(0), T12=np.zeros((4, 4), f32))
    if it >= 0:
        R, t, s = g["hR"][b][it], g["ht"][b][it], g["hs"][b][it]
        T12 = np.eye(4, dtype=f32); T12[:3, :3] = (R.astype(f64) * f64(s)).astype(f32); T12[:3, 3] = t
        e.update(R12=R, t12=t, s12=s, T12=T12)
    if st == T.FOUND:
        e.update(n_inliers=int(g["counts"][b][it]), inliers=g["flags"][b][it][:n])
    return e


def _same(got, want, ctx):
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), (ctx, k, got[k], v)


@pytest.mark.parametrize("name", NAMES)
def test_end_to_end_equals_the_chain_of_stages_bit_for_bit(name):
    probs, sets, mi, fix, special = cases(name)
    B, g = batch(name), stage(name)
    for st in (dict(per=ITERS), dict(first=3, best=12, per=5), dict(first=100, best=0, per=150)):
        first, best, per = st.get("first", 0), st.get("best", 0), st["per"]
        out = B.ransac(first_iteration=first, best_inliers_in=best, iterations_per_call=per)
        for b in range(len(probs)):
            _same(out[b], _expect(B, g, probs, mi, b, first, best, per), (name, st, b))
    if "few" in special:
        out = B.ransac(iterations_per_call=ITERS)
        assert out[special["few"]]["status"] == T.FEW and out[special["few"]]["best_iter"] == -1 and not out[special["few"]]["inliers"].any()
        found = [o["status"] == T.FOUND for o in out]
        assert sum(found) >= 8 and not all(found)                       # both outcomes occur in the batch


@pytest.mark.parametrize("name", NAMES)
def test_chunks_of_five_with_the_carried_state_equal_one_call_and_resume_after_found(name):
    probs, sets, mi, fix, _ = cases(name)
    B, g = batch(name), stage(name)
    nb = len(probs)
    whole = B.ransac(iterations_per_call=ITERS)
    first, best = np.zeros(nb, np.int32), np.zeros(nb, np.int32)
    reached = [None] * nb
    for _ in range(ITERS // 5 + 1):
        out = B.ransac(first_iteration=first, best_inliers_in=best, iterations_per_call=5)
        for b in range(nb):
            if reached[b] is None:
                _same(out[b], _expect(B, g, probs, mi, b, int(first[b]), int(best[b]), 5), (name, "chunk", b, int(first[b])))
                if out[b]["status"] != T.CONTINUE:
                    reached[b] = out[b]
                else:
                    first[b], best[b] = out[b]["iterations_done"], out[b]["best_inliers"]
        if all(r is not None for r in reached):
            break
    for b in range(nb):
        for k in ("status", "iterations_done", "best_inliers", "n_inliers", "inliers"):
            assert np.array_equal(np.asarray(reached[b][k]), np.asarray(whole[b][k])), (name, b, k)
        if whole[b]["status"] == T.FOUND:
            _same(reached[b], {k: whole[b][k] for k in ("best_iter", "R12", "t12", "s12", "T12")}, (name, b))
    # LoopClosing resumes a solver whose model failed the optimisation: the next model the literal rule allows
    first = np.array([w["iterations_done"] for w in whole], np.int32); best = np.array([w["best_inliers"] for w in whole], np.int32)
    nxt = B.ransac(first_iteration=first, best_inliers_in=best, iterations_per_call=ITERS)
    resumed = 0
    for b in range(nb):
        _same(nxt[b], _expect(B, g, probs, mi, b, int(first[b]), int(best[b]), ITERS), (name, "resume", b))
        if whole[b]["status"] == T.FOUND and nxt[b]["status"] == T.FOUND:
            resumed += 1
            assert nxt[b]["best_iter"] > whole[b]["best_iter"] and nxt[b]["n_inliers"] >= whole[b]["n_inliers"]
    assert name == "three" or resumed >= 3


def test_host_buffer_entry_equals_the_device_entry():
    probs, sets, mi, fix, special = cases("free")
    B = batch("free")
    dev = B.ransac(first_iteration=2, best_inliers_in=5, iterations_per_call=40)
    for b in (0, 5, 13, special["few"], special["zero"]):
        host = sim3.sim3_ransac(probs[b], sets[b], first_iteration=2, best_inliers_in=5, min_inliers=mi, fix_scale=fix, iterations_per_call=40)
        _same(host, dev[b], ("host", b))
    with pytest.raises(viorb_amd.ViorbError) as e:                     # the host form refuses what the device form reports per set
        sim3.sim3_ransac(probs[special["bad"]], sets[special["bad"]])
    assert e.value.code == capi.ERR_INVALID_ARG
    p = dict(probs[0]); p["X1c"], p["X2c"], p["sigma2_1"], p["sigma2_2"] = p["X1c"][:0], p["X2c"][:0], p["sigma2_1"][:0], p["sigma2_2"][:0]
    r = sim3.sim3_ransac(p, sets[0])                                   # no correspondences at all
    assert r["status"] == T.FEW and r["n_inliers"] == 0 and len(r["inliers"]) == 0
