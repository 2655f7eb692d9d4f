"""GPU tests of OptimizeSim3 (viorb_optimize_sim3_device, include/viorb_sim3.h) against the numeric-Jacobian mode of the numpy checker
tests/sim3_ref.py. Cases (sim3_ref.OPT_CASES): 9 valid correspondences (the early return: S12 unchanged, 0 returned), 10, 63, 64, 65 and
257, both fix_scale values, 0 % outliers (5 more iterations) and 20 % (10 more), `valid` holes in the middle of the arrays, and a case
whose round ends on a rejected trial. Two batches (one per fix_scale value), each computed once. For every case: the iteration counts
and the accept / reject counts equal, keep equal outside the bands, nIn consistent with keep, both chi2 within 1e-5 relative, S12
within GPU_FACTOR x the measured numeric-against-analytic deviation. The counts are compared on sim3_ref.OPT_CASES only: on
OPT_CASES_FLOOR (see there) the last trials of a round are decided at the rounding floor of chi2, in the checker's two modes as well."""
import functools
import numpy as np
import pytest
import viorb_amd
from viorb_amd import sim3
import sim3_ref as T

pytestmark = pytest.mark.gpu
ALL = T.OPT_CASES + T.OPT_CASES_FLOOR


@functools.lru_cache(maxsize=None)
def batch(fix):
    idx = [i for i, c in enumerate(ALL) if c[1] == fix]
    cs = [T.opt_case(ALL[i]) for i in idx]
    out = sim3.optimize_sim3_batch([c[0] for c in cs], [c[1] for c in cs], 10.0, fix, [c[2] for c in cs])
    return idx, cs, out


@functools.lru_cache(maxsize=None)
def reference(i):
    p, S0, valid, fix, th2 = T.opt_case(ALL[i])
    return T.optimize_sim3(p, S0, th2, fix, valid, "numeric")


@pytest.mark.parametrize("fix", [False, True])
def test_optimiser_matches_the_checker(fix):
    idx, cs, out = batch(fix)
    sizes = set()
    for i, (p, S0, valid, _, th2), g in zip(idx, cs, out):
        ref = reference(i)
        sizes.add(ALL[i][2])
        strict = ALL[i] in T.OPT_CASES                                   # every LM decision of the case is above the rounding floor
        print(ALL[i], "strict" if strict else "floor", "info", g["info"], "ref", ref["info"], "dS %.3g" % np.abs(g["S12"] - ref["S12"]).max())
        assert np.array_equal(g["info"][:2], ref["info"][:2]), (ALL[i], g["info"], ref["info"])                  # nCorrespondences, nBad
        if strict:
            assert np.array_equal(g["info"][2:4], ref["info"][2:4]), (ALL[i], g["info"], ref["info"])            # the iterations of both rounds
            assert np.array_equal(g["info"][6:], ref["info"][6:]), (ALL[i], g["info"], ref["info"])              # accepted, rejected trials
        else:
            assert g["info"][2] == ref["info"][2] or g["info"][2] >= 3, (ALL[i], g["info"])
        band = T.chi_band(ref, th2, T.GPU_FACTOR * T.OPT_EDGE_DEV)
        assert band.sum() <= T.MAX_BAND_SHARE_GPU * len(band) + 1
        assert np.array_equal(g["keep"][~band], ref["keep"][~band]) and not g["keep"][valid == 0].any()
        for k in (4, 5):
            assert abs(g["info"][k] - ref["info"][k]) <= T.CHI2_TOL * max(ref["info"][k], 1e-300), (k, g["info"], ref["info"])
        if ref["info"][0] - ref["info"][1] < 10:
            assert g["n_in"] == 0 and np.array_equal(g["S12"], S0)           # the early return: S12 unchanged, bit for bit
        else:
            assert g["n_in"] == g["keep"].sum() and abs(g["n_in"] - ref["n_in"]) <= band.sum()
            assert np.abs(g["S12"] - ref["S12"]).max() <= T.GPU_FACTOR * T.OPT_S_DEV
            assert not fix or g["S12"][7] == S0[7]
    assert sizes == set(T.OPT_SIZES)
    assert any(any(reference(i)["last_rejected"]) for i in idx)


def test_host_form_equals_device_form():
    idx, cs, out = batch(False)
    for j in (0, 3, len(cs) - 1):
        p, S0, valid, fix, th2 = cs[j]
        h = sim3.optimize_sim3(p, S0, th2, fix, valid)
        for k in ("S12", "keep", "info"):
            assert np.array_equal(h[k], out[j][k]), (j, k)
        assert h["n_in"] == out[j]["n_in"]
