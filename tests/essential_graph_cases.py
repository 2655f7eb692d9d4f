"""The case list of the essential-graph tests: tests/test_essential_graph_ref.py measures the checker's two Jacobian modes on it (no GPU),
tests/test_gpu_essential_graph.py runs the library on it. A case is (name, seed, N, fix_scale, options of
synth.make_essential_graph_problem). With key frame 0 fixed, N = 2, 9, 10, 11, 37, 110 give systems of order 7, 56, 63, 70, 252, 763:
one free vertex, just under a 64-tile of the factorisation, the last order that fits one tile, just past it, a non-multiple near four
tiles, a dozen block columns. The checker's results are computed once per process and shared."""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viorb_amd import synth  # noqa: E402
import essential_graph_ref as ER  # noqa: E402

SIZES = (2, 9, 10, 11, 37, 110)
# The drift of a scene is chosen so that Gauss-Newton needs at least three iterations before its gain reaches the rounding floor of chi2
# (the condition tests/test_essential_graph_ref.py asserts on the checker alone): a strong drift per step on the short loops, a weak one
# that accumulates on the long loop.
_STRONG = dict(turn=0.3, rot_drift=0.1, scale_drift=0.1, trans_drift=0.1)
_DRIFT = {2: (dict(turn=0.3, rot_drift=0.4, scale_drift=0.4, trans_drift=0.4), dict(turn=0.3, rot_drift=0.7, scale_drift=0.7, trans_drift=0.7)),
          37: (dict(turn=0.3, rot_drift=0.05, scale_drift=0.05, trans_drift=0.05), _STRONG),
          110: (dict(rot_drift=0.02, scale_drift=0.01, trans_drift=0.03),) * 2}
CASES = [("n%d_%s" % (N, "fix" if fs else "free"), 700 + N, N, fs, _DRIFT.get(N, (_STRONG, _STRONG))[int(fs)]) for N in SIZES for fs in (False, True)] + [
    ("duplicated_pair", 731, 12, False, dict(duplicate_pair=True, **_STRONG)),
    ("two_fixed_edge", 732, 12, False, dict(extra_fixed=(1,), **_STRONG)),
    ("three_fixed_inside", 733, 24, False, dict(extra_fixed=(8, 12, 16), loop_edges=2, **_STRONG)),
    ("consistent", 734, 12, False, dict(consistent=True)),
    ("points", 735, 16, False, dict(n_points=200, skip_frac=0.15, **_STRONG)),
]
ZERO_CHI2 = ("consistent",)            # chi2 is the squared rounding of the errors from the start: no trial of it is decidable
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def problem(name):
    _, seed, N, fs, opt = CASES[NAMES.index(name)]
    return synth.make_essential_graph_problem(seed, N=N, fix_scale=fs, **opt)


@functools.lru_cache(maxsize=None)
def reference(name, mode="numeric"):
    """The checker's result of a case; computed once, never modified by a test."""
    return ER.optimize(problem(name), mode)
