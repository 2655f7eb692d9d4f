"""The hand-built matcher cases (tests/kf_matcher_cases.py) on the CPU: the oracle equals the literal restatement on every case, and every
decision rule a case claims to decide does change the literal's output when altered — so a kernel with that rule wrong cannot pass the
GPU parity tests that run the same cases (tests/test_gpu_kf_matcher.py, tests/test_gpu_bow.py)."""
import numpy as np
import pytest
import kf_matcher_ref as T
import bow_ref
import kf_matcher_cases as K


@pytest.mark.parametrize("name", sorted(K.TRI_CASES))
def test_triangulation_case(oracle, name):
    c = K.TRI_CASES[name]()
    for ori in sorted({c["ori"], False}):
        n, m = oracle.search_for_triangulation(*K.tri_args(c, ori))
        n_lit, m_lit = T.literal_triangulation(c["p"], c["only_stereo"], ori)
        assert n == n_lit and np.array_equal(m, m_lit), (name, ori)
    assert name == "tri_f_zero" or n_lit >= 24                       # the planted structures sit inside an ordinary problem
    for rule in c["rules"]:
        assert not np.array_equal(T.literal_triangulation(c["p"], c["only_stereo"], c["ori"], rule)[1], m_lit), (name, rule)


def test_triangulation_specifics():
    c = K.tri_f_zero()
    n, m = T.literal_triangulation(c["p"], False, True)
    assert n == 0 and (m == -1).all()
    p = K.tri_ties_thresholds()["p"]
    assert len(p["k2"]) < len(p["k1"]) and all(v & (v - 1) for v in (len(p["k1"]), len(p["k2"])))      # sort padding: n2 < n1, no power of two
    assert p["node1"].max() == 2 ** 31 - 2 and p["node1"].min() == -1 and 0 in p["node1"] and 0 in p["node2"]
    assert set(p["node1"]) - set(p["node2"]) and set(p["node2"]) - set(p["node1"])                       # nodes present in one frame only
    ex, ey = T.epipole(K.tri_epipole()["p"])
    assert abs(ex - p["intr4"][2]) < 0.01 and abs(ey - p["intr4"][3]) < 0.01                             # forward motion: the epipole is at (cx, cy)
    kept = lambda counts: sorted(T.three_maxima([counts.get(b, 0) for b in range(30)]))
    assert kept({3: 20, 6: 20, 1: 2, 8: 2}) == [1, 3, 6] and kept({4: 30, 9: 3, 11: 2}) == [4, 9] and kept({4: 30, 9: 2, 11: 2}) == [4]
    assert kept({2: 20, 5: 7, 12: 2, 0: 1}) == [2, 5, 12] and kept({2: 20, 5: 7, 12: 1}) == [2, 5] and kept({}) == []


@pytest.mark.parametrize("name", sorted(K.FUSE_CASES))
def test_fuse_case(oracle, name):
    c = K.FUSE_CASES[name]()
    n, b = K.fuse_oracle(oracle, c)
    n_lit, b_lit = K.fuse_literal(c)
    assert n == n_lit and np.array_equal(b, b_lit), name
    assert n_lit >= 24
    for rule in c["rules"]:
        assert not np.array_equal(K.fuse_literal(c, rule)[1], b_lit), (name, rule)


@pytest.mark.parametrize("name", sorted(K.BOW_CASES))
def test_bow_case(oracle, name):
    c = K.BOW_CASES[name]()
    for ori in (True, False):
        n, m = oracle.search_by_bow(*c["args"], c["ratio"], ori)
        n_lit, m_lit = bow_ref.literal_search(*c["args"], c["ratio"], ori)
        assert n == n_lit and np.array_equal(m, m_lit), (name, ori)
    assert n_lit >= 24
    n_lit, m_lit = bow_ref.literal_search(*c["args"], c["ratio"], c["ori"])
    for rule in c["rules"]:
        assert not np.array_equal(bow_ref.literal_search(*c["args"], c["ratio"], c["ori"], rule)[1], m_lit), (name, rule)
    assert max(np.bincount(c["args"][6][c["args"][6] >= 0])) >= 65    # a node whose frame features need a second pass of the 64-lane scan


def test_every_rule_is_decided_by_a_case():
    """Each rule of the three lists is claimed by at least one case (and test_*_case proves each claim)."""
    for rules, cases in ((T.TRIANGULATION_RULES, K.TRI_CASES), (T.FUSE_RULES, K.FUSE_CASES), (bow_ref.BOW_RULES, K.BOW_CASES)):
        decided = {r: [n for n, f in cases.items() if r in f()["rules"]] for r in rules}
        assert all(decided.values()), {r: v for r, v in decided.items() if not v}
        assert {r for f in cases.values() for r in f()["rules"]} <= set(rules)
