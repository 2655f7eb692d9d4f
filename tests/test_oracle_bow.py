"""Pins the oracle's DBoW2 transform and SearchByBoW restatements (oracle/bow.cpp) with literal numpy/pure-Python
re-derivations (the reference has no vectors for them: parity unpinned, see oracle/bow.h). The SearchByBoW literal lives in tests/bow_ref.py."""
import numpy as np
import pytest
from viorb_amd.synth import make_vocabulary, descriptors_near_words
from bow_ref import literal_search
from kf_matcher_ref import ham


def descend(voc, d, levelsup):
    node, cur, lvl, nid = 0, 0, 0, 0
    nid_level = voc["L"] - levelsup
    while True:
        lvl += 1
        ch = voc["child_ids"][voc["child_start"][cur]:voc["child_start"][cur + 1]]
        dist = [ham(d, voc["desc"][c]) for c in ch]
        cur = int(ch[int(np.argmin(dist))])             # argmin = first minimum, as the strict '<' of the reference
        if lvl == nid_level:
            nid = cur
        if voc["child_start"][cur + 1] == voc["child_start"][cur]:
            break
    return voc["word_id"][cur], voc["weight"][cur], nid


@pytest.mark.parametrize("k,L,levelsup", [(10, 4, 2), (8, 5, 4), (3, 6, 4), (10, 3, 4)])
def test_transform_matches_literal_descent(oracle, k, L, levelsup):
    voc = make_vocabulary(1, k, L)
    assert len(voc["word_id"]) == sum(k ** l for l in range(L + 1)) and (voc["word_id"] >= 0).sum() == k ** L
    desc = np.concatenate([descriptors_near_words(2, voc, 150), np.random.default_rng(3).integers(0, 256, (50, 32), dtype=np.uint8)])
    r = oracle.bow_transform(voc, desc, levelsup)
    bow = {}
    for i, d in enumerate(desc):
        w, wt, nid = descend(voc, d, levelsup)
        assert (r["word"][i], r["weight"][i], r["node"][i]) == (w, wt, nid)
        if wt > 0:
            bow[int(w)] = bow.get(int(w), 0.0) + wt
    keys = sorted(bow)
    norm = 0.0
    for kk in keys:
        norm += abs(bow[kk])
    assert list(r["bow_ids"]) == keys
    assert np.array_equal(r["bow_vals"], np.array([bow[kk] / norm for kk in keys]))
    if L - levelsup <= 0:
        assert (r["node"] == 0).all()


@pytest.mark.parametrize("seed,ori", [(0, True), (1, False), (2, True)])
def test_search_by_bow_matches_literal(oracle, seed, ori):
    rng = np.random.default_rng(seed)
    voc = make_vocabulary(5, 6, 5)
    nK, nF = 300, 340
    kd = descriptors_near_words(seed, voc, nK, 4)
    # frame descriptors: noisy copies of a subset of the key frame's + fresh ones, shuffled
    src = rng.permutation(nK)[:220]
    fd = kd[src].copy()
    for _ in range(10):
        b = rng.integers(0, 256, len(fd)); fd[np.arange(len(fd)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    fd = np.concatenate([fd, descriptors_near_words(seed + 50, voc, nF - len(fd), 4)])
    ka = rng.uniform(0, 360, nK).astype(np.float32)
    fa = np.concatenate([ka[src] + rng.choice([5.0, 5.0, 5.0, 130.0], len(src)) + rng.normal(0, 3, len(src)), rng.uniform(0, 360, nF - len(src))]).astype(np.float32) % np.float32(360)
    perm = rng.permutation(nF); fd, fa = fd[perm], fa[perm]
    kn = oracle.bow_transform(voc, kd)["node"].copy(); fn = oracle.bow_transform(voc, fd)["node"].copy()
    kn[rng.random(nK) < 0.02] = -1                       # stopped words: not in the FeatureVector
    kh = (rng.random(nK) < 0.8).astype(np.uint8)
    n, m = oracle.search_by_bow(kd, ka, kn, kh, fd, fa, fn, 0.7, ori)
    n2, m2 = literal_search(kd, ka, kn, kh, fd, fa, fn, 0.7, ori)
    assert n == n2 and np.array_equal(m, m2)
    assert n > 60                                        # the planted correspondences are found
