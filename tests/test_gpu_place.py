"""GPU tests of place recognition (viorb_bow_vector*, viorb_bow_score*, viorb_kfdb_*): everything is compared bit for bit with the
checker tests/place_ref.py (and the oracle's BowVector), candidate order included."""
import ctypes as C
import functools
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi, place
from viorb_amd.capi import ptr
from viorb_amd.synth import make_place_problem, make_place_descriptors, make_vocabulary, descriptors_near_words
import place_ref as pr

pytestmark = pytest.mark.gpu

PROBLEMS = [(N, per, seed) for (N, per) in ((48, 120), (130, 300)) for seed in range(4)]


def rand_bow(rng, n_words, n):
    ids = np.sort(rng.choice(n_words, n, replace=False)).astype(np.int32)
    v = rng.uniform(0.05, 8.0, n)
    return pr.bow_vector(ids, v)


@functools.lru_cache(maxsize=None)
def problem(N, per, seed):
    p = make_place_problem(seed, N, per, 4096)
    return p, pr.loop_min_score(p)


def device_db(p, **hints):
    db = place.KeyFrameDatabase(p["n_words"], **hints)
    for s, b in enumerate(p["bows"][:-1]):
        assert db.add(b) == s
    for e in p["erased"]:
        db.erase(e)
    return db


def assert_query_equals(got, q, ref):
    assert got["stats"][q].tolist() == ref["stats"]
    assert np.array_equal(got["common"][q], ref["common"])
    assert np.array_equal(got["score"][q].view(np.uint32), ref["score"].view(np.uint32))
    assert got["cand"][q] == ref["cand"]


# ---- BowVector ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,L", [(1, 3, 3), (64, 3, 3), (65, 3, 3), (1000, 3, 3), (2000, 3, 3), (1000, 10, 4)])
def test_bow_vector_equals_the_oracle(oracle, n, k, L):
    voc = make_vocabulary(2, k=k, L=L)
    ref = oracle.bow_transform(voc, descriptors_near_words(n, voc, n))
    ids, vals = viorb_amd.BowVector(ref["word"], ref["weight"])
    assert np.array_equal(ids, ref["bow_ids"])
    assert np.array_equal(vals.view(np.uint64), ref["bow_vals"].view(np.uint64))
    if k == 3 and n >= 1000:
        assert len(ids) <= 27 and n / len(ids) > 30          # many features per word: the order inside a segment matters


def test_bow_vector_of_stopped_words_only_is_empty():
    ids, vals = viorb_amd.BowVector(np.arange(100, dtype=np.int32) % 7, np.zeros(100))
    assert len(ids) == 0 and len(vals) == 0


def test_bow_vector_batch_of_unequal_counts_equals_the_singles():
    import torch
    rng = np.random.default_rng(3)
    counts = [300, 0, 1, 257, 190]
    cap = 300
    word, weight = rng.integers(0, 40, (5, cap)).astype(np.int32), rng.uniform(0.05, 8.0, (5, cap))
    weight[rng.random((5, cap)) < 0.1] = 0.0
    dev = torch.device("cuda", 0)
    bw, bv, bc = place.BowVector_device(torch.from_numpy(word).to(dev), torch.from_numpy(weight).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    bw, bv, bc = bw.cpu().numpy(), bv.cpu().numpy(), bc.cpu().numpy()
    for b, n in enumerate(counts):
        ids, vals = pr.bow_vector(word[b, :n], weight[b, :n])
        assert bc[b] == len(ids)
        assert np.array_equal(bw[b, :bc[b]], ids) and np.array_equal(bv[b, :bc[b]].view(np.uint64), vals.view(np.uint64))
        si, sv = viorb_amd.BowVector(word[b, :n], weight[b, :n])
        assert np.array_equal(si, ids) and np.array_equal(sv.view(np.uint64), vals.view(np.uint64))


def test_bow_vector_at_and_over_the_capacity():
    rng = np.random.default_rng(4)
    n = place.BOW_VECTOR_MAX_FEATURES
    word, weight = rng.integers(0, 1000, n + 1).astype(np.int32), rng.uniform(0.05, 8.0, n + 1)
    ids, vals = viorb_amd.BowVector(word[:n], weight[:n])
    ri, rv = pr.bow_vector(word[:n], weight[:n])
    assert np.array_equal(ids, ri) and np.array_equal(vals.view(np.uint64), rv.view(np.uint64))
    with pytest.raises(viorb_amd.ViorbError) as e:          # refused, never truncated
        viorb_amd.BowVector(word, weight)
    assert e.value.code == capi.ERR_CAPACITY


# ---- score --------------------------------------------------------------------------------------------------------------------------
def test_score_pairs_equal_the_checker():
    rng = np.random.default_rng(7)
    nw = 5000
    A = [rand_bow(rng, nw, n) for n in (63, 64, 65, 1000, 1, 200)]
    B = [rand_bow(rng, nw, n) for n in (65, 64, 63, 1000, 900, 3)]
    A.append(A[3]); B.append(A[3])                                           # identical vectors: every word common
    lo, hi = np.arange(0, 100, dtype=np.int32), np.arange(100, 150, dtype=np.int32)
    A.append(pr.bow_vector(lo, np.ones(100))); B.append(pr.bow_vector(hi, np.ones(50)))          # no common word
    A.append(pr.bow_vector(np.append(lo, 120).astype(np.int32), rng.uniform(1, 2, 101))); B.append(B[-1])   # exactly one, the shorter vector on side b
    B.append(A[-1]); A.append(B[-2])                                         # ... and on side a
    pairs = [(i, j) for i in range(len(A)) for j in range(len(B))]
    got = viorb_amd.BowScorePairs(A, B, pairs)
    ref = np.array([pr.score(A[i], B[j]) for i, j in pairs])
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    common = [len(np.intersect1d(A[i][0], B[j][0])) for i, j in pairs]
    assert 0 in common and 1 in common and 1000 in common
    assert viorb_amd.BowScore(A[0], B[0]) == pr.score(A[0], B[0])
    assert pr.score(A[7], B[7]) == 0.0 and got[pairs.index((7, 7))] == 0.0


def test_score_300_pairs_in_one_call():
    rng = np.random.default_rng(8)
    V = [rand_bow(rng, 800, int(rng.integers(1, 400))) for _ in range(30)]
    pairs = rng.integers(0, 30, (300, 2))
    got = viorb_amd.BowScorePairs(V, V, pairs)
    ref = np.array([pr.score(V[i], V[j]) for i, j in pairs.tolist()])
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


# ---- the key-frame database ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pr.LOOP, pr.RELOC])
@pytest.mark.parametrize("N,per,seed", PROBLEMS)
def test_database_query_equals_the_checker(N, per, seed, mode):
    p, ms = problem(N, per, seed)
    q = p["bows"][-1]
    ref = pr.build(p).detect(mode, q, p["covis10"], ms, p["connected"])
    db = device_db(p)
    assert db.size() == (N - 1, N - 1 - len(p["erased"]))
    got = db.query(mode, [q], p["covis10"], [ms], [p["connected"]])
    assert_query_equals(got, 0, ref)
    one = db.detect_loop_candidates(q, ms, p["connected"], p["covis10"]) if mode == pr.LOOP else db.detect_relocalization_candidates(q, p["covis10"])
    assert one == ref["cand"]


def test_min_score_between_two_scores_removes_a_scored_slot():
    p, _ = problem(48, 120, 0)
    q = p["bows"][-1]
    sc = pr.build(p).detect(pr.LOOP, q, p["covis10"], 0.0, p["connected"])["score"]
    sc = np.sort(sc[sc >= 0])
    mid = np.float32((float(sc[0]) + float(sc[-1])) / 2)
    ref = pr.build(p).detect(pr.LOOP, q, p["covis10"], mid, p["connected"])
    assert 0 < ref["stats"][3] < ref["stats"][2]
    assert_query_equals(device_db(p).query(pr.LOOP, [q], p["covis10"], [mid], [p["connected"]]), 0, ref)
    exact = np.float32(sc[1])                                               # si >= minScore keeps the equal one
    ref = pr.build(p).detect(pr.LOOP, q, p["covis10"], exact, p["connected"])
    assert_query_equals(device_db(p).query(pr.LOOP, [q], p["covis10"], [exact], [p["connected"]]), 0, ref)


@pytest.mark.parametrize("mode", [pr.LOOP, pr.RELOC])
def test_five_queries_in_one_call_equal_five_calls(mode):
    p, _ = problem(130, 300, 1)
    db, rdb = device_db(p), pr.build(p)
    qs = [p["bows"][i] for i in (129, 3, 70, 100, 128)]
    conn = [p["connected"], [0, 1, 2, 4, 5], [], [99, 101, 98], list(range(100, 129))]
    ms = [np.float32(x) for x in (0.15, 0.1, 0.0, 0.2, 0.05)]
    got = db.query(mode, qs, p["covis10"], ms, conn)
    for i in range(5):
        ref = rdb.detect(mode, qs[i], p["covis10"], ms[i], conn[i])
        assert_query_equals(got, i, ref)
        assert_query_equals(db.query(mode, [qs[i]], p["covis10"], [ms[i]], [conn[i]]), 0, ref)


def test_empty_database_and_every_slot_excluded():
    p, ms = problem(48, 120, 2)
    q = p["bows"][-1]
    db = place.KeyFrameDatabase(4096)
    for mode in (pr.LOOP, pr.RELOC):
        got = db.query(mode, [q], np.zeros((0, 10), np.int32), [ms], [[]])
        assert got["cand"] == [[]] and got["stats"][0].tolist() == [0, 0, 0, 0]
    db = device_db(p)
    got = db.query(pr.LOOP, [q], p["covis10"], [ms], [list(range(47))])
    assert got["cand"] == [[]] and got["stats"][0].tolist() == [0, 0, 0, 0] and not got["common"].any() and (got["score"] == -1).all()
    db.clear()
    assert db.size() == (0, 0)
    assert db.add(q) == 0                                                    # as a new database
    assert db.detect_relocalization_candidates(q, np.full((1, 10), -1)) == [0]


@pytest.mark.parametrize("S", [1, 63, 65])
def test_small_databases_and_a_key_frame_with_one_word(S):
    rng = np.random.default_rng(20 + S)
    nw = 300
    bows = [rand_bow(rng, nw, int(rng.integers(20, 90))) for _ in range(S)]
    q = rand_bow(rng, nw, 80)
    bows[S // 2] = pr.bow_vector(q[0][5:6], np.ones(1))                      # one word, shared with the query
    cov = np.full((S, 10), -1, np.int32)
    for s in range(S):
        near = [t for d in range(1, 6) for t in (s + d, s - d) if 0 <= t < S]
        cov[s, :len(near)] = near
    db, rdb = place.KeyFrameDatabase(nw), pr.KeyFrameDB()
    for b in bows:
        db.add(b); rdb.add(b)
    if S > 1:
        db.erase(1); rdb.erase(1)
        db.erase(1)                                                          # erasing twice changes nothing
        assert db.size() == (S, S - 1)
    for mode in (pr.LOOP, pr.RELOC):
        ref = rdb.detect(mode, q, cov, 0.01, [0] if S > 1 else [])
        assert ref["common"][S // 2] == 1 or S == 1 or S // 2 in (0, 1)
        assert_query_equals(db.query(mode, [q], cov, [0.01], [[0] if S > 1 else []]), 0, ref)


def test_query_longer_than_the_lds_form():
    rng = np.random.default_rng(31)
    nw = 20000
    bows = [rand_bow(rng, nw, 300) for _ in range(20)]
    q = rand_bow(rng, nw, 9000)
    assert len(q[0]) == 9000
    cov = np.full((20, 10), -1, np.int32)
    cov[:, 0] = (np.arange(20) + 1) % 20
    db, rdb = place.KeyFrameDatabase(nw), pr.KeyFrameDB()
    for b in bows:
        db.add(b); rdb.add(b)
    for mode in (pr.LOOP, pr.RELOC):
        ref = rdb.detect(mode, q, cov, 0.0, [3])
        assert ref["stats"][0] >= 19 and ref["stats"][1] > 100
        assert_query_equals(db.query(mode, [q], cov, [0.0], [[3]]), 0, ref)


def test_more_candidates_than_cand_cap_is_an_error():
    p, ms = problem(48, 120, 1)
    q = p["bows"][-1]
    ref = pr.build(p).detect(pr.LOOP, q, p["covis10"], ms, p["connected"])
    assert len(ref["cand"]) == 2
    db = device_db(p)
    with pytest.raises(viorb_amd.ViorbError) as e:
        db.query(pr.LOOP, [q], p["covis10"], [ms], [p["connected"]], cand_cap=1)
    assert e.value.code == capi.ERR_CAPACITY
    assert db.query(pr.LOOP, [q], p["covis10"], [ms], [p["connected"]], cand_cap=2)["cand"][0] == ref["cand"]


def test_a_grown_arena_equals_one_created_large():
    p, ms = problem(130, 300, 3)
    q = p["bows"][-1]
    small, large = device_db(p, kf_capacity_hint=4, entry_capacity_hint=256), device_db(p, kf_capacity_hint=4096, entry_capacity_hint=1 << 20)
    for mode in (pr.LOOP, pr.RELOC):
        ref = pr.build(p).detect(mode, q, p["covis10"], ms, p["connected"])
        assert_query_equals(small.query(mode, [q], p["covis10"], [ms], [p["connected"]]), 0, ref)
        assert_query_equals(large.query(mode, [q], p["covis10"], [ms], [p["connected"]]), 0, ref)


def test_interleaved_query_add_erase_follows_the_checker():
    """The order DetectLoop produces: query with the current key frame, then add it; now and then a key frame is culled."""
    p = make_place_problem(5, 41, 120, 4096, erase_frac=0.0)
    rng = np.random.default_rng(6)
    db, rdb = place.KeyFrameDatabase(4096, kf_capacity_hint=8, entry_capacity_hint=512), pr.KeyFrameDB()
    n_cand = 0
    for step in range(40):
        bow, S = p["bows"][step], step
        cov = p["covis10"][:S].copy()
        cov[cov >= S] = -1
        conn = list(range(max(S - 4, 0), S))
        mode = pr.LOOP if step % 3 else pr.RELOC
        ms = np.float32(0.05)
        ref = rdb.detect(mode, bow, cov, ms, conn)
        got = db.query(mode, [bow], cov if S else np.zeros((0, 10), np.int32), [ms], [conn])
        assert_query_equals(got, 0, ref)
        n_cand += len(ref["cand"])
        assert db.add(bow) == rdb.add(bow) == S
        if step % 7 == 6:
            e = int(rng.integers(0, S))
            db.erase(e); rdb.erase(e)
    assert n_cand >= 10


def test_device_chain_without_a_host_copy_equals_the_host_forms():
    """viorb_bow_transform_device -> viorb_bow_vector_device -> viorb_kfdb_add_device -> viorb_kfdb_query_device on one stream."""
    import torch
    voc = make_vocabulary(4, k=10, L=3)
    p = make_place_descriptors(1, voc, N=24, per_kf=100)
    N, per, S = 24, 100, 23
    V = viorb_amd.ORBVocabulary(voc)
    dev = torch.device("cuda", 0)
    desc = torch.from_numpy(np.stack(p["desc"])).to(dev)
    count = torch.full((N,), per, dtype=torch.int32, device=dev)
    word, node = torch.zeros((N, per), dtype=torch.int32, device=dev), torch.zeros((N, per), dtype=torch.int32, device=dev)
    weight = torch.zeros((N, per), dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    capi.check(viorb_amd.lib().viorb_bow_transform_device(V.h, ptr(desc), ptr(count), per, N, 4, ptr(word), ptr(weight), ptr(node), st))
    bw, bv, bc = place.BowVector_device(word, weight, count)
    db = place.KeyFrameDatabase(1000, kf_capacity_hint=32, entry_capacity_hint=32 * per)
    assert db.add_device(bw[:10], bv[:10], bc[:10]) == 0
    assert db.add_device(bw[10:S], bv[10:S], bc[10:S]) == 10
    for e in p["erased"]:
        db.erase(e)
    cov = torch.from_numpy(p["covis10"]).to(dev)
    conn = np.array(p["connected"], np.int32)
    ms = torch.tensor([0.02, 0.02], dtype=torch.float32, device=dev)
    es, ex = torch.tensor([0, len(conn), len(conn)], dtype=torch.int32, device=dev), torch.from_numpy(conn).to(dev)
    qsel = [S, 2]
    out = {m: db.query_device(m, bw[qsel].contiguous(), bv[qsel].contiguous(), bc[qsel].contiguous(), cov, ms, es, ex, cand_cap=32) for m in (pr.LOOP, pr.RELOC)}
    torch.cuda.synchronize()
    # the host forms, and the checker
    bows = [viorb_amd.BowVector(*V.transform_features(d, 4)[:2]) for d in p["desc"]]
    hb, hc = bw.cpu().numpy(), bc.cpu().numpy()
    for i in range(N):
        assert np.array_equal(hb[i, :hc[i]], bows[i][0])
    hdb, rdb = place.KeyFrameDatabase(1000), pr.KeyFrameDB()
    for b in bows[:S]:
        hdb.add(b); rdb.add(b)
    for e in p["erased"]:
        hdb.erase(e); rdb.erase(e)
    for m in (pr.LOOP, pr.RELOC):
        host = hdb.query(m, [bows[S], bows[2]], p["covis10"], [0.02, 0.02], [p["connected"], []])
        o = out[m]
        ncand, cand = o["n_cand"].cpu().numpy(), o["cand"].cpu().numpy()
        for qi in range(2):
            assert cand[qi, :ncand[qi]].tolist() == host["cand"][qi]
            ref = rdb.detect(m, [bows[S], bows[2]][qi], p["covis10"], np.float32(0.02), [p["connected"], []][qi])
            assert_query_equals(host, qi, ref)
        assert np.array_equal(o["stats"].cpu().numpy(), host["stats"])
        assert np.array_equal(o["common"].cpu().numpy(), host["common"])
        assert np.array_equal(o["score"].cpu().numpy().view(np.uint32), host["score"].view(np.uint32))
    assert len(host["cand"][0]) >= 1
