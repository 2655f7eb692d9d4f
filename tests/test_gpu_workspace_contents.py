"""The results of the device entry points that take a caller workspace do not depend on what the workspace held. The headers promise
"contents on entry are ignored"; a caller of the drop-in keeps one allocation across key frames and problems of different sizes, while
the wrappers (and so every other GPU test) hand over zeroed or fresh memory. Each case here runs on one allocation of capi.Workspace
under three conditions:
  (a) zeroed: every byte 0, twice, which also tells whether the entry point is bit-reproducible;
  (b) 0xFF:   every byte 0xFF, the 4096 guard bytes behind the workspace included (NaN as f32 / f64, -1 as an index or a count);
  (c) stale:  what a different, larger case of the same entry point left behind on the same allocation, untouched in between.
(b) and (c) must equal (a): bit for bit where (a) is bit-reproducible, which every entry point but the two global bundle adjustments is
(their own tests state it); the bundle adjustments within the tolerance of their test_run_to_run_agreement. The result of every condition
must also still equal the module's checker, as the existing test of that case asserts it, and the guard bytes behind the workspace must
be what they were before the call. The cases are the smallest existing ones of each module's tests that reach every kernel of the call;
each test names the kernels."""
import functools
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd.capi import lib

pytestmark = pytest.mark.gpu
f32 = np.float32


# ---- the three conditions ---------------------------------------------------------------------------------------------------------------
def _flat(x, path=""):
    """(path, array) of every leaf of nested dicts / lists / arrays / tensors / numbers; the wrappers' own "workspace" entries are left out."""
    if isinstance(x, dict):
        return [l for k in sorted(x) if k != "workspace" for l in _flat(x[k], "%s.%s" % (path, k))]
    if isinstance(x, (list, tuple)):
        return [l for i, v in enumerate(x) for l in _flat(v, "%s[%d]" % (path, i))]
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return [(path, np.asarray(x))] if x is not None else [(path, np.zeros(0))]


def _differing(a, b):
    """The leaves of two results that are not bit for bit the same."""
    fa, fb = _flat(a), _flat(b)
    assert [p for p, _ in fa] == [p for p, _ in fb]
    return [p for (p, x), (_, y) in zip(fa, fb) if x.shape != y.shape or x.dtype != y.dtype or np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes()]


def conditions(nbytes, nbytes_big, run, run_big):
    """run(ws) / run_big(ws) solve the case under test / the larger case on the capi.Workspace ws (of which they may use the first nbytes /
    nbytes_big) with fresh output arrays and return the results. Returns dict(zero, again, ff, stale) of the case under test; the guard
    behind the workspace is compared around every call."""
    import torch
    nbytes, nbytes_big = int(nbytes), int(nbytes_big)
    assert 0 < nbytes < nbytes_big, (nbytes, nbytes_big)                # a different, LARGER case: its words lie all over the smaller one's
    ws = capi.Workspace(torch, torch.device("cuda", 0), nbytes_big)

    def guarded(fn, n, what):
        before = ws.guard(n).clone()
        out = fn(ws)
        torch.cuda.synchronize()
        assert torch.equal(ws.guard(n), before), "%s: the guard bytes behind the workspace were written" % what
        return out
    out = {}
    for what, fill in (("zero", 0), ("again", 0), ("ff", 0xFF)):
        ws.fill(fill)
        out[what] = guarded(run, nbytes, what)
    ws.fill(0)
    guarded(run_big, nbytes_big, "the larger case")
    assert bool(ws.body(nbytes).any()), "the larger case left nothing behind"
    out["stale"] = guarded(run, nbytes, "stale")
    return out


def exact(res, check):
    """Bit-reproducible, and the same bits whatever the workspace held; every condition still passes the module's own check."""
    assert _differing(res["zero"], res["again"]) == [], "not bit-reproducible on a zeroed workspace"
    for what in ("ff", "stale"):
        assert _differing(res["zero"], res[what]) == [], what
    for what in ("zero", "ff", "stale"):
        check(res[what])


def _inject(obj, ws, nbytes, attr="ws"):
    """The wrapper's own workspace replaced by the shared allocation."""
    assert ws.fits(nbytes)
    setattr(obj, attr, ws)
    return obj


# ---- viorb_search_init_workspace_bytes -----------------------------------------------------------------------------------------------------
def _search_init(cases, cap):
    from viorb_amd import search_init as M
    import test_gpu_search_init as G
    c0 = cases[0]

    def run(ws):
        bt = M.SearchInitBatch([(c["kps1"], c["desc1"]) for c in cases], [c["prev_matched"] for c in cases], c0["bounds4"], cap)
        _inject(bt, ws, bt.ws_bytes)
        g = G._garbage(c0)
        bt.set_frame1([(c["kps1"], c["desc1"]) for c in cases], g)
        return bt.search([(c["kps2"], c["desc2"]) for c in cases], garbage=g, window_size=c0["window_size"], nnratio=c0["nnratio"],
                         check_orientation=c0["check_orientation"])
    return lib().viorb_search_init_workspace_bytes(cap, len(cases)), run


@pytest.mark.parametrize("which", ["overfull", "staircase"])
def test_search_for_initialization(which):
    """k_si_candidates and k_si_ordered. overfull (test_a_window_with_more_candidates_than_a_list_holds): a point whose window holds more
    candidates than its list in the workspace, so k_si_ordered rescans it beside points it reads from the list; descending staircase
    (test_descending_staircase): 50 displaced points, the chains of `next` and both state arrays over many sweeps. Larger case: the fixture
    of test_device_entry_batch_1_equals_the_checker."""
    from viorb_amd import search_init as M
    import search_init_cases as K
    import test_gpu_search_init as G
    c, cap = (K.overfull(M.shape()[2]), 64) if which == "overfull" else (K.descending_staircase(70), 128)
    want = G._want(c, K.run_ref(c))
    n, run = _search_init([c], cap)
    nb, run_big = _search_init([G._fixture_case(0)], 512)
    exact(conditions(n, nb, run, run_big), lambda r: G._check_device(r, [c], [want]))


# ---- viorb_two_view_workspace_bytes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("planar", 65), ("general", 130)])
def test_two_view_init(kind, n):
    """viorb_two_view_init_device: k_tv_prepare, k_tv_hypotheses, k_tv_score (all sets, then the two winners' flags), k_tv_select,
    k_tv_decompose, k_tv_check_rt and k_tv_accept; planar 65 is accepted from H (eight motion hypotheses), general 130 from F (four), as
    test_accepted_cases_recover_the_ground_truth asserts. Larger case: both kinds at n = 300 as one batch. The checker: the end-to-end
    result of the suite's one batch, which its tests hold to tests/two_view_ref.py stage by stage ("the batch a stream sits in does not
    matter", test_failure_reasons_and_the_host_entry)."""
    from viorb_amd import two_view as tv
    import test_gpu_two_view as G
    import two_view_ref as T
    p, sets = G.problem(kind, n)
    big = [G.problem(k, 300) for k in ("general", "planar")]

    def runner(probs, ss):
        def run(ws):
            B = tv.TwoViewBatch(probs, ss)
            return _inject(B, ws, B.ws_bytes).init()
        return lib().viorb_two_view_workspace_bytes(max(max(len(q["xy1"]), len(q["xy2"])) for q in probs), G.ITER, len(probs)), run
    want = G.device()["e2e"][G.idx(kind, n)]

    def check(r):
        assert r[0]["status"] == (T.FROM_H if kind == "planar" else T.FROM_F) and r[0]["reason"] == T.OK
        assert _differing(r[0], want) == []
    nb, run_big = runner([b[0] for b in big], [b[1] for b in big])
    n_, run = runner([p], [sets])
    exact(conditions(n_, nb, run, run_big), check)


# ---- viorb_sim3_workspace_bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", [dict(), dict(first=3, best=0, per=5)], ids=["all", "window"])
def test_sim3_ransac(state):
    """viorb_sim3_ransac_device: k_sim3_prepare, k_sim3_hypotheses, k_sim3_inliers (counts of the window, then the flags of the winner) and
    k_sim3_select, on the batch "three" of tests/test_gpu_sim3.py (three pairs of three correspondences, min_inliers 2): once over all 300
    iterations and once over the window [3, 8), outside of which the models and counts in the workspace are never written. Larger case:
    the batch "free" (17 pairs of up to 300 correspondences). The checker: the chain of the stage entries, as
    test_end_to_end_equals_the_chain_of_stages_bit_for_bit."""
    from viorb_amd import sim3
    import test_gpu_sim3 as G
    import sim3_ref as T
    first, best, per = state.get("first", 0), state.get("best", 0), state.get("per", G.ITERS)
    probs, sets, mi, fix, _ = G.cases("three")
    g = G.stage("three")

    def runner(name):
        ps, ss, m, fx, _ = G.cases(name)

        def run(ws):
            B = sim3.Sim3Batch(ps, ss, min_inliers=m, fix_scale=fx)
            return _inject(B, ws, B.ws_bytes).ransac(first_iteration=first, best_inliers_in=best, iterations_per_call=per)
        return lib().viorb_sim3_workspace_bytes(max(len(q["X1c"]) for q in ps), G.ITERS, len(ps)), run

    def check(r):
        assert any(o["status"] == T.FOUND for o in r)
        for b in range(len(probs)):
            G._same(r[b], G._expect(G.batch("three"), g, probs, mi, b, first, best, per), ("three", state, b))
    n, run = runner("three")
    nb, run_big = runner("free")
    exact(conditions(n, nb, run, run_big), check)


# ---- viorb_sim3_match_workspace_bytes -----------------------------------------------------------------------------------------------------
def _s3m(P, cap, call):
    """call(batch of P's first key frame, or of its fuse frames) on a fresh Sim3MatchBatch that owns nothing but the shared workspace."""
    import test_gpu_sim3_match as G

    def run(ws):
        return call(lambda frames, c=cap: _inject(G._batch(P, frames, cap=c), ws, 0))
    return run


@pytest.mark.parametrize("entry", ["search_by_sim3", "search_by_projection", "fuse"])
def test_sim3_matchers(entry):
    """The three entries that share viorb_sim3_match_workspace_bytes, on the problem SMALL of tests/test_gpu_sim3_match.py (300 features,
    150 common points, 60 duplicates): search_by_sim3 without the optional outputs, so that the one-way matches of k_s3m_oneway go
    through the workspace to k_s3m_mutual; search_by_projection: k_s3m_scw<ordered> and k_s3m_claim over the candidate lists;
    fuse: k_s3m_scw<unordered> and k_s3m_counts over the partial counts. Larger case: all three entries, one after the other as LoopClosing
    calls them on one allocation, on the fixture (1000 features, three key frames): each entry writes its own arrays only, and the partial
    counts of the small Fuse lie where the large SearchBySim3 kept its one-way matches. The checker: tests/sim3_match_ref.py."""
    from viorb_amd import sim3_match as M
    import sim3_match_cases as K
    import sim3_match_ref as T
    import test_gpu_sim3_match as G
    small, big = K.problem(*G.SMALL), K.problem()
    wb = lib().viorb_sim3_match_workspace_bytes

    def make(P, entry):
        a, b, L, F = P["kf1"], P["kf2"], P["loop"], P["fuse"]
        kf = K.ref_keyframe(P, a["kps"], a["desc"])
        if entry == "search_by_sim3":
            cap = max(len(a["kps"]), len(b["kps"])) + 3

            def call(batch):
                b1, b2 = batch([(a["kps"], a["desc"])]), batch([(b["kps"], b["desc"])])
                side = lambda bt, s: bt.side(*[[s[k]] for k in ("pose12", "has_point", "pts_f", "pts_desc", "already")])
                return b1.search_by_sim3(side(b1, a), b2, side(b2, b), P["R12"][None], P["t12"][None], np.array([P["s12"]], f32), th=K.TH_SIM3, raw=False)
            want = K.ref_search_by_sim3(P)
            check = lambda r: K.same(r[0], want, ("match12", "nfound"))
            return wb(cap, 1, 1), _s3m(P, cap, call), check
        if entry == "search_by_projection":
            cap, pcap = len(a["kps"]) + 24, len(L["pts_f"]) + 77
            call = lambda batch: batch([(a["kps"], a["desc"])]).search_by_projection(L["Scw"][None], [L["pts_f"]], [L["pts_desc"]], [L["valid"]], [L["feat_taken"]],
                                                                                    K.TH_PROJ, pcap=pcap)
            want = T.search_by_projection(kf, L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], L["feat_taken"], K.TH_PROJ)

            def check(r):
                K.same(r[0], want, G.PROJ_KEYS)
                assert (r[0]["tail"] == -1).all()
            return wb(cap, pcap, 1), _s3m(P, cap, call), check
        cap, pcap = max(len(k) for k, _ in F["frames"]) + 10, len(L["pts_f"]) + 5
        call = lambda batch: batch(F["frames"]).fuse(F["Scw"], L["pts_f"], L["pts_desc"], F["valid"], K.TH_FUSE, pcap=pcap)
        want = [T.fuse(K.ref_keyframe(P, k, d), F["Scw"][j], L["pts_f"], L["pts_desc"], F["valid"][j], K.TH_FUSE) for j, (k, d) in enumerate(F["frames"])]

        def check(r):
            for j in range(len(want)):
                K.same(r[j], want[j], G.FUSE_KEYS)
                assert (r[j]["tail"] == -1).all()
        return wb(cap, pcap, len(F["frames"])), _s3m(P, cap, call), check
    n, run, check = make(small, entry)
    larger = [make(big, e) for e in ("search_by_sim3", "search_by_projection", "fuse")]
    res = conditions(n, max(x[0] for x in larger), run, lambda ws: [x[1](ws) for x in larger])
    assert (res["zero"][0]["nfound"] if entry == "search_by_sim3" else res["zero"][0]["nmatches"] if entry == "search_by_projection" else res["zero"][0]["nfused"]) > 0
    exact(res, check)


# ---- viorb_create_new_map_points_workspace_bytes ---------------------------------------------------------------------------------------------
def test_create_new_map_points(oracle):
    """viorb_create_new_map_points_device over the first six neighbours of stream 0 of
    test_create_new_map_points_equals_the_sequential_loop[1-0.0] (monocular): per neighbour k_stage_neighbour (the staged copy of key
    frame 2 in the workspace), k_search_triangulation, k_triangulate_pairs and k_append_new_points. Larger case: three streams of that
    test. The checker: the sequential loop of tests/mapping_ref.py with the oracle's matcher."""
    from viorb_amd.synth import make_mapping_problem
    import test_gpu_mapping as G
    G.need_gpu()
    J = 6

    def problems(seeds):
        out = []
        for s in seeds:
            p = make_mapping_problem(s, J=20, stereo_frac=0.0)
            p["neigh"] = p["neigh"][:J]
            out.append(p)
        return out
    small, big = problems([10]), problems([10, 11, 12])

    def runner(probs):
        probe = [len(p["kf1"]["kps"]) for p in probs] + [len(n["kps"]) for p in probs for n in p["neigh"]]

        def run(ws):
            r = viorb_amd.CreateNewMapPoints(probs[0]["cam"], probs, J, pcap=1000, monocular=True)
            return _inject(r, ws, r.ws_bytes)().results()
        return lib().viorb_create_new_map_points_workspace_bytes(max(probe + [1]), len(probs)), run
    ref = G._run_ref(small[0], oracle, True)
    assert len(ref["new_idx"]) > 50 and len(np.unique(ref["new_idx"][:, 1])) >= 3

    def check(r):
        assert r[0]["status"] == 0
        G._compare_stream(r[0], ref, small[0], dict(pos=0.0, pairs=0, band=0))
    n, run = runner(small)
    nb, run_big = runner(big)
    exact(conditions(n, nb, run, run_big), check)


# ---- viorb_kfdb_query_workspace_bytes --------------------------------------------------------------------------------------------------------
def _kfdb_query(db, mode, bows, covis10, min_scores, connected):
    """viorb_kfdb_query_device on uploaded host arrays; returns (workspace bytes, run(ws) -> the dictionary of KeyFrameDatabase.query)."""
    import torch
    from viorb_amd import place
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n_q, S = len(bows), db.size()[0]
    qw, qv, qc = [up(a) for a in place.pack_bows(bows)]
    start, flat = db._csr(connected, n_q)
    cov, ms, es, ex = up(np.asarray(covis10, np.int32).reshape(-1, 10)), up(np.asarray(min_scores, np.float32)), up(start), up(flat)

    def run(ws):
        o = db.query_device(mode, qw, qv, qc, cov, ms, es, ex, cand_cap=max(S, 1), workspace=ws)
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in o.items() if k != "workspace"}
        return dict(cand=[h["cand"][q, :h["n_cand"][q]].tolist() for q in range(n_q)], stats=h["stats"], common=h["common"], score=h["score"], cand_all=h["cand"])
    return int(lib().viorb_kfdb_query_workspace_bytes(db.h, n_q)), run


@pytest.mark.parametrize("which", ["loop", "reloc", "long_query"])
def test_kfdb_query(which):
    """viorb_kfdb_query_device: k_kfdb_common (the query's words in LDS; long_query: 9000 words, the form that reads them from memory, as
    test_query_longer_than_the_lds_form), k_kfdb_threshold, k_kfdb_score and k_kfdb_select over the eight workspace arrays. loop / reloc:
    the problem (48, 120, 0) of test_database_query_equals_the_checker in either mode. Larger case: five queries on the problem
    (130, 300, 1), as test_five_queries_in_one_call_equal_five_calls. The checker: tests/place_ref.py."""
    from viorb_amd import place
    import place_ref as pr
    import test_gpu_place as G
    mode = pr.RELOC if which == "reloc" else pr.LOOP
    if which == "long_query":
        rng = np.random.default_rng(31)
        bows = [G.rand_bow(rng, 20000, 300) for _ in range(20)]
        q = G.rand_bow(rng, 20000, 9000)
        cov = np.full((20, 10), -1, np.int32)
        cov[:, 0] = (np.arange(20) + 1) % 20
        db, rdb = place.KeyFrameDatabase(20000), pr.KeyFrameDB()
        for b in bows:
            db.add(b); rdb.add(b)
        ms, conn = np.float32(0.0), [3]
    else:
        p, ms = G.problem(48, 120, 0)
        q, cov, conn = p["bows"][-1], p["covis10"], p["connected"]
        db, rdb = G.device_db(p), pr.build(p)
    ref = rdb.detect(mode, q, cov, ms, conn)
    assert len(ref["cand"]) >= 1
    n, run = _kfdb_query(db, mode, [q], cov, [ms], [conn])
    P, _ = G.problem(130, 300, 1)
    big_db = G.device_db(P)
    nb, run_big = _kfdb_query(big_db, mode, [P["bows"][i] for i in (129, 3, 70, 100, 128)], P["covis10"], [0.15, 0.1, 0.0, 0.2, 0.05],
                              [P["connected"], [0, 1, 2, 4, 5], [], [99, 101, 98], list(range(100, 129))])
    exact(conditions(n, nb, run, run_big), lambda r: G.assert_query_equals(r, 0, ref))


# ---- viorb_relocalization_workspace_bytes -----------------------------------------------------------------------------------------------------
def test_search_by_projection_reloc():
    """viorb_search_by_projection_reloc_device: k_reloc_gates and k_reloc_claim over the candidate lists, on the eight point counts of
    test_point_counts_around_the_workgroup_and_the_wavefront (one frame of 300 features, up to 513 points, rotation removals among
    them). Larger case: 24 hypotheses of 513 points on the same frame. The checker: tests/reloc_ref.py."""
    from viorb_amd import relocalization as R
    import reloc_ref as T
    import reloc_cases as K
    import test_gpu_relocalization as G
    P = K.small_problem(1, 513, 300)
    frame = T.Frame(P["cam"], P["kps"], P["desc"])
    hyps = []
    for npts in G.COUNTS:
        hyp = {k: (v if k in ("pose12", "feat_taken") else v[:npts]) for k, v in P["hyp"].items()}
        hyps.append(dict(hyp, frame=0, want=K.small_expected(P, hyp=hyp, frame=frame)))
    assert hyps[-1]["want"]["nmatches"] >= 40 and (hyps[-1]["want"]["reason"] == T.ROTATION).sum() > 0

    def runner(hs):
        run = lambda ws: _inject(G._batch([P]), ws, 0).search(hs)
        return lib().viorb_relocalization_workspace_bytes(len(P["kps"]), max(len(h["pts_f"]) for h in hs), len(hs)), run

    def check(r):
        for g, h in zip(r, hyps):
            K.same(g, h["want"])
            assert (g["tail"] == -1).all()
    n, run = runner(hyps)
    nb, run_big = runner([hyps[-1]] * 24)
    exact(conditions(n, nb, run, run_big), check)


# ---- viorb_relocalization_refine_workspace_bytes ------------------------------------------------------------------------------------------------
def test_relocalization_refine(oracle):
    """viorb_relocalization_refine_device: k_reloc_step between the three pose solves (k_pose_opt_se3) and the two searches (k_reloc_gates,
    k_reloc_claim), on three hypotheses of the monocular cascade fixture: the two that run all three solves (rejected and accepted at the
    third) and the one that leaves after the second, so that a hypothesis that has left rides along in the later launches. Larger case:
    all eight exits, as test_cascade_equals_the_checker_at_every_exit_in_either_order. The checker: the cascade of tests/reloc_ref.py
    with the oracle's solver."""
    import ctypes as C
    from viorb_amd import relocalization as R
    import reloc_ref as T
    import reloc_cases as K
    import test_gpu_relocalization as G
    F = K.cascade_fixture(False)
    want = K.cascade_expected(oracle.pose_opt_se3, False)
    order = [K.CASCADE_EXITS.index(e) for e in (T.THIRD_REJECTED, T.ACCEPTED_THIRD, T.SECOND_WEAK)]
    cam16 = np.zeros(16); cam16[:4] = K.INTR

    def runner(which):
        scenes = [F["scenes"][k] for k in which]
        cap = max(len(s["kps"]) for s in scenes)
        fe = viorb_amd.Frontend(cam16, [0, 0, -9.81], F["sf"], F["inv_sigma2"], tuple(K.BOUNDS), max_batch=len(which), cap=cap + 3)
        kcap = max(len(s["hyp"]["pts_f"]) for s in scenes)

        def run(ws):
            bt = R.RelocBatch([(s["kps"], s["desc"]) for s in scenes], K.lib_camera(F["sf"]), K.BOUNDS)
            return _inject(bt, ws, 0).refine(fe, [dict(s["hyp"], frame=b) for b, s in enumerate(scenes)], bf=K.BF)
        return lib().viorb_relocalization_refine_workspace_bytes(cap, kcap, cap + 3, len(which)), run

    def check(r):
        assert sorted(g["stage"] for g in r) == sorted((T.THIRD_REJECTED, T.ACCEPTED_THIRD, T.SECOND_WEAK))
        for g, k in zip(r, order):
            G._same_cascade(g, want[k])
    n, run = runner(order)
    nb, run_big = runner(list(range(len(want))))
    exact(conditions(n, nb, run, run_big), check)


# ---- viorb_update_local_map_workspace_bytes, viorb_local_points_gather_workspace_bytes -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _local_map_scenes():
    import local_map_cases as K
    return dict(K.sized_scenes())


def _local_map_names():
    from viorb_amd import local_map as M
    lds_kf = M.shape()[3]
    return lds_kf, ["kf_%d" % lds_kf, "kf_%d" % (lds_kf + 1), "loop_kf_%d" % (lds_kf + 1)]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["votes_in_lds", "votes_in_workspace", "neighbour_loop_in_workspace"])
def test_update_local_map(which):
    """viorb_update_local_map_device: k_ulm_prepare (the distinctness marks), k_ulm_key_frames, k_ulm_claim_points and k_ulm_local_points.
    kf_<lds>: the votes and marks of k_ulm_key_frames in LDS, the list, estart, first and info in the workspace; kf_<lds + 1>: votes and
    marks in the workspace as well; loop_kf_<lds + 1>: there the neighbour loop's pushes (test_edges_of_the_kernels_shapes). Larger
    case: the three as one batch. The checker: tests/local_map_ref.py."""
    from viorb_amd import local_map as M
    import local_map_ref as T
    lds_kf, names = _local_map_names()
    scenes = _local_map_scenes()
    scene = scenes[names[which]]
    want = T.update_local_map(scene)

    def runner(ss):
        P = M.pack(ss)

        def run(ws):
            b = M.LocalMapBatch(ss, packed=P)
            _inject(b, ws, b._wb).run()
            return b.results()
        return lib().viorb_update_local_map_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"]), run
    n, run = runner([scene])
    nb, run_big = runner([scenes[k] for k in names])
    exact(conditions(n, nb, run, run_big), lambda r: T.differences(r[0], want) == [] or pytest.fail(str(T.differences(r[0], want))))


def test_local_points_gather():
    """viorb_local_points_gather_device: k_ulm_frame_marks (the held marks in the workspace) and k_ulm_gather, on the first 20 random
    streams of test_gather_equals_the_numpy_packing with a refused stream among them. Larger case: 60 of them. The checker:
    local_map.gather_reference."""
    import torch
    from viorb_amd import local_map as M
    import local_map_cases as K
    import test_gpu_local_map as G
    streams, _ = K.random_streams()
    bad = K.broken(K.breakable_scene())[0][1]

    def runner(ss, seed):
        b = M.LocalMapBatch(ss)
        b.run()
        res = b.results()
        host, dev = G.point_store(torch, b.P, seed)

        def run(ws):
            return [t.cpu().numpy() for t in _inject(b, ws, b._gb, "gather_ws").gather(*dev)]
        return b._gb, run, M.gather_reference(b.P, res, *host)
    n, run, want = runner(streams[:10] + [bad] + streams[10:20], 3)
    nb, run_big, _ = runner(streams[:60], 4)
    assert (want[2] > 0).sum() >= 10 and len(set(np.unique(want[3]).tolist())) >= 4

    def check(r):
        for g, w, name in zip(r, want, ("pts_f", "pts_desc", "pts_count", "pts_flags")):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
    exact(conditions(n, nb, run, run_big), check)


# ---- viorb_key_frame_culling_workspace_bytes -------------------------------------------------------------------------------------------------
def test_key_frame_culling():
    """viorb_key_frame_culling_device: k_cull_prepare (the working copies of the point and observation words, the candidate ordinals and
    the links) and k_cull_ordered, on shape_scene(65, 4) of test_shape_edges_keypoints_and_observation_lists (three candidates, culls that
    change the later ones). Larger case: three shape scenes of up to 2051 keypoints as one batch. The checker: tests/kf_culling_ref.py."""
    from viorb_amd import culling as M
    import kf_culling_ref as T
    import kf_culling_cases as K
    scene = K.shape_scene(65, 4, seed=65)
    want = T.key_frame_culling(scene, True)
    assert want["n_culled"] >= 1

    def runner(ss):
        P = M.pack(ss)

        def run(ws):
            bt = M.CullBatch(ss, True, packed=P)
            _inject(bt, ws, bt._wb).run()
            return bt.results()
        return lib().viorb_key_frame_culling_workspace_bytes(P["batch"], P["n_kf"], P["n_cand"], P["n_pt"], P["n_obs"]), run
    n, run = runner([scene])
    nb, run_big = runner([K.shape_scene(2051, 4, seed=2051), K.shape_scene(70, 200, seed=200), K.shape_scene(1024, 4, seed=1024)])
    exact(conditions(n, nb, run, run_big), lambda r: K.differences(r[0], want) == [] or pytest.fail(str(K.differences(r[0], want))))


# ---- viorb_global_ba_navstate_workspace_bytes, viorb_global_ba_se3_workspace_bytes -----------------------------------------------------------------
def _within_run_to_run(res, kf_tol, pt_tol, compare):
    """The two global bundle adjustments sum their Schur blocks with FP64 atomics in an order the hardware picks: (b) and (c) equal (a) as
    two runs of test_run_to_run_agreement equal each other (same iterations and trials, key frames and points within the case's band,
    chi2 within 1e-9 relative), bit for bit if (a) twice is; and every condition passes the comparison with the checker."""
    a = res["zero"]
    same_bits = _differing(a, res["again"]) == []
    print("bit-reproducible on a zeroed workspace:", same_bits)
    for what in ("again", "ff", "stale"):
        b = res[what]
        assert (a["iterations"], a["trials"], a["accepted"]) == (b["iterations"], b["trials"], b["accepted"]), what
        print("%s: key frames %.3g points %.3g" % (what, np.abs(a["kfs"] - b["kfs"]).max(), np.abs(a["points"] - b["points"]).max()))
        np.testing.assert_allclose(a["kfs"], b["kfs"], rtol=0, atol=kf_tol)
        np.testing.assert_allclose(a["points"], b["points"], rtol=0, atol=pt_tol)
        assert abs(a["chi2_after"] - b["chi2_after"]) <= 1e-9 * b["chi2_after"], what
        assert np.array_equal(a["point_included"], b["point_included"]), what
        if same_bits:
            assert _differing(a, b) == [], what
    for what in ("zero", "ff", "stale"):
        compare(res[what])


@pytest.mark.parametrize("which", ["degenerate", "cross"])
def test_global_ba_navstate(which):
    """viorb_global_ba_navstate_device: k_gba_setup, k_gba_edges_scan, the key-frame lists (k_gba_kf_offsets / fill / sort), k_gba_errors,
    k_gba_imu_errors, k_gba_lin_edges, k_gba_hll, k_gba_hpp, k_gba_imu, k_gba_max_diag, k_gba_dinv, k_gba_init_reduced, k_gba_schur, the
    Cholesky chain (k_gba_potrf / trsm / syrk / bwd), k_gba_backsub and k_gba_update. cross: CASES[7] (N = 21, robust, revisits; a reduced
    system of four 64-tiles, so k_gba_syrk runs); degenerate: test_points_with_no_edge_and_with_a_single_edge, robust, where a point
    without an edge must come back untouched although every per-point array holds a slot for it. Larger case: CASES[11] (N = 60)."""
    from viorb_amd import GlobalBundleAdjustmentNavStateDevice, gba_workspace_bytes
    import global_ba_ref as R
    import global_ba_cases as GC
    import test_gpu_global_ba as G
    if which == "cross":
        seed, N, robust, revisit = GC.CASES[7]
        p, its = G._problem(seed, N, revisit), GC.ITERATIONS
        ref, kf_tol, pt_tol = G._reference(seed, N, robust, revisit)
    else:
        p, robust, its = GC.degenerate_points_variant(G._problem(*GC.DEGENERATE_SEED)), 1, GC.ITERATIONS
        ref, kf_tol, pt_tol = R.global_ba(*GC.args(p), iterations=its, robust=True), G.KF_FLOOR, G.PT_FLOOR
    bs, bN, br, bf = GC.CASES[11]
    big = G._problem(bs, bN, bf)
    size = lambda q: gba_workspace_bytes(len(q["kfs"]), len(q["points"]), len(q["edge_idx"]))
    run = lambda ws: GlobalBundleAdjustmentNavStateDevice(*GC.args(p), iterations=its, robust=robust, workspace=ws)
    run_big = lambda ws: GlobalBundleAdjustmentNavStateDevice(*GC.args(big), iterations=GC.ITERATIONS, robust=br, workspace=ws)

    def compare(got):
        G._compare(got, ref, kf_tol, pt_tol)
        if which == "degenerate":
            assert got["point_included"][9] == 0 and got["point_included"][-1] == 0
            assert np.array_equal(got["points"][9], p["points"][9]) and np.array_equal(got["points"][-1], p["points"][-1])
    _within_run_to_run(conditions(size(p), size(big), run, run_big), kf_tol, pt_tol, compare)


@pytest.mark.parametrize("which", ["degenerate", "cross"])
def test_global_ba_se3(which):
    """viorb_global_ba_se3_device: k_gse3_setup, k_gba_edges_scan, the key-frame lists, k_gse3_errors, k_gse3_lin_edges, k_gse3_hll,
    k_gse3_hpp, k_gba_max_diag, k_gba_dinv, k_gse3_init_reduced, k_gse3_schur, the Cholesky chain, k_gse3_backsub and k_gse3_update.
    cross: CASES[21] (N = 12, robust, half the edges stereo, revisits: 66 unknowns, two tiles); degenerate: test_degenerate_points[1]
    (points without an edge, with one edge, seen by fixed key frames only). Larger case: CASES[33] (N = 43)."""
    from viorb_amd import GlobalBundleAdjustmentSE3Device, gba_se3_workspace_bytes
    import global_ba_se3_cases as GC
    import test_gpu_global_ba_se3 as G
    if which == "cross":
        seed, N, robust, stereo, revisit = GC.CASES[21]
        assert (N, robust, stereo, revisit) == (12, 1, 0.5, 0.2)
        p, its = GC.problem(seed, N, stereo, revisit), GC.ITERATIONS
        ref, kf_tol, pt_tol = G._reference(seed, N, robust, stereo, revisit)
    else:
        p, robust, its, ref, kf_tol, pt_tol = G._reference_of("degenerate-1")
    bs, bN, br, bst, bf = GC.CASES[33]
    big = GC.problem(bs, bN, bst, bf)
    size = lambda q: gba_se3_workspace_bytes(len(q["kfs"]), len(q["points"]), len(q["edge_idx"]))
    run = lambda ws: GlobalBundleAdjustmentSE3Device(*GC.args(p), iterations=its, robust=robust, workspace=ws)
    run_big = lambda ws: GlobalBundleAdjustmentSE3Device(*GC.args(big), iterations=GC.ITERATIONS, robust=br, workspace=ws)

    def compare(got):
        G._compare(got, ref, kf_tol, pt_tol)
        if which == "degenerate":
            assert got["point_included"][9] == 0 and got["point_included"][-1] == 0 and got["point_included"][5:9].all()
            assert np.array_equal(got["points"][9], p["points"][9]) and np.array_equal(got["points"][-1], p["points"][-1])
    _within_run_to_run(conditions(size(p), size(big), run, run_big), kf_tol, pt_tol, compare)


# ---- viorb_essential_graph_workspace_bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["points", "duplicated_pair"])
def test_essential_graph(name):
    """viorb_optimize_essential_graph_device: k_eg_setup, the vertex lists (k_eg_csr_offsets / fill / sort), k_eg_errors, k_eg_linearise,
    k_eg_hpp, k_gba_max_diag, k_eg_init_reduced, the Cholesky chain, k_eg_update and k_eg_recover. points (N = 16, 200 map points moved
    by k_eg_recover) and duplicated_pair (N = 12, two edges adding into one off-diagonal block by atomics) are the cases whose runs
    test_run_to_run_and_device_form_agree_bit_for_bit holds bit for bit, so (b) and (c) are held to that. Larger case: n37_free. The
    checker: tests/essential_graph_ref.py."""
    from viorb_amd import essential_graph as EG
    import essential_graph_cases as EC
    import test_gpu_essential_graph as G
    p, big = EC.problem(name), EC.problem("n37_free")
    size = lambda q: EG.essential_graph_workspace_bytes(len(q["Scw"]), len(q["edge_idx"]), len(q["points"]) if q.get("points") is not None else 0)
    run = lambda ws: EG.solve(p, device=True, workspace=ws)
    run_big = lambda ws: EG.solve(big, device=True, workspace=ws)
    exact(conditions(size(p), size(big), run, run_big), lambda r: G._compare(r, EC.reference(name), p, name))
