"""GPU tests of key-frame and map-point culling (include/viorb_culling.h): the device and host forms of viorb_key_frame_culling equal the
literal checker tests/kf_culling_ref.py in every output, on the hand-built scenes of tests/kf_culling_cases.py, on the sizes at which
the kernels take another path (read from viorb_key_frame_culling_shape), on batches of unequal streams and on 300 random streams whose
conditions are asserted on the checker's output first. cand_recounted has no counterpart in the reference: it is 1 exactly for the
candidates that no skip test removed, which the ordered phase counts itself. One test puts every kind of broken snapshot between two
valid streams; every other snapshot here is valid."""
import numpy as np
import pytest
from viorb_amd import capi
from viorb_amd import culling as M
import kf_culling_ref as T
import kf_culling_cases as K

pytestmark = pytest.mark.gpu


def _check(scenes, mono, want=None, host_form=False):
    """The device entry (twice, on the same buffers) and optionally the host entry on one batch; returns the device results."""
    want = want or [T.key_frame_culling(s, mono) for s in scenes]
    P = M.pack(scenes)
    bt = M.CullBatch(scenes, mono, packed=P)
    before = bt.inputs()
    bt.run()
    first = bt.results()
    bt.run()
    second = bt.results()
    after = bt.inputs()
    for f in before:
        assert before[f].tobytes() == after[f].tobytes() == P[f].tobytes(), f                 # the inputs are const
    core = M.key_frame_culling_host_core(scenes, mono, packed=P)
    for b, (g, g2, e, h) in enumerate(zip(first, second, want, core)):
        assert K.differences(g, e) == [], (b, K.differences(g, e))
        assert K.differences(g2, e) == [] and (g2["cand_recounted"] == g["cand_recounted"]).all(), b
        assert (g["cand_recounted"] == h["cand_recounted"]).all() and (g["cand_recounted"] == (e["cand_reason"] >= T.KEPT)).all(), b
    if host_form:
        for b, (g, e, h) in enumerate(zip(M.key_frame_culling(scenes, mono, packed=P), want, core)):
            assert K.differences(g, e) == [] and (g["cand_recounted"] == h["cand_recounted"]).all(), b
    return first


def test_hand_built_scenes_one_by_one_and_as_batches():
    for name, scene, mono, want in K.CASES:
        g = _check([scene], mono, [K.expected(name)], host_form=True)[0]
        for f, v in want.items():
            assert np.asarray(g[f]).tolist() == list(v), (name, f)
    for mono in (True, False):
        names = [c[0] for c in K.CASES if c[2] == mono]
        _check([c[1] for c in K.CASES if c[2] == mono], mono, [K.expected(n) for n in names], host_form=True)


def test_shape_edges_keypoints_and_observation_lists():
    threads, chunk, wave, shared = M.shape()
    assert wave == 64 and shared == 0
    sizes = sorted({0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, threads - 1, threads, threads + 1, 2 * threads + 3})
    scenes = [K.shape_scene(n, 4, seed=n) for n in sizes] + [K.shape_scene(70, m, seed=m) for m in (0, 1, 3, 4, 64, 65, 200)]
    want = [T.key_frame_culling(s, True) for s in scenes]
    assert sum(e["n_culled"] for e in want) >= len(sizes) and sum(e["n_culled"] >= 2 for e in want) >= 3
    got = _check(scenes, True, want, host_form=True)
    assert any(g["cand_recounted"].any() for g in got)
    for s in scenes[3::4]:                                               # alone as well as in the batch
        _check([s], True)


def _empty_and_skipped():
    no_cand = M.scene_from_lists(K.chain([0.0, 0.1, 0.2]), 2, [], K.pts_seen_by(3, [0, 1, 2]))
    all_skipped = M.scene_from_lists(K.chain([0.0, 0.1, 0.2, 0.25], first=(0,)), 3, [(2, K.table(0, 3)), (0, K.table(0, 3)), (1, K.table(0, 3))],
                                     K.pts_seen_by(3, [0, 1, 2, 3]), vins_inited=True)
    return no_cand, all_skipped


@pytest.mark.parametrize("n", [1, 3, 70])
def test_batches_of_unequal_streams(n):
    no_cand, all_skipped = _empty_and_skipped()
    e = T.key_frame_culling(all_skipped, True)
    assert e["cand_reason"].tolist() == [T.BEFORE_CURRENT, T.FIRST_KF, T.RECENT] and T.key_frame_culling(no_cand, True)["n_culled"] == 0
    rnd, _ = K.random_batch(3, 70, True)
    scenes = {1: [rnd[5]], 3: [no_cand, rnd[6], all_skipped]}.get(n) or ([rnd[0], no_cand, all_skipped] + list(rnd[3:70]))
    assert len(scenes) == n
    for mono in (True, False):
        _check(scenes, mono, host_form=n == 3)


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams():
    """Every kind of broken snapshot of kf_culling_cases.broken in the middle of three streams: the device form refuses it alone and
    leaves its ranges of every output array as they were; the host-buffer form copies its zeroed device outputs over a refused stream's
    rows (DESIGN.md "Map culling"), so only its statuses and the neighbours are asserted."""
    good, (name, other) = K.breakable_scene(), next((c[0], c[1]) for c in K.CASES if c[0] == "shrinking_mps_ab")
    e_good, e_other = T.key_frame_culling(good, True), K.expected(name)
    for what, bad in K.broken(good):
        scenes = [other, bad, good]
        bt = M.CullBatch(scenes, True)
        bt.run()
        got = bt.results()
        assert got[1] == dict(status=capi.ERR_INVALID_ARG, n_culled=0), what
        assert K.untouched(scenes, 1, {f: v.cpu().numpy() for f, v in bt.o.items()}), what
        assert K.differences(got[0], e_other) == [] and K.differences(got[2], e_good) == [], what
        host = M.key_frame_culling(scenes, True)
        assert [h["status"] for h in host] == [0, capi.ERR_INVALID_ARG, 0], what
        assert K.differences(host[0], e_other) == [] and K.differences(host[2], e_good) == [], what


def test_three_hundred_random_streams():
    """Streams 0-199 go through a monocular call, 200-299 through a stereo call (mbMonocular belongs to the call); the conditions hold
    for the 300 together."""
    sm, em = K.random_batch(1, 200, True)
    ss, es = K.random_batch(2, 100, False)
    scenes, want = list(sm) + list(ss), list(em) + list(es)
    reasons = np.bincount(np.concatenate([e["cand_reason"] for e in want]), minlength=7)
    assert (reasons > 0).all(), reasons
    assert sum(e["n_culled"] for e in want) >= 50 and sum(e["n_culled"] >= 2 for e in want) >= 20
    assert sum(int(e["pt_bad_out"].sum()) - int(s["pt_bad"].sum()) for s, e in zip(scenes, want)) >= 20
    frozen = [T.key_frame_culling(s, i < 200, frozen=True) for i, s in enumerate(scenes)]
    assert sum(int((f["cand_reason"] != e["cand_reason"]).sum()) for f, e in zip(frozen, want)) >= 1
    assert any(s["vins_inited"] for s in scenes) and not all(s["vins_inited"] for s in scenes) and any((s["kf_flags"] & 2).any() for s in scenes)
    nk, nc, npt = [len(s["kf_flags"]) for s in scenes], [len(s["cand_kf"]) for s in scenes], [len(s["pt_nobs"]) for s in scenes]
    assert min(nk) >= 5 and max(nk) <= 40 and min(nc) >= 1 and max(nc) <= 30 and min(npt) >= 50 and max(npt) <= 600
    assert max(int(np.diff(s["kp_start"]).max()) for s in scenes) <= 300 and max(int(np.diff(s["obs_start"]).max()) for s in scenes) <= 12
    got = _check(list(sm), True, list(em)) + _check(list(ss), False, list(es))
    rec = np.concatenate([g["cand_recounted"] for g in got])
    assert rec.any() and not rec.all()


def test_map_point_culling_every_branch_and_threshold():
    rng = np.random.default_rng(2)
    f = np.concatenate([[0, 0, 1, 1, 1, 5, 4194303, 4194303, 4194304, 4194303], rng.integers(0, 2 ** 22, 500), rng.integers(0, 40, 500)])
    d = np.concatenate([[0, 1, 0, -1, 1, 0, 0, 1, -1, -1], rng.integers(-1, 2, 1000)])
    v = np.clip(4 * f + d, 0, 2 ** 24 - 1)
    n = len(f)
    assert ((d == 0).sum() > 100) and ((d == 1).sum() > 100) and ((d == -1).sum() > 100) and (v > 2 ** 24 - 8).sum() >= 3
    bad, first, nobs = (rng.random(n) < 0.1), rng.integers(0, 5, n), rng.integers(1, 6, n)
    for mono in (True, False):
        for cur in (3, 4):
            want = T.map_point_culling(bad, f, v, first, nobs, cur, mono)
            assert set(want.tolist()) == set(range(5))
            assert np.array_equal(M.map_point_culling(bad, f, v, first, nobs, cur, mono), want)
    # age 1, 2, 3 x nObs 2, 3, 4 for both sensors, found ratio out of the way
    age, ob = np.repeat([1, 2, 3], 3), np.tile([2, 3, 4], 3)
    for mono in (True, False):
        want = T.map_point_culling(np.zeros(9), np.ones(9), np.ones(9), 10 - age, ob, 10, mono)
        th = 2 if mono else 3
        assert want.tolist() == [T.MPC_CULL_FEW_OBS if a >= 2 and o <= th else T.MPC_RETIRE if a >= 3 else T.MPC_KEEP for a, o in zip(age, ob)]
        assert np.array_equal(M.map_point_culling(np.zeros(9), np.ones(9), np.ones(9), 10 - age, ob, 10, mono), want)
    # the batched form: unequal counts, -1 from the count on, a cap that is no multiple of the workgroup
    cap, counts, curs = 301, [301, 0, 17, 300], [3, 4, 2, 9]
    pick = lambda a: np.stack([np.resize(np.roll(a, 37 * b), cap) for b in range(4)])
    B = [pick(x) for x in (bad, f, v, first, nobs)]
    for mono in (True, False):
        code = M.map_point_culling_batch(*B, counts, curs, mono)
        for b in range(4):
            c = counts[b]
            assert np.array_equal(code[b, :c], T.map_point_culling(*[x[b, :c] for x in B], curs[b], mono)) and (code[b, c:] == -1).all()
