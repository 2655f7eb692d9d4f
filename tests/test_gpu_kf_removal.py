"""Key-frame removal on the device (include/viorb_kf_removal.h) against the checker tests/kf_removal_ref.py: every output array of
viorb_remove_key_frames_device and of the host-buffer form, compared exactly (mTcp bit for bit), on the hand-built scenes of
tests/kf_removal_cases.py singly and as one batch of unequal streams, on scenes sized around the kernels' strides (read from
viorb_remove_key_frames_shape), on the seeded random set in one batch and again one stream per call, and on every kind of broken snapshot
in the middle of three streams; optional outputs left out and a second run; caller workspaces that hold garbage; regions outside the
written ranges; two batches on two HIP streams; the chain in from viorb_key_frame_culling and the chain out into
viorb_update_connections_device and viorb_update_local_map_device."""
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import kf_removal as M
import kf_removal_ref as T
import kf_removal_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    import torch
    return torch


def device(scenes, **args):
    b = M.KfRemovalBatch(scenes, **args)
    b.run()
    return b.results()


def test_hand_built_scenes_device_and_host_form(torch_cuda):
    for name, scene, want in K.CASES:
        e = K.expected(name)
        for got in (device([scene])[0], M.remove_key_frames([scene])[0]):
            assert T.differences(got, e) == [] and K.compare_want(got, want) == [] and got["untouched"], name
    # all of them as one batch of unequal streams with one row length, an empty stream and one without operations among them
    scenes = [c[1] for c in K.CASES]
    exp = [T.remove_key_frames(s, ccap=5) for s in scenes]
    for got in (device(scenes, ccap=5), M.remove_key_frames(scenes, ccap=5)):
        assert [(c[0], T.differences(g, e)) for c, g, e in zip(K.CASES, got, exp) if T.differences(g, e)] == []


def test_edges_of_the_kernels_shapes(torch_cuda):
    named = K.sized_scenes()
    lds_kf = M.shape()[2]
    for name, s, cc in named:
        e = T.remove_key_frames(s, ccap=cc)
        got = device([s], ccap=cc)[0]                                    # alone: at batch position 0
        assert T.differences(got, e) == [] and got["untouched"], name
    # the streams at and above the LDS limit (marks in LDS / in the workspace) in one batch, either way round
    big = [s for n, s, _ in named if n in ("kf_%d" % lds_kf, "kf_%d" % (lds_kf + 1))]
    exp = [T.remove_key_frames(s, ccap=8) for s in big]
    for batch, want in ((big, exp), (big[::-1], exp[::-1])):
        assert [T.differences(g, e) for g, e in zip(device(batch, ccap=8), want)] == [[], []]


def test_random_streams_in_one_batch(torch_cuda):
    scenes, exp, _ = K.random_streams()
    for got in (device(scenes, ccap=K.RANDOM_CCAP), M.remove_key_frames(scenes, ccap=K.RANDOM_CCAP)):
        assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * len(scenes)
        assert all(g["untouched"] for g in got)


def test_random_streams_one_per_call(torch_cuda):
    scenes, exp, _ = K.random_streams()
    batch = device(scenes, ccap=K.RANDOM_CCAP)
    for i, (s, e) in enumerate(zip(scenes, exp)):
        one = device([s], ccap=K.RANDOM_CCAP)[0]
        assert T.differences(one, e) == [], i
        assert all(np.array_equal(one[f], batch[i][f]) for f in T.FIELDS), i


def test_optional_outputs_left_out_and_a_second_run_gives_the_same(torch_cuda):
    scenes, exp, _ = K.random_streams()
    b = M.KfRemovalBatch(scenes[:30], ccap=K.RANDOM_CCAP)
    b.run(optional=False)
    first = b.results()
    optional = [f for f in T.FIELDS if f not in capi.KFR_RESULT_REQUIRED]
    required = [f for f in T.FIELDS if f in capi.KFR_RESULT_REQUIRED]
    assert [T.differences(g, e, required) for g, e in zip(first, exp[:30])] == [[]] * 30
    assert all((np.asarray(g[f]) == M.S.FILL).all() for g in first for f in optional)      # NULL: not written
    b.run(optional=False)
    again = b.results()
    assert all(np.array_equal(a[f], c[f]) for a, c in zip(first, again) for f in required)
    b.run(); b.run()
    assert [T.differences(g, e) for g, e in zip(b.results(), exp[:30])] == [[]] * 30


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams(torch_cuda):
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "points")
    e_good, e_other = T.remove_key_frames(good, ccap=4), T.remove_key_frames(other, ccap=4)
    for what, bad in K.broken(good):
        for got in (device([other, bad, good], ccap=4), M.remove_key_frames([other, bad, good], ccap=4)):
            assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
            assert T.differences(got[0], e_other) == [] and T.differences(got[2], e_good) == [], what
    got = device([other, good, other], ccap=1)                          # an input row longer than ccap
    assert [g["status"] for g in got] == [T.OK, T.INVALID, T.OK] and got[1]["untouched"]


def test_the_workspace_contents_on_entry_are_ignored(torch_cuda):
    """k_kfr_prepare (rank, flags, parents, links, point words, mpRefKF, info) and k_kfr_ordered (the children; above the LDS limit the
    marks) on one allocation: zeroed twice, every byte 0xFF, and what a larger batch left behind."""
    import test_gpu_workspace_contents as WS
    lds_kf = M.shape()[2]
    named = {n: s for n, s, _ in K.sized_scenes()}
    for name in ("kf_%d" % lds_kf, "kf_%d" % (lds_kf + 1)):
        scene = named[name]
        want = T.remove_key_frames(scene, ccap=8)

        def runner(ss):
            P = M.pack(ss, ccap=8)

            def run(ws):
                b = M.KfRemovalBatch(ss, packed=P)
                WS._inject(b, ws, b._wb).run()
                return b.results()
            return viorb_amd.lib().viorb_remove_key_frames_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"], P["n_op"]), run
        n, run = runner([scene])
        nb, run_big = runner([named["kf_%d" % (lds_kf + 1)], named["kf_%d" % lds_kf], K.random_streams()[0][0]])
        WS.exact(WS.conditions(n, nb, run, run_big), lambda r: T.differences(r[0], want) == [] or pytest.fail(str(T.differences(r[0], want))))


def test_two_batches_on_two_streams_at_once(torch_cuda):
    torch = torch_cuda
    scenes, exp, _ = K.random_streams()
    halves = (scenes[:30], scenes[30:])
    batches = [M.KfRemovalBatch(h, ccap=K.RANDOM_CCAP) for h in halves]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for b, st in zip(batches, streams):
            with torch.cuda.stream(st):
                b.run()
    torch.cuda.synchronize()
    got = batches[0].results() + batches[1].results()
    assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * len(scenes)


def test_the_culling_decides_the_operations_and_both_leave_the_same_state(torch_cuda):
    """The chain in: viorb_key_frame_culling_device on a map, its culled and deferred candidates as the operations of the removal on the same
    map; what both entries report about the points, the observations, the links and the two flags must be the same."""
    from viorb_amd import culling as CU
    pairs = [K.chain_in_scene(seed) for seed in range(8)]
    cb = CU.CullBatch([c for c, _ in pairs], True)
    cb.run()
    crs = cb.results()
    assert all(cr["status"] == 0 for cr in crs) and sum(cr["n_culled"] for cr in crs) >= 12
    assert sum(int((cr["cand_reason"] == CU.DEFERRED).sum()) for cr in crs) >= 2
    scenes = [removal(K.chain_in_operations(c, cr)) for (c, removal), cr in zip(pairs, crs)]
    got = device(scenes, ccap=12)
    assert [K.chain_in_differences(cr, g) for cr, g in zip(crs, got)] == [[]] * len(pairs)
    assert [T.differences(g, T.remove_key_frames(s, ccap=12)) for g, s in zip(got, scenes)] == [[]] * len(pairs)
    assert all(set(g["op_reason"].tolist()) <= {T.REMOVED, T.DEFERRED} for g in got)


def test_the_result_feeds_the_covisibility_graph_and_the_local_map(torch_cuda):
    """The chain out, on the device with no host step in between: the rows (compacted by their counts), kf_parent_out, pt_bad_out, kp_point_out
    and the observations that obs_alive keeps go into viorb_update_connections_device with surviving targets; the result must equal the
    covisibility checker continued on the removal checker's state, and its first ten ord_kf_out are accepted as covis10 by
    viorb_update_local_map_device."""
    torch = torch_cuda
    from viorb_amd import covisibility as CV, local_map as LM
    import covis_ref as CT
    import local_map_ref as LT
    scenes, exp, _ = K.random_streams()
    scenes, exp = scenes[:24], exp[:24]
    rng = np.random.default_rng(9)
    cc = K.RANDOM_CCAP
    cov_want = [K.covis_scene_after(s, e, K.surviving_targets(s, e, rng)) for s, e in zip(scenes, exp)]
    b = M.KfRemovalBatch(scenes, ccap=cc)
    b.run()
    # a covisibility batch of the expected sizes, its device arrays overwritten by the removal's device outputs
    placeholder = [dict(c, conn_kf=np.zeros_like(c["conn_kf"]), conn_w=np.zeros_like(c["conn_w"]), ord_kf=np.zeros_like(c["ord_kf"]), ord_w=np.zeros_like(c["ord_w"]),
                        kf_parent=np.full_like(c["kf_parent"], -1), pt_bad=np.ones_like(c["pt_bad"]), kp_point=np.full_like(c["kp_point"], -1), obs=np.zeros_like(c["obs"]))
                   for c in cov_want]
    cb = CV.CovisBatch(placeholder, ccap=cc)
    nk, n_kp, n_pt, n_obs = b.P["n_kf"], b.P["n_kp"], b.P["n_pt"], b.P["n_obs"]
    col = torch.arange(cc, device=b.dev)[None, :]
    for what in ("conn", "ord"):
        keep = col < b.o[what + "_n_out"][:nk, None]
        for f in ("kf", "w"):
            cb.d["%s_%s" % (what, f)][:int(cb.P["n_" + what])].copy_(b.o["%s_%s_out" % (what, f)].view(-1, cc)[:nk][keep])
    cb.d["kf_parent"].copy_(b.o["kf_parent_out"][:nk])
    cb.d["pt_bad"].copy_(b.o["pt_bad_out"][:n_pt])
    cb.d["kp_point"][:n_kp].copy_(b.o["kp_point_out"][:n_kp])
    cb.d["obs"][:cb.P["n_obs"]].copy_(b.d["obs"][:n_obs][b.o["obs_alive"][:n_obs] != 0])
    cb.run()
    got = cb.results()
    want = [CT.update_connections(c, ccap=cc) for c in cov_want]
    assert all(w["status"] == CT.OK for w in want) and sum(int(w["t_added"].sum()) for w in want) >= 50
    assert [CT.differences(g, w) for g, w in zip(got, want)] == [[]] * len(scenes)
    assert [T.differences(g, e) for g, e in zip(b.results(), exp)] == [[]] * len(scenes)

    def local_scene(c, covis10, parent, bad, frame):
        n = len(c["kf_flags"])
        return dict(c, kf_bad=bad, kf_parent=parent, kf_prev=np.full(n, -1, np.int32), kf_next=np.full(n, -1, np.int32), covis10=covis10,
                    child_start=np.zeros(n + 1, np.int32), child_kf=np.zeros(0, np.int32), frame_point=np.array(frame, np.int32), prev_lkf=np.zeros(0, np.int32), prev_ref=-1)
    first10 = lambda w: np.where(np.arange(10)[None, :] < w["ord_n_out"][:, None], w["ord_kf_out"][:, :10], -1).astype(np.int32)
    frames = [[int(p) for p in rng.integers(-1, len(c["pt_bad"]), 6)] for c in cov_want]
    bads = [((e["kf_flags_out"] & T.KF_BAD) != 0).astype(np.uint8) for e in exp]
    lm_want = [local_scene(c, first10(w), w["kf_parent_out"], bad, f) for c, w, bad, f in zip(cov_want, want, bads, frames)]
    lm_placeholder = [local_scene(c, np.full((len(c["kf_flags"]), 10), -1, np.int32), np.full(len(c["kf_flags"]), -1, np.int32), bad, f) for c, bad, f in zip(cov_want, bads, frames)]
    lb = LM.LocalMapBatch(lm_placeholder)
    lb.d["covis10"].view(-1, 10).copy_(cb.o["ord_kf_out"].view(-1, cc)[:nk, :10])
    lb.d["kf_parent"].copy_(cb.o["kf_parent_out"][:nk])
    lb.run()
    lm_exp = [LT.update_local_map(s) for s in lm_want]
    assert [LT.differences(g, w) for g, w in zip(lb.results(), lm_exp)] == [[]] * len(scenes)
