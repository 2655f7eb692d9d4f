"""KeyFrame::UpdateConnections on the device (include/viorb_covisibility.h) against the checker tests/covis_ref.py: every output array of
viorb_update_connections_device and of the host-buffer form, compared exactly, on the hand-built scenes of tests/covis_cases.py singly and
as one batch of unequal streams, on scenes sized around the kernels' strides, on 300 random streams in one batch and again one stream
per call, and on every kind of broken snapshot in the middle of three streams; optional outputs left out and a second run; erase_targets
both ways; caller workspaces that hold garbage; two batches on two HIP streams; and the chain into viorb_update_local_map_device, whose
covis10 is the first ten of ord_kf_out."""
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import covisibility as M
import covis_ref as T
import covis_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    import torch
    return torch


def device(scenes, **args):
    b = M.CovisBatch(scenes, **args)
    b.run()
    return b.results()


def test_hand_built_scenes_device_and_host_form(torch_cuda):
    for name, scene, args, want in K.CASES:
        e = K.expected(name)
        for got in (device([scene], **args)[0], M.update_connections([scene], **args)[0]):
            assert T.differences(got, e) == [] and K.compare_want(got, want) == [], name
    # all of them as one batch of unequal streams with one row length (nothing overflows), an empty stream and one without targets among them
    scenes = [c[1] for c in K.CASES]
    cc = max(len(s["kf_flags"]) for s in scenes)
    for erase in (0, 1):
        exp = [T.update_connections(s, ccap=cc, erase_targets=erase) for s in scenes]
        for got in (device(scenes, ccap=cc, erase_targets=erase), M.update_connections(scenes, ccap=cc, erase_targets=erase)):
            assert [(c[0], T.differences(g, e)) for c, g, e in zip(K.CASES, got, exp) if T.differences(g, e)] == []


def test_edges_of_the_kernels_shapes(torch_cuda):
    named = K.sized_scenes()
    thr, wave, lds_kf, th = M.shape()
    for name, s, cc in named:
        e = T.update_connections(s, ccap=cc)
        assert T.differences(device([s], ccap=cc)[0], e) == [], name                          # alone: at batch position 0
        if name == "row_needs_ccap_plus_1":
            assert (e["status"], e["need"]) == (T.OVERFLOW, wave + 1)
    # as one batch with one row length; the streams above and at the LDS limit (counters and marks in the workspace / in LDS) in the middle
    small = [(n, s) for n, s, cc in named if cc is None] + [(n, s) for n, s, cc in named if n.startswith("kf_%d" % lds_kf) or n == "kf_%d" % (lds_kf + 1)]
    order = small[-2:] + small[:-2]
    for batch in (small, order):
        scenes = [s for _, s in batch]
        exp = [T.update_connections(s, ccap=300, erase_targets=1) for s in scenes]
        got = device(scenes, ccap=300, erase_targets=1)
        assert [(n, T.differences(g, e)) for (n, _), g, e in zip(batch, got, exp) if T.differences(g, e)] == []
        assert all(e["status"] == T.OK for e in exp)


def test_random_streams_in_one_batch(torch_cuda):
    scenes, exp, _ = K.random_streams()
    for got in (device(scenes, ccap=K.RANDOM_CCAP, erase_targets=1), M.update_connections(scenes, ccap=K.RANDOM_CCAP, erase_targets=1)):
        assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * 300


def test_random_streams_one_per_call(torch_cuda):
    scenes, exp, _ = K.random_streams()
    bad = [i for i, (s, e) in enumerate(zip(scenes, exp)) if T.differences(device([s], ccap=K.RANDOM_CCAP, erase_targets=1)[0], e)]
    assert bad == []


def test_erase_targets_off_keeps_the_group_in_loop_connections(torch_cuda):
    scenes, exp1, _ = K.random_streams()
    scenes, exp1 = scenes[:60], exp1[:60]
    exp0 = [T.update_connections(s, ccap=K.RANDOM_CCAP, erase_targets=0) for s in scenes]
    got0 = device(scenes, ccap=K.RANDOM_CCAP, erase_targets=0)
    assert [T.differences(g, e) for g, e in zip(got0, exp0)] == [[]] * 60
    assert sum(not np.array_equal(a["loop_conn"], b["loop_conn"]) for a, b in zip(exp0, exp1)) >= 10      # the argument decides something


def test_optional_outputs_left_out_and_a_second_run_gives_the_same(torch_cuda):
    scenes, exp, _ = K.random_streams()
    b = M.CovisBatch(scenes[:40], ccap=K.RANDOM_CCAP, erase_targets=1)
    b.run(optional=False)
    first = b.results()
    optional = [f for f in T.FIELDS if f not in capi.COVIS_RESULT_REQUIRED]
    required = [f for f in T.FIELDS if f in capi.COVIS_RESULT_REQUIRED]
    assert [T.differences(g, dict(e, need=g["need"]), required) for g, e in zip(first, exp[:40])] == [[]] * 40
    assert all((np.asarray(g[f]) == M.S.FILL).all() and g["need"] == M.S.FILL for g in first for f in optional)      # NULL: not written
    b.run(optional=False)
    again = b.results()
    assert all(np.array_equal(a[f], c[f]) for a, c in zip(first, again) for f in required)
    b.run(); b.run()
    assert [T.differences(g, e) for g, e in zip(b.results(), exp[:40])] == [[]] * 40


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams(torch_cuda):
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "loop_connections")
    e_good, e_other = T.update_connections(good, ccap=4), T.update_connections(other, ccap=4)
    kinds = K.broken(good)
    for what, bad in kinds:
        for got in (device([other, bad, good], ccap=4), M.update_connections([other, bad, good], ccap=4)):
            assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
            assert T.differences(got[0], e_other) == [] and T.differences(got[2], e_good) == [], what
    # an input row longer than ccap: key frame 0 of `good` holds two entries
    got = device([other, good, other], ccap=1)
    assert [g["status"] for g in got] == [T.OVERFLOW, T.INVALID, T.OVERFLOW] and got[1]["untouched"]


def test_the_workspace_contents_on_entry_are_ignored(torch_cuda):
    """k_covis_prepare (rank, flags, info), k_covis_votes (the counters of every target; above the LDS limit the votes themselves) and
    k_covis_ordered (above the LDS limit the marks) on one allocation: zeroed twice, every byte 0xFF, and what a larger batch left behind."""
    import test_gpu_workspace_contents as WS
    lds_kf = M.shape()[2]
    named = {n: s for n, s, _ in K.sized_scenes()}
    for name in ("kf_%d" % lds_kf, "kf_%d" % (lds_kf + 1)):
        scene = named[name]
        want = T.update_connections(scene, ccap=300, erase_targets=1)

        def runner(ss):
            P = M.pack(ss, ccap=300)

            def run(ws):
                b = M.CovisBatch(ss, packed=P, erase_targets=1)
                WS._inject(b, ws, b._wb).run()
                return b.results()
            return viorb_amd.lib().viorb_update_connections_workspace_bytes(P["batch"], P["n_kf"], P["n_target"], P["ccap"]), run
        n, run = runner([scene])
        nb, run_big = runner([named["kf_%d" % (lds_kf + 1)], named["kf_%d" % lds_kf], named["insert_middle_64"]])
        WS.exact(WS.conditions(n, nb, run, run_big), lambda r: T.differences(r[0], want) == [] or pytest.fail(str(T.differences(r[0], want))))


def test_two_batches_on_two_streams_at_once(torch_cuda):
    torch = torch_cuda
    scenes, exp, _ = K.random_streams()
    halves = (scenes[:150], scenes[150:])
    batches = [M.CovisBatch(h, ccap=K.RANDOM_CCAP, erase_targets=1) for h in halves]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for b, st in zip(batches, streams):
            with torch.cuda.stream(st):
                b.run()
    torch.cuda.synchronize()
    got = batches[0].results() + batches[1].results()
    assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * 300


def test_ordered_lists_feed_the_local_map(torch_cuda):
    """The chain: the first ten of ord_kf_out become covis10 of a local-map scene, on the device with no host step in between, and
    viorb_update_local_map_device on it must equal local_map_ref on the checker's graph."""
    torch = torch_cuda
    from viorb_amd import local_map as LM
    import local_map_ref as LT
    rng = np.random.default_rng(3)
    cov = [K.random_scene(rng, min_kf=12, max_kf=30) for _ in range(8)]
    cov = [dict(s, targets=np.arange(len(s["kf_flags"]), dtype=np.int32)) for s in cov]             # every key frame a target: every list is rebuilt
    cc = 29
    exp = [T.update_connections(s, ccap=cc) for s in cov]
    assert all(e["status"] == T.OK for e in exp) and sum(int((e["ord_n_out"] > 10).sum()) for e in exp) >= 5
    b = M.CovisBatch(cov, ccap=cc)
    b.run()

    def local_scene(s, covis10, parent, frame):
        nk = len(s["kf_flags"])
        return dict(s, kf_bad=np.zeros(nk, np.uint8), kf_parent=parent, kf_prev=np.full(nk, -1, np.int32), kf_next=np.full(nk, -1, np.int32), covis10=covis10,
                    child_start=np.zeros(nk + 1, np.int32), child_kf=np.zeros(0, np.int32), frame_point=np.array(frame, np.int32), prev_lkf=np.zeros(0, np.int32), prev_ref=-1)
    first10 = lambda e: np.where(np.arange(10)[None, :] < e["ord_n_out"][:, None], e["ord_kf_out"][:, :10], -1).astype(np.int32)
    frames = [[int(p) for p in rng.integers(-1, len(s["pt_bad"]), 6)] for s in cov]
    want_scenes = [local_scene(s, first10(e), e["kf_parent_out"], f) for s, e, f in zip(cov, exp, frames)]
    placeholder = [local_scene(s, np.full((len(s["kf_flags"]), 10), -1, np.int32), np.full(len(s["kf_flags"]), -1, np.int32), f) for s, f in zip(cov, frames)]
    lb = LM.LocalMapBatch(placeholder)
    ord_kf = b.o["ord_kf_out"].view(-1, cc)[:b.P["n_kf"], :10]                                       # on the device: rows are -1 from the count on
    lb.d["covis10"].view(-1, 10).copy_(ord_kf)
    lb.d["kf_parent"].copy_(b.o["kf_parent_out"][:b.P["n_kf"]])
    lb.run()
    got = lb.results()
    assert [T.differences(g, e) for g, e in zip(b.results(), exp)] == [[]] * len(cov)
    want = [LT.update_local_map(s) for s in want_scenes]
    assert [LT.differences(g, w) for g, w in zip(got, want)] == [[]] * len(cov)
    assert sum(w["n_lkf"] > w["n_voted"] for w in want) >= 3                                          # the neighbour loop used the lists
