"""Map fusion on the device (include/viorb_map_fusion.h) against the checker tests/map_fusion_ref.py: every output array of
viorb_apply_fuse_device and of the host-buffer form, compared exactly, on the hand-built scenes of tests/map_fusion_cases.py singly and as
one batch of unequal streams, on scenes sized around the kernels' strides (read from viorb_apply_fuse_shape), on the seeded random set in
one batch and again one stream per call, and on every kind of broken snapshot in the middle of three streams; optional outputs left out
and a second run; caller workspaces that hold garbage; regions outside the written ranges; overflow with need; two batches on two HIP
streams; the chain in from viorb_fuse_sim3_device and the chains out into viorb_update_connections_device and into
viorb_map_points_update_device + viorb_fuse_merge_descriptors_device."""
import ctypes as C
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import map_fusion as M
from viorb_amd.capi import lib, check, ptr
import map_fusion_ref as T
import map_fusion_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    import torch
    return torch


def device(scenes, **args):
    b = M.FuseBatch(scenes, **args)
    b.run()
    return b.results()


def test_hand_built_scenes_device_and_host_form(torch_cuda):
    for name, scene, want in K.CASES:
        e = K.expected(name)
        for got in (device([scene])[0], M.apply_fuse([scene])[0]):
            assert T.differences(got, e) == [] and K.compare_want(got, want) == [] and got["untouched"], name
    scenes = [c[1] for c in K.CASES]                                    # all of them as one batch of unequal streams
    exp = [K.expected(c[0]) for c in K.CASES]
    for got in (device(scenes), M.apply_fuse(scenes)):
        assert [(c[0], T.differences(g, e)) for c, g, e in zip(K.CASES, got, exp) if T.differences(g, e)] == []
        assert got[0]["untouched"]


def test_edges_of_the_kernels_shapes(torch_cuda):
    named = K.sized_scenes()
    for name, s in named:
        got = device([s])[0]                                            # alone: at batch position 0
        assert T.differences(got, T.apply_fuse(s)) == [] and got["untouched"], name
    scenes = [s for _, s in named][::-1]                                # and as one batch, the largest first
    got = device(scenes)
    assert [T.differences(g, T.apply_fuse(s)) for g, s in zip(got, scenes)] == [[]] * len(scenes)


def test_random_streams_in_one_batch(torch_cuda):
    scenes, exp, _ = K.random_streams()
    for got in (device(scenes), M.apply_fuse(scenes)):
        assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * len(scenes)
        assert all(g["untouched"] for g in got)


def test_random_streams_one_per_call(torch_cuda):
    scenes, exp, _ = K.random_streams()
    batch = device(scenes)
    for i, (s, e) in enumerate(zip(scenes, exp)):
        one = device([s])[0]
        assert T.differences(one, e) == [], i
        assert all(np.array_equal(one[f], batch[i][f]) for f in T.FIELDS) and one["obs"] == batch[i]["obs"] and one["dirty"] == batch[i]["dirty"], i


def test_optional_outputs_left_out_and_a_second_run_gives_the_same(torch_cuda):
    scenes, exp, _ = K.random_streams()
    b = M.FuseBatch(scenes[:30])
    b.run(optional=False)
    optional = [f for f in capi.FUSE_RESULT_FIELDS if f not in capi.FUSE_RESULT_REQUIRED]
    required = ("kp_point_out", "pt_bad_out", "pt_nobs_out")
    b.torch.cuda.synchronize()
    assert all(bool((b.o[f] == M.S.FILL).all()) for f in optional)       # NULL: not written
    first = b.results(optional=False)
    assert [T.differences(g, e, required) for g, e in zip(first, exp[:30])] == [[]] * 30 and first[0]["untouched"]
    regions = [(w.copy(), f.copy()) for w, f in (g["obs_region"] for g in first)]
    for (w, f), e in zip(regions, exp[:30]):                            # the packed entries of every stream, in point order
        flat = [o for p in e["obs"] for o in p]
        assert [int(x) & 0xffff for x in w[:len(flat)]] == [o[0] for o in flat] and list(f[:len(flat)]) == [o[3] for o in flat]
    b.run(optional=False)
    again = b.results(optional=False)
    assert all(np.array_equal(a[f], c[f]) for a, c in zip(first, again) for f in required)
    assert all(np.array_equal(a["obs_region"][0], w) for a, (w, _) in zip(again, regions))
    b.run(); b.run()
    assert [T.differences(g, e) for g, e in zip(b.results(), exp[:30])] == [[]] * 30


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams(torch_cuda):
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "shared_observer")
    e_good, e_other = T.apply_fuse(good), T.apply_fuse(other)
    for what, P, statuses in K.broken(other, good):
        for got in (device(None, packed=P), M.apply_fuse(None, packed=P)):
            assert [g["status"] for g in got] == statuses and got[0]["untouched"], what
            assert T.differences(got[0], e_other) == [], what
            if statuses[2] == T.OK:
                assert T.differences(got[2], e_good) == [], what


def test_overflow_reports_need_and_leaves_the_others_alone(torch_cuda):
    scenes = [c[1] for c in K.CASES]
    exp = [K.expected(c[0]) for c in K.CASES]
    regions = [M.region_bound(s) for s in scenes]
    regions[1] = exp[1]["need"] - 1
    regions[4] = 0
    e1, e4 = T.apply_fuse(scenes[1], region=regions[1]), T.apply_fuse(scenes[4], region=0)
    for got in (device(scenes, regions=regions), M.apply_fuse(scenes, regions=regions)):
        assert got[1]["status"] == got[4]["status"] == T.OVERFLOW and got[1]["need"] == exp[1]["need"] and got[4]["need"] == exp[4]["need"]
        assert T.differences(got[1], e1) == [] and T.differences(got[4], e4) == []
        assert [T.differences(g, e) for i, (g, e) in enumerate(zip(got, exp)) if i not in (1, 4)] == [[]] * (len(scenes) - 2)
        assert got[0]["untouched"]
    tight = device(scenes, regions=[e["need"] for e in exp])            # exactly as long as needed: one CSR over the batch
    assert [T.differences(g, e) for g, e in zip(tight, exp)] == [[]] * len(scenes) and tight[0]["untouched"]


def test_the_workspace_contents_on_entry_are_ignored(torch_cuda):
    """k_fuse_prepare (rank, the per-point state, the chains, the pool, vpReplacePoint, info) and k_fuse_ordered (counts and totals) on one
    allocation: zeroed twice, every byte 0xFF, and what a larger batch left behind."""
    import test_gpu_workspace_contents as WS
    named = dict(K.sized_scenes())
    rnd = K.random_streams()[0]
    for scene in (named["entries_65"], rnd[3]):
        want = T.apply_fuse(scene)

        def runner(ss):
            P = M.pack(ss)

            def run(ws):
                b = M.FuseBatch(ss, packed=P)
                WS._inject(b, ws, b._wb).run()
                return b.results()
            return viorb_amd.lib().viorb_apply_fuse_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"], P["n_obs"], P["n_op"]), run
        n, run = runner([scene])
        nb, run_big = runner([named["observers_257"], named["entries_257"]] + rnd[:8])
        WS.exact(WS.conditions(n, nb, run, run_big), lambda r: T.differences(r[0], want) == [] or pytest.fail(str(T.differences(r[0], want))))


def test_two_batches_on_two_streams_at_once(torch_cuda):
    torch = torch_cuda
    scenes, exp, _ = K.random_streams()
    halves = (scenes[:30], scenes[30:])
    batches = [M.FuseBatch(h) for h in halves]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for b, st in zip(batches, streams):
            with torch.cuda.stream(st):
                b.run()
    torch.cuda.synchronize()
    got = batches[0].results() + batches[1].results()
    assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * len(scenes)


def test_best_idx_of_the_sim3_fuse_search_passes_unchanged(torch_cuda):
    """The chain in: viorb_fuse_sim3_device over one shared point list for K key frames; its best_idx [K][pcap] is op_feat of K calls with
    call_list = 0 and call_feat = c * pcap, on the device, as it lies."""
    torch = torch_cuda
    from viorb_amd import sim3_match as SM
    import sim3_match_cases as SK
    P = SK.problem()
    L, F = P["loop"], P["fuse"]
    frames, npts, nk = F["frames"], len(L["pts_f"]), len(F["frames"])
    pcap = npts + 5
    rng = np.random.default_rng(5)
    # a map around the search's inputs: every loop point is observed by up to two of the key frames, the other features hold points of their own
    table = [np.full(len(k), -1, np.int64) for k, _ in frames]
    pts = [dict(obs=[], bad=bool(rng.random() < 0.05), found=int(rng.integers(0, 30)), visible=int(rng.integers(0, 60))) for _ in range(npts)]
    for p in range(npts):
        for k in rng.permutation(nk)[:int(rng.integers(0, 3))]:
            f = int(rng.integers(len(table[k])))
            if table[k][f] < 0:
                table[k][f] = p
                pts[p]["obs"].append((int(k), f))
    for k in range(nk):
        for f in np.where(table[k] < 0)[0][::2]:
            table[k][f] = len(pts)
            pts.append(dict(obs=[(k, int(f))], bad=bool(rng.random() < 0.05)))
    held = [set(table[k].tolist()) for k in range(nk)]
    valid = np.array([[0 if pts[p]["bad"] or p in held[k] else 1 for p in range(npts)] for k in range(nk)], np.uint8)
    kfs = [dict(pts=[int(q) for q in table[k]], octave=[int(o) for o in frames[k][0]["octave"]], stereo=[int(v) for v in rng.integers(0, 2, len(table[k]))]) for k in range(nk)]
    scene = M.scene_from_lists(kfs, pts, [(k, T.SIM3, [-1] * npts) for k in range(nk)], shared_list=list(range(npts)), by_key=[int(v) for v in rng.permutation(nk)])
    scene["call_feat"] = (np.arange(nk) * pcap).astype(np.int32)
    scene["op_feat"] = np.full(nk * pcap, -1, np.int32)
    bt = SM.Sim3MatchBatch(frames, SK.lib_camera(P), P["bounds4"], cap=1010)
    d = [capi._torch_up(np.ascontiguousarray(F["Scw"], np.float32).reshape(nk, 12)),
         capi._torch_up(np.concatenate([np.asarray(L["pts_f"], np.float32).reshape(-1, 8), np.zeros((5, 8), np.float32)])),
         capi._torch_up(np.concatenate([np.asarray(L["pts_desc"], np.uint8).reshape(-1, 32), np.zeros((5, 32), np.uint8)])),
         capi._torch_up(np.concatenate([valid, np.zeros((nk, 5), np.uint8)], axis=1))]
    best_idx = torch.zeros((nk, pcap), dtype=torch.int32, device=bt.dev)
    nfused = torch.zeros(nk, dtype=torch.int32, device=bt.dev)
    ws, wb = bt._workspace(bt.cap, pcap)
    check(lib().viorb_fuse_sim3_device(C.byref(bt.kf), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), npts, pcap, C.byref(bt.cam), ptr(bt.bounds), float(SK.TH_FUSE), nk,
                                       ptr(best_idx), ptr(nfused), None, ws, wb, bt._stream()))
    b = M.FuseBatch([scene], regions=[len(scene["obs"]) + nk * npts], arrays=dict(op_feat=best_idx.view(-1)))
    b.run()
    got = b.results()[0]
    scene["op_feat"] = best_idx.cpu().numpy().reshape(-1)
    e = T.apply_fuse(scene)
    assert T.differences(got, e) == [] and got["untouched"]
    searched = nfused.cpu().numpy().tolist()                            # the search's guards are those of the call's start; the application's only tighten
    assert int(got["call_nfused"][0]) == searched[0] and all(int(a) <= s for a, s in zip(got["call_nfused"], searched))
    assert int((e["op_reason"] == T.REPLACED_KF_POINT).sum()) >= 5 and int((e["op_reason"] == T.ADDED).sum()) >= 5 and int(e["pt_bad_out"].sum() - scene["pt_bad"].sum()) >= 5


def _tight(scenes):
    """The device run with regions exactly as long as a first run's `need` says: obs_start_out is then one CSR over the batch."""
    first = M.FuseBatch(scenes)
    first.run()
    first.torch.cuda.synchronize()
    b = M.FuseBatch(scenes, regions=first.o["need"].cpu().numpy().tolist())
    b.run()
    return b


def _state_after(s, e):
    """The scene the checker's result e leaves behind (the calls as they were)."""
    c = dict(s)
    c["kp_point"], c["pt_bad"], c["pt_nobs"], c["pt_found"], c["pt_visible"] = e["kp_point_out"], e["pt_bad_out"], e["pt_nobs_out"], e["pt_found_out"], e["pt_visible_out"]
    c["obs_start"] = M.S.starts(e["obs"])
    c["obs"] = np.array([k | (o << 16) | (st << 24) for p in e["obs"] for k, o, st, _ in p], np.uint32)
    c["obs_feat"] = np.array([f for p in e["obs"] for _, _, _, f in p], np.int32)
    return c


def _only_call(s, orig, c):
    """Scene s with call c of the scene `orig` as its only call (the lists and rows stay whole)."""
    s = dict(s)
    for f in ("call_kf", "call_kind", "call_list", "call_n", "call_feat"):
        s[f] = orig[f][c:c + 1]
    return s


def test_the_result_feeds_the_covisibility_graph(torch_cuda):
    """The chain out: kp_point_out, pt_bad_out and the observation CSR go into viorb_update_connections_device on the device, with the calls'
    key frames as targets; the result must equal the covisibility checker continued on the fusion checker's state."""
    from viorb_amd import covisibility as CV
    import covis_ref as CT
    scenes, exp, _ = K.random_streams()
    scenes, exp = scenes[:24], exp[:24]
    cc = 12

    def covis_scene(s, e):
        n = len(s["kf_bad"])
        z = np.zeros(n + 1, np.int32)
        targets = list(dict.fromkeys(int(k) for k in s["call_kf"]))
        return dict(targets=np.array(targets, np.int32), kf_by_key=s["kf_by_key"], kf_flags=np.zeros(n, np.uint8), kf_parent=np.full(n, -1, np.int32), kp_start=s["kp_start"],
                    kp_point=e["kp_point_out"], pt_bad=e["pt_bad_out"], obs_start=M.S.starts(e["obs"]), obs=_state_after(s, e)["obs"],
                    conn_start=z, conn_kf=np.zeros(0, np.int32), conn_w=np.zeros(0, np.int32), ord_start=z, ord_kf=np.zeros(0, np.int32), ord_w=np.zeros(0, np.int32))
    cov_want = [covis_scene(s, e) for s, e in zip(scenes, exp)]
    b = _tight(scenes)
    placeholder = [dict(c, pt_bad=np.ones_like(c["pt_bad"]), kp_point=np.full_like(c["kp_point"], -1), obs=np.zeros_like(c["obs"]), obs_start=np.zeros_like(c["obs_start"]))
                   for c in cov_want]
    cb = CV.CovisBatch(placeholder, ccap=cc)
    n_kp, n_pt, n_obs = b.P["n_kp"], b.P["n_pt"], int(cb.P["n_obs"])
    assert n_obs == b.P["n_obs_out"]
    cb.d["pt_bad"][:n_pt].copy_(b.o["pt_bad_out"][:n_pt])
    cb.d["kp_point"][:n_kp].copy_(b.o["kp_point_out"][:n_kp])
    cb.d["obs_start"].copy_(b.o["obs_start_out"])
    cb.d["obs"][:n_obs].copy_(b.o["obs_out"][:n_obs])
    cb.run()
    got = cb.results()
    want = [CT.update_connections(c, ccap=cc) for c in cov_want]
    assert all(w["status"] == CT.OK for w in want) and sum(int(w["t_observers"].sum()) for w in want) >= 50
    assert [CT.differences(g, w) for g, w in zip(got, want)] == [[]] * len(scenes)
    assert [T.differences(g, e) for g, e in zip(b.results(), exp)] == [[]] * len(scenes)


def test_the_dirty_lists_feed_the_point_update_and_the_merge_one_call_per_launch(torch_cuda):
    """The chain out, for two calls of two streams run one call per launch: the dirty CSR of the whole batch goes into
    viorb_map_points_update_device as it lies, viorb_fuse_merge_descriptors_device puts the recomputed rows into the map's descriptors,
    and the second launch starts from the first one's outputs on the device. Against the checkers' composition."""
    torch = torch_cuda
    import mapping_ref as MR
    from viorb_amd.mapping import mapping_camera
    scenes = [s for s in K.random_streams()[0] if len(s["call_kf"]) >= 2][:2]
    assert len(scenes) == 2
    rng = np.random.default_rng(11)
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    cam = mapping_camera(dict(intr4=[458.0, 457.0, 367.0, 248.0], mb=0.11, mbf=50.0, scale_factor=1.2, sf=sf, level_sigma2=sf * sf))
    kf_desc = [[rng.integers(0, 256, (int(s["kp_start"][k + 1] - s["kp_start"][k]), 32), dtype=np.uint8) for k in range(len(s["kf_bad"]))] for s in scenes]
    kf_oct = [[s["kp_octave"][s["kp_start"][k]:s["kp_start"][k + 1]].astype(np.int32) for k in range(len(s["kf_bad"]))] for s in scenes]
    kf_Ow = [[rng.normal(0, 1.5, 3).astype(np.float32) for _ in s["kf_bad"]] for s in scenes]
    Pw = [(rng.normal(0, 4, (len(s["pt_bad"]), 3)) + [0, 0, 9]).astype(np.float32) for s in scenes]
    desc = [rng.integers(0, 256, (len(s["pt_bad"]), 32), dtype=np.uint8) for s in scenes]           # the map's mDescriptor before the launches
    up = capi._torch_up
    d_desc = up(np.concatenate(desc))
    d_rows, d_oct = up(np.concatenate([r for kd in kf_desc for r in kd])), up(np.concatenate([o for ko in kf_oct for o in ko]))
    d_Ow, d_Pw = up(np.array([o for ko in kf_Ow for o in ko], np.float32)), up(np.concatenate(Pw))
    state, b_prev, n_dirty = scenes, None, 0
    for launch in (0, 1):
        step = [_only_call(s, orig, launch) for s, orig in zip(state, scenes)]
        exp = [T.apply_fuse(s) for s in step]
        b = _tight(step)
        if b_prev is not None:                                         # the inputs of this launch are the outputs of the last one, on the device
            for f, o in (("kp_point", "kp_point_out"), ("pt_bad", "pt_bad_out"), ("pt_nobs", "pt_nobs_out"), ("pt_found", "pt_found_out"), ("pt_visible", "pt_visible_out"),
                         ("obs_start", "obs_start_out"), ("obs", "obs_out"), ("obs_feat", "obs_feat_out")):
                b.d[f][:len(b_prev.o[o])].copy_(b_prev.o[o][:len(b.d[f])])
            b.run()
        got = b.results()
        assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * 2
        n_pt, n_kf = b.P["n_pt"], b.P["n_kf"]
        new_desc = torch.zeros((n_pt, 32), dtype=torch.uint8, device=b.dev)
        best = torch.zeros(n_pt, dtype=torch.int32, device=b.dev)
        pts_f = torch.zeros((n_pt, 8), dtype=torch.float32, device=b.dev)
        ref_obs = torch.zeros(n_pt, dtype=torch.int32, device=b.dev)
        base = up(b.P["kp_start"][:n_kf].astype(np.int64))
        st = M.S.stream_ptr(torch, b.dev)
        check(lib().viorb_map_points_update_device(ptr(b.o["dirty_obs_start"]), ptr(b.o["dirty_obs_kf"]), ptr(b.o["dirty_obs_feat"]), ptr(ref_obs), ptr(d_Pw), n_pt, ptr(base),
                                                   ptr(d_Ow), n_kf, ptr(d_rows), ptr(d_oct), int(d_rows.shape[0]), C.byref(cam), ptr(new_desc), ptr(best), ptr(pts_f), st))
        M.merge_descriptors(b.o["pt_dirty"], b.o["dirty_obs_start"], new_desc, d_desc, st)
        torch.cuda.synchronize()
        for i, (s, e) in enumerate(zip(step, exp)):                    # ComputeDistinctiveDescriptors of the checker's dirty lists
            for p, lst in enumerate(e["dirty"]):
                if lst:
                    desc[i][p] = MR.map_point_update([k for k, _ in lst], [f for _, f in lst], 0, Pw[i][p], kf_desc[i], kf_oct[i], kf_Ow[i], sf)[0]
                    n_dirty += 1
        assert np.array_equal(d_desc.cpu().numpy(), np.concatenate(desc)), launch
        state = [_state_after(s, e) for s, e in zip(step, exp)]
        b_prev = b
    assert n_dirty >= 3
