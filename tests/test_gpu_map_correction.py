"""The propagation of LoopClosing::CorrectLoop on the device (include/viorb_map_correction.h) against the checker
tests/map_correction_ref.py. The bar is bit equality: every element of every output array of viorb_correct_loop_device and of the
host-buffer form, floats and doubles as their bit patterns, on the hand-built scenes of tests/map_correction_cases.py, the scenes sized
around the kernels' strides and the first 64 random streams as one batch; one stream above the LDS key-frame limit; the largest scene
(80 key frames, 3000 points, points with 63, 64, 65 and 70 observers); two runs; every kind of broken snapshot in the middle of three
streams; caller workspaces that hold garbage; and the chain into viorb_optimize_essential_graph_device and viorb_fuse_sim3_device, which
read the results where they lie on the device."""
import ctypes as C
import numpy as np
import pytest
import viorb_amd
from viorb_amd import capi
from viorb_amd import map_correction as M
import map_correction_ref as T
import map_correction_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    import torch
    return torch


def device(scenes):
    b = M.CorrectLoopBatch(scenes)
    b.run()
    return b.results()


def bad_streams(names, got, exp):
    return [(n, T.differences(g, e)) for n, g, e in zip(names, got, exp) if T.differences(g, e)]


def test_hand_built_sized_and_random_scenes_as_one_batch_device_and_host_form(torch_cuda):
    named = [(c[0], c[1]) for c in K.CASES] + K.sized_scenes()
    scenes, rexp, _ = K.random_streams()
    names = [n for n, _ in named] + ["random_%d" % i for i in range(64)]
    batch = [s for _, s in named] + scenes[:64]
    exp = [K.expected(c[0]) for c in K.CASES] + [T.correct_loop(s) for _, s in K.sized_scenes()] + rexp[:64]
    b = M.CorrectLoopBatch(batch)
    b.run()
    first = b.results()
    assert bad_streams(names, first, exp) == []
    assert [(c[0], K.compare_want(g, c[2])) for c, g in zip(K.CASES, first) if K.compare_want(g, c[2])] == []
    b.run()                                                             # a second run over its own outputs' memory gives the same bits
    assert bad_streams(names, b.results(), exp) == []
    assert bad_streams(names, M.correct_loop(batch), exp) == []
    for (name, scene), e in list(zip(named, exp))[:len(K.CASES)]:       # and alone: at batch position 0
        assert T.differences(device([scene])[0], e) == [], name


def test_a_stream_above_the_lds_key_frame_limit(torch_cuda):
    lds_kf = M.shape()[3]
    big = K.random_scene(11, nk=lds_kf + 1, n_pt=300, n_kp=1, max_obs=9, n_members=400)
    at = K.random_scene(12, nk=lds_kf, n_pt=100, n_kp=1, max_obs=9, n_members=300)
    below = K.random_scene(13, nk=lds_kf - 1, n_pt=100, n_kp=1, max_obs=9, n_members=300)
    small = K.CASES[4][1]
    exp = [T.correct_loop(s) for s in (small, big, at, below)]
    assert exp[1]["pt_touched"].sum() >= 50 and exp[2]["pt_touched"].sum() >= 20 and exp[3]["pt_touched"].sum() >= 20
    assert bad_streams(("small", "above", "at", "below"), device([small, big, at, below]), exp) == []


def test_the_largest_scene_observers_across_the_wavefront(torch_cuda):
    s = K.large_scene()
    e = T.correct_loop(s)
    assert np.diff(s["obs_start"])[:4].tolist() == [63, 64, 65, 70] and e["pt_touched"][:4].all() and e["pt_touched"].sum() >= 1000
    assert len(s["kf_by_key"]) == 80 and len(s["pt_bad"]) == 3000 and K.full_observers(s) == 70
    for got in (device([s])[0], M.correct_loop([s])[0]):
        assert T.differences(got, e) == []


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams(torch_cuda):
    good, other = K.breakable_scene(), K.CASES[4][1]
    e_good, e_other = T.correct_loop(good), T.correct_loop(other)
    for i, (what, bad) in enumerate(K.broken(good)):
        forms = (device, M.correct_loop) if i % 6 == 0 else (device,)
        for form in forms:
            got = form([other, bad, good])
            assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
            assert T.differences(got[0], e_other) == [] and T.differences(got[2], e_good) == [], what


def test_the_workspace_contents_on_entry_are_ignored(torch_cuda):
    """k_correct_loop_prepare (key, memb, claim, Ow_in, Swi, info) and k_correct_loop_points (terms; above the LDS limit the key
    positions) on one allocation: zeroed twice, every byte 0xFF, and what a larger batch left behind."""
    import test_gpu_workspace_contents as WS
    named = dict(K.sized_scenes())
    scene = named["obs_65"]
    want = T.correct_loop(scene)

    def runner(ss):
        P = M.pack(ss)

        def run(ws):
            b = M.CorrectLoopBatch(ss, packed=P)
            WS._inject(b, ws, b._wb).run()
            return b.results()
        return viorb_amd.lib().viorb_correct_loop_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"], P["n_obs"]), run
    n, run = runner([scene])
    nb, run_big = runner([named["pt_257"], K.large_scene(), named["obs_64"]])
    WS.exact(WS.conditions(n, nb, run, run_big), lambda r: T.differences(r[0], want) == [] or pytest.fail(str(T.differences(r[0], want))))


def _sim3_of_f12(F):
    """r(x y z w) t s of a float [12], the top three rows of [s R | t]."""
    M4 = np.asarray(F, np.float64).reshape(3, 4)
    s = float(np.linalg.norm(M4[0, :3]))
    return list(T.mat2q((M4[:, :3] / s).tolist())) + [float(v) for v in M4[:, 3]] + [s]


def test_the_results_feed_the_essential_graph_and_fuse_where_they_lie(torch_cuda):
    """The chain: Scw_out / Smeas_out / pt_corrected_ref_out of viorb_correct_loop_device go into viorb_optimize_essential_graph_device and
    Scw_f12 into viorb_fuse_sim3_device as device pointers, with no host copy in between; both must give what the same calls give when
    fed from the checker's arrays."""
    torch = torch_cuda
    L = viorb_amd.lib()
    dev = torch.device("cuda", 0)
    up = capi._torch_up
    # ---- the essential graph over one stream: the spanning chain k - 1 -> k, the current key frame's neighbour fixed
    s = K.random_scene(21, nk=14, n_pt=60, n_kp=12, n_members=5)
    e = T.correct_loop(s)
    assert e["pt_touched"].sum() >= 10
    nk, npt = 14, 60
    edges = np.array([(k - 1, k) for k in range(1, nk)], np.int32)
    fixed = np.zeros(nk, np.uint8)
    fixed[int(s["conn"][0])] = 1
    b = M.CorrectLoopBatch([s])
    b.run()
    point_ref_want = np.where(e["pt_corrected_ref_out"] >= 0, e["pt_corrected_ref_out"], s["pt_ref"]).astype(np.int32)

    def essential_graph(Scw, Smeas, points, ref):
        d = dict(fixed=up(fixed), ei=up(edges), ec=up(np.zeros(len(edges), np.uint8)))
        So = torch.zeros((nk, 8), dtype=torch.float64, device=dev); To = torch.zeros((nk, 12), dtype=torch.float64, device=dev)
        Po = torch.zeros((npt, 3), dtype=torch.float32, device=dev)
        nbytes = L.viorb_essential_graph_workspace_bytes(nk, len(edges), npt)
        ws = capi.Workspace(torch, dev, nbytes)
        info = np.zeros(6)
        cfg = capi.EgConfig(5, 0)
        capi.check(L.viorb_optimize_essential_graph_device(C.byref(cfg), capi.ptr(Scw), capi.ptr(Smeas), capi.ptr(d["fixed"]), nk, capi.ptr(d["ei"]), capi.ptr(d["ec"]),
                                                           len(edges), capi.ptr(points), capi.ptr(ref), npt, capi.ptr(So), capi.ptr(To), capi.ptr(Po), capi.ptr(info),
                                                           ws.ptr, nbytes, None))
        torch.cuda.synchronize()
        return So.cpu().numpy(), To.cpu().numpy(), Po.cpu().numpy(), info
    # on the device: the positions are the first three of every pts_f_out row, point_ref is one select of two device arrays
    pts = b.o["pts_f_out"].view(-1, 8)[:npt, :3].contiguous()
    cref = b.o["pt_corrected_ref_out"][:npt]
    ref = torch.where(cref >= 0, cref, b.d["pt_ref"][:npt]).contiguous()
    got = essential_graph(b.o["Scw_out"], b.o["Smeas_out"], pts, ref)
    want = essential_graph(up(e["Scw_out"]), up(e["Smeas_out"]), up(np.ascontiguousarray(e["pts_f_out"][:, :3])), up(point_ref_want))
    assert T.differences(b.results()[0], e) == []
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert want[3][2] >= 1 and np.abs(want[2] - e["pts_f_out"][:, :3]).max() > 0                        # the solve ran and moved points
    # ---- fuse: three loop closures with an empty list; the corrected Sim3 of each current key frame is a fuse problem's Scw
    import sim3_match_cases as SK
    from viorb_amd import sim3_match as SM
    P = SK.problem(0, 60, 0, 3, 8, 300, 300, 300, 150)
    Lp, F = P["loop"], P["fuse"]
    B = len(F["frames"])
    scenes = [M.scene_from_lists([K.kf()], [], 0, [], _sim3_of_f12(F["Scw"][i]), K.CUR_ID) for i in range(B)]
    exp = [T.correct_loop(sc) for sc in scenes]
    cb = M.CorrectLoopBatch(scenes)
    cb.run()
    bt = SM.Sim3MatchBatch(F["frames"], SK.lib_camera(P), P["bounds4"])
    npts = len(Lp["pts_f"])
    d = [up(np.ascontiguousarray(Lp["pts_f"], np.float32)), up(np.ascontiguousarray(Lp["pts_desc"], np.uint8)), up(np.ascontiguousarray(F["valid"], np.uint8).reshape(B, npts))]

    def fuse(Scw):
        bi, re = [torch.zeros((B, npts), dtype=torch.int32, device=dev) for _ in range(2)]
        nf = torch.zeros(B, dtype=torch.int32, device=dev)
        ws, wb = bt._workspace(bt.cap, npts)
        capi.check(L.viorb_fuse_sim3_device(C.byref(bt.kf), capi.ptr(Scw), capi.ptr(d[0]), capi.ptr(d[1]), capi.ptr(d[2]), npts, npts, C.byref(bt.cam), capi.ptr(bt.bounds),
                                            float(SK.TH_FUSE), B, capi.ptr(bi), capi.ptr(nf), capi.ptr(re), ws, wb, bt._stream()))
        torch.cuda.synchronize()
        return bi.cpu().numpy(), nf.cpu().numpy(), re.cpu().numpy()
    got = fuse(cb.o["Scw_f12"])                                         # rows conn_start[b] + b = b: one member per stream
    want = fuse(up(np.concatenate([x["Scw_f12"] for x in exp]).astype(np.float32)))
    assert bad_streams(range(B), cb.results(), exp) == []
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert want[1].sum() >= 50                                          # the rows are poses under which the fuse finds its points


# ---- the map update after a global bundle adjustment ---------------------------------------------------------------------------------------------
def gba_bad(names, got, exp):
    return [(n, T.differences(g, e, T.AG_FIELDS)) for n, g, e in zip(names, got, exp) if T.differences(g, e, T.AG_FIELDS)]


def test_apply_global_ba_hand_built_sized_and_random_maps_device_and_host_form(torch_cuda):
    hand, want = K.gba_all_rules()
    for got in (M.ApplyGbaBatch([hand], K.TBC_I), ):
        got.run()
        r = got.results()[0]
        assert T.differences(r, T.apply_global_ba(hand, K.TBC_I), T.AG_FIELDS) == [] and K.compare_want(r, want) == []
    assert T.differences(M.apply_global_ba([hand], K.TBC_I)[0], T.apply_global_ba(hand, K.TBC_I), T.AG_FIELDS) == []
    scenes, rexp, _ = K.gba_random_streams()
    sized = K.gba_sized_scenes()
    batch = [hand] + [s for _, s in sized] + scenes[:64]
    names = ["hand"] + [n for n, _ in sized] + ["random_%d" % i for i in range(64)]
    exp = [T.apply_global_ba(hand, K.TBC)] + [T.apply_global_ba(s, K.TBC) for _, s in sized] + rexp[:64]
    b = M.ApplyGbaBatch(batch, K.TBC)
    b.run()
    assert gba_bad(names, b.results(), exp) == []
    b.run()                                                             # a second run gives the same bits
    assert gba_bad(names, b.results(), exp) == []
    assert gba_bad(names, M.apply_global_ba(batch, K.TBC), exp) == []


def test_apply_global_ba_the_largest_map_and_a_long_run_outside_the_adjustment(torch_cuda):
    big = K.gba_random_scene(9, nk=80, n_pt=3000)
    chain = K.gba_random_scene(10, nk=40, n_pt=50)                      # one chain of 40, only its root in the adjustment
    chain = dict(chain, child_start=np.arange(41, dtype=np.int32).clip(0, 39), child_kf=np.arange(1, 40, dtype=np.int32), origins=np.array([0], np.int32),
                 kf_in_gba=np.array([1] + [0] * 39, np.uint8))
    exp = [T.apply_global_ba(s, K.TBC) for s in (big, chain)]
    assert exp[1]["kf_reached"].all() and exp[1]["kf_in_gba_out"].all() and (exp[0]["pt_code"] == T.AG_BY_REF).sum() >= 300
    b = M.ApplyGbaBatch([big, chain], K.TBC)
    b.run()
    assert gba_bad(("big", "chain"), b.results(), exp) == []


def test_apply_global_ba_a_broken_map_is_refused_alone_and_a_dirty_workspace(torch_cuda):
    import test_gpu_workspace_contents as WS
    good, _ = K.gba_all_rules()
    other = K.gba_random_streams()[0][3]
    e_good, e_other = T.apply_global_ba(good, K.TBC_I), T.apply_global_ba(other, K.TBC_I)
    for what, bad in K.gba_broken(good):
        b = M.ApplyGbaBatch([other, bad, good], K.TBC_I)
        b.run()
        got = b.results()
        assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
        assert T.differences(got[0], e_other, T.AG_FIELDS) == [] and T.differences(got[2], e_good, T.AG_FIELDS) == [], what
    named = dict(K.gba_sized_scenes())
    scene = named["kf_257"]
    want = T.apply_global_ba(scene, K.TBC)

    def runner(ss):
        P = M.gba_pack(ss)

        def run(ws):
            b = M.ApplyGbaBatch(ss, K.TBC, packed=P)
            WS._inject(b, ws, b._wb).run()
            return b.results()
        return viorb_amd.lib().viorb_apply_global_ba_workspace_bytes(P["batch"], P["n_kf"]), run
    n, run = runner([scene])
    nb, run_big = runner([named["kf_256"], K.gba_random_scene(9, nk=80, n_pt=3000), named["kf_257"], named["kf_255"]])
    WS.exact(WS.conditions(n, nb, run, run_big), lambda r: T.differences(r[0], want, T.AG_FIELDS) == [] or pytest.fail(str(T.differences(r[0], want, T.AG_FIELDS))))
