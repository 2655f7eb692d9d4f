"""Tracking::UpdateLocalMap on the device (include/viorb_local_map.h) against the checker tests/local_map_ref.py: every output array of
viorb_update_local_map_device and of the host-buffer form, compared exactly, on the hand-built scenes of tests/local_map_cases.py, on
scenes sized around the kernels' strides and chunks, on 300 random streams in one batch and again one stream per call, and on every kind
of broken snapshot in the middle of three streams; the four outputs of viorb_local_points_gather_device against a numpy packing; and the
chain into viorb_frontend_search_local_points_device, which must give the same matches from the gathered arrays as from the same points
packed by numpy."""
import numpy as np
import pytest
import viorb_amd
from viorb_amd import local_map as M
from viorb_amd.synth import make_vi_stream, cam_pose_from_navstate
import local_map_ref as T
import local_map_cases as K

pytestmark = pytest.mark.gpu
BOUNDS = (0.0, 752.0, 0.0, 480.0)


@pytest.fixture(scope="module")
def torch_cuda():
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")
    import torch
    return torch


def device(scenes, **caps):
    b = M.LocalMapBatch(scenes, **caps)
    b.run()
    return b.results()


def test_hand_built_scenes_device_and_host_form(torch_cuda):
    for name, scene, caps, _ in K.CASES:
        e = K.expected(name)
        assert T.differences(device([scene], **caps)[0], e) == [], name
        assert T.differences(M.update_local_map([scene], **caps)[0], e) == [], name
    # all of them as one batch of unequal streams (default row lengths: nothing overflows), an empty stream among them
    scenes = [c[1] for c in K.CASES]
    exp = [T.update_local_map(s) for s in scenes]
    for got in (device(scenes), M.update_local_map(scenes)):
        assert [(c[0], T.differences(g, e)) for c, g, e in zip(K.CASES, got, exp) if T.differences(g, e)] == []


def test_edges_of_the_kernels_shapes(torch_cuda):
    named = K.sized_scenes()
    scenes = [s for _, s in named]
    exp = [T.update_local_map(s) for s in scenes]
    got = device(scenes)
    assert [(n, T.differences(g, e)) for (n, _), g, e in zip(named, got, exp) if T.differences(g, e)] == []
    thr, chunk, wave, lds_kf = M.shape()
    big = next(s for n, s in named if n == "kf_%d" % (lds_kf + 1))                          # votes and marks in the workspace, alone and at batch position 0
    assert T.differences(device([big])[0], T.update_local_map(big)) == []
    loop = next(s for n, s in named if n == "loop_kf_%d" % (lds_kf + 1))                    # and there the neighbour loop's pushes: few voted, most of the list added
    e = T.update_local_map(loop)
    assert e["n_voted"] <= 12 and e["n_lkf"] >= e["n_voted"] + 15 and T.differences(device([loop])[0], e) == []


def test_random_streams_in_one_batch(torch_cuda):
    scenes, exp = K.random_streams()
    for got in (device(scenes), M.update_local_map(scenes)):
        assert [T.differences(g, e) for g, e in zip(got, exp)] == [[]] * 300


def test_random_streams_one_per_call(torch_cuda):
    scenes, exp = K.random_streams()
    bad = []
    for i, (s, e) in enumerate(zip(scenes, exp)):
        if T.differences(device([s])[0], e):
            bad.append(i)
    assert bad == []


def test_outputs_are_optional_and_a_second_run_gives_the_same(torch_cuda):
    scenes, exp = K.random_streams()
    b = M.LocalMapBatch(scenes[:40])
    b.run(outputs=False)
    b.run(); b.run()
    assert [T.differences(g, e) for g, e in zip(b.results(), exp[:40])] == [[]] * 40


def test_a_broken_snapshot_is_refused_alone_between_two_good_streams(torch_cuda):
    good, other = K.breakable_scene(), next(c[1] for c in K.CASES if c[0] == "neighbour_choice")
    e_good, e_other = T.update_local_map(good), T.update_local_map(other)
    for what, bad in K.broken(good):
        for got in (device([other, bad, good]), M.update_local_map([other, bad, good])):
            assert got[1]["status"] == T.INVALID and got[1]["untouched"], what
            assert T.differences(got[0], e_other) == [] and T.differences(got[2], e_good) == [], what


def pad(torch, arrs, cap, dtype, tail=()):
    """[len(arrs)][cap] on the device, each row holding one array and zeros after it (key-point records as their bytes)."""
    out = np.zeros((len(arrs), cap) + tuple(tail), dtype)
    for b, a in enumerate(arrs):
        out[b, :len(a)] = a
    return torch.from_numpy(out.view(np.uint8).reshape(out.shape + (-1,)) if dtype == viorb_amd.KP_DTYPE else out).cuda()


def point_store(torch, P, seed):
    rng = np.random.default_rng(seed)
    n = max(P["n_pt"], 1)
    f, d = rng.standard_normal((n, 8)).astype(np.float32), rng.integers(0, 256, (n, 32)).astype(np.uint8)
    nobs = rng.integers(-1, 4, n).astype(np.int32)
    return (f, d, nobs), tuple(torch.from_numpy(a).cuda() for a in (f, d, nobs))


def test_gather_equals_the_numpy_packing(torch_cuda):
    torch = torch_cuda
    scenes, _ = K.random_streams()
    # a refused stream, a stream that overflows pcap (the largest of the batch by one) and the rest
    scenes = scenes[:60] + [K.broken(K.breakable_scene())[0][1]] + scenes[60:120]
    exp = [T.update_local_map(s) for s in scenes[:60] + scenes[61:]]
    pcap = max(e["n_lpt"] for e in exp) - 1
    b = M.LocalMapBatch(scenes, pcap=pcap)
    b.run()
    res = b.results()
    assert sorted(set(r["status"] for r in res)) == [T.INVALID, T.OK, T.NO_VOTES, T.OVERFLOW]
    host, dev = point_store(torch, b.P, 3)
    got = [t.cpu().numpy() for t in b.gather(*dev)]
    want = M.gather_reference(b.P, res, *host)
    for g, w, name in zip(got, want, ("pts_f", "pts_desc", "pts_count", "pts_flags")):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
    assert set(np.unique(want[3]).tolist()) == {0, 1, 3, 5, 7} and (want[2] > 0).sum() >= 100


def test_gathered_points_give_search_local_points_the_same_matches(torch_cuda, oracle):
    """Frame matches -> local map -> SearchLocalPoints with no host step in between: two key frames per stream hold the points made from
    their keypoints, the current frame holds a few of them, and the search runs on what the gather wrote."""
    torch = torch_cuda
    from viorb_amd.synth import make_local_map, plane_points_f32
    ex = oracle.Extractor()
    sf = ex.tables()["scale"]
    scenes, stores, cur = [], [], []
    for seed in (4, 6):
        s = make_vi_stream(seed, 3)
        feats = [ex(f) for f in s["frames"]]
        rng = np.random.default_rng(seed)
        pf, pd, kfs, pts = [], [], [], []
        for j in (0, 1):
            k, d = feats[j]
            Rcw, tcw = cam_pose_from_navstate(s["ns_true"][j], s["cam"])
            Pw = plane_points_f32(np.stack([k["x"], k["y"]], 1), np.concatenate([Rcw.ravel(), tcw]), s["cam"])
            base = len(pts)
            pf.append(make_local_map(k, Pw, s["ns_true"][j], s["cam"], sf)); pd.append(d)
            pts += [K.pt(j, bad=bool(rng.random() < 0.05)) for _ in range(len(k))]
            kfs.append(K.kf([base + i if rng.random() < 0.9 else -1 for i in range(len(k))]))
        k2, d2 = feats[2]
        frame = [int(p) if rng.random() < 0.3 else -1 for p in rng.integers(0, len(pts), len(k2))]
        Rcw, tcw = cam_pose_from_navstate(s["ns_true"][2], s["cam"])
        scenes.append(M.scene_from_lists(kfs, pts, frame, by_key=[1, 0]))
        stores.append((np.concatenate(pf), np.concatenate(pd), rng.integers(0, 3, len(pts)).astype(np.int32)))
        cur.append(dict(s=s, k2=k2, d2=d2, pose=np.concatenate([Rcw.ravel(), tcw]).astype(np.float32)))
    B, cap, pcap = 2, 1016, 2100
    b = M.LocalMapBatch(scenes, cap=cap, pcap=pcap)
    b.run()
    host = tuple(np.concatenate([st[i] for st in stores]) for i in range(3))
    g_f, g_d, g_c, g_fl = b.gather(*[torch.from_numpy(a).cuda() for a in host])
    res = b.results()
    assert [T.differences(r, T.update_local_map(s)) for r, s in zip(res, scenes)] == [[], []] and all(r["n_lpt"] > 1000 for r in res)
    w_f, w_d, w_c, w_fl = [torch.from_numpy(a).cuda() for a in M.gather_reference(b.P, res, *host)]
    assert ((w_fl.cpu().numpy() & 2) != 0).sum() > 100
    t = ex.tables()
    fe = viorb_amd.Frontend(cur[0]["s"]["cam"], cur[0]["s"]["gw"], t["scale"], t["inv_sigma2"], BOUNDS, max_batch=B, cap=cap)
    ck = pad(torch, [c["k2"] for c in cur], cap, viorb_amd.KP_DTYPE); cd = pad(torch, [c["d2"] for c in cur], cap, np.uint8, (32,))
    cc = torch.tensor([len(c["k2"]) for c in cur], dtype=torch.int32, device="cuda")
    cs = torch.zeros((B, 3073), dtype=torch.int32, device="cuda"); ci = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    fe.grid(ck.data_ptr(), cc.data_ptr(), B, cs, ci)
    fpo = np.stack([np.asarray(r["frame_point_out"]) for r in res])
    own = torch.from_numpy(np.stack([((fpo[i] >= 0) & (stores[i][2][np.maximum(fpo[i], 0)] > 0)).astype(np.uint8) for i in range(B)])).cuda()
    pose = torch.from_numpy(np.stack([c["pose"] for c in cur])).cuda()
    outs = []
    for pf, pfl, pd, pc in ((g_f, g_fl, g_d, g_c), (w_f, w_fl, w_d, w_c)):
        match = torch.full((B, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.zeros(B, dtype=torch.int32, device="cuda")
        fr = torch.zeros((B, pcap, 5), dtype=torch.float32, device="cuda"); status = torch.zeros(B, dtype=torch.int32, device="cuda")
        fe.search_local_points(ck.data_ptr(), cd.data_ptr(), cc.data_ptr(), cs, ci, pose, pf, pfl, pd, pc, 1.0, 0.8, own, B, match, nm, fr, status)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        outs.append((match.cpu().numpy(), nm.cpu().numpy(), fr.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2].view(np.uint32), outs[1][2].view(np.uint32))
    assert (outs[0][1] > 50).all()
