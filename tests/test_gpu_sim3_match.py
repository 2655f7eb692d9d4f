"""GPU tests of the Sim3 matchers (include/viorb_sim3_match.h): the host and device forms of viorb_keyframe_grid, viorb_search_by_sim3,
viorb_search_by_projection_sim3 and viorb_fuse_sim3 are np.array_equal to the numpy checker tests/sim3_match_ref.py (indices, counts and
reason codes), on the fixture whose conditions tests/test_sim3_match_ref.py asserts and on the small shapes where a kernel can go wrong."""
import ctypes as C
import numpy as np
import pytest
from viorb_amd import capi, sim3
from viorb_amd import sim3_match as M
from viorb_amd.capi import lib, check, ptr
import sim3_match_ref as T
import sim3_match_cases as K

pytestmark = pytest.mark.gpu
f32 = np.float32
SIM3_KEYS = ("match12", "nfound", "match1", "match2", "reason1", "reason2")
PROJ_KEYS = ("best_idx", "nmatches", "reason")
FUSE_KEYS = ("best_idx", "nfused", "reason")
SMALL = (0, 60, 0, 1, 8, 300, 300, 300, 150)            # problem(): 60 duplicates, no cluster, one key frame, 300 features, 150 common


def _cut_side(s, n):
    return {k: (v if k == "pose12" else v[:n]) for k, v in s.items()}


def _batch(P, frames, cap=None):
    return M.Sim3MatchBatch(frames, K.lib_camera(P), P["bounds4"], cap=cap)


# ---- the key-frame grid -------------------------------------------------------------------------------------------------------------------
def test_keyframe_grid_equals_the_checker_and_the_frontend_grid():
    from viorb_amd.frontend import Frontend
    import torch
    P = K.problem()
    frames = [(P["kf1"]["kps"], P["kf1"]["desc"]), (P["kf2"]["kps"][:517].copy(), P["kf2"]["desc"][:517]), (P["kf2"]["kps"][:0], P["kf2"]["desc"][:0])]
    frames[1][0]["x"][:3] = [-40.0, 800.0, 751.9]                                        # features the grid drops, and one in its last column
    bt = _batch(P, frames, cap=1100)
    cs, ci = bt.grid()
    for b, (k, d) in enumerate(frames):
        ecs, eci = K.ref_keyframe(P, k, d).csr()
        assert np.array_equal(cs[b], ecs) and np.array_equal(ci[b, :ecs[-1]], eci)
        hcs, hci = M.keyframe_grid(k, P["bounds4"])
        assert np.array_equal(hcs, ecs) and np.array_equal(hci, eci)
    cam16 = np.zeros(16); cam16[:4] = P["intr4"]
    fe = Frontend(cam16, [0, 0, -9.81], P["sf"], 1 / P["sf"] ** 2, bounds=tuple(P["bounds4"]), max_batch=3, cap=1100)
    fcs, fci = torch.zeros_like(bt.cell_start), torch.zeros_like(bt.cell_idx)
    fe.grid(bt.kps.data_ptr(), bt.count.data_ptr(), 3, fcs, fci)
    torch.cuda.synchronize()
    assert np.array_equal(fcs.cpu().numpy(), cs) and np.array_equal(fci.cpu().numpy(), ci)


# ---- equality on the fixture ----------------------------------------------------------------------------------------------------------------
def test_search_by_sim3_host_and_device_equal_the_checker():
    P, want = K.problem(), K.expected_sim3()
    cam, a, b = K.lib_camera(P), P["kf1"], P["kf2"]
    K.same(M.search_by_sim3(a, b, P["R12"], P["t12"], P["s12"], cam, P["bounds4"], K.TH_SIM3), want, SIM3_KEYS)
    # a batch of three pairs with different counts (one side empty in the last), cap larger than every count
    cuts = [(1000, 1000), (640, 777), (300, 0)]
    s1 = [_cut_side(a, n) for n, _ in cuts]; s2 = [_cut_side(b, n) for _, n in cuts]
    b1, b2 = _batch(P, [(s["kps"], s["desc"]) for s in s1], cap=1030), _batch(P, [(s["kps"], s["desc"]) for s in s2], cap=1001)
    side = lambda bt, ss: bt.side(*[[s[k] for s in ss] for k in ("pose12", "has_point", "pts_f", "pts_desc", "already")])
    model = (np.stack([P["R12"]] * 3), np.stack([P["t12"]] * 3), np.full(3, P["s12"], f32))
    got = b1.search_by_sim3(side(b1, s1), b2, side(b2, s2), *model, th=K.TH_SIM3)
    K.same(got[0], want, SIM3_KEYS)
    for j in (1, 2):
        K.same(got[j], K.ref_search_by_sim3(P, s1[j], s2[j]), SIM3_KEYS)
    assert got[2]["nfound"] == 0 and (got[2]["match1"] == -1).all() and len(got[2]["match2"]) == 0
    only = b1.search_by_sim3(side(b1, s1), b2, side(b2, s2), *model, th=K.TH_SIM3, raw=False)       # without the optional outputs
    for j in range(3):
        assert np.array_equal(only[j]["match12"], got[j]["match12"]) and only[j]["nfound"] == got[j]["nfound"]


def test_search_by_sim3_reads_the_ransac_model_where_it_lies():
    """R12 / t12 / s12 go from viorb_sim3_ransac_device to viorb_search_by_sim3_device as device arrays; the result equals the host form
    fed the downloaded model."""
    import torch
    P = K.problem()
    a, b = P["kf1"], P["kf2"]
    common = np.nonzero(P["truth12"] >= 0)[0][:300]
    X = lambda s, idx: (s["pts_f"][idx, :3].astype(np.float64) @ s["pose12"][:9].reshape(3, 3).astype(np.float64).T + s["pose12"][9:]).astype(f32)
    sig = lambda s, idx: (P["sf"][s["kps"]["octave"][idx]] ** 2).astype(f32)
    prob = dict(X1c=X(a, common), X2c=X(b, P["truth12"][common]), sigma2_1=sig(a, common), sigma2_2=sig(b, P["truth12"][common]), K1=P["intr4"], K2=P["intr4"])
    sets = sim3.draw_sets(len(common), 60, 3)
    sb = sim3.Sim3Batch([prob], [sets])
    dev = sb.dev
    out = dict(status=torch.zeros(1, dtype=torch.int32, device=dev), R12=torch.zeros((1, 3, 3), device=dev), t12=torch.zeros((1, 3), device=dev),
               s12=torch.zeros(1, device=dev))
    O = capi.Sim3Outputs(**{f: ptr(out.get(f)) for f in capi.SIM3_OUTPUT_FIELDS})
    cfg = sb._cfg(60)
    mx, fi, bi = sb._state(None, 60), sb._state(None, 0), sb._state(None, 0)
    check(lib().viorb_sim3_ransac_device(C.byref(sb.inputs), C.byref(cfg), ptr(sb.sets), ptr(mx), ptr(fi), ptr(bi), 1, C.byref(O), sb.ws_ptr, sb.ws_bytes, sb._stream()))
    b1, b2 = _batch(P, [(a["kps"], a["desc"])]), _batch(P, [(b["kps"], b["desc"])])
    side = lambda bt, s: bt.side(*[[s[k]] for k in ("pose12", "has_point", "pts_f", "pts_desc", "already")])
    got = b1.search_by_sim3(side(b1, a), b2, side(b2, b), out["R12"], out["t12"], out["s12"], th=K.TH_SIM3)[0]
    assert int(out["status"].cpu()[0]) == sim3.FOUND
    R, t, s = out["R12"].cpu().numpy()[0], out["t12"].cpu().numpy()[0], out["s12"].cpu().numpy()[0]
    assert abs(s - P["s12"]) < 0.02 and np.abs(R - P["R12"]).max() < 0.01
    K.same(got, M.search_by_sim3(a, b, R, t, s, K.lib_camera(P), P["bounds4"], K.TH_SIM3), SIM3_KEYS)
    K.same(got, K.ref_search_by_sim3(P, model=(R, t, s)), SIM3_KEYS)
    assert got["nfound"] >= 100


def test_search_by_projection_is_the_ordered_loop_not_the_unordered_one():
    P, want, unordered = K.problem(), K.expected_projection(True), K.expected_projection(False)
    L, a = P["loop"], P["kf1"]
    host = M.search_by_projection_sim3(a["kps"], a["desc"], L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], L["feat_taken"], K.lib_camera(P), P["bounds4"], K.TH_PROJ)
    K.same(host, want, PROJ_KEYS)
    dev = _batch(P, [(a["kps"], a["desc"])], cap=1024).search_by_projection(L["Scw"][None], [L["pts_f"]], [L["pts_desc"]], [L["valid"]], [L["feat_taken"]],
                                                                          K.TH_PROJ, pcap=len(L["pts_f"]) + 77)[0]
    K.same(dev, want, PROJ_KEYS)
    assert (dev["tail"] == -1).all()
    assert not np.array_equal(dev["best_idx"], unordered["best_idx"]) and (dev["best_idx"] != unordered["best_idx"]).sum() >= 20


def test_fuse_shared_list_with_different_valid_flags_equals_the_checker():
    P, want = K.problem(), K.expected_fuse()
    L, F = P["loop"], P["fuse"]
    cam = K.lib_camera(P)
    for b, (k, d) in enumerate(F["frames"]):
        K.same(M.fuse_sim3(k, d, F["Scw"][b], L["pts_f"], L["pts_desc"], F["valid"][b], cam, P["bounds4"], K.TH_FUSE), want[b], FUSE_KEYS)
    got = _batch(P, F["frames"], cap=1010).fuse(F["Scw"], L["pts_f"], L["pts_desc"], F["valid"], K.TH_FUSE, pcap=len(L["pts_f"]) + 5)
    for b in range(len(want)):
        K.same(got[b], want[b], FUSE_KEYS)
        assert (got[b]["tail"] == -1).all()


# ---- small shapes ---------------------------------------------------------------------------------------------------------------------------
def _edge_counts():
    block, wave, _ = M.shape()
    return sorted({0, 1, wave - 1, wave, wave + 1, block - 1, block, block + 1, 2 * block + 1})


def test_point_counts_around_the_workgroup_and_the_wavefront():
    P = K.problem(*SMALL)
    L, a, cam = P["loop"], P["kf1"], K.lib_camera(P)
    assert len(L["pts_f"]) > max(_edge_counts())
    kf = K.ref_keyframe(P, a["kps"], a["desc"])
    for n in _edge_counts():
        pf, pd, pv = L["pts_f"][:n], L["pts_desc"][:n], L["valid"][:n]
        K.same(M.search_by_projection_sim3(a["kps"], a["desc"], L["Scw"], pf, pd, pv, L["feat_taken"], cam, P["bounds4"], K.TH_PROJ),
               T.search_by_projection(kf, L["Scw"], pf, pd, pv, L["feat_taken"], K.TH_PROJ), PROJ_KEYS)
        K.same(M.fuse_sim3(a["kps"], a["desc"], L["Scw"], pf, pd, pv, cam, P["bounds4"], K.TH_FUSE), T.fuse(kf, L["Scw"], pf, pd, pv, K.TH_FUSE), FUSE_KEYS)
        s1, s2 = _cut_side(a, n), _cut_side(P["kf2"], min(n + 1, 300))
        K.same(M.search_by_sim3(s1, s2, P["R12"], P["t12"], P["s12"], cam, P["bounds4"], K.TH_SIM3), K.ref_search_by_sim3(P, s1, s2), SIM3_KEYS)


def test_a_key_frame_with_one_feature_and_a_batch_with_an_empty_and_a_full_key_frame():
    P = K.problem(*SMALL)
    L, a, cam = P["loop"], P["kf1"], K.lib_camera(P)
    full = T.search_by_projection(K.ref_keyframe(P, a["kps"], a["desc"]), L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], L["feat_taken"], K.TH_PROJ)
    f = int(full["best_idx"][np.nonzero(full["best_idx"] == L["source"])[0][0]])                  # a feature its own point takes, alone in its key frame
    k1, d1 = a["kps"][f:f + 1], a["desc"][f:f + 1]
    kf = K.ref_keyframe(P, k1, d1)
    want = T.search_by_projection(kf, L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], [0], K.TH_PROJ)
    assert want["nmatches"] == 1
    K.same(M.search_by_projection_sim3(k1, d1, L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], [0], cam, P["bounds4"], K.TH_PROJ), want, PROJ_KEYS)
    K.same(M.fuse_sim3(k1, d1, L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], cam, P["bounds4"], K.TH_FUSE),
           T.fuse(kf, L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], K.TH_FUSE), FUSE_KEYS)
    # three key frames, three point counts (one 0), every feature of the last one taken on entry; cap and pcap larger than every count
    frames = [(a["kps"], a["desc"]), (a["kps"][:120], a["desc"][:120]), (a["kps"][:200], a["desc"][:200])]
    counts = [len(L["pts_f"]), 0, 333]
    taken = [L["feat_taken"], L["feat_taken"][:120], np.ones(200, np.uint8)]
    bt = _batch(P, frames, cap=310)
    got = bt.search_by_projection(np.stack([L["Scw"]] * 3), [L["pts_f"][:n] for n in counts], [L["pts_desc"][:n] for n in counts],
                                  [L["valid"][:n] for n in counts], taken, K.TH_PROJ, pcap=counts[0] + 9)
    for b, (k, d) in enumerate(frames):
        n = counts[b]
        K.same(got[b], T.search_by_projection(K.ref_keyframe(P, k, d), L["Scw"], L["pts_f"][:n], L["pts_desc"][:n], L["valid"][:n], taken[b], K.TH_PROJ), PROJ_KEYS)
        assert (got[b]["tail"] == -1).all()
    assert got[0]["nmatches"] > 0 and got[1]["nmatches"] == 0 and got[2]["nmatches"] == 0
    assert (got[2]["reason"] == T.ABOVE_THRESHOLD).sum() > 0 and (got[2]["reason"] == T.MATCHED).sum() == 0
    fused = bt.fuse(np.stack([L["Scw"]] * 3), L["pts_f"][:0], L["pts_desc"][:0], np.zeros((3, 0), np.uint8), K.TH_FUSE, pcap=4)       # 0 points
    assert all(r["nfused"] == 0 and (r["tail"] == -1).all() for r in fused)


def test_a_single_scale_level():
    P = K.problem(1, 20, 0, 1, 1, 100, 300, 300, 150, True)            # one level: the distance gate only passes at a unit scale
    assert len(P["sf"]) == 1
    L, a, cam = P["loop"], P["kf1"], K.lib_camera(P)
    kf = K.ref_keyframe(P, a["kps"], a["desc"])
    want = T.search_by_projection(kf, L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], L["feat_taken"], K.TH_PROJ)
    assert want["nmatches"] >= 50
    K.same(M.search_by_projection_sim3(a["kps"], a["desc"], L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], L["feat_taken"], cam, P["bounds4"], K.TH_PROJ), want, PROJ_KEYS)
    K.same(M.fuse_sim3(a["kps"], a["desc"], L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], cam, P["bounds4"], K.TH_FUSE),
           T.fuse(kf, L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], K.TH_FUSE), FUSE_KEYS)
    want = K.ref_search_by_sim3(P)
    assert want["nfound"] >= 50
    K.same(M.search_by_sim3(a, P["kf2"], P["R12"], P["t12"], P["s12"], cam, P["bounds4"], K.TH_SIM3), want, SIM3_KEYS)


def test_the_largest_capacity():
    """cap == VIORB_S3M_MAX_FEATURES: the grid's sort and the claim's owner table take 64 KiB of LDS, which both kernels have to ask for."""
    P = K.problem(*SMALL)
    L, a = P["loop"], P["kf1"]
    bt = _batch(P, [(a["kps"], a["desc"])], cap=M.MAX_FEATURES)
    cs, ci = bt.grid()
    ecs, eci = K.ref_keyframe(P, a["kps"], a["desc"]).csr()
    assert np.array_equal(cs[0], ecs) and np.array_equal(ci[0, :ecs[-1]], eci)
    got = bt.search_by_projection(L["Scw"][None], [L["pts_f"]], [L["pts_desc"]], [L["valid"]], [L["feat_taken"]], K.TH_PROJ)[0]
    K.same(got, T.search_by_projection(K.ref_keyframe(P, a["kps"], a["desc"]), L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], L["feat_taken"], K.TH_PROJ), PROJ_KEYS)
