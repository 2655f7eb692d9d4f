"""-m gpu: map-point creation on the device (viorb_amd/csrc/mapping.hip) against the numpy restatement tests/mapping_ref.py.

Tolerances (mapping_ref.py holds the constants, tests/test_mapping_ref.py::test_float32_restatement_against_float64 measures them):
  POS_DEV_F32 = 1.6e-7   the largest relative deviation of the restatement's own float32 path (LAPACK's float32 SVD) from the float64
                         definitional position on the parameter sets below (median 3.4e-8 over 20 255 pairs);
  POS_TOL_GPU = 4 x that = 6.4e-7: triangulated positions cannot be bit-compared because the device's SVD is a Jacobi and the
                         checker's is LAPACK's; a different SVD has the same order of backward error but not the same constants.
  DECISION_BAND[g] = 10 x GATE_DEV_F32[g], per gate quantity (parallax cosine 1.5e-6, depth against 0 2.5e-4, squared reprojection
                         error 3e-3, distance ratio 6.5e-6): a pair with a gate quantity that close to its threshold may flip between
                         two correct float32 implementations; it is left out of the accept / reason comparison and its i1 out of later
                         neighbours'. At most MAX_BAND_SHARE = 2 % of the pairs of a test case may be left out (asserted; the reference
                         alone leaves out 0.1 - 0.4 %). Everything else must match exactly."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viorb_amd
from viorb_amd import capi
from viorb_amd.synth import make_mapping_problem
import mapping_ref as mr

pytestmark = pytest.mark.gpu

# The two measured numbers (see the module docstring; one source: mapping_ref.py, re-measured by the CPU suite on every run)
POS_DEV_F32 = mr.POS_DEV_F32                    # 1.6e-7: float32 restatement (LAPACK) against float64, largest relative position deviation
POS_TOL_GPU = 4 * POS_DEV_F32                   # 6.4e-7: what the device's positions may deviate from the float64 definitional check
GATE_DEV_F32 = mr.GATE_DEV_F32                  # per gate quantity: cos 1.5e-7, depth 2.5e-5, reproj 3.0e-4, ratio 6.5e-7
DECISION_BAND = {g: 10 * v for g, v in GATE_DEV_F32.items()}
MAX_BAND_SHARE = 0.02
assert POS_TOL_GPU == mr.POS_TOL_GPU and DECISION_BAND == mr.DECISION_BAND and MAX_BAND_SHARE == mr.MAX_BAND_SHARE


def need_gpu():
    if viorb_amd.lib().viorb_device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (and never fall back)")


def oracle_search(oracle, cam):
    def f(kf1, hp1, kf2):
        return oracle.search_for_triangulation(kf1["kps"], kf1["desc"], hp1, kf1["ur"], kf1["node"], kf2["kps"], kf2["desc"], kf2["hp"], kf2["ur"], kf2["node"],
                                               kf2["F12"], kf1["Ow"], kf2["pose12"], cam["intr4"], cam["sf"], cam["level_sigma2"], False, False)[1]
    return f


def check_pairs(cam, kf1, kf2, m12, got, tally):
    acc, Pw, rea = got
    r32 = mr.triangulate_pairs(cam, kf1, kf2, m12, "f32")
    r64 = mr.triangulate_pairs(cam, kf1, kf2, m12, "f64")
    band = mr.in_band(r32)
    keep = ~band
    np.testing.assert_array_equal(rea[keep], r32["reason"][keep])
    np.testing.assert_array_equal(acc[keep], r32["accept"][keep])
    np.testing.assert_array_equal(acc, (rea == mr.ACCEPT).astype(np.uint8))
    pt = keep & (r32["reason"] != mr.NO_PAIR) & (r32["reason"] != mr.NO_POINT)          # a 3-D point exists: compare it whatever gate ended the pair
    if pt.any():
        dev = np.linalg.norm(Pw[pt] - r64["Pw"][pt], axis=1) / np.linalg.norm(r64["Pw"][pt], axis=1)
        a = pt & (r32["accept"] == 1)
        tally["pos"] = max(tally["pos"], float(dev[a[pt]].max(initial=0.0)))
        assert dev[a[pt]].max(initial=0.0) <= POS_TOL_GPU
    assert (Pw[r32["reason"] == mr.NO_PAIR] == 0).all()
    tally["pairs"] += len(r32["idx1"]); tally["band"] += int(band.sum())
    tally["reasons"] += np.bincount(r32["reason"], minlength=256)[:7]


@pytest.mark.parametrize("params", mr.PARAM_SETS)
@pytest.mark.parametrize("batch", [1, 7])
def test_triangulate_pairs_equals_the_restatement(params, batch, oracle):
    need_gpu()
    seed, J, n, sfrac = params
    p = make_mapping_problem(seed, J=J, n1=n, n2=n, stereo_frac=sfrac)
    cam, kf1 = p["cam"], p["kf1"]
    tally = dict(pos=0.0, pairs=0, band=0, reasons=np.zeros(7, np.int64))
    if batch == 1:
        for kf2 in p["neigh"]:
            check_pairs(cam, kf1, kf2, kf2["match_gen"], viorb_amd.TriangulatePairs(cam, kf1, kf2, kf2["match_gen"]), tally)
        kf2 = p["neigh"][J - 2]                              # and the pairs the search itself finds
        m12 = oracle_search(oracle, cam)(kf1, kf1["hp"], kf2)
        assert (m12 >= 0).sum() > 20
        check_pairs(cam, kf1, kf2, m12, viorb_amd.TriangulatePairs(cam, kf1, kf2, m12), tally)
    else:
        kf2s = [p["neigh"][(3 * b + 1) % J] for b in range(batch)]
        got = viorb_amd.TriangulatePairsBatch(cam, [kf1] * batch, kf2s, [k["match_gen"] for k in kf2s])
        for kf2, g in zip(kf2s, got):
            check_pairs(cam, kf1, kf2, kf2["match_gen"], g, tally)
    print("params", params, "batch", batch, tally)
    assert (tally["reasons"] >= (10 if batch == 1 else 1)).all()          # batch 1 runs every neighbour, the batch of 7 a third of them
    assert tally["band"] <= MAX_BAND_SHARE * tally["pairs"]


def _points_problem(seed, npts, nkf=40, nfeat=500):
    rng = np.random.Generator(np.random.PCG64(seed))
    kf_desc = [rng.integers(0, 256, (nfeat, 32), dtype=np.uint8) for _ in range(nkf)]
    kf_oct = [rng.integers(0, 8, nfeat).astype(np.int32) for _ in range(nkf)]
    kf_Ow = [rng.normal(0, 1.5, 3).astype(np.float32) for _ in range(nkf)]
    obs, ref, Pw = [], [], []
    for p in range(npts):
        u = rng.random()
        N = int(rng.integers(1, 21)) if u < 0.9 else int(rng.integers(21, 65)) if u < 0.97 else int(rng.integers(65, 301)) if u < 0.995 else 64 + int(rng.integers(0, 2))
        kfs = rng.integers(0, nkf, N); feats = rng.integers(0, nfeat, N)
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for k, f in zip(kfs, feats):                       # look-alike observations (a later point may overwrite: still a valid input)
            d = base.copy()
            for bit in rng.integers(0, 256, rng.integers(0, 30)):
                d[bit >> 3] ^= np.uint8(1 << (bit & 7))
            kf_desc[k][f] = d
        if p % 9 == 0 and N >= 3:
            for e in range(1, N, 2):
                kf_desc[kfs[e]][feats[e]] = kf_desc[kfs[0]][feats[0]]          # ties
        obs.append([(int(k), int(f)) for k, f in zip(kfs, feats)]); ref.append(int(rng.integers(0, N)))
        Pw.append(rng.normal(0, 4, 3).astype(np.float32) + np.float32([0, 0, 9]))
    return obs, ref, np.array(Pw, np.float32), kf_desc, kf_oct, kf_Ow


@pytest.mark.parametrize("npts,device", [(300, False), (4000, True)])
def test_map_point_update_equals_the_restatement(npts, device):
    need_gpu()
    obs, ref, Pw, kf_desc, kf_oct, kf_Ow = _points_problem(77 + npts, npts)
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    cam = dict(intr4=[458.0, 457.0, 367.0, 248.0], mb=0.11, mbf=50.0, scale_factor=1.2, sf=sf, level_sigma2=sf * sf)
    pd, bo, pf = viorb_amd.MapPointUpdate(cam, obs, ref, Pw, kf_desc, kf_oct, kf_Ow, device=device)
    counts = np.array([len(o) for o in obs])
    assert (counts > 64).sum() >= 3 and (counts == 1).any()
    for p in range(npts):
        wd, wb, wf = mr.map_point_update([o[0] for o in obs[p]], [o[1] for o in obs[p]], ref[p], Pw[p], kf_desc, kf_oct, kf_Ow, sf)
        assert bo[p] == wb and (pd[p] == wd).all(), (p, counts[p], bo[p], wb)
        assert pf[p].tobytes() == wf.tobytes(), (p, pf[p], wf)


def _run_ref(p, oracle, mono, j_list=None, hp1=None):
    return mr.create_new_map_points(p, oracle_search(oracle, p["cam"]), mono, j_list=j_list, has_point1=hp1)


def _compare_stream(got, ref, p, tally):
    """new_idx (order included), descriptors, positions and the final has_point1, leaving out the i1 whose pair lay in the band."""
    unc = ref["uncertain_i1"]
    kg = np.array([i not in unc for i in got["new_idx"][:, 0]], bool); kr = np.array([i not in unc for i in ref["new_idx"][:, 0]], bool)
    np.testing.assert_array_equal(got["new_idx"][kg], ref["new_idx"][kr])
    if not unc:
        assert got["n_new"] == len(ref["new_idx"])
    assert abs(got["n_new"] - len(ref["new_idx"])) <= len(unc) * len(p["neigh"])
    np.testing.assert_array_equal(got["new_desc"][kg], ref["desc"][kr])
    if kg.any():
        P64 = ref["Pw64"][kr]
        dev = np.linalg.norm(got["new_pts_f"][kg, :3] - P64, axis=1) / np.linalg.norm(P64, axis=1)
        assert dev.max() <= POS_TOL_GPU
        tally["pos"] = max(tally["pos"], float(dev.max()))
        np.testing.assert_allclose(got["new_pts_f"][kg, 3:], ref["pts_f"][kr, 3:], rtol=2e-6, atol=2e-6)
    hp_keep = np.ones(len(ref["has_point1"]), bool); hp_keep[list(unc)] = False
    np.testing.assert_array_equal(got["has_point1"][hp_keep], ref["has_point1"][hp_keep])
    npairs = sum(len(x[1]["idx1"]) for x in ref["per_neighbour"] if x is not None)
    tally["pairs"] += npairs; tally["band"] += sum(int(mr.in_band(x[1]).sum()) for x in ref["per_neighbour"] if x is not None)


@pytest.mark.parametrize("batch,sfrac", [(1, 0.0), (5, 0.0), (5, 0.4)])
def test_create_new_map_points_equals_the_sequential_loop(batch, sfrac, oracle):
    need_gpu()
    J, mono = 20, sfrac == 0.0
    n_neigh = [20, 13, 0, 7, 20][:batch]
    probs = []
    for b in range(batch):
        p = make_mapping_problem(10 + b, J=J, stereo_frac=sfrac)
        p["neigh"] = p["neigh"][:n_neigh[b]] if b != 3 else p["neigh"][6:13]
        probs.append(p)
    cam = probs[0]["cam"]
    run = viorb_amd.CreateNewMapPoints(cam, probs, J, pcap=1000, monocular=mono)
    got = run().results()
    tally = dict(pos=0.0, pairs=0, band=0)
    refs = [_run_ref(p, oracle, mono) for p in probs]
    for b in range(batch):
        assert got[b]["status"] == 0
        _compare_stream(got[b], refs[b], probs[b], tally)
    assert len(refs[0]["new_idx"]) > 200 and len(np.unique(refs[0]["new_idx"][:, 1])) >= 10
    if batch > 2:
        assert got[2]["n_new"] == 0 and (got[2]["has_point1"] == probs[2]["kf1"]["hp"]).all()
    print("batch", batch, "stereo", sfrac, "n_new", [g["n_new"] for g in got], tally)
    assert tally["band"] <= MAX_BAND_SHARE * max(tally["pairs"], 1)

    # chunked calls equal the single call, bit for bit: 0..2 then 3..5 against 0..5, and 0..7 then 7..20 against the run above
    def chunks(cuts):
        r = viorb_amd.CreateNewMapPoints(cam, probs, J, pcap=1000, monocular=mono)
        for a, b_ in zip(cuts[:-1], cuts[1:]):
            r(a, b_)
        return r.results()
    for cuts, whole in (((0, 3, 6), chunks((0, 6))), ((0, 7, 20), got)):
        part = chunks(cuts)
        for b in range(batch):
            assert part[b]["n_new"] == whole[b]["n_new"] and part[b]["status"] == whole[b]["status"]
            for k in ("new_idx", "new_pts_f", "new_desc", "has_point1"):
                assert part[b][k].tobytes() == whole[b][k].tobytes(), (cuts, b, k)

    # a pcap one short of the need: VIORB_ERR_CAPACITY for that stream only, its first pcap points, nothing beyond
    need = [g["n_new"] for g in got]
    bmax = int(np.argmax(need))
    assert sorted(need)[-1] > (sorted(need)[-2] if batch > 1 else 0)
    short = viorb_amd.CreateNewMapPoints(cam, probs, J, pcap=need[bmax] - 1, monocular=mono)().results()
    for b in range(batch):
        if b == bmax:
            assert short[b]["status"] == capi.ERR_CAPACITY and short[b]["n_new"] == need[b] - 1
            for k, key in (("new_idx", "new_idx"), ("new_pts_f", "new_pts_f"), ("new_desc", "new_desc")):
                assert short[b][k].tobytes() == got[b][key][:need[b] - 1].tobytes()
        else:
            assert short[b]["status"] == 0 and short[b]["n_new"] == need[b]
            for k in ("new_idx", "new_pts_f", "new_desc", "has_point1"):
                assert short[b][k].tobytes() == got[b][k].tobytes()

    # the host-buffer drop-in equals stream 0 of the device form
    h = viorb_amd.CreateNewMapPointsHost(cam, probs[0], 1000, monocular=mono)
    assert h["status"] == 0 and h["n_new"] == got[0]["n_new"]
    for k in ("new_idx", "new_pts_f", "new_desc", "has_point1"):
        assert h[k].tobytes() == got[0][k].tobytes(), k
    h = viorb_amd.CreateNewMapPointsHost(cam, probs[0], need[0] - 1, monocular=mono)
    assert h["status"] == capi.ERR_CAPACITY and h["n_new"] == need[0] - 1


def test_created_points_feed_fuse(oracle):
    """Closing the loop: new_pts_f / new_desc exactly as the call produced them go into the existing Fuse for a third key frame; the
    result equals the CPU oracle's Fuse fed with the restatement's points (the layout is the one Fuse reads, not just the values)."""
    need_gpu()
    p = make_mapping_problem(21, J=20)
    cam = p["cam"]
    got = viorb_amd.CreateNewMapPoints(cam, [p], 20, pcap=1000, monocular=True)().results()[0]
    ref = _run_ref(p, oracle, True)
    assert got["n_new"] > 200
    intr5 = np.concatenate([cam["intr4"], [cam["mbf"]]]).astype(np.float32)
    fused_any = 0
    for third in (p["neigh"][19], p["neigh"][10]):
        valid = np.ones(got["n_new"], np.uint8)
        n_g, bi_g = viorb_amd.Fuse(third["kps"], third["desc"], third["ur"], p["bounds"], third["pose12"], intr5, cam["sf"], cam["inv_level_sigma2"],
                                   got["new_pts_f"], valid, got["new_desc"], th=3.0)
        n_r, bi_r = oracle.fuse(third["kps"], third["desc"], third["ur"], p["bounds"], third["pose12"], intr5, cam["sf"], cam["inv_level_sigma2"],
                                float(np.log(np.float32(1.2))), ref["pts_f"], np.ones(len(ref["pts_f"]), np.uint8), ref["desc"], th=3.0)
        unc = ref["uncertain_i1"]
        kg = np.array([i not in unc for i in got["new_idx"][:, 0]], bool); kr = np.array([i not in unc for i in ref["new_idx"][:, 0]], bool)
        np.testing.assert_array_equal(bi_g[kg], bi_r[kr])
        fused_any += int((bi_g >= 0).sum())
    assert fused_any > 50
