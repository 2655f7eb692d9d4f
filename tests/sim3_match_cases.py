"""Fixtures shared by tests/test_sim3_match_ref.py (CPU) and tests/test_gpu_sim3_match.py: the synthetic loop of
synth.make_sim3_match_problem and the checker's (tests/sim3_match_ref.py) results on it, computed once."""
import functools
import numpy as np
from viorb_amd import sim3_match as M
from viorb_amd.synth import make_sim3_match_problem
import sim3_match_ref as T

TH_SIM3, TH_PROJ, TH_FUSE = 7.5, 10.0, 4.0          # LoopClosing: SearchBySim3(…, 7.5), SearchByProjection(…, 10), Fuse(…, 4)


@functools.lru_cache(maxsize=None)
def problem(seed=0, duplicates=60, cluster=12, n_kf=3, nlevels=8, n_extra=600, n1=1000, n2=1000, n_common=500, fix_scale=False):
    return make_sim3_match_problem(seed, n1=n1, n2=n2, n_common=n_common, duplicates=duplicates, cluster=cluster, n_kf=n_kf, nlevels=nlevels,
                                   n_extra=n_extra, fix_scale=fix_scale)


def ref_camera(P):
    return T.Camera(P["intr4"], P["bounds4"], P["sf"])


def lib_camera(P):
    return M.camera(P["intr4"], P["sf"])


def ref_keyframe(P, kps, desc):
    return T.KeyFrame(ref_camera(P), kps, desc)


def ref_search_by_sim3(P, side1=None, side2=None, model=None):
    a, b = side1 or P["kf1"], side2 or P["kf2"]
    R12, t12, s12 = model or (P["R12"], P["t12"], P["s12"])
    return T.search_by_sim3(ref_keyframe(P, a["kps"], a["desc"]), a["pose12"], a["has_point"], a["pts_f"], a["pts_desc"], a["already"],
                            ref_keyframe(P, b["kps"], b["desc"]), b["pose12"], b["has_point"], b["pts_f"], b["pts_desc"], b["already"], R12, t12, s12, TH_SIM3)


@functools.lru_cache(maxsize=None)
def expected_sim3(*key):
    return ref_search_by_sim3(problem(*key))


@functools.lru_cache(maxsize=None)
def expected_projection(ordered=True, *key):
    P = problem(*key)
    L = P["loop"]
    return T.search_by_projection(ref_keyframe(P, P["kf1"]["kps"], P["kf1"]["desc"]), L["Scw"], L["pts_f"], L["pts_desc"], L["valid"], L["feat_taken"],
                                  TH_PROJ, ordered)


@functools.lru_cache(maxsize=None)
def expected_fuse(*key):
    P = problem(*key)
    L, F = P["loop"], P["fuse"]
    return [T.fuse(ref_keyframe(P, k, d), F["Scw"][b], L["pts_f"], L["pts_desc"], F["valid"][b], TH_FUSE) for b, (k, d) in enumerate(F["frames"])]


def same(got, want, keys):
    """np.array_equal over the named entries, with the entry that differs in the message."""
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
