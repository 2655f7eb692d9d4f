"""Relocalisation after the PnP hypothesis (Tracking::Relocalization, reference src/Tracking.cc:2209-2273), through the C ABI of
include/viorb_relocalization.h: the key-frame projection matcher ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th,
ORBdist) (src/ORBmatcher.cc:1473-1600) and the solve / search / solve cascade. A lost frame is (kps [n] of capi.KP_DTYPE, desc [n,32]); a
hypothesis is a dict(pose12 [12], kf_angle [k], kf_valid [k], pts_f [k,8], pts_desc [k,32]) indexed by the candidate key frame's feature,
plus kf_found [k] and feat_taken [n] for the matcher, or bow_match [n] and inlier [n] for the cascade, plus frame (the index of its lost
frame, default: its own position). The camera is sim3_match.camera(intr4, scale_factors). The host hooks (no device) are the debug_*
functions at the end."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as _up
from .sim3_match import Sim3MatchBatch, camera, MAX_FEATURES  # noqa: F401

MATCHED, NOT_CANDIDATE, BEHIND, OUT_OF_IMAGE, OUT_OF_RANGE, VIEW_ANGLE, NO_FEATURE_IN_WINDOW, ABOVE_THRESHOLD, NOT_MUTUAL, ROTATION = range(10)
RUNNING, FEW_INLIERS, ACCEPTED_FIRST, COARSE_SHORT, SECOND_WEAK, ACCEPTED_SECOND, NARROW_SHORT, THIRD_REJECTED, ACCEPTED_THIRD = range(9)
STAGE_NAMES = ("RUNNING", "FEW_INLIERS", "ACCEPTED_FIRST", "COARSE_SHORT", "SECOND_WEAK", "ACCEPTED_SECOND", "NARROW_SHORT", "THIRD_REJECTED",
               "ACCEPTED_THIRD")

_f32 = lambda a: np.ascontiguousarray(a, np.float32)
_i32 = lambda a: np.ascontiguousarray(a, np.int32)
_u8 = lambda a: np.ascontiguousarray(a, np.uint8)
_kp = lambda a: np.ascontiguousarray(a, capi.KP_DTYPE)


def shape():
    """(points per workgroup, wavefront size, candidates per list) of the built kernels."""
    o = np.zeros(3, np.int32)
    check(lib().viorb_relocalization_shape(ptr(o)))
    return tuple(int(v) for v in o)


def default_config(**over):
    """viorb_reloc_config with the reference's constants; keyword arguments replace fields."""
    c = capi.RelocConfig()
    check(lib().viorb_reloc_config_default(C.byref(c)))
    for k, v in over.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


def search_by_projection_reloc(kps, desc, pose12, kf_angle, kf_valid, kf_found, pts_f, pts_desc, feat_taken, cam, bounds4, th=10.0, orb_dist=100,
                               check_orientation=True):
    """viorb_search_by_projection_reloc (host buffers, one hypothesis): dict(best_idx [npts], nmatches, reason [npts])."""
    k, pf = _kp(kps), _f32(pts_f).reshape(-1, 8)
    bi, re, nm = np.full(len(pf), -1, np.int32), np.zeros(len(pf), np.int32), C.c_int32(0)
    check(lib().viorb_search_by_projection_reloc(ptr(k), ptr(_u8(desc)), len(k), ptr(_f32(pose12)), ptr(_f32(kf_angle)), ptr(_u8(kf_valid)), ptr(_u8(kf_found)),
                                                 ptr(pf), ptr(_u8(pts_desc)), len(pf), ptr(_u8(feat_taken)), C.byref(cam), ptr(_f32(bounds4)), float(th),
                                                 int(orb_dist), int(bool(check_orientation)), ptr(bi), C.byref(nm), ptr(re)))
    return dict(best_idx=bi, nmatches=nm.value, reason=re)


class RelocBatch:
    """Lost frames on the device (uploaded once, grids built by viorb_keyframe_grid_device) and the device entries on torch tensors.
    frames: a list of (kps, desc); cap: the capacity of the per-frame arrays (default: the largest count)."""

    def __init__(self, frames, cam, bounds4, cap=None, device=0, uright=None):
        self.fr = Sim3MatchBatch(frames, cam, bounds4, cap=cap, device=device)
        self.torch, self.dev, self.device = self.fr.torch, self.fr.dev, device
        self.cam, self.bounds, self.cap, self.n = cam, self.fr.bounds, self.fr.cap, self.fr.n
        self.uright = None
        if uright is not None:
            u = np.full((len(frames), self.cap), -1.0, np.float32)
            for b, r in enumerate(uright):
                u[b, :len(r)] = _f32(r)
            self.uright = _up(u, device)
        self.ws = None                                              # a capi.Workspace once a call needed one; a test may put its own here

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _workspace(self, wb):
        self.ws_bytes = wb                                          # what the last call was handed
        if self.ws is None or not self.ws.fits(wb):
            self.ws = capi.Workspace(self.torch, self.dev, wb)
        return self.ws.ptr, wb

    def _pad(self, rows, cap, tail, dtype, fill=0):
        a = np.full((len(rows), cap) + tail, fill, dtype)
        for b, r in enumerate(rows):
            r = np.asarray(r, dtype).reshape((-1,) + tail)
            a[b, :len(r)] = r
        return _up(a, self.device)

    def _common(self, hyps, kcap, share):
        B = len(hyps)
        npts = [len(_f32(h["pts_f"]).reshape(-1, 8)) for h in hyps]
        kcap = int(kcap or max(max(npts), 1))
        hf = _up(_i32([h.get("frame", b) for b, h in enumerate(hyps)]), self.device) if share else None
        d = dict(pose12=_up(_f32(np.stack([_f32(h["pose12"]) for h in hyps])), self.device), kf_angle=self._pad([h["kf_angle"] for h in hyps], kcap, (), np.float32),
                 kf_valid=self._pad([h["kf_valid"] for h in hyps], kcap, (), np.uint8), pts_f=self._pad([h["pts_f"] for h in hyps], kcap, (8,), np.float32),
                 pts_desc=self._pad([h["pts_desc"] for h in hyps], kcap, (32,), np.uint8), kf_count=_up(_i32(npts), self.device))
        return B, npts, kcap, hf, d

    def search_call(self, hyps, th=10.0, orb_dist=100, check_orientation=True, kcap=None, share=True, with_reason=True):
        """The inputs of viorb_search_by_projection_reloc_device uploaded once: (call, fetch). call() launches on the current stream and
        does not synchronise; fetch() synchronises and returns one dict(best_idx, nmatches, reason, tail) per hypothesis."""
        t = self.torch
        B, npts, kcap, hf, d = self._common(hyps, kcap, share)
        kf_found = self._pad([h["kf_found"] for h in hyps], kcap, (), np.uint8)
        taken = self._pad([h["feat_taken"] for h in hyps], self.cap, (), np.uint8)
        bi = t.zeros((B, kcap), dtype=t.int32, device=self.dev)
        re = t.zeros((B, kcap), dtype=t.int32, device=self.dev) if with_reason else None
        nm = t.zeros(B, dtype=t.int32, device=self.dev)
        ws, wb = self._workspace(lib().viorb_relocalization_workspace_bytes(self.cap, kcap, B))
        buf = self.ws.tensor                                        # the closures keep the workspace and the uploads alive

        def call():
            check(lib().viorb_search_by_projection_reloc_device(C.byref(self.fr.kf), self.fr.B, ptr(hf), ptr(d["pose12"]), ptr(d["kf_angle"]), ptr(d["kf_valid"]),
                                                                ptr(kf_found), ptr(d["pts_f"]), ptr(d["pts_desc"]), ptr(d["kf_count"]), kcap, ptr(taken),
                                                                C.byref(self.cam), ptr(self.bounds), float(th), int(orb_dist), int(bool(check_orientation)), B,
                                                                ptr(bi), ptr(nm), ptr(re), ws, wb, self._stream()))

        def fetch():
            t.cuda.synchronize(self.dev)
            b_, n_, r_ = bi.cpu().numpy(), nm.cpu().numpy(), None if re is None else re.cpu().numpy()
            return [dict(best_idx=b_[b, :npts[b]], nmatches=int(n_[b]), reason=None if r_ is None else r_[b, :npts[b]], tail=b_[b, npts[b]:], workspace=buf)
                    for b in range(B)]
        return call, fetch

    def search(self, hyps, **kw):
        """viorb_search_by_projection_reloc_device: one dict(best_idx, nmatches, reason, tail) per hypothesis. share=False passes
        hyp_frame = NULL (hypothesis b uses frame b)."""
        call, fetch = self.search_call(hyps, **kw)
        call()
        return fetch()

    def refine_call(self, frontend, hyps, bf=0.0, config=None, kcap=None, share=True):
        """The inputs of viorb_relocalization_refine_device uploaded once: (call, fetch), as search_call."""
        t = self.torch
        B, npts, kcap, hf, d = self._common(hyps, kcap, share)
        cfg = config or default_config()
        bow = self._pad([h["bow_match"] for h in hyps], self.cap, (), np.int32, fill=-1)
        inl = self._pad([h["inlier"] for h in hyps], self.cap, (), np.uint8)
        hcap = C.c_int32(0)
        check(lib().viorb_frontend_capacity(frontend.h, None, C.byref(hcap)))
        I = capi.RelocInputs(C.pointer(self.fr.kf), self.fr.B, ptr(hf), ptr(self.uright), ptr(d["pose12"]), ptr(d["kf_angle"]), ptr(d["kf_valid"]), ptr(d["pts_f"]),
                             ptr(d["pts_desc"]), ptr(d["kf_count"]), kcap, ptr(bow), ptr(inl))
        z = lambda shape, dt: t.zeros(shape, dtype=dt, device=self.dev)
        o = dict(accepted=z(B, t.int32), n_good=z(B, t.int32), stage=z(B, t.int32), counts=z((B, 8), t.int32), out_pose12=z((B, 12), t.float32),
                 chi2=z(B, t.float64), frame_match=z((B, self.cap), t.int32), outlier=z((B, self.cap), t.uint8))
        O = capi.RelocOutputs(**{k: ptr(o[k]) for k in capi.RELOC_OUTPUT_FIELDS})
        ws, wb = self._workspace(lib().viorb_relocalization_refine_workspace_bytes(self.cap, kcap, hcap.value, B))
        buf = self.ws.tensor

        def call():
            check(lib().viorb_relocalization_refine_device(frontend.h, C.byref(I), C.byref(cfg), C.byref(self.cam), ptr(self.bounds), float(bf), B, C.byref(O), ws, wb,
                                                           self._stream()))

        def fetch():
            t.cuda.synchronize(self.dev)
            h_ = {k: v.cpu().numpy() for k, v in o.items()}
            out = []
            for b, h in enumerate(hyps):
                n = self.n[h.get("frame", b) if share else b]
                out.append(dict(accepted=int(h_["accepted"][b]), n_good=int(h_["n_good"][b]), stage=int(h_["stage"][b]), counts=h_["counts"][b], pose12=h_["out_pose12"][b],
                                chi2=float(h_["chi2"][b]), frame_match=h_["frame_match"][b, :n], outlier=h_["outlier"][b, :n], workspace=buf))
            return out
        return call, fetch

    def refine(self, frontend, hyps, **kw):
        """viorb_relocalization_refine_device on the front-end handle `frontend` (viorb_amd.frontend.Frontend: its intrinsics, max_batch >=
        len(hyps), cap >= this batch's cap). One dict(accepted, n_good, stage, counts [8], pose12, chi2, frame_match [n], outlier [n]) per
        hypothesis."""
        call, fetch = self.refine_call(frontend, hyps, **kw)
        call()
        return fetch()


# ---- host hooks (reloc_core.h compiled for the host) -------------------------------------------------------------------------------------
def debug_project(pose12, pt8, cam, bounds4, th):
    """One point through the gates: dict(u, v, dist3D, radius, level, rect, reason)."""
    o4, o6 = np.zeros(4, np.float32), np.zeros(6, np.int32)
    check(lib().viorb_debug_reloc_project(ptr(_f32(pose12)), ptr(_f32(pt8)), C.byref(cam), ptr(_f32(bounds4)), float(th), ptr(o4), ptr(o6)))
    return dict(u=o4[0], v=o4[1], dist3D=o4[2], radius=o4[3], level=int(o6[0]), rect=tuple(int(v) for v in o6[1:5]), reason=int(o6[5]))


def debug_match(cands, taken_in, angle_kf, angle_f, orb_dist=100, check_orientation=True):
    """The claim loop plus the histogram over candidate lists cands[p] = [(distance, feature), ...]: (best_idx, removed, nmatches)."""
    npts, lcap = len(cands), max([len(c) for c in cands] + [1])
    cand, cn = np.zeros((max(npts, 1), lcap), np.uint32), np.zeros(max(npts, 1), np.int32)
    for p, lst in enumerate(cands):
        cn[p] = len(lst)
        for k, (d, idx) in enumerate(lst):
            cand[p, k] = (int(d) << 16) | int(idx)
    tk, ak, af = _u8(taken_in), _f32(np.concatenate([_f32(angle_kf), [0]])), _f32(np.concatenate([_f32(angle_f), [0]]))
    bi, rm, nm = np.full(max(npts, 1), -1, np.int32), np.zeros(max(npts, 1), np.uint8), C.c_int32(0)
    check(lib().viorb_debug_reloc_match(ptr(cand), ptr(cn), npts, lcap, ptr(tk), len(tk), int(orb_dist), int(bool(check_orientation)), ptr(ak), ptr(af),
                                        ptr(bi), ptr(rm), C.byref(nm)))
    return bi[:npts], rm[:npts], nm.value


def debug_decide(cfg, step, n_good, n_additional=0):
    """The cascade's decision after `step` (1 first solve, 2 coarse search, 3 second solve, 4 narrow search, 5 third solve)."""
    return lib().viorb_debug_reloc_decide(C.byref(cfg), int(step), int(n_good), int(n_additional))
