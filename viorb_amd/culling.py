"""LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:1665-1824) and LocalMapping::MapPointCulling (:1198-1233) through the C ABI
of include/viorb_culling.h. A stream's snapshot is a `scene`: a dict of numpy arrays with stream-local offsets and indices,
    kf_flags u8 [nk], kf_time f64 [nk], kf_prev / kf_next i32 [nk], cur, vins_inited, th_depth,
    cand_kf i32 [nc], kp_start i32 [nc+1], kp_point i32 / kp_octave u8 / kp_depth f32 [n keypoints],
    pt_nobs i32 [np], pt_bad u8 [np], obs_start i32 [np+1], obs u32 [n observations] (obs_word),
which scene_from_lists builds from Python lists; pack() lays a list of scenes out as the flat arrays of viorb_cull_map. Results come back
as one dict per stream, cut to the stream's ranges. The host hook (no device) is key_frame_culling_host_core."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr, _torch_up as _up

FIRST_KF, TIME_GAP, BEFORE_CURRENT, RECENT, KEPT, CULLED, DEFERRED = range(7)
REASON_NAMES = ("FIRST_KF", "TIME_GAP", "BEFORE_CURRENT", "RECENT", "KEPT", "CULLED", "DEFERRED")
MPC_KEEP, MPC_DROP_BAD, MPC_CULL_FOUND_RATIO, MPC_CULL_FEW_OBS, MPC_RETIRE = range(5)
MPC_NAMES = ("KEEP", "DROP_BAD", "CULL_FOUND_RATIO", "CULL_FEW_OBS", "RETIRE")
KF_FIRST, KF_NOT_ERASE = 1, 2
MAX_KF = 65535

_DT = dict(kf_start=np.int32, kf_flags=np.uint8, kf_time=np.float64, kf_prev=np.int32, kf_next=np.int32, cur_kf=np.int32, vins_inited=np.uint8,
           th_depth=np.float32, cand_start=np.int32, cand_kf=np.int32, kp_start=np.int32, kp_point=np.int32, kp_octave=np.uint8, kp_depth=np.float32,
           pt_start=np.int32, pt_nobs=np.int32, pt_bad=np.uint8, obs_start=np.int32, obs=np.uint32)
_OUT_DT = dict(cand_reason=np.int32, cand_redundant=np.int32, cand_mps=np.int32, cand_recounted=np.int32, culled_order=np.int32, n_culled=np.int32,
               status=np.int32, kf_bad=np.uint8, kf_to_be_erased=np.uint8, kf_prev_out=np.int32, kf_next_out=np.int32, kf_repreint=np.uint8,
               pt_nobs_out=np.int32, pt_bad_out=np.uint8, obs_alive=np.uint8)
_OUT_LEN = dict(cand_reason="n_cand", cand_redundant="n_cand", cand_mps="n_cand", cand_recounted="n_cand", culled_order="n_cand", n_culled="batch",
                status="batch", kf_bad="n_kf", kf_to_be_erased="n_kf", kf_prev_out="n_kf", kf_next_out="n_kf", kf_repreint="n_kf", pt_nobs_out="n_pt",
                pt_bad_out="n_pt", obs_alive="n_obs")


def obs_word(slot, octave, stereo=False):
    """One observation: the observing key frame's slot, the octave of its keypoint, mvuRight >= 0."""
    return (int(slot) & 0xffff) | ((int(octave) & 0xff) << 16) | ((1 << 24) if stereo else 0)


def shape():
    """(threads of the ordered phase, keypoints per workgroup and pass of the count, wavefront size, shared observation chunk)."""
    o = np.zeros(4, np.int32)
    check(lib().viorb_key_frame_culling_shape(ptr(o)))
    return tuple(int(v) for v in o)


def scene_from_lists(kfs, cur, cands, pts, vins_inited=False, th_depth=40.0):
    """kfs: [dict(t=, prev=-1, next=-1, first=False, not_erase=False)]; cands: [(slot, [(point or -1, octave, depth)])] in the reference's
    order; pts: [dict(obs=[(slot, octave, stereo)], nobs=None (the weighted count of obs), bad=False)]."""
    s = dict(cur=int(cur), vins_inited=bool(vins_inited), th_depth=float(th_depth))
    s["kf_flags"] = np.array([(KF_FIRST if k.get("first") else 0) | (KF_NOT_ERASE if k.get("not_erase") else 0) for k in kfs], np.uint8)
    s["kf_time"] = np.array([k["t"] for k in kfs], np.float64)
    s["kf_prev"] = np.array([k.get("prev", -1) for k in kfs], np.int32)
    s["kf_next"] = np.array([k.get("next", -1) for k in kfs], np.int32)
    s["cand_kf"] = np.array([c[0] for c in cands], np.int32)
    s["kp_start"] = np.concatenate([[0], np.cumsum([len(c[1]) for c in cands])]).astype(np.int32)
    kps = [k for c in cands for k in c[1]]
    s["kp_point"] = np.array([k[0] for k in kps], np.int32)
    s["kp_octave"] = np.array([k[1] for k in kps], np.uint8)
    s["kp_depth"] = np.array([k[2] for k in kps], np.float32)
    s["pt_nobs"] = np.array([p["nobs"] if p.get("nobs") is not None else sum(2 if o[2] else 1 for o in p["obs"]) for p in pts], np.int32)
    s["pt_bad"] = np.array([1 if p.get("bad") else 0 for p in pts], np.uint8)
    s["obs_start"] = np.concatenate([[0], np.cumsum([len(p["obs"]) for p in pts])]).astype(np.int32)
    s["obs"] = np.array([obs_word(*o) for p in pts for o in p["obs"]], np.uint32)
    return s


def pack(scenes):
    """The flat arrays of viorb_cull_map for a list of scenes (every array at least one element long), with the totals."""
    B = len(scenes)
    cnt = lambda f: np.array([len(s[f]) for s in scenes], np.int64)
    start = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    cat = lambda f: np.concatenate([np.asarray(s[f], _DT[f]) for s in scenes]) if B else np.zeros(0, _DT[f])
    P = dict(batch=B, n_kf=int(cnt("kf_flags").sum()), n_cand=int(cnt("cand_kf").sum()), n_kp=int(cnt("kp_point").sum()), n_pt=int(cnt("pt_nobs").sum()),
             n_obs=int(cnt("obs").sum()))
    P["kf_start"], P["cand_start"], P["pt_start"] = start(cnt("kf_flags")), start(cnt("cand_kf")), start(cnt("pt_nobs"))
    for f in ("kf_flags", "kf_time", "kf_prev", "kf_next", "cand_kf", "kp_point", "kp_octave", "kp_depth", "pt_nobs", "pt_bad", "obs"):
        P[f] = cat(f)
    kp0, ob0 = start(cnt("kp_point")), start(cnt("obs"))
    P["kp_start"] = np.concatenate([np.asarray(s["kp_start"][:-1], np.int32) + kp0[b] for b, s in enumerate(scenes)] + [[P["n_kp"]]]).astype(np.int32)
    P["obs_start"] = np.concatenate([np.asarray(s["obs_start"][:-1], np.int32) + ob0[b] for b, s in enumerate(scenes)] + [[P["n_obs"]]]).astype(np.int32)
    P["cur_kf"] = np.array([s["cur"] for s in scenes], np.int32)
    P["vins_inited"] = np.array([1 if s["vins_inited"] else 0 for s in scenes], np.uint8)
    P["th_depth"] = np.array([s["th_depth"] for s in scenes], np.float32)
    for f in capi.CULL_MAP_ARRAYS:
        a = np.ascontiguousarray(P[f], _DT[f])
        P[f] = a if len(a) else np.zeros(1, _DT[f])
    return P


def _map_struct(P, arrays=None):
    arrays = arrays or P
    return capi.CullMap(*([P[f] for f in capi.CULL_MAP_INTS] + [ptr(arrays[f]) for f in capi.CULL_MAP_ARRAYS]))


def _host_outputs(P):
    return {f: np.full(max(P[_OUT_LEN[f]], 1), 77, _OUT_DT[f]) for f in capi.CULL_RESULT_FIELDS}


def split(P, o):
    """One dict per stream from flat result arrays: the fields of viorb_cull_result cut to the stream's ranges; culled_order cut to
    n_culled, its tail in culled_tail. A refused stream (status != 0) has only status and n_culled."""
    res = []
    for b in range(P["batch"]):
        r = dict(status=int(o["status"][b]), n_culled=int(o["n_culled"][b]))
        if r["status"] == 0:
            k0, k1, c0, c1, p0, p1 = P["kf_start"][b], P["kf_start"][b + 1], P["cand_start"][b], P["cand_start"][b + 1], P["pt_start"][b], P["pt_start"][b + 1]
            o0, o1 = P["obs_start"][p0], P["obs_start"][p1]
            for f in ("cand_reason", "cand_redundant", "cand_mps", "cand_recounted"):
                r[f] = o[f][c0:c1]
            r["culled_order"], r["culled_tail"] = o["culled_order"][c0:c0 + r["n_culled"]], o["culled_order"][c0 + r["n_culled"]:c1]
            for f in ("kf_bad", "kf_to_be_erased", "kf_prev_out", "kf_next_out", "kf_repreint"):
                r[f] = o[f][k0:k1]
            r["pt_nobs_out"], r["pt_bad_out"], r["obs_alive"] = o["pt_nobs_out"][p0:p1], o["pt_bad_out"][p0:p1], o["obs_alive"][o0:o1]
        res.append(r)
    return res


def _run_host(fn, scenes, monocular, packed):
    P = packed or pack(scenes)
    o = _host_outputs(P)
    m, r = _map_struct(P), capi.CullResult(*[ptr(o[f]) for f in capi.CULL_RESULT_FIELDS])
    check(fn(C.byref(m), int(bool(monocular)), C.byref(r)))
    return split(P, o)


def key_frame_culling(scenes, monocular, packed=None):
    """viorb_key_frame_culling (host buffers): one result dict per scene."""
    return _run_host(lib().viorb_key_frame_culling, scenes, monocular, packed)


def key_frame_culling_host_core(scenes, monocular, packed=None):
    """viorb_debug_key_frame_culling_host: culling_core.h on the host (no device), the phases of the device form on one thread."""
    return _run_host(lib().viorb_debug_key_frame_culling_host, scenes, monocular, packed)


class CullBatch:
    """A packed batch of scenes on the device: run() enqueues viorb_key_frame_culling_device on torch tensors; results() downloads."""

    def __init__(self, scenes, monocular, device=0, packed=None):
        import torch
        self.torch, self.dev, self.monocular = torch, torch.device("cuda", device), bool(monocular)
        self.P = packed or pack(scenes)
        self.d = {f: _up(self.P[f].view(np.int32) if self.P[f].dtype == np.uint32 else self.P[f], device) for f in capi.CULL_MAP_ARRAYS}
        self.map = _map_struct(self.P, self.d)
        tdt = {np.int32: torch.int32, np.uint8: torch.uint8}
        self.o = {f: torch.full((max(self.P[_OUT_LEN[f]], 1),), 77, dtype=tdt[_OUT_DT[f]], device=self.dev) for f in capi.CULL_RESULT_FIELDS}
        self.res = capi.CullResult(*[ptr(self.o[f]) for f in capi.CULL_RESULT_FIELDS])
        P = self.P
        self._wb = lib().viorb_key_frame_culling_workspace_bytes(P["batch"], P["n_kf"], P["n_cand"], P["n_pt"], P["n_obs"])
        self._ws = torch.zeros(self._wb + 256, dtype=torch.uint8, device=self.dev)

    def run(self, outputs=True):
        ws = C.c_void_p(self._ws.data_ptr() + (-self._ws.data_ptr()) % 256)
        check(lib().viorb_key_frame_culling_device(C.byref(self.map), int(self.monocular), C.byref(self.res) if outputs else None, ws, self._wb,
                                                   C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)))

    def inputs(self):
        """The snapshot as it lies on the device now."""
        return {f: v.cpu().numpy().view(_DT[f]) for f, v in self.d.items()}

    def results(self):
        self.torch.cuda.synchronize(self.dev)
        return split(self.P, {f: v.cpu().numpy() for f, v in self.o.items()})


def map_point_culling(bad, found, visible, first_kf_id, nobs, cur_kf_id, monocular):
    """viorb_map_point_culling (host buffers, one list): code [n] of MPC_*."""
    a = [np.ascontiguousarray(bad, np.uint8)] + [np.ascontiguousarray(x, np.int32) for x in (found, visible, first_kf_id, nobs)]
    n = len(a[0])
    code = np.full(max(n, 1), 77, np.int32)
    check(lib().viorb_map_point_culling(*[ptr(x) if n else None for x in a], n, int(cur_kf_id), int(bool(monocular)), ptr(code)))
    return code[:n]


def map_point_culling_batch(bad, found, visible, first_kf_id, nobs, count, cur_kf_id, monocular, device=0):
    """viorb_map_point_culling_device over [batch][cap] arrays: code [batch][cap], -1 from count[b] on."""
    import torch
    a = [np.ascontiguousarray(bad, np.uint8)] + [np.ascontiguousarray(x, np.int32) for x in (found, visible, first_kf_id, nobs)]
    B, cap = a[0].shape
    d = [_up(x, device) for x in a] + [_up(np.ascontiguousarray(count, np.int32), device), _up(np.ascontiguousarray(cur_kf_id, np.int32), device)]
    dev = torch.device("cuda", device)
    code = torch.full((B, cap), 77, dtype=torch.int32, device=dev)
    check(lib().viorb_map_point_culling_device(*[ptr(x) for x in d], cap, B, int(bool(monocular)), ptr(code), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    return code.cpu().numpy()


def map_point_code(bad, found, visible, first_kf_id, nobs, cur_kf_id, monocular):
    """viorb_debug_map_point_code (no device): one point."""
    return lib().viorb_debug_map_point_code(int(bool(bad)), int(found), int(visible), int(first_kf_id), int(nobs), int(cur_kf_id), int(bool(monocular)))
