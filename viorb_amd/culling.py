"""LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:1665-1824) and LocalMapping::MapPointCulling (:1198-1233) through the C ABI
of include/viorb_culling.h. A stream's snapshot is a `scene`: a dict of numpy arrays with stream-local offsets and indices,
    kf_flags u8 [nk], kf_time f64 [nk], kf_prev / kf_next i32 [nk], cur, vins_inited, th_depth,
    cand_kf i32 [nc], kp_start i32 [nc+1], kp_point i32 / kp_octave u8 / kp_depth f32 [n keypoints],
    pt_nobs i32 [np], pt_bad u8 [np], obs_start i32 [np+1], obs u32 [n observations] (obs_word),
which scene_from_lists builds from Python lists; pack() lays a list of scenes out as the flat arrays of viorb_cull_map. Results come back
as one dict per stream, cut to the stream's ranges. The host hook (no device) is key_frame_culling_host_core."""
import ctypes as C
import numpy as np
from . import capi, snapshot as S
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
    s["kp_start"], s["kp_point"] = S.csr([c[1] for c in cands], np.int32, lambda k: k[0])
    kps = [k for c in cands for k in c[1]]
    s["kp_octave"] = np.array([k[1] for k in kps], np.uint8)
    s["kp_depth"] = np.array([k[2] for k in kps], np.float32)
    s["pt_nobs"] = np.array([p["nobs"] if p.get("nobs") is not None else sum(2 if o[2] else 1 for o in p["obs"]) for p in pts], np.int32)
    s["pt_bad"] = np.array([1 if p.get("bad") else 0 for p in pts], np.uint8)
    s["obs_start"], s["obs"] = S.csr([p["obs"] for p in pts], np.uint32, lambda o: obs_word(*o))
    return s


def pack(scenes):
    """The flat arrays of viorb_cull_map for a list of scenes (every array at least one element long), with the totals."""
    cnt = lambda f: sum(len(s[f]) for s in scenes)
    P = dict(batch=len(scenes), n_kf=cnt("kf_flags"), n_cand=cnt("cand_kf"), n_kp=cnt("kp_point"), n_pt=cnt("pt_nobs"), n_obs=cnt("obs"))
    for f, src in (("kf_start", "kf_flags"), ("cand_start", "cand_kf"), ("pt_start", "pt_nobs")):
        P[f] = S.starts([s[src] for s in scenes])
    for f in ("kf_flags", "kf_time", "kf_prev", "kf_next", "cand_kf", "kp_point", "kp_octave", "kp_depth", "pt_nobs", "pt_bad", "obs"):
        P[f] = S.cat(scenes, f, _DT[f])
    P["kp_start"], P["obs_start"] = S.rebase(scenes, "kp_start", "kp_point"), S.rebase(scenes, "obs_start", "obs")
    P["cur_kf"] = np.array([s["cur"] for s in scenes], np.int32)
    P["vins_inited"] = np.array([1 if s["vins_inited"] else 0 for s in scenes], np.uint8)
    P["th_depth"] = np.array([s["th_depth"] for s in scenes], np.float32)
    return S.finish(P, capi.CULL_MAP_ARRAYS, _DT)


def _map_struct(P, arrays=None):
    return S.struct(capi.CullMap, capi.CULL_MAP_INTS, capi.CULL_MAP_ARRAYS, P, arrays)


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


def _run_host(fn, P, monocular):
    """The flat result arrays one call of a host entry leaves."""
    o = S.outputs(capi.CULL_RESULT_FIELDS, lambda f: max(P[_OUT_LEN[f]], 1), _OUT_DT.get)
    m, r = _map_struct(P), S.struct(capi.CullResult, (), capi.CULL_RESULT_FIELDS, o)
    check(fn(C.byref(m), int(bool(monocular)), C.byref(r)))
    return o


def key_frame_culling(scenes, monocular, packed=None):
    """viorb_key_frame_culling (host buffers): one result dict per scene."""
    P = packed or pack(scenes)
    return split(P, _run_host(lib().viorb_key_frame_culling, P, monocular))


def key_frame_culling_host_core(scenes, monocular, packed=None):
    """viorb_debug_key_frame_culling_host: culling_core.h on the host (no device), the phases of the device form on one thread."""
    P = packed or pack(scenes)
    return split(P, _run_host(lib().viorb_debug_key_frame_culling_host, P, monocular))


class CullBatch:
    """A packed batch of scenes on the device: run() enqueues viorb_key_frame_culling_device on torch tensors; results() downloads."""

    def __init__(self, scenes, monocular, device=0, packed=None):
        import torch
        self.torch, self.dev, self.monocular = torch, torch.device("cuda", device), bool(monocular)
        self.P = P = packed or pack(scenes)
        self.d = S.upload(P, capi.CULL_MAP_ARRAYS, device)
        self.map = _map_struct(P, self.d)
        self.o = S.outputs(capi.CULL_RESULT_FIELDS, lambda f: max(P[_OUT_LEN[f]], 1), _OUT_DT.get, torch, self.dev)
        self.res = S.struct(capi.CullResult, (), capi.CULL_RESULT_FIELDS, self.o)
        self._wb = lib().viorb_key_frame_culling_workspace_bytes(P["batch"], P["n_kf"], P["n_cand"], P["n_pt"], P["n_obs"])
        self.ws = capi.Workspace(torch, self.dev, self._wb)         # may be re-filled or replaced by a larger one between calls

    def run(self, outputs=True):
        check(lib().viorb_key_frame_culling_device(C.byref(self.map), int(self.monocular), C.byref(self.res) if outputs else None, self.ws.ptr, self._wb,
                                                   S.stream_ptr(self.torch, self.dev)))

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
