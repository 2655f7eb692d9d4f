"""Tracking::UpdateLocalMap (reference src/Tracking.cc:1960-2125) through the C ABI of include/viorb_local_map.h. A stream's snapshot is a
`scene`: a dict of numpy arrays with stream-local offsets and indices,
    kf_bad u8 [nk], kf_parent / kf_prev / kf_next i32 [nk], covis10 i32 [nk][10], child_start i32 [nk+1], child_kf i32, kf_by_key i32 [nk],
    kp_start i32 [nk+1], kp_point i32, pt_bad u8 [np], obs_start i32 [np+1], obs u32, frame_point i32 [N], prev_lkf i32, prev_ref,
which scene_from_lists builds from Python lists; pack() lays a list of scenes out as the flat arrays of viorb_local_map_snapshot with
the row lengths cap / lcap / pcap. Results come back as one dict per stream. The host hook (no device) is update_local_map_host_core."""
import ctypes as C
import numpy as np
from . import capi, snapshot as S
from .capi import lib, check, ptr

OK, NO_VOTES, OVERFLOW, INVALID = 0, 1, 2, -1
STATUS_NAMES = {OK: "OK", NO_VOTES: "NO_VOTES", OVERFLOW: "OVERFLOW", INVALID: "ERR_INVALID_ARG"}
MAX_KF, LIMIT, COVIS = 65535, 80, 10

_DT = dict(kf_start=np.int32, kf_bad=np.uint8, kf_parent=np.int32, kf_prev=np.int32, kf_next=np.int32, covis10=np.int32, child_start=np.int32,
           child_kf=np.int32, kf_by_key=np.int32, kp_start=np.int32, kp_point=np.int32, pt_start=np.int32, pt_bad=np.uint8, obs_start=np.int32,
           obs=np.uint32, frame_point=np.int32, frame_count=np.int32, prev_lkf=np.int32, prev_n_lkf=np.int32, prev_ref_kf=np.int32)
_ROW = dict(lkf="lcap", lpt="pcap", frame_point_out="cap")             # per-stream rows; the other per-stream fields are scalars


def shape():
    """(threads of the key-frame phase, entries per pass of the point compaction, wavefront size, key frames whose votes fit in LDS)."""
    o = np.zeros(4, np.int32)
    check(lib().viorb_update_local_map_shape(ptr(o)))
    return tuple(int(v) for v in o)


def scene_from_lists(kfs, pts, frame, by_key=None, prev_lkf=(), prev_ref=-1):
    """kfs: [dict(bad=False, parent=-1, prev=-1, next=-1, covis=[slots], children=[slots], pts=[point or -1])]; pts: [dict(obs=[slots],
    bad=False)]; frame: [point or -1]; by_key: the slots in pointer order (default: slot order)."""
    nk = len(kfs)
    s = dict(prev_ref=int(prev_ref), prev_lkf=np.array(list(prev_lkf), np.int32), frame_point=np.array(list(frame), np.int32))
    s["kf_bad"] = np.array([1 if k.get("bad") else 0 for k in kfs], np.uint8)
    for f, key in (("kf_parent", "parent"), ("kf_prev", "prev"), ("kf_next", "next")):
        s[f] = np.array([k.get(key, -1) for k in kfs], np.int32)
    s["covis10"] = np.full((nk, COVIS), -1, np.int32)
    for i, k in enumerate(kfs):
        c = list(k.get("covis", ()))[:COVIS]
        s["covis10"][i, :len(c)] = c
    s["child_start"], s["child_kf"] = S.csr([k.get("children", ()) for k in kfs], np.int32)
    s["kf_by_key"] = np.array(list(by_key) if by_key is not None else list(range(nk)), np.int32)
    s["kp_start"], s["kp_point"] = S.csr([k.get("pts", ()) for k in kfs], np.int32)
    s["pt_bad"] = np.array([1 if p.get("bad") else 0 for p in pts], np.uint8)
    s["obs_start"], s["obs"] = S.csr([p.get("obs", ()) for p in pts], np.uint32)
    return s


def pack(scenes, cap=None, lcap=None, pcap=None):
    """The flat arrays of viorb_local_map_snapshot for a list of scenes (every array at least one element long), with the totals and the
    row lengths. Defaults: cap = the longest frame, lcap = 96 or the most key frames of a stream, pcap = the most points of a stream."""
    B = len(scenes)
    cnt = lambda f: sum(len(s[f]) for s in scenes)
    P = dict(batch=B, n_kf=cnt("kf_bad"), n_child=cnt("child_kf"), n_kp=cnt("kp_point"), n_pt=cnt("pt_bad"), n_obs=cnt("obs"))
    P["cap"] = int(cap or max(1, max(len(s["frame_point"]) for s in scenes)))
    P["lcap"] = int(lcap or max(96, max(len(s["kf_bad"]) for s in scenes)))
    P["pcap"] = int(pcap or max(1, max(len(s["pt_bad"]) for s in scenes)))
    P["kf_start"], P["pt_start"] = S.starts([s["kf_bad"] for s in scenes]), S.starts([s["pt_bad"] for s in scenes])
    for f in ("kf_bad", "kf_parent", "kf_prev", "kf_next", "covis10", "child_kf", "kf_by_key", "kp_point", "pt_bad", "obs"):
        P[f] = S.cat(scenes, f, _DT[f])
    for f, src in (("child_start", "child_kf"), ("kp_start", "kp_point"), ("obs_start", "obs")):
        P[f] = S.rebase(scenes, f, src)
    P["frame_point"] = np.full((B, P["cap"]), -1, np.int32)
    P["prev_lkf"] = np.full((B, P["lcap"]), -1, np.int32)
    for b, s in enumerate(scenes):
        P["frame_point"][b, :len(s["frame_point"])] = s["frame_point"]
        P["prev_lkf"][b, :len(s["prev_lkf"])] = s["prev_lkf"]
    P["frame_count"] = np.array([len(s["frame_point"]) for s in scenes], np.int32)
    P["prev_n_lkf"] = np.array([len(s["prev_lkf"]) for s in scenes], np.int32)
    P["prev_ref_kf"] = np.array([s["prev_ref"] for s in scenes], np.int32)
    return S.finish(P, capi.LOCAL_MAP_ARRAYS, _DT)


def _map_struct(P, arrays=None):
    return S.struct(capi.LocalMapSnapshot, capi.LOCAL_MAP_INTS, capi.LOCAL_MAP_ARRAYS, P, arrays)


def out_len(P, f):
    return P["batch"] * P[_ROW[f]] if f in _ROW else max(P["n_kf"], 1) if f == "kf_votes" else P["batch"]


def split(P, o):
    """One dict per stream from flat result arrays: the fields of viorb_local_map_result cut to the stream; lkf / lpt cut to their counts
    (what fits), their tails in lkf_tail / lpt_tail. A refused stream has only status and `untouched`: whether all its rows still hold the fill value."""
    res = []
    for b in range(P["batch"]):
        r = dict(status=int(o["status"][b]))
        rows = {f: np.asarray(o[f]).reshape(P["batch"], -1)[b] for f in _ROW}
        if r["status"] == INVALID:
            r["untouched"] = all((rows[f] == S.FILL).all() for f in _ROW) and all(int(o[f][b]) == S.FILL for f in ("n_lkf", "n_voted", "ref_kf", "n_lpt"))
        else:
            for f in ("n_lkf", "n_voted", "ref_kf", "n_lpt"):
                r[f] = int(o[f][b])
            r["lkf"], r["lkf_tail"] = rows["lkf"][:r["n_lkf"]], rows["lkf"][r["n_lkf"]:]
            r["lpt"], r["lpt_tail"] = rows["lpt"][:r["n_lpt"]], rows["lpt"][r["n_lpt"]:]
            r["frame_point_out"] = rows["frame_point_out"]
            r["kf_votes"] = np.asarray(o["kf_votes"])[P["kf_start"][b]:P["kf_start"][b + 1]]
        res.append(r)
    return res


def _run_host(fn, scenes, packed, **caps):
    P = packed or pack(scenes, **caps)
    o = S.outputs(capi.LOCAL_MAP_RESULT_FIELDS, lambda f: out_len(P, f), lambda f: np.int32)
    m, r = _map_struct(P), S.struct(capi.LocalMapResult, (), capi.LOCAL_MAP_RESULT_FIELDS, o)
    check(fn(C.byref(m), C.byref(r), P["cap"], P["lcap"], P["pcap"]))
    return split(P, o)


def update_local_map(scenes, packed=None, **caps):
    """viorb_update_local_map (host buffers): one result dict per scene."""
    return _run_host(lib().viorb_update_local_map, scenes, packed, **caps)


def update_local_map_host_core(scenes, packed=None, **caps):
    """viorb_debug_update_local_map_host: local_map_core.h on the host (no device), the phases of the device form on one thread."""
    return _run_host(lib().viorb_debug_update_local_map_host, scenes, packed, **caps)


class LocalMapBatch:
    """A packed batch of scenes on the device: run() enqueues viorb_update_local_map_device on torch tensors; results() downloads;
    gather() enqueues viorb_local_points_gather_device on the result and returns pts_f, pts_desc, pts_count, pts_flags as tensors."""

    def __init__(self, scenes, device=0, packed=None, **caps):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.P = P = packed or pack(scenes, **caps)
        self.d = S.upload(P, capi.LOCAL_MAP_ARRAYS, device)
        self.map = _map_struct(P, self.d)
        self.o = S.outputs(capi.LOCAL_MAP_RESULT_FIELDS, lambda f: out_len(P, f), lambda f: np.int32, torch, self.dev)
        self.res = S.struct(capi.LocalMapResult, (), capi.LOCAL_MAP_RESULT_FIELDS, self.o)
        self._wb = lib().viorb_update_local_map_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"])
        self.ws = capi.Workspace(torch, self.dev, self._wb)         # both may be re-filled or replaced by larger ones between calls
        self._gb = lib().viorb_local_points_gather_workspace_bytes(P["n_pt"])
        self.gather_ws = capi.Workspace(torch, self.dev, self._gb)

    def run(self, outputs=True):
        P = self.P
        check(lib().viorb_update_local_map_device(C.byref(self.map), C.byref(self.res) if outputs else None, P["cap"], P["lcap"], P["pcap"], self.ws.ptr, self._wb,
                                                  S.stream_ptr(self.torch, self.dev)))

    def results(self):
        self.torch.cuda.synchronize(self.dev)
        return split(self.P, {f: v.cpu().numpy() for f, v in self.o.items()})

    def gather(self, map_pts_f, map_pts_desc, pt_nobs, out=None):
        """map_pts_f [n_pt][8] f32, map_pts_desc [n_pt][32] u8, pt_nobs [n_pt] i32: device tensors indexed as the packed points. out: the four
        tensors of an earlier call, to be written again."""
        torch, P = self.torch, self.P
        B, pcap = P["batch"], P["pcap"]
        if out is not None:
            pf, pd, pc, pfl = out
        else:
            pf = torch.full((B, pcap, 8), 7.0, dtype=torch.float32, device=self.dev); pd = torch.full((B, pcap, 32), 7, dtype=torch.uint8, device=self.dev)
            pc = torch.full((B,), 77, dtype=torch.int32, device=self.dev); pfl = torch.full((B, pcap), 77, dtype=torch.uint8, device=self.dev)
        check(lib().viorb_local_points_gather_device(C.byref(self.map), C.byref(self.res), P["cap"], pcap, ptr(map_pts_f), ptr(map_pts_desc), ptr(pt_nobs),
                                                     ptr(pf), ptr(pd), ptr(pc), ptr(pfl), self.gather_ws.ptr, self._gb, S.stream_ptr(self.torch, self.dev)))
        return pf, pd, pc, pfl


def gather_reference(P, results, map_pts_f, map_pts_desc, pt_nobs):
    """The numpy packing viorb_local_points_gather_device must equal: (pts_f [B][pcap][8], pts_desc [B][pcap][32], pts_count [B], pts_flags [B][pcap])
    from the per-stream result dicts."""
    B, pcap = P["batch"], P["pcap"]
    pf, pd = np.zeros((B, pcap, 8), np.float32), np.zeros((B, pcap, 32), np.uint8)
    pc, pfl = np.zeros(B, np.int32), np.zeros((B, pcap), np.uint8)
    for b, r in enumerate(results):
        if r["status"] not in (OK, NO_VOTES):
            continue
        p0, n = int(P["pt_start"][b]), r["n_lpt"]
        g = p0 + np.asarray(r["lpt"], np.int64)
        held = np.zeros(int(P["pt_start"][b + 1]) - p0, bool)
        fp = r["frame_point_out"][:int(P["frame_count"][b])]
        held[fp[fp >= 0]] = True
        pc[b] = n
        pf[b, :n], pd[b, :n] = map_pts_f[g], map_pts_desc[g]
        pfl[b, :n] = 1 | (2 * held[g - p0]) | (4 * (pt_nobs[g] > 0))
    return pf, pd, pc, pfl
