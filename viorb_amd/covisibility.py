"""The covisibility graph (KeyFrame::UpdateConnections for an ordered list of targets, reference src/KeyFrame.cc:414-448, 580-676, and the
LoopConnections of src/LoopClosing.cc:572-590) through the C ABI of include/viorb_covisibility.h. A stream's snapshot is a `scene`: a dict
of numpy arrays with stream-local offsets and indices,
    kf_by_key i32 [nk], kf_flags u8 [nk], kf_parent i32 [nk], kp_start i32 [nk+1], kp_point i32, pt_bad u8 [np], obs_start i32 [np+1], obs u32,
    conn_start i32 [nk+1], conn_kf, conn_w i32, ord_start i32 [nk+1], ord_kf, ord_w i32, targets i32,
which scene_from_lists builds from Python lists; pack() lays a list of scenes out as the flat arrays of viorb_covis_map with the row
length ccap. Results come back as one dict per stream. The host hook (no device) is update_connections_host_core."""
import ctypes as C
import numpy as np
from . import capi, snapshot as S
from .capi import lib, check, ptr

OK, OVERFLOW, INVALID = 0, 1, -1
STATUS_NAMES = {OK: "OK", OVERFLOW: "OVERFLOW", INVALID: "ERR_INVALID_ARG"}
MAX_KF = 65535
KF_ID0, KF_FIRST, MAP_CHANGED, ORD_REBUILT = 1, 2, 1, 2

_DT = dict(kf_start=np.int32, kf_by_key=np.int32, kf_flags=np.uint8, kf_parent=np.int32, kp_start=np.int32, kp_point=np.int32, pt_start=np.int32, pt_bad=np.uint8,
           obs_start=np.int32, obs=np.uint32, conn_start=np.int32, conn_kf=np.int32, conn_w=np.int32, ord_start=np.int32, ord_kf=np.int32, ord_w=np.int32,
           target_start=np.int32, target_kf=np.int32)
KF_ROWS = ("conn_kf_out", "conn_w_out", "ord_kf_out", "ord_w_out")                       # [n_kf][ccap]
KF_FIELDS = ("conn_n_out", "ord_n_out", "kf_parent_out", "kf_flags_out", "kf_touched")   # [n_kf]
T_FIELDS = ("t_observers", "t_max_kf", "t_max_w", "t_added", "t_parent", "n_loop_conn")  # [n_target]; loop_conn is [n_target][ccap]
_U8 = ("kf_flags_out", "kf_touched")


def shape():
    """(threads of the vote and the ordered phase, wavefront size, key frames whose counters and marks fit in LDS, the threshold th)."""
    o = np.zeros(4, np.int32)
    check(lib().viorb_update_connections_shape(ptr(o)))
    return tuple(int(v) for v in o)


def scene_from_lists(kfs, pts, targets, by_key=None):
    """kfs: [dict(pts=[point or -1], conn={slot: weight}, ord=[(slot, weight)], id0=False, first=True, parent=-1)]; pts: [dict(obs=[slots],
    bad=False)]; targets: the slots in call order; by_key: the slots in pointer order (default: slot order). conn is laid out in key order."""
    nk = len(kfs)
    by_key = list(by_key) if by_key is not None else list(range(nk))
    rank = {k: j for j, k in enumerate(by_key)}
    s = dict(targets=np.array(list(targets), np.int32), kf_by_key=np.array(by_key, np.int32))
    s["kf_flags"] = np.array([(KF_ID0 if k.get("id0") else 0) | (KF_FIRST if k.get("first", True) else 0) for k in kfs], np.uint8)
    s["kf_parent"] = np.array([k.get("parent", -1) for k in kfs], np.int32)
    s["kp_start"], s["kp_point"] = S.csr([k.get("pts", ()) for k in kfs], np.int32)
    s["pt_bad"] = np.array([1 if p.get("bad") else 0 for p in pts], np.uint8)
    s["obs_start"], s["obs"] = S.csr([p.get("obs", ()) for p in pts], np.uint32)
    conn = [sorted(dict(k.get("conn", {})).items(), key=lambda kv: rank[kv[0]]) for k in kfs]
    s["conn_start"], s["conn_kf"] = S.csr(conn, np.int32, lambda kv: kv[0])
    s["conn_w"] = S.csr(conn, np.int32, lambda kv: kv[1])[1]
    s["ord_start"], s["ord_kf"] = S.csr([k.get("ord", ()) for k in kfs], np.int32, lambda kv: kv[0])
    s["ord_w"] = S.csr([k.get("ord", ()) for k in kfs], np.int32, lambda kv: kv[1])[1]
    return s


def pack(scenes, ccap=None):
    """The flat arrays of viorb_covis_map for a list of scenes (every array at least one element long), with the totals and the row
    length. Default ccap: the most key frames of a stream - 1, which can never overflow."""
    B = len(scenes)
    cnt = lambda f: sum(len(s[f]) for s in scenes)
    P = dict(batch=B, n_kf=cnt("kf_flags"), n_kp=cnt("kp_point"), n_pt=cnt("pt_bad"), n_obs=cnt("obs"), n_conn=cnt("conn_kf"), n_ord=cnt("ord_kf"), n_target=cnt("targets"))
    P["ccap"] = int(ccap or max(1, max(len(s["kf_flags"]) for s in scenes) - 1))
    P["kf_start"], P["pt_start"], P["target_start"] = S.starts([s["kf_flags"] for s in scenes]), S.starts([s["pt_bad"] for s in scenes]), S.starts([s["targets"] for s in scenes])
    for f in ("kf_by_key", "kf_flags", "kf_parent", "kp_point", "pt_bad", "obs", "conn_kf", "conn_w", "ord_kf", "ord_w"):
        P[f] = S.cat(scenes, f, _DT[f])
    P["target_kf"] = S.cat(scenes, "targets", np.int32)
    for f, src in (("kp_start", "kp_point"), ("obs_start", "obs"), ("conn_start", "conn_kf"), ("ord_start", "ord_kf")):
        P[f] = S.rebase(scenes, f, src)
    return S.finish(P, capi.COVIS_ARRAYS, _DT)


def _map_struct(P, arrays=None):
    return S.struct(capi.CovisMap, capi.COVIS_INTS, capi.COVIS_ARRAYS, P, arrays)


def out_len(P, f):
    if f in KF_ROWS:
        return max(P["n_kf"], 1) * P["ccap"]
    if f in KF_FIELDS:
        return max(P["n_kf"], 1)
    if f == "loop_conn":
        return max(P["n_target"], 1) * P["ccap"]
    return max(P["n_target"], 1) if f in T_FIELDS else P["batch"]


def out_dtype(f):
    return np.uint8 if f in _U8 else np.int32


def split(P, o):
    """One dict per stream from flat result arrays: the fields of viorb_covis_result cut to the stream's key frames and targets, rows as
    [n][ccap]. A refused stream has only status and `untouched`: whether all its ranges still hold the fill value."""
    res, cc = [], P["ccap"]
    for b in range(P["batch"]):
        r = dict(status=int(o["status"][b]))
        if r["status"] == INVALID:
            # the stream's own ranges are whatever its (possibly broken) offsets say; every array outside the accepted streams must be untouched
            r["untouched"] = int(o["need"][b]) == S.FILL
            res.append(r)
            continue
        k0, k1, t0, t1 = (int(P[f][b + d]) for f in ("kf_start", "target_start") for d in (0, 1))
        r["need"] = int(o["need"][b])
        for f in KF_ROWS:
            r[f] = np.asarray(o[f])[k0 * cc:k1 * cc].reshape(k1 - k0, cc)
        for f in KF_FIELDS:
            r[f] = np.asarray(o[f])[k0:k1]
        for f in T_FIELDS:
            r[f] = np.asarray(o[f])[t0:t1]
        r["loop_conn"] = np.asarray(o["loop_conn"])[t0 * cc:t1 * cc].reshape(t1 - t0, cc)
        res.append(r)
    return res


def fill_outside(P, o, accepted):
    """Whether every element of the result arrays outside the key-frame and target ranges of the accepted streams still holds FILL."""
    cc = P["ccap"]
    kf, tg = np.ones(max(P["n_kf"], 1), bool), np.ones(max(P["n_target"], 1), bool)
    for b in accepted:
        kf[int(P["kf_start"][b]):int(P["kf_start"][b + 1])] = False
        tg[int(P["target_start"][b]):int(P["target_start"][b + 1])] = False
    ok = all((np.asarray(o[f]).reshape(-1, cc)[kf] == S.FILL).all() for f in KF_ROWS) and all((np.asarray(o[f])[kf] == S.FILL).all() for f in KF_FIELDS)
    ok = ok and all((np.asarray(o[f])[tg] == S.FILL).all() for f in T_FIELDS) and (np.asarray(o["loop_conn"]).reshape(-1, cc)[tg] == S.FILL).all()
    return bool(ok)


def _finish(P, o):
    res = split(P, o)
    outside = fill_outside(P, o, [b for b, r in enumerate(res) if r["status"] != INVALID])
    for r in res:
        if r["status"] == INVALID:
            r["untouched"] = r["untouched"] and outside
    return res


def _run_host(fn, scenes, packed, erase_targets, ccap):
    P = packed or pack(scenes, ccap=ccap)
    o = S.outputs(capi.COVIS_RESULT_FIELDS, lambda f: out_len(P, f), out_dtype)
    m, r = _map_struct(P), S.struct(capi.CovisResult, (), capi.COVIS_RESULT_FIELDS, o)
    check(fn(C.byref(m), C.byref(r), P["ccap"], int(erase_targets)))
    return _finish(P, o)


def update_connections(scenes, packed=None, erase_targets=0, ccap=None):
    """viorb_update_connections (host buffers): one result dict per scene."""
    return _run_host(lib().viorb_update_connections, scenes, packed, erase_targets, ccap)


def update_connections_host_core(scenes, packed=None, erase_targets=0, ccap=None):
    """viorb_debug_update_connections_host: covis_core.h on the host (no device), the phases of the device form on one thread."""
    return _run_host(lib().viorb_debug_update_connections_host, scenes, packed, erase_targets, ccap)


class CovisBatch:
    """A packed batch of scenes on the device: run() enqueues viorb_update_connections_device on torch tensors; results() downloads.
    optional=False passes NULL for every optional result array."""

    def __init__(self, scenes, device=0, packed=None, ccap=None, erase_targets=0):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.P = P = packed or pack(scenes, ccap=ccap)
        self.erase_targets = int(erase_targets)
        self.d = S.upload(P, capi.COVIS_ARRAYS, device)
        self.map = _map_struct(P, self.d)
        self.o = S.outputs(capi.COVIS_RESULT_FIELDS, lambda f: out_len(P, f), out_dtype, torch, self.dev)
        self.res = S.struct(capi.CovisResult, (), capi.COVIS_RESULT_FIELDS, self.o)
        self.res_required = capi.CovisResult(*[ptr(self.o[f]) if f in capi.COVIS_RESULT_REQUIRED else None for f in capi.COVIS_RESULT_FIELDS])
        self._wb = lib().viorb_update_connections_workspace_bytes(P["batch"], P["n_kf"], P["n_target"], P["ccap"])
        self.ws = capi.Workspace(torch, self.dev, self._wb)         # may be re-filled or replaced by a larger one between calls

    def run(self, optional=True):
        check(lib().viorb_update_connections_device(C.byref(self.map), C.byref(self.res if optional else self.res_required), self.P["ccap"], self.erase_targets,
                                                    self.ws.ptr, self._wb, S.stream_ptr(self.torch, self.dev)))

    def results(self):
        self.torch.cuda.synchronize(self.dev)
        return _finish(self.P, {f: v.cpu().numpy() for f, v in self.o.items()})
