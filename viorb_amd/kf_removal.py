"""Key-frame removal (KeyFrame::SetBadFlag and KeyFrame::SetErase for an ordered list of operations, reference src/KeyFrame.cc:728-904 and
src/MapPoint.cc:118-175) through the C ABI of include/viorb_kf_removal.h. A stream's snapshot is a `scene`: a dict of numpy arrays with
stream-local offsets and indices,
    kf_by_key i32 [nk], kf_flags u8 [nk], kf_parent, kf_prev, kf_next i32 [nk], kf_pose12 f32 [nk][12], kp_start i32 [nk+1], kp_point i32,
    pt_bad u8 [np], pt_nobs, pt_ref i32 [np], obs_start i32 [np+1], obs u32, conn_start i32 [nk+1], conn_kf, conn_w i32,
    ord_start i32 [nk+1], ord_kf, ord_w i32, op_kf i32, op_kind u8,
which scene_from_lists builds from Python lists; pack() lays a list of scenes out as the flat arrays of viorb_kfr_map with the row
length ccap. Results come back as one dict per stream. The host hook (no device) is remove_key_frames_host_core."""
import ctypes as C
import numpy as np
from . import capi, snapshot as S
from .capi import lib, check, ptr

OK, INVALID = 0, -1
MAX_KF = 65535
KF_ID0, KF_BAD, KF_NOT_ERASE, KF_TO_BE_ERASED, KF_LOOP_EDGES = 1, 2, 4, 8, 16
SET_BAD_FLAG, SET_ERASE = 0, 1
REMOVED, ALREADY_BAD, FIRST_KF, DEFERRED, RELEASED = 0, 1, 2, 3, 4
MAP_CHANGED, ORD_REBUILT, PARENT_CHANGED = 1, 2, 4
OBS_STEREO = 1 << 24

_DT = dict(kf_start=np.int32, kf_by_key=np.int32, kf_flags=np.uint8, kf_parent=np.int32, kf_prev=np.int32, kf_next=np.int32, kf_pose12=np.float32,
           kp_start=np.int32, kp_point=np.int32, pt_start=np.int32, pt_bad=np.uint8, pt_nobs=np.int32, pt_ref=np.int32, obs_start=np.int32, obs=np.uint32,
           conn_start=np.int32, conn_kf=np.int32, conn_w=np.int32, ord_start=np.int32, ord_kf=np.int32, ord_w=np.int32,
           op_start=np.int32, op_kf=np.int32, op_kind=np.uint8)
KF_ROWS = ("conn_kf_out", "conn_w_out", "ord_kf_out", "ord_w_out")                       # [n_kf][ccap]
KF_FIELDS = ("conn_n_out", "ord_n_out", "kf_parent_out", "kf_flags_out", "kf_prev_out", "kf_next_out", "kf_repreint", "kf_touched")   # [n_kf]; kf_Tcp_out is [n_kf][12]
PT_FIELDS = ("pt_nobs_out", "pt_bad_out", "pt_ref_out")                                  # [n_pt]
OP_FIELDS = ("op_reason", "op_children", "op_fallback", "op_rebuilt", "op_points_bad")   # [n_op]
_U8 = ("kf_flags_out", "kf_repreint", "kf_touched", "pt_bad_out", "obs_alive")
IDENTITY12 = (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)


def shape():
    """(threads of the ordered phase, wavefront size, key frames whose candidate marks fit in LDS, wavefronts that share the neighbours)."""
    o = np.zeros(4, np.int32)
    check(lib().viorb_remove_key_frames_shape(ptr(o)))
    return tuple(int(v) for v in o)


def scene_from_lists(kfs, pts, ops, by_key=None):
    """kfs: [dict(pts=[point or -1], conn={slot: weight}, ord=[(slot, weight)], id0, bad, not_erase, to_be_erased, loop_edges=False, parent=-1,
    prev=-1, next=-1, pose=12 floats (default: the identity))]; pts: [dict(obs=[slot or (slot, stereo)], bad=False, nobs=None (default: what
    the observations add up to), ref=None (default: the first observer or -1))]; ops: [(slot, kind)] or [slot] (SetBadFlag) in call order;
    by_key: the slots in pointer order (default: slot order). conn is laid out in key order."""
    nk = len(kfs)
    by_key = list(by_key) if by_key is not None else list(range(nk))
    rank = {k: j for j, k in enumerate(by_key)}
    ops = [(o, SET_BAD_FLAG) if np.isscalar(o) else tuple(o) for o in ops]
    s = dict(op_kf=np.array([o[0] for o in ops], np.int32), op_kind=np.array([o[1] for o in ops], np.uint8), kf_by_key=np.array(by_key, np.int32))
    bit = lambda k, name, v: v if k.get(name) else 0
    s["kf_flags"] = np.array([bit(k, "id0", KF_ID0) | bit(k, "bad", KF_BAD) | bit(k, "not_erase", KF_NOT_ERASE) | bit(k, "to_be_erased", KF_TO_BE_ERASED)
                              | bit(k, "loop_edges", KF_LOOP_EDGES) for k in kfs], np.uint8)
    for f, key in (("kf_parent", "parent"), ("kf_prev", "prev"), ("kf_next", "next")):
        s[f] = np.array([k.get(key, -1) for k in kfs], np.int32)
    s["kf_pose12"] = np.array([k.get("pose", IDENTITY12) for k in kfs], np.float32).reshape(nk, 12)
    s["kp_start"], s["kp_point"] = S.csr([k.get("pts", ()) for k in kfs], np.int32)
    obs = [[(o, 0) if np.isscalar(o) else tuple(o) for o in p.get("obs", ())] for p in pts]
    s["pt_bad"] = np.array([1 if p.get("bad") else 0 for p in pts], np.uint8)
    s["pt_nobs"] = np.array([p["nobs"] if p.get("nobs") is not None else sum(2 if st else 1 for _, st in o) for p, o in zip(pts, obs)], np.int32)
    s["pt_ref"] = np.array([p["ref"] if p.get("ref") is not None else (o[0][0] if o else -1) for p, o in zip(pts, obs)], np.int32)
    s["obs_start"], s["obs"] = S.csr(obs, np.uint32, lambda o: int(o[0]) | (OBS_STEREO if o[1] else 0))
    conn = [sorted(dict(k.get("conn", {})).items(), key=lambda kv: rank[kv[0]]) for k in kfs]
    s["conn_start"], s["conn_kf"] = S.csr(conn, np.int32, lambda kv: kv[0])
    s["conn_w"] = S.csr(conn, np.int32, lambda kv: kv[1])[1]
    s["ord_start"], s["ord_kf"] = S.csr([k.get("ord", ()) for k in kfs], np.int32, lambda kv: kv[0])
    s["ord_w"] = S.csr([k.get("ord", ()) for k in kfs], np.int32, lambda kv: kv[1])[1]
    return s


def pack(scenes, ccap=None):
    """The flat arrays of viorb_kfr_map for a list of scenes (every array at least one element long), with the totals and the row
    length. Default ccap: the most key frames of a stream - 1, at least 1."""
    B = len(scenes)
    cnt = lambda f: sum(len(s[f]) for s in scenes)
    P = dict(batch=B, n_kf=cnt("kf_flags"), n_kp=cnt("kp_point"), n_pt=cnt("pt_bad"), n_obs=cnt("obs"), n_conn=cnt("conn_kf"), n_ord=cnt("ord_kf"), n_op=cnt("op_kf"))
    P["ccap"] = int(ccap or max(1, max(len(s["kf_flags"]) for s in scenes) - 1))
    P["kf_start"], P["pt_start"], P["op_start"] = S.starts([s["kf_flags"] for s in scenes]), S.starts([s["pt_bad"] for s in scenes]), S.starts([s["op_kf"] for s in scenes])
    for f in ("kf_by_key", "kf_flags", "kf_parent", "kf_prev", "kf_next", "kf_pose12", "kp_point", "pt_bad", "pt_nobs", "pt_ref", "obs", "conn_kf", "conn_w",
              "ord_kf", "ord_w", "op_kf", "op_kind"):
        P[f] = S.cat(scenes, f, _DT[f])
    for f, src in (("kp_start", "kp_point"), ("obs_start", "obs"), ("conn_start", "conn_kf"), ("ord_start", "ord_kf")):
        P[f] = S.rebase(scenes, f, src)
    return S.finish(P, capi.KFR_ARRAYS, _DT)


def _map_struct(P, arrays=None):
    return S.struct(capi.KfrMap, capi.KFR_INTS, capi.KFR_ARRAYS, P, arrays)


def out_len(P, f):
    if f in KF_ROWS:
        return max(P["n_kf"], 1) * P["ccap"]
    if f == "kf_Tcp_out":
        return max(P["n_kf"], 1) * 12
    if f in KF_FIELDS:
        return max(P["n_kf"], 1)
    if f in PT_FIELDS:
        return max(P["n_pt"], 1)
    if f in OP_FIELDS:
        return max(P["n_op"], 1)
    return {"obs_alive": max(P["n_obs"], 1), "kp_point_out": max(P["n_kp"], 1)}.get(f, P["batch"])


def out_dtype(f):
    return np.uint8 if f in _U8 else np.float32 if f == "kf_Tcp_out" else np.int32


def _ranges(P, b):
    k0, k1, p0, p1, j0, j1 = (int(P[f][b + d]) for f in ("kf_start", "pt_start", "op_start") for d in (0, 1))
    return k0, k1, p0, p1, j0, j1, int(P["kp_start"][k0]), int(P["kp_start"][k1]), int(P["obs_start"][p0]), int(P["obs_start"][p1])


def split(P, o):
    """One dict per stream from flat result arrays: the fields of viorb_kfr_result cut to the stream's key frames, points, keypoints,
    observations and operations, rows as [n][ccap]. A refused stream has only its status."""
    res, cc = [], P["ccap"]
    for b in range(P["batch"]):
        r = dict(status=int(o["status"][b]))
        if r["status"] == INVALID:
            res.append(r)
            continue
        k0, k1, p0, p1, j0, j1, i0, i1, o0, o1 = _ranges(P, b)
        for f in KF_ROWS:
            r[f] = np.asarray(o[f])[k0 * cc:k1 * cc].reshape(k1 - k0, cc)
        for f in KF_FIELDS:
            r[f] = np.asarray(o[f])[k0:k1]
        r["kf_Tcp_out"] = np.asarray(o["kf_Tcp_out"])[k0 * 12:k1 * 12].reshape(k1 - k0, 12)
        for f in PT_FIELDS:
            r[f] = np.asarray(o[f])[p0:p1]
        for f in OP_FIELDS:
            r[f] = np.asarray(o[f])[j0:j1]
        r["kp_point_out"], r["obs_alive"] = np.asarray(o["kp_point_out"])[i0:i1], np.asarray(o["obs_alive"])[o0:o1]
        res.append(r)
    return res


def fill_outside(P, o, accepted):
    """Whether every element of the result arrays outside the ranges of the accepted streams still holds FILL (kf_Tcp_out: also the rows of
    the key frames that were not removed, which kf_flags_out tells apart from the snapshot's flags)."""
    cc = P["ccap"]
    kf, pt, op = np.ones(max(P["n_kf"], 1), bool), np.ones(max(P["n_pt"], 1), bool), np.ones(max(P["n_op"], 1), bool)
    kp, ob = np.ones(max(P["n_kp"], 1), bool), np.ones(max(P["n_obs"], 1), bool)
    for b in accepted:
        k0, k1, p0, p1, j0, j1, i0, i1, o0, o1 = _ranges(P, b)
        kf[k0:k1], pt[p0:p1], op[j0:j1], kp[i0:i1], ob[o0:o1] = False, False, False, False, False
    ok = all((np.asarray(o[f]).reshape(-1, cc)[kf] == S.FILL).all() for f in KF_ROWS) and all((np.asarray(o[f])[kf] == S.FILL).all() for f in KF_FIELDS)
    ok = ok and all((np.asarray(o[f])[pt] == S.FILL).all() for f in PT_FIELDS) and all((np.asarray(o[f])[op] == S.FILL).all() for f in OP_FIELDS)
    ok = ok and (np.asarray(o["kp_point_out"])[kp] == S.FILL).all() and (np.asarray(o["obs_alive"])[ob] == S.FILL).all()
    fl = np.asarray(o["kf_flags_out"])
    if not (fl == S.FILL).all():                                      # the optional outputs were written
        n = P["n_kf"]
        removed = np.zeros(max(n, 1), bool)
        removed[:n] = ~kf[:n] & ((fl[:n] & KF_BAD) != 0) & ((P["kf_flags"][:n] & KF_BAD) == 0)
        ok = ok and (np.asarray(o["kf_Tcp_out"]).reshape(-1, 12)[~removed] == S.FILL).all()
    else:
        ok = ok and (np.asarray(o["kf_Tcp_out"])[np.repeat(kf, 12)] == S.FILL).all()
    return bool(ok)


def _finish(P, o):
    res = split(P, o)
    outside = fill_outside(P, o, [b for b, r in enumerate(res) if r["status"] != INVALID])
    for r in res:
        r["untouched"] = outside                                      # nothing outside the accepted streams' ranges was written
    return res


def _run_host(fn, scenes, packed, ccap):
    P = packed or pack(scenes, ccap=ccap)
    o = S.outputs(capi.KFR_RESULT_FIELDS, lambda f: out_len(P, f), out_dtype)
    m, r = _map_struct(P), S.struct(capi.KfrResult, (), capi.KFR_RESULT_FIELDS, o)
    check(fn(C.byref(m), C.byref(r), P["ccap"]))
    return _finish(P, o)


def remove_key_frames(scenes, packed=None, ccap=None):
    """viorb_remove_key_frames (host buffers): one result dict per scene."""
    return _run_host(lib().viorb_remove_key_frames, scenes, packed, ccap)


def remove_key_frames_host_core(scenes, packed=None, ccap=None):
    """viorb_debug_remove_key_frames_host: kf_removal_core.h on the host (no device), the phases of the device form on one thread."""
    return _run_host(lib().viorb_debug_remove_key_frames_host, scenes, packed, ccap)


class KfRemovalBatch:
    """A packed batch of scenes on the device: run() enqueues viorb_remove_key_frames_device on torch tensors; results() downloads.
    optional=False passes NULL for every optional result array."""

    def __init__(self, scenes, device=0, packed=None, ccap=None):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.P = P = packed or pack(scenes, ccap=ccap)
        self.d = S.upload(P, capi.KFR_ARRAYS, device)
        self.map = _map_struct(P, self.d)
        self.o = S.outputs(capi.KFR_RESULT_FIELDS, lambda f: out_len(P, f), out_dtype, torch, self.dev)
        self.res = S.struct(capi.KfrResult, (), capi.KFR_RESULT_FIELDS, self.o)
        self.res_required = capi.KfrResult(*[ptr(self.o[f]) if f in capi.KFR_RESULT_REQUIRED else None for f in capi.KFR_RESULT_FIELDS])
        self._wb = lib().viorb_remove_key_frames_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"], P["n_op"])
        self.ws = capi.Workspace(torch, self.dev, self._wb)         # may be re-filled or replaced by a larger one between calls

    def run(self, optional=True):
        check(lib().viorb_remove_key_frames_device(C.byref(self.map), C.byref(self.res if optional else self.res_required), self.P["ccap"],
                                                   self.ws.ptr, self._wb, S.stream_ptr(self.torch, self.dev)))

    def results(self):
        self.torch.cuda.synchronize(self.dev)
        return _finish(self.P, {f: v.cpu().numpy() for f, v in self.o.items()})
