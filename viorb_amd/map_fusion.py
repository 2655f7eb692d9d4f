"""Map fusion (the replace / add block of both ORBmatcher::Fuse, the Replace loop of LoopClosing::SearchAndFuse and MapPoint::Replace for
an ordered list of calls, reference src/ORBmatcher.cc:842-972 / :1000-1097, src/LoopClosing.cc:632-640, src/MapPoint.cc:184-222) through
the C ABI of include/viorb_map_fusion.h. A stream's snapshot is a `scene`: a dict of numpy arrays with stream-local offsets and indices,
    kf_by_key i32 [nk], kf_bad u8 [nk], kp_start i32 [nk+1], kp_point i32, kp_octave u8, kp_stereo u8, pt_bad u8 [np], pt_nobs, pt_found,
    pt_visible i32 [np], obs_start i32 [np+1], obs u32, obs_feat i32, call_kf i32 [nc], call_kind u8, call_list, call_n, call_feat i32,
    list_point i32, op_feat i32,
which scene_from_lists builds from Python lists; pack() lays a list of scenes out as the flat arrays of viorb_fuse_map. Results come back
as one dict per stream. The host hook (no device) is apply_fuse_host_core."""
import ctypes as C
import numpy as np
from . import capi, snapshot as S
from .capi import lib, check, ptr

OK, OVERFLOW, INVALID = 0, 1, -1
MAX_KF = 65535
POSE, SIM3 = 0, 1
ADDED, REPLACED_KF_POINT, REPLACED_CANDIDATE, COUNTED_ONLY, SKIP_BAD, SKIP_IN_KF, NONE, NULL_POINT = range(8)
OBS_STEREO = 1 << 24

_DT = dict(kf_start=np.int32, kf_by_key=np.int32, kf_bad=np.uint8, kp_start=np.int32, kp_point=np.int32, kp_octave=np.uint8, kp_stereo=np.uint8,
           pt_start=np.int32, pt_bad=np.uint8, pt_nobs=np.int32, pt_found=np.int32, pt_visible=np.int32, obs_start=np.int32, obs=np.uint32, obs_feat=np.int32,
           call_start=np.int32, call_kf=np.int32, call_kind=np.uint8, call_list=np.int32, call_n=np.int32, call_feat=np.int32, call_op=np.int32,
           list_point=np.int32, op_feat=np.int32, obs_out_start=np.int32)
KP_FIELDS = ("kp_point_out",)                                                                 # [n_kp]
PT_FIELDS = ("pt_bad_out", "pt_nobs_out", "pt_found_out", "pt_visible_out", "pt_replaced_out", "pt_dirty")          # [n_pt]
PT_STARTS = ("obs_start_out", "dirty_obs_start")                                              # [n_pt + 1]
OUT_FIELDS = ("obs_out", "obs_feat_out", "dirty_obs_kf", "dirty_obs_feat")                    # [n_obs_out]
OP_FIELDS = ("op_reason", "op_other")                                                         # [n_op]
_U8 = ("pt_bad_out", "pt_dirty", "obs_touched")


def shape():
    """(threads of the validating and emitting kernels, threads of the ordered phase = one wavefront, key frames whose state fits in LDS
    (0: none), 0)."""
    o = np.zeros(4, np.int32)
    check(lib().viorb_apply_fuse_shape(ptr(o)))
    return tuple(int(v) for v in o)


def scene_from_lists(kfs, pts, calls, by_key=None, shared_list=None):
    """kfs: [dict(pts=[point or -1], octave=[...] (default 0), stereo=[...] (default 0), bad=False)]; pts: [dict(obs=[(slot, feat)], bad=False,
    nobs=None (default: what the observations add up to), found=0, visible=0)]; calls: [(slot, kind, points, feats)] in order, each with a
    list and a best_idx row of its own, or with shared_list = the one point list of every call: [(slot, kind, feats)], the rows laid end
    to end (LoopClosing::SearchAndFuse). by_key: the slots in pointer order (default: slot order)."""
    nk = len(kfs)
    s = dict(kf_by_key=np.array(list(by_key) if by_key is not None else list(range(nk)), np.int32), kf_bad=np.array([1 if k.get("bad") else 0 for k in kfs], np.uint8))
    s["kp_start"], s["kp_point"] = S.csr([k.get("pts", ()) for k in kfs], np.int32)
    s["kp_octave"] = np.array([o for k in kfs for o in k.get("octave", [0] * len(k.get("pts", ())))], np.uint8)
    s["kp_stereo"] = np.array([o for k in kfs for o in k.get("stereo", [0] * len(k.get("pts", ())))], np.uint8)
    assert len(s["kp_octave"]) == len(s["kp_stereo"]) == len(s["kp_point"])
    st = lambda k, f: int(s["kp_stereo"][s["kp_start"][k] + f])
    oc = lambda k, f: int(s["kp_octave"][s["kp_start"][k] + f])
    obs = [list(p.get("obs", ())) for p in pts]
    s["pt_bad"] = np.array([1 if p.get("bad") else 0 for p in pts], np.uint8)
    s["pt_nobs"] = np.array([p["nobs"] if p.get("nobs") is not None else sum(2 if st(k, f) else 1 for k, f in o) for p, o in zip(pts, obs)], np.int32)
    s["pt_found"] = np.array([p.get("found", 0) for p in pts], np.int64).astype(np.uint32).view(np.int32)
    s["pt_visible"] = np.array([p.get("visible", 0) for p in pts], np.int64).astype(np.uint32).view(np.int32)
    s["obs_start"], s["obs"] = S.csr(obs, np.uint32, lambda o: int(o[0]) | (oc(*o) << 16) | (OBS_STEREO if st(*o) else 0))
    s["obs_feat"] = S.csr(obs, np.int32, lambda o: o[1])[1]
    if shared_list is not None:
        calls = [(k, kind, shared_list, feats) for k, kind, feats in calls]
    s["call_kf"], s["call_kind"] = np.array([c[0] for c in calls], np.int32), np.array([c[1] for c in calls], np.uint8)
    s["call_n"] = np.array([len(c[2]) for c in calls], np.int32)
    assert all(len(c[2]) == len(c[3]) for c in calls)
    off = S.starts([c[3] for c in calls])[:-1]
    s["call_feat"] = off.astype(np.int32)
    s["call_list"] = np.zeros(len(calls), np.int32) if shared_list is not None else off.astype(np.int32)
    s["list_point"] = np.array(list(shared_list) if shared_list is not None else [p for c in calls for p in c[2]], np.int32)
    s["op_feat"] = np.array([f for c in calls for f in c[3]], np.int32)
    return s


def region_bound(s):
    """A region length that cannot overflow: the input observations plus the list entries with a non-negative op_feat."""
    return len(s["obs"]) + sum(int((s["op_feat"][f:f + n] >= 0).sum()) for f, n in zip(s["call_feat"], s["call_n"]))


def pack(scenes, regions=None):
    """The flat arrays of viorb_fuse_map for a list of scenes (every array at least one element long), with the totals. regions: the
    length of every stream's region of the output observation arrays (default: region_bound)."""
    B = len(scenes)
    cnt = lambda f: sum(len(s[f]) for s in scenes)
    regions = [region_bound(s) for s in scenes] if regions is None else [int(r) for r in regions]
    P = dict(batch=B, n_kf=cnt("kf_bad"), n_kp=cnt("kp_point"), n_pt=cnt("pt_bad"), n_obs=cnt("obs"), n_call=cnt("call_kf"), n_list=cnt("list_point"), n_feat=cnt("op_feat"),
             n_op=int(sum(int(s["call_n"].sum()) for s in scenes)), n_obs_out=int(sum(regions)))
    P["kf_start"], P["pt_start"], P["call_start"] = S.starts([s["kf_bad"] for s in scenes]), S.starts([s["pt_bad"] for s in scenes]), S.starts([s["call_kf"] for s in scenes])
    P["obs_out_start"] = np.concatenate([[0], np.cumsum(regions)]).astype(np.int32)
    for f in ("kf_by_key", "kf_bad", "kp_point", "kp_octave", "kp_stereo", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "obs", "obs_feat", "call_kf", "call_kind", "call_n",
              "list_point", "op_feat"):
        P[f] = S.cat(scenes, f, _DT[f])
    for f, src in (("kp_start", "kp_point"), ("obs_start", "obs")):
        P[f] = S.rebase(scenes, f, src)
    lb, fb = S.starts([s["list_point"] for s in scenes]), S.starts([s["op_feat"] for s in scenes])
    P["call_list"] = np.concatenate([np.asarray(s["call_list"], np.int32) + lb[b] for b, s in enumerate(scenes)] + [np.zeros(0, np.int32)]).astype(np.int32)
    P["call_feat"] = np.concatenate([np.asarray(s["call_feat"], np.int32) + fb[b] for b, s in enumerate(scenes)] + [np.zeros(0, np.int32)]).astype(np.int32)
    P["call_op"] = np.concatenate([[0], np.cumsum(P["call_n"], dtype=np.int64)]).astype(np.int32)
    return S.finish(P, capi.FUSE_ARRAYS, _DT)


def _map_struct(P, arrays=None):
    return S.struct(capi.FuseMap, capi.FUSE_INTS, capi.FUSE_ARRAYS, P, arrays)


def out_len(P, f):
    if f in KP_FIELDS:
        return max(P["n_kp"], 1)
    if f in PT_FIELDS:
        return max(P["n_pt"], 1)
    if f in PT_STARTS:
        return P["n_pt"] + 1
    if f in OUT_FIELDS:
        return max(P["n_obs_out"], 1)
    if f in OP_FIELDS:
        return max(P["n_op"], 1)
    return {"obs_touched": max(P["n_obs"], 1), "call_nfused": max(P["n_call"], 1)}.get(f, P["batch"])


def out_dtype(f):
    return np.uint8 if f in _U8 else np.int32                  # obs_out: the words as int32 (bit 31 is never set)


def _ranges(P, b):
    k0, k1, p0, p1, c0, c1 = (int(P[f][b + d]) for f in ("kf_start", "pt_start", "call_start") for d in (0, 1))
    return dict(k0=k0, k1=k1, p0=p0, p1=p1, c0=c0, c1=c1, i0=int(P["kp_start"][k0]), i1=int(P["kp_start"][k1]), o0=int(P["obs_start"][p0]), o1=int(P["obs_start"][p1]),
                j0=int(P["call_op"][c0]), j1=int(P["call_op"][c1]), q0=int(P["obs_out_start"][b]), q1=int(P["obs_out_start"][b + 1]))


def split(P, o):
    """One dict per stream from flat result arrays: the fields of viorb_fuse_result cut to the stream's ranges; obs = per point the list of
    (slot, octave, stereo, feature) in output order, dirty = per point the list of (stream-local slot, feature). A refused stream has only
    its status; an overflowed one has no obs and empty dirty lists."""
    res, statuses = [], [int(v) for v in np.asarray(o["status"])[:P["batch"]]]
    have = lambda f: f in o and o[f] is not None
    dat = 0
    for b, status in enumerate(statuses):
        r = dict(status=status)
        if status == INVALID:
            res.append(r)
            continue
        g = _ranges(P, b)
        np_ = g["p1"] - g["p0"]
        r["kp_point_out"] = np.asarray(o["kp_point_out"])[g["i0"]:g["i1"]]
        for f in PT_FIELDS:
            if have(f):
                r[f] = np.asarray(o[f])[g["p0"]:g["p1"]]
        for f in OP_FIELDS:
            if have(f):
                r[f] = np.asarray(o[f])[g["j0"]:g["j1"]]
        if have("call_nfused"):
            r["call_nfused"] = np.asarray(o["call_nfused"])[g["c0"]:g["c1"]]
        if have("obs_touched"):
            r["obs_touched"] = np.asarray(o["obs_touched"])[g["o0"]:g["o1"]]
        if have("need"):
            r["need"] = int(o["need"][b])
        last = b + 1 == P["batch"] or statuses[b + 1] == INVALID
        r["boundary"] = last
        if status == OK:
            st = np.asarray(o["obs_start_out"])[g["p0"]:g["p1"] + (1 if last else 0)].astype(np.int64)
            if not last:                                                # the boundary element is the next stream's: the entries are packed, so
                st = np.append(st, -1)                                  # the last point ends where `need` says, or where the region's last written entry lies
                st[-1] = g["q0"] + r["need"] if have("need") else -1
            r["obs_start_local"] = st - g["q0"]
            r["obs_region"] = (np.asarray(o["obs_out"])[g["q0"]:g["q1"]], np.asarray(o["obs_feat_out"])[g["q0"]:g["q1"]])
            if st[-1] >= 0:
                w, f = np.asarray(o["obs_out"]), np.asarray(o["obs_feat_out"])
                r["obs"] = [[(int(w[e]) & 0xffff, (int(w[e]) >> 16) & 0xff, (int(w[e]) >> 24) & 1, int(f[e])) for e in range(st[p], st[p + 1])] for p in range(np_)]
        if have("dirty_obs_start"):
            ds = np.asarray(o["dirty_obs_start"])
            r["dirty_base"] = int(ds[g["p0"]])
            r["dirty"] = [[(int(o["dirty_obs_kf"][e]) - g["k0"], int(o["dirty_obs_feat"][e])) for e in range(int(ds[g["p0"] + p]), int(ds[g["p0"] + p + 1]))] for p in range(np_)]
            dat = r["dirty_base"] + sum(len(d) for d in r["dirty"])
            r["dirty_end"] = dat
        res.append(r)
    return res


def fill_outside(P, o, results):
    """Whether every element of the result arrays outside what the accepted streams write still holds FILL."""
    n = lambda f: np.ones(len(np.asarray(o[f])), bool)
    masks = {f: n(f) for f in o if o[f] is not None}
    for b, r in enumerate(results):
        masks["status"][b] = False                                    # a refused stream writes its status and nothing else
        if r["status"] == INVALID:
            continue
        g = _ranges(P, b)
        for f, (a, e) in [(f, (g["i0"], g["i1"])) for f in KP_FIELDS] + [(f, (g["p0"], g["p1"])) for f in PT_FIELDS] + [(f, (g["j0"], g["j1"])) for f in OP_FIELDS] \
                + [("call_nfused", (g["c0"], g["c1"])), ("obs_touched", (g["o0"], g["o1"])), ("need", (b, b + 1))]:
            if f in masks:
                masks[f][a:e] = False
        if "dirty_obs_start" in masks:
            masks["dirty_obs_start"][g["p0"]:g["p1"] + 1] = False
            for f in ("dirty_obs_kf", "dirty_obs_feat"):
                masks[f][r["dirty_base"]:r["dirty_end"]] = False
        if r["status"] == OK:
            masks["obs_start_out"][g["p0"]:g["p1"] + (1 if r["boundary"] else 0)] = False
            used = int(r["obs_start_local"][-1]) if r["obs_start_local"][-1] >= 0 else g["q1"] - g["q0"]
            for f in ("obs_out", "obs_feat_out"):
                masks[f][g["q0"]:g["q0"] + used] = False
    return all(bool((np.asarray(o[f])[m] == S.FILL).all()) for f, m in masks.items())


def _finish(P, o):
    res = split(P, o)
    outside = fill_outside(P, o, res)
    for r in res:
        r["untouched"] = outside                                      # nothing outside the accepted streams' ranges was written
    return res


def _result_struct(o, fields):
    return capi.FuseResult(*[ptr(o[f]) if f in fields else None for f in capi.FUSE_RESULT_FIELDS])


def _run_host(fn, scenes, packed, regions, fields):
    P = packed or pack(scenes, regions=regions)
    o = S.outputs(fields, lambda f: out_len(P, f), out_dtype)
    m, r = _map_struct(P), _result_struct(o, fields)
    check(fn(C.byref(m), C.byref(r)))
    return _finish(P, o)


def apply_fuse(scenes, packed=None, regions=None, fields=capi.FUSE_RESULT_FIELDS):
    """viorb_apply_fuse (host buffers): one result dict per scene."""
    return _run_host(lib().viorb_apply_fuse, scenes, packed, regions, fields)


def apply_fuse_host_core(scenes, packed=None, regions=None, fields=capi.FUSE_RESULT_FIELDS):
    """viorb_debug_apply_fuse_host: map_fusion_core.h on the host (no device), the phases of the device form on one thread."""
    return _run_host(lib().viorb_debug_apply_fuse_host, scenes, packed, regions, fields)


class FuseBatch:
    """A packed batch of scenes on the device: run() enqueues viorb_apply_fuse_device on torch tensors; results() downloads.
    optional=False passes NULL for every optional result array. arrays: device tensors that replace uploaded inputs by name (op_feat:
    the best_idx of viorb_fuse_sim3_device as it is)."""

    def __init__(self, scenes, device=0, packed=None, regions=None, arrays=None):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.P = P = packed or pack(scenes, regions=regions)
        self.d = S.upload(P, capi.FUSE_ARRAYS, device)
        self.d.update(arrays or {})
        self.map = _map_struct(P, self.d)
        self.o = S.outputs(capi.FUSE_RESULT_FIELDS, lambda f: out_len(P, f), out_dtype, torch, self.dev)
        self.res = _result_struct(self.o, capi.FUSE_RESULT_FIELDS)
        self.res_required = _result_struct(self.o, capi.FUSE_RESULT_REQUIRED)
        self._wb = lib().viorb_apply_fuse_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"], P["n_obs"], P["n_op"])
        self.ws = capi.Workspace(torch, self.dev, self._wb)         # may be re-filled or replaced by a larger one between calls

    def run(self, optional=True):
        check(lib().viorb_apply_fuse_device(C.byref(self.map), C.byref(self.res if optional else self.res_required), self.ws.ptr, self._wb,
                                            S.stream_ptr(self.torch, self.dev)))

    def results(self, optional=True):
        self.torch.cuda.synchronize(self.dev)
        fields = capi.FUSE_RESULT_FIELDS if optional else capi.FUSE_RESULT_REQUIRED
        return _finish(self.P, {f: self.o[f].cpu().numpy() for f in fields})


def merge_descriptors(pt_dirty, dirty_obs_start, new_desc, pts_desc, stream=None):
    """viorb_fuse_merge_descriptors_device on device tensors: pts_desc [n_pt][32] takes the rows of new_desc of the dirty points that
    have a dirty list."""
    check(lib().viorb_fuse_merge_descriptors_device(ptr(pt_dirty), ptr(dirty_obs_start), ptr(new_desc), ptr(pts_desc), int(pts_desc.shape[0]), stream))
