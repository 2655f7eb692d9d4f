"""The map correction of loop closing (the propagation of LoopClosing::CorrectLoop, reference src/LoopClosing.cc:460-542, with SetPose and
UpdateNormalAndDepth of what it moves) through the C ABI of include/viorb_map_correction.h. A stream's snapshot is a `scene`: a dict of
numpy arrays with stream-local offsets and indices,
    kf_by_key i32 [nk], kp_start i32 [nk+1], kp_point i32, pt_bad u8 [np], obs_start i32 [np+1], obs u32 (slot | octave << 16),
    pose12 f32 [nk][12], pts_f f32 [np][8], pt_ref i32 [np], pt_corrected_by i32 [np], cur_kf, cur_id (ints), Scw8 f64 [8], conn i32,
which scene_from_lists builds from Python lists; pack() lays a list of scenes out as the flat arrays of viorb_correct_loop_map. Results
come back as one dict per stream. The host hook (no device) is correct_loop_host_core. The second half of the module is the map update
after a global bundle adjustment (viorb_apply_global_ba): gba_scene, gba_pack, apply_global_ba, apply_global_ba_host_core, ApplyGbaBatch."""
import ctypes as C
import numpy as np
from . import capi, snapshot as S
from .capi import lib, check, ptr

OK, INVALID = 0, -1
MAX_KF = 65535
NLEVELS, SCALE_FACTOR = 8, 1.2

_DT = dict(kf_start=np.int32, kf_by_key=np.int32, kp_start=np.int32, kp_point=np.int32, pt_start=np.int32, pt_bad=np.uint8, obs_start=np.int32, obs=np.uint32,
           pose12=np.float32, pts_f=np.float32, pt_ref=np.int32, pt_corrected_by=np.int32, cur_kf=np.int32, cur_id=np.int32, Scw8=np.float64,
           conn_start=np.int32, conn_kf=np.int32)
# result field -> (what it is indexed by, row length, dtype)
OUT = dict(status=("b", 1, np.int32), n_member=("b", 1, np.int32), member_kf=("m", 1, np.int32), Scw_f12=("m", 12, np.float32), Scw_out=("k", 8, np.float64),
           Smeas_out=("k", 8, np.float64), pose12_out=("k", 12, np.float32), Ow_out=("k", 3, np.float32), pts_f_out=("p", 8, np.float32),
           pt_corrected_by_out=("p", 1, np.int32), pt_corrected_ref_out=("p", 1, np.int32), pt_touched=("p", 1, np.uint8))
FIELDS = tuple(f for f in capi.CORRECT_LOOP_RESULT_FIELDS if f != "status")


def camera(nlevels=NLEVELS, scale_factor=SCALE_FACTOR):
    """A viorb_mapping_camera with the scale table the extractor builds (float32 products of the factor)."""
    c = capi.MappingCamera()
    c.nlevels, c.scale_factor = nlevels, scale_factor
    sf = np.float32(1.0)
    for i in range(16):
        c.scale_factors[i] = float(sf)
        c.level_sigma2[i] = float(sf * sf)
        sf = np.float32(sf * np.float32(scale_factor))
    return c


def scale_factors(cam):
    """mvScaleFactors as the library reads them: float32 [16], the levels from nlevels on repeat the last."""
    return np.array([cam.scale_factors[min(i, cam.nlevels - 1)] for i in range(16)], np.float32)


def shape():
    """(threads of the key-frame phase, threads of the point phase, wavefront size, key frames whose key positions fit in LDS)."""
    o = np.zeros(4, np.int32)
    check(lib().viorb_correct_loop_shape(ptr(o)))
    return tuple(int(v) for v in o)


def obs_word(slot, octave=0):
    return int(slot) | (int(octave) << 16)


def scene_from_lists(kfs, pts, cur_kf, conn, Scw8, cur_id=7, by_key=None):
    """kfs: [dict(pts=[point or -1], pose=f32 [12])]; pts: [dict(obs=[(slot, octave)], bad=False, P=f32 [8], ref=slot, by=mnCorrectedByKF)];
    conn: the covisible slots in list order; by_key: the slots in pointer order (default: slot order)."""
    nk = len(kfs)
    s = dict(kf_by_key=np.array(list(by_key) if by_key is not None else list(range(nk)), np.int32), cur_kf=int(cur_kf), cur_id=int(cur_id),
             Scw8=np.asarray(Scw8, np.float64).reshape(8), conn=np.array(list(conn), np.int32))
    s["kp_start"], s["kp_point"] = S.csr([k.get("pts", ()) for k in kfs], np.int32)
    s["pose12"] = np.array([k["pose"] for k in kfs], np.float32).reshape(nk, 12)
    s["pt_bad"] = np.array([1 if p.get("bad") else 0 for p in pts], np.uint8)
    s["obs_start"], s["obs"] = S.csr([p.get("obs", ()) for p in pts], np.uint32, lambda so: obs_word(*so))
    s["pts_f"] = np.array([p["P"] for p in pts], np.float32).reshape(len(pts), 8)
    s["pt_ref"] = np.array([p.get("ref", -1) for p in pts], np.int32)
    s["pt_corrected_by"] = np.array([p.get("by", 0) for p in pts], np.int32)
    return s


def pack(scenes):
    """The flat arrays of viorb_correct_loop_map for a list of scenes (every array at least one element long), with the totals."""
    cnt = lambda f: sum(len(s[f]) for s in scenes)
    P = dict(batch=len(scenes), n_kf=cnt("kf_by_key"), n_kp=cnt("kp_point"), n_pt=cnt("pt_bad"), n_obs=cnt("obs"), n_conn=cnt("conn"))
    P["kf_start"], P["pt_start"], P["conn_start"] = S.starts([s["kf_by_key"] for s in scenes]), S.starts([s["pt_bad"] for s in scenes]), S.starts([s["conn"] for s in scenes])
    for f in ("kf_by_key", "kp_point", "pt_bad", "obs", "pose12", "pts_f", "pt_ref", "pt_corrected_by", "Scw8"):
        P[f] = S.cat(scenes, f, _DT[f])
    P["conn_kf"] = S.cat(scenes, "conn", np.int32)
    P["cur_kf"], P["cur_id"] = np.array([s["cur_kf"] for s in scenes], np.int32), np.array([s["cur_id"] for s in scenes], np.int32)
    for f, src in (("kp_start", "kp_point"), ("obs_start", "obs")):
        P[f] = S.rebase(scenes, f, src)
    return S.finish(P, capi.CORRECT_LOOP_ARRAYS, _DT)


def _map_struct(P, arrays=None):
    return S.struct(capi.CorrectLoopMap, capi.CORRECT_LOOP_INTS, capi.CORRECT_LOOP_ARRAYS, P, arrays)


def rows_of(P, f):
    return dict(b=P["batch"], m=P["n_conn"] + P["batch"], k=max(P["n_kf"], 1), p=max(P["n_pt"], 1))[OUT[f][0]]


def out_len(P, f):
    return rows_of(P, f) * OUT[f][1]


def out_dtype(f):
    return OUT[f][2]


def _range(P, what, b):
    """Rows [i0, i1) of stream b in an array indexed by `what`."""
    if what == "b":
        return b, b + 1
    if what == "m":
        return int(P["conn_start"][b]) + b, int(P["conn_start"][b + 1]) + b + 1
    start = P["kf_start" if what == "k" else "pt_start"]
    return int(start[b]), int(start[b + 1])


def split(P, o):
    """One dict per stream from flat result arrays, rows as [n][row length]. A refused stream has only its status."""
    res = []
    for b in range(P["batch"]):
        r = dict(status=int(o["status"][b]))
        if r["status"] != INVALID:
            for f in FIELDS:
                what, row, _ = OUT[f]
                i0, i1 = _range(P, what, b)
                a = np.asarray(o[f])[i0 * row:i1 * row]
                r[f] = int(a[0]) if what == "b" else (a.reshape(i1 - i0, row) if row > 1 else a)
        res.append(r)
    return res


def fill_outside(P, o, accepted):
    """Whether every element of the result arrays outside the ranges of the accepted streams still holds FILL."""
    ok = True
    for f in FIELDS:
        what, row, dt = OUT[f]
        keep = np.ones(rows_of(P, f), bool)
        for b in accepted:
            i0, i1 = _range(P, what, b)
            keep[i0:i1] = False
        ok = ok and bool((np.asarray(o[f]).reshape(-1, row)[keep] == np.array(S.FILL, dt)).all())
    return ok


def _finish(P, o):
    res = split(P, o)
    outside = fill_outside(P, o, [b for b, r in enumerate(res) if r["status"] != INVALID])
    for r in res:
        if r["status"] == INVALID:
            r["untouched"] = outside
    return res


def _run_host(fn, scenes, packed, cam):
    P = packed or pack(scenes)
    cam = cam or camera()
    o = S.outputs(capi.CORRECT_LOOP_RESULT_FIELDS, lambda f: out_len(P, f), out_dtype)
    m, r = _map_struct(P), S.struct(capi.CorrectLoopResult, (), capi.CORRECT_LOOP_RESULT_FIELDS, o)
    check(fn(C.byref(m), C.byref(cam), C.byref(r)))
    return _finish(P, o)


def correct_loop(scenes, packed=None, cam=None):
    """viorb_correct_loop (host buffers): one result dict per scene."""
    return _run_host(lib().viorb_correct_loop, scenes, packed, cam)


def correct_loop_host_core(scenes, packed=None, cam=None):
    """viorb_debug_correct_loop_host: map_correct_core.h on the host (no device), the phases of the device form on one thread."""
    return _run_host(lib().viorb_debug_correct_loop_host, scenes, packed, cam)


class CorrectLoopBatch:
    """A packed batch of scenes on the device: run() enqueues viorb_correct_loop_device on torch tensors; results() downloads. The
    result tensors self.o stay on the device for the stages that follow (member_kf, Scw_f12, Scw_out, Smeas_out, pt_corrected_ref_out)."""

    def __init__(self, scenes, device=0, packed=None, cam=None):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.P = P = packed or pack(scenes)
        self.cam = cam or camera()
        self.d = S.upload(P, capi.CORRECT_LOOP_ARRAYS, device)
        self.map = _map_struct(P, self.d)
        self.o = S.outputs(capi.CORRECT_LOOP_RESULT_FIELDS, lambda f: out_len(P, f), out_dtype, torch, self.dev)
        self.res = S.struct(capi.CorrectLoopResult, (), capi.CORRECT_LOOP_RESULT_FIELDS, self.o)
        self._wb = lib().viorb_correct_loop_workspace_bytes(P["batch"], P["n_kf"], P["n_pt"], P["n_obs"])
        self.ws = capi.Workspace(torch, self.dev, self._wb)         # may be re-filled or replaced by a larger one between calls

    def run(self):
        check(lib().viorb_correct_loop_device(C.byref(self.map), C.byref(self.cam), C.byref(self.res), self.ws.ptr, self._wb, S.stream_ptr(self.torch, self.dev)))

    def results(self):
        self.torch.cuda.synchronize(self.dev)
        return _finish(self.P, {f: v.cpu().numpy() for f, v in self.o.items()})


# ---- the map update after a global bundle adjustment (viorb_apply_global_ba) --------------------------------------------------------------------
# A scene: dict(children=[[slots]] per key frame, origins=[slots], kf_in_gba u8 [nk], pose12 / TcwGBA12 f32 [nk][12], ns22 / nsGBA22 f64 [nk][22],
# pt_bad / pt_in_gba u8 [np], Pw / PosGBA f32 [np][3], pt_ref i32 [np]).
AG_BAD, AG_POS_GBA, AG_BY_REF, AG_UNTOUCHED, AG_REF_UNREACHED = 0, 1, 2, 3, 4
_AG_DT = dict(kf_start=np.int32, child_start=np.int32, child_kf=np.int32, origin_start=np.int32, origin_kf=np.int32, kf_in_gba=np.uint8, pose12=np.float32,
              TcwGBA12=np.float32, ns22=np.float64, nsGBA22=np.float64, pt_start=np.int32, pt_bad=np.uint8, pt_in_gba=np.uint8, Pw=np.float32, PosGBA=np.float32,
              pt_ref=np.int32)
AG_OUT = dict(status=("b", 1, np.int32), pose12_out=("k", 12, np.float32), ns22_out=("k", 22, np.float64), TcwBef_out=("k", 12, np.float32), nsBef_out=("k", 22, np.float64),
              TcwGBA_out=("k", 12, np.float32), nsGBA_out=("k", 22, np.float64), kf_in_gba_out=("k", 1, np.uint8), kf_reached=("k", 1, np.uint8),
              Pw_out=("p", 3, np.float32), pt_code=("p", 1, np.uint8))
AG_FIELDS = tuple(f for f in capi.APPLY_GBA_RESULT_FIELDS if f != "status")


def gba_shape():
    o = np.zeros(4, np.int32)
    check(lib().viorb_apply_global_ba_shape(ptr(o)))
    return tuple(int(v) for v in o)


def gba_scene(children, origins, kf_in_gba, pose12, TcwGBA12, ns22, nsGBA22, pt_bad=(), pt_in_gba=(), Pw=(), PosGBA=(), pt_ref=()):
    nk, npt = len(children), len(pt_bad)
    s = dict(origins=np.array(list(origins), np.int32), kf_in_gba=np.array(kf_in_gba, np.uint8), pose12=np.array(pose12, np.float32).reshape(nk, 12),
             TcwGBA12=np.array(TcwGBA12, np.float32).reshape(nk, 12), ns22=np.array(ns22, np.float64).reshape(nk, 22), nsGBA22=np.array(nsGBA22, np.float64).reshape(nk, 22),
             pt_bad=np.array(pt_bad, np.uint8), pt_in_gba=np.array(pt_in_gba, np.uint8), Pw=np.array(Pw, np.float32).reshape(npt, 3),
             PosGBA=np.array(PosGBA, np.float32).reshape(npt, 3), pt_ref=np.array(pt_ref, np.int32))
    s["child_start"], s["child_kf"] = S.csr(children, np.int32)
    return s


def gba_pack(scenes):
    cnt = lambda f: sum(len(s[f]) for s in scenes)
    P = dict(batch=len(scenes), n_kf=cnt("kf_in_gba"), n_child=cnt("child_kf"), n_origin=cnt("origins"), n_pt=cnt("pt_bad"))
    P["kf_start"], P["pt_start"], P["origin_start"] = S.starts([s["kf_in_gba"] for s in scenes]), S.starts([s["pt_bad"] for s in scenes]), S.starts([s["origins"] for s in scenes])
    for f in ("child_kf", "kf_in_gba", "pose12", "TcwGBA12", "ns22", "nsGBA22", "pt_bad", "pt_in_gba", "Pw", "PosGBA", "pt_ref"):
        P[f] = S.cat(scenes, f, _AG_DT[f])
    P["origin_kf"] = S.cat(scenes, "origins", np.int32)
    P["child_start"] = S.rebase(scenes, "child_start", "child_kf")
    return S.finish(P, capi.APPLY_GBA_ARRAYS, _AG_DT)


def _gba_rows(P, f):
    return dict(b=P["batch"], k=max(P["n_kf"], 1), p=max(P["n_pt"], 1))[AG_OUT[f][0]]


def _gba_finish(P, o):
    res, keep = [], {f: np.ones(_gba_rows(P, f), bool) for f in AG_FIELDS}
    for b in range(P["batch"]):
        r = dict(status=int(o["status"][b]))
        if r["status"] != INVALID:
            for f in AG_FIELDS:
                what, row, _ = AG_OUT[f]
                i0, i1 = _range(P, what, b)
                a = np.asarray(o[f])[i0 * row:i1 * row]
                r[f] = a.reshape(i1 - i0, row) if row > 1 else a
                keep[f][i0:i1] = False
        res.append(r)
    outside = all(bool((np.asarray(o[f]).reshape(-1, AG_OUT[f][1])[keep[f]] == np.array(S.FILL, AG_OUT[f][2])).all()) for f in AG_FIELDS)
    for r in res:
        if r["status"] == INVALID:
            r["untouched"] = outside
    return res


def _gba_struct(P, arrays=None):
    return S.struct(capi.ApplyGbaMap, capi.APPLY_GBA_INTS, capi.APPLY_GBA_ARRAYS, P, arrays)


def _gba_run_host(fn, scenes, Tbc12, packed):
    P = packed or gba_pack(scenes)
    T = np.ascontiguousarray(Tbc12, np.float32).reshape(12)
    o = S.outputs(capi.APPLY_GBA_RESULT_FIELDS, lambda f: _gba_rows(P, f) * AG_OUT[f][1], lambda f: AG_OUT[f][2])
    m, r = _gba_struct(P), S.struct(capi.ApplyGbaResult, (), capi.APPLY_GBA_RESULT_FIELDS, o)
    check(fn(C.byref(m), ptr(T), C.byref(r)))
    return _gba_finish(P, o)


def apply_global_ba(scenes, Tbc12, packed=None):
    """viorb_apply_global_ba (host buffers): one result dict per scene."""
    return _gba_run_host(lib().viorb_apply_global_ba, scenes, Tbc12, packed)


def apply_global_ba_host_core(scenes, Tbc12, packed=None):
    """viorb_debug_apply_global_ba_host: the core header on the host (no device)."""
    return _gba_run_host(lib().viorb_debug_apply_global_ba_host, scenes, Tbc12, packed)


class ApplyGbaBatch:
    """A packed batch of scenes on the device: run() enqueues viorb_apply_global_ba_device on torch tensors; results() downloads."""

    def __init__(self, scenes, Tbc12, device=0, packed=None):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.P = P = packed or gba_pack(scenes)
        self.Tbc = np.ascontiguousarray(Tbc12, np.float32).reshape(12)
        self.d = S.upload(P, capi.APPLY_GBA_ARRAYS, device)
        self.map = _gba_struct(P, self.d)
        self.o = S.outputs(capi.APPLY_GBA_RESULT_FIELDS, lambda f: _gba_rows(P, f) * AG_OUT[f][1], lambda f: AG_OUT[f][2], torch, self.dev)
        self.res = S.struct(capi.ApplyGbaResult, (), capi.APPLY_GBA_RESULT_FIELDS, self.o)
        self._wb = lib().viorb_apply_global_ba_workspace_bytes(P["batch"], P["n_kf"])
        self.ws = capi.Workspace(torch, self.dev, self._wb)

    def run(self):
        check(lib().viorb_apply_global_ba_device(C.byref(self.map), ptr(self.Tbc), C.byref(self.res), self.ws.ptr, self._wb, S.stream_ptr(self.torch, self.dev)))

    def results(self):
        self.torch.cuda.synchronize(self.dev)
        return _gba_finish(self.P, {f: v.cpu().numpy() for f, v in self.o.items()})
