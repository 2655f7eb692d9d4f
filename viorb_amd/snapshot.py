"""What the wrappers of the map-reading stages (culling.py, local_map.py) share: laying a list of per-stream scenes out as the flat arrays
of a batched snapshot (stream-local offsets and indices, DESIGN.md "Map snapshots"), the ctypes structs over host or device arrays, the
result arrays with their fill value, and the file that the host test programs' `time` mode reads."""
import ctypes as C
import numpy as np
from .capi import ptr, _torch_up as _up

FILL = 77           # what every result array holds before a call: a refused stream's ranges still hold it afterwards


def starts(lists):
    """Offsets i32 [n + 1] of n lists laid end to end; the last is the total."""
    return np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)


def cat(scenes, f, dtype):
    """Field f of every scene, flattened and concatenated."""
    return np.concatenate([np.asarray(s[f], dtype).reshape(-1) for s in scenes]) if scenes else np.zeros(0, dtype)


def rebase(scenes, f, src):
    """The nested offsets f of every scene (into its field src) as offsets into the batch's src: each scene's last entry dropped, its
    base added, the total appended."""
    base = starts([s[src] for s in scenes])
    return np.concatenate([np.asarray(s[f][:-1], np.int32) + base[b] for b, s in enumerate(scenes)] + [base[-1:]]).astype(np.int32)


def csr(lists, dtype, item=lambda x: x):
    """(start i32 [n + 1], flat array of item(x)) from n lists."""
    return starts(lists), np.array([item(x) for l in lists for x in l], dtype)


def finish(P, arrays, dtypes):
    """Every named array of P flat, contiguous and at least one element long (the library refuses a null pointer whatever the count);
    P["length"] keeps the lengths before that."""
    P["length"] = {}
    for f in arrays:
        a = np.ascontiguousarray(P[f], dtypes[f]).reshape(-1)
        P["length"][f], P[f] = len(a), a if len(a) else np.zeros(1, dtypes[f])
    return P


def struct(cls, ints, arrays, P, where=None):
    """The ctypes struct cls(ints..., arrays...) with the totals of P and pointers to the arrays of `where` (host or device; default P)."""
    return cls(*([P[f] for f in ints] + [ptr((where or P)[f]) for f in arrays]))


def upload(P, arrays, device):
    """The named arrays of P as device tensors (uint32 as its int32 view)."""
    return {f: _up(P[f].view(np.int32) if P[f].dtype == np.uint32 else P[f], device) for f in arrays}


def outputs(fields, length, dtype, torch=None, dev=None):
    """{f: FILL [length(f)] of dtype(f)} for a result struct's fields: numpy arrays or, given torch and dev, device tensors."""
    if torch is None:
        return {f: np.full(length(f), FILL, dtype(f)) for f in fields}
    return {f: torch.full((length(f),), FILL, dtype=getattr(torch, np.dtype(dtype(f)).name), device=dev) for f in fields}


def stream_ptr(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def write_snapshot(path, header, P, arrays):
    """The file of the host test programs' `time` mode: the header as int32, then every array without the padding of finish()."""
    with open(path, "wb") as f:
        f.write(np.array(header, np.int32).tobytes())
        for k in arrays:
            f.write(P[k][:P["length"][k]].tobytes())
