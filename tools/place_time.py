"""Time of the key-frame database query (viorb_kfdb_query_device) for N key frames of ~800 words over 10^6 words and n_q queries per
call, and of viorb_bow_vector_device at 1000 features x 1 and x 256 frames.
  call     ms per query call from device events around it, median of --reps after warm-up (loop mode; the queries revisit the first places);
  kernels  the per-kernel split from viorb_profile_* in a separate run of the same call (an event pair per launch adds ~8 us);
  floor    the byte model: pass 1 (k_kfdb_common) reads 4 B per stored word and query, scoring (k_kfdb_score) reads 12 B per entry of the
           scored key frames only; each against HBM_BYTES_PER_S (the measured copy rate). Pass 1 is expected to sit far above its floor:
           every word costs a binary search in LDS.
Prints one JSON line per configuration. Needs a HIP device (no fallback)."""
import argparse
import ctypes as C
import json
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viorb_amd
from viorb_amd import place
from viorb_amd.capi import ptr, check

HBM_BYTES_PER_S = 6.29e12          # float4 copy, measured
N_WORDS = 1000000
PLACE_LEN, POOL, FROM_POOL, ANYWHERE = 12, 1600, 560, 280


def profile():
    L = viorb_amd.lib()
    names = C.create_string_buffer(8192); ms = (C.c_double * 64)(); calls = (C.c_int * 64)(); n = C.c_int()
    L.viorb_profile_read(names, 8192, ms, calls, 64, C.byref(n))
    return {nm: (ms[i], calls[i]) for i, nm in enumerate(names.value.decode().split("\n")[:n.value])}


def make_bows(rng, pools, places):
    """word [n, cap] int32 ascending, val [n, cap] float64 (rows sum to 1), count [n]: FROM_POOL draws from the place's pool, ANYWHERE from anywhere."""
    n = len(places)
    w = np.concatenate([pools[places[:, None], rng.integers(0, POOL, (n, FROM_POOL))], rng.integers(0, N_WORDS, (n, ANYWHERE))], axis=1)
    w.sort(axis=1)
    w[:, 1:][w[:, 1:] == w[:, :-1]] = N_WORDS                      # duplicates to the end
    w.sort(axis=1)
    count = (w < N_WORDS).sum(axis=1).astype(np.int32)
    v = rng.uniform(0.05, 8.0, w.shape) * (w < N_WORDS)
    v /= v.sum(axis=1, keepdims=True)
    w[w >= N_WORDS] = 0
    return w.astype(np.int32), v, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024, 4096, 16384])
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    L = viorb_amd.lib()
    if L.viorb_device_count() < 1:
        raise SystemExit("place_time.py needs a HIP device")
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(1)

    def timed(fn, reps):
        ms = []
        for rep in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            if rep >= 2:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    for frames in (1, 256):
        n = 1000
        word, weight = up(rng.integers(0, N_WORDS, (frames, n)).astype(np.int32)), up(rng.uniform(0.05, 8.0, (frames, n)))
        count = torch.full((frames,), n, dtype=torch.int32, device=dev)
        bw, bv, bc = torch.zeros_like(word), torch.zeros_like(weight), torch.zeros_like(count)
        med, mn = timed(lambda: check(L.viorb_bow_vector_device(ptr(word), ptr(weight), ptr(count), n, frames, ptr(bw), ptr(bv), ptr(bc), st)), a.reps)
        print(json.dumps({"what": "viorb_bow_vector_device", "features": n, "frames": frames, "ms_median": med, "ms_min": mn}), flush=True)

    for N in a.sizes:
        n_places = (N + PLACE_LEN - 1) // PLACE_LEN
        pools = rng.integers(0, N_WORDS, (n_places, POOL))
        w, v, c = make_bows(rng, pools, np.arange(N) // PLACE_LEN)
        db = place.KeyFrameDatabase(N_WORDS, kf_capacity_hint=N, entry_capacity_hint=int(c.sum()))
        db.add_device(up(w), up(v), up(c))
        near = np.arange(N)[:, None] + np.array([-1, 1, -2, 2, -3, 3, -4, 4, -5, 5])[None, :]
        covis = up(np.where((near >= 0) & (near < N), near, -1).astype(np.int32))
        for n_q in a.queries:
            qw, qv, qc = make_bows(rng, pools, np.arange(n_q) % n_places)          # the queries look at the first places again
            q_word, q_val, q_count = up(qw), up(qv), up(qc)
            q_cap = qw.shape[1]
            min_score = torch.full((n_q,), 0.02, dtype=torch.float32, device=dev)
            conn = np.arange(N - 6, N, dtype=np.int32)                             # the last six key frames are connected to every query
            es, ex = up((np.arange(n_q + 1) * len(conn)).astype(np.int32)), up(np.tile(conn, n_q))
            cand_cap = 64
            cand, ncand, stats = torch.zeros((n_q, cand_cap), dtype=torch.int32, device=dev), torch.zeros(n_q, dtype=torch.int32, device=dev), torch.zeros((n_q, 4), dtype=torch.int32, device=dev)
            wb = int(L.viorb_kfdb_query_workspace_bytes(db.h, n_q))
            ws = torch.empty(wb + 256, dtype=torch.uint8, device=dev)
            wp = C.c_void_p((ws.data_ptr() + 255) & ~255)
            call = lambda: check(L.viorb_kfdb_query_device(db.h, place.LOOP, n_q, ptr(q_word), ptr(q_val), ptr(q_count), q_cap, ptr(min_score), ptr(es), ptr(ex), ptr(covis),
                                                           cand_cap, ptr(cand), ptr(ncand), ptr(stats), None, None, wp, wb, st))
            med, mn = timed(call, a.reps)
            torch.cuda.synchronize(); L.viorb_profile_select(None); L.viorb_profile_reset(); L.viorb_profile_enable(1)
            for _ in range(a.reps):
                call()
            torch.cuda.synchronize(); L.viorb_profile_enable(0)
            kern = {k: round(t / max(n, 1), 4) for k, (t, n) in profile().items() if k.startswith("k_kfdb")}
            L.viorb_profile_reset()
            s = stats.cpu().numpy()
            scored_entries = float(s[:, 2].sum()) * float(c.mean())
            floor1 = 4.0 * float(c.sum()) * n_q / HBM_BYTES_PER_S * 1e3
            floor3 = 12.0 * scored_entries / HBM_BYTES_PER_S * 1e3
            print(json.dumps({"what": "viorb_kfdb_query_device", "key_frames": N, "n_q": n_q, "stored_words": int(c.sum()), "words_per_kf": round(float(c.mean()), 1),
                              "call_ms_median": med, "call_ms_min": mn, "call_ms_per_query": med / n_q, "kernel_ms": kern,
                              "common_hbm_floor_ms": round(floor1, 5), "common_over_floor": round(kern.get("k_kfdb_common", 0.0) / floor1, 1),
                              "score_hbm_floor_ms": round(floor3, 6), "score_over_floor": round(kern.get("k_kfdb_score", 0.0) / max(floor3, 1e-9), 1),
                              "sharing_max_scored_kept_q0": s[0].tolist(), "candidates_q0": int(ncand[0].item())}), flush=True)
        db.close()


if __name__ == "__main__":
    main()
