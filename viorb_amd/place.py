"""Place recognition through the C ABI of include/viorb.h: the BowVector of a frame, ORBVocabulary::score and the key-frame database
(KeyFrameDatabase::add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates, reference src/KeyFrameDatabase.cc:40-309).
A BoW vector is a pair (ids int32 ascending, vals float64); covis10 is an [n_slots, 10] int array of GetBestCovisibilityKeyFrames(10)
as slots, padded with -1. Host forms take numpy arrays; the *_device forms take torch tensors on the GPU and only enqueue work."""
import ctypes as C
import numpy as np
from . import capi
from .capi import lib, check, ptr

LOOP, RELOC = 0, 1
BOW_VECTOR_MAX_FEATURES = 8192

_i32 = lambda a: np.ascontiguousarray(a, np.int32)
_f64 = lambda a: np.ascontiguousarray(a, np.float64)


def _stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def BowVector(word, weight):
    """BowVector::addWeight + normalize(L1) of one frame from the transform's per-feature word / weight: (ids, vals)."""
    word, weight = _i32(word).ravel(), _f64(weight).ravel()
    n = len(word)
    ids, vals, cnt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1)), C.c_int(0)
    check(lib().viorb_bow_vector(ptr(word), ptr(weight), n, ptr(ids), ptr(vals), C.byref(cnt)))
    return ids[:cnt.value].copy(), vals[:cnt.value].copy()


def BowVector_device(word, weight, count):
    """viorb_bow_vector_device on torch tensors word / weight [batch, cap], count [batch]: (bow_word, bow_val, bow_count) tensors."""
    import torch
    batch, cap = word.shape
    bw, bv = torch.zeros_like(word), torch.zeros_like(weight)
    bc = torch.zeros(batch, dtype=torch.int32, device=word.device)
    check(lib().viorb_bow_vector_device(ptr(word), ptr(weight), ptr(count), cap, batch, ptr(bw), ptr(bv), ptr(bc), _stream(word)))
    return bw, bv, bc


def pack_bows(bows, cap=None):
    """A list of (ids, vals) as word [n, cap] int32, val [n, cap] float64, count [n] int32."""
    cap = max([cap or 1] + [len(b[0]) for b in bows])
    w, v, c = np.zeros((len(bows), cap), np.int32), np.zeros((len(bows), cap)), np.zeros(len(bows), np.int32)
    for i, b in enumerate(bows):
        c[i] = len(b[0]); w[i, :c[i]] = b[0]; v[i, :c[i]] = b[1]
    return w, v, c


def BowScorePairs(a_bows, b_bows, pairs):
    """ORBVocabulary::score(a_bows[i], b_bows[j]) for every (i, j) of pairs, one call: float64 [len(pairs)]."""
    aw, av, ac = pack_bows(a_bows)
    bw, bv, bc = pack_bows(b_bows)
    pairs = _i32(pairs).reshape(-1, 2)
    pa, pb = _i32(pairs[:, 0]), _i32(pairs[:, 1])
    out = np.zeros(max(len(pairs), 1))
    check(lib().viorb_bow_score(ptr(aw), ptr(av), ptr(ac), aw.shape[1], len(a_bows), ptr(bw), ptr(bv), ptr(bc), bw.shape[1], len(b_bows),
                                ptr(pa), ptr(pb), len(pairs), ptr(out)))
    return out[:len(pairs)]


def BowScore(a, b):
    """ORBVocabulary::score(a, b) of two BoW vectors."""
    return float(BowScorePairs([a], [b], [(0, 0)])[0])


class KeyFrameDatabase:
    """KeyFrameDatabase of the reference over slots: add returns the key frame's slot (add order, never reused), the caller keeps the map
    KeyFrame <-> slot. One instance per map, used from one stream at a time."""

    def __init__(self, n_words, kf_capacity_hint=0, entry_capacity_hint=0):
        h = C.c_void_p()
        check(lib().viorb_kfdb_create(int(n_words), int(kf_capacity_hint), int(entry_capacity_hint), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().viorb_kfdb_destroy(self.h); self.h = None

    __del__ = close

    def add(self, bow):
        ids, vals = _i32(bow[0]).ravel(), _f64(bow[1]).ravel()
        slot = C.c_int(-1)
        check(lib().viorb_kfdb_add(self.h, ptr(ids), ptr(vals), len(ids), C.byref(slot)))
        return slot.value

    def add_device(self, bow_word, bow_val, bow_count):
        """Appends bow_word.shape[0] key frames from device tensors [n, cap] / [n] (BowVector_device's outputs): the first new slot."""
        n, cap = bow_word.shape
        first = C.c_int(-1)
        check(lib().viorb_kfdb_add_device(self.h, ptr(bow_word), ptr(bow_val), ptr(bow_count), cap, n, C.byref(first), _stream(bow_word)))
        return first.value

    def erase(self, slot):
        check(lib().viorb_kfdb_erase(self.h, int(slot)))

    def clear(self):
        check(lib().viorb_kfdb_clear(self.h))

    def size(self):
        """(slots handed out, slots alive)"""
        a, b = C.c_int(0), C.c_int(0)
        check(lib().viorb_kfdb_size(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @staticmethod
    def _csr(lists, n_q):
        start = np.zeros(n_q + 1, np.int32)
        for q in range(n_q):
            start[q + 1] = start[q] + len(lists[q])
        flat = _i32([s for l in lists for s in l]) if start[n_q] else np.zeros(1, np.int32)
        return start, flat

    def query(self, mode, bows, covis10, min_scores=None, connected=None, cand_cap=None):
        """viorb_kfdb_query for a list of BoW vectors: dict(cand = one list of slots per query in the reference's output order, stats
        [n_q, 4], common [n_q, n_slots], score [n_q, n_slots] float32 with -1 where not scored)."""
        n_q, S = len(bows), self.size()[0]
        qw, qv, qc = pack_bows(bows)
        cand_cap = int(cand_cap or max(S, 1))
        cov = _i32(covis10).reshape(-1, 10) if S else np.full((1, 10), -1, np.int32)
        if len(cov) != max(S, 1):
            raise ValueError("covis10 must have one row per slot")
        ms = np.ascontiguousarray(min_scores if min_scores is not None else np.zeros(n_q), np.float32)
        start, flat = self._csr(connected if connected is not None else [[]] * n_q, n_q)
        cand, ncand = np.full((max(n_q, 1), cand_cap), -1, np.int32), np.zeros(max(n_q, 1), np.int32)
        stats = np.zeros((max(n_q, 1), 4), np.int32)
        common, score = np.zeros((max(n_q, 1), max(S, 1)), np.int32), np.full((max(n_q, 1), max(S, 1)), -1, np.float32)
        loop = mode == LOOP
        check(lib().viorb_kfdb_query(self.h, int(mode), n_q, ptr(qw), ptr(qv), ptr(qc), qw.shape[1], ptr(ms) if loop else None, ptr(start) if loop else None,
                                     ptr(flat) if loop else None, ptr(cov), cand_cap, ptr(cand), ptr(ncand), ptr(stats), ptr(common), ptr(score)))
        return dict(cand=[cand[q, :ncand[q]].tolist() for q in range(n_q)], stats=stats[:n_q], common=common[:n_q, :S], score=score[:n_q, :S])

    def query_device(self, mode, q_word, q_val, q_count, covis10, min_scores=None, excl_start=None, excl_slot=None, cand_cap=64, want_rows=True, workspace=None):
        """viorb_kfdb_query_device on torch tensors (q_word / q_val [n_q, q_cap], q_count [n_q], covis10 [n_slots, 10] int32, loop mode:
        min_scores float32 [n_q], excl_start int32 [n_q + 1], excl_slot int32): dict of device tensors cand [n_q, cand_cap], n_cand, stats,
        common, score. Nothing is copied to the host and the stream is not waited for, also after adds and erasures (they reach the
        device's alive[] by memsets on the same stream). workspace: a capi.Workspace at least as large as the query needs, used as it is;
        default: a fresh one, not cleared."""
        import torch
        n_q, q_cap = q_word.shape
        S, dev = self.size()[0], q_word.device
        z = lambda shape, dt, fill=0: torch.full(shape, fill, dtype=dt, device=dev)
        cand, ncand, stats = z((n_q, cand_cap), torch.int32, -1), z((n_q,), torch.int32), z((n_q, 4), torch.int32)
        common = z((n_q, max(S, 1)), torch.int32) if want_rows else None
        score = z((n_q, max(S, 1)), torch.float32, -1.0) if want_rows else None
        wb = int(lib().viorb_kfdb_query_workspace_bytes(self.h, n_q))
        ws = workspace if workspace is not None else capi.Workspace(torch, dev, wb, fill=None)
        assert ws.fits(wb)
        check(lib().viorb_kfdb_query_device(self.h, int(mode), n_q, ptr(q_word), ptr(q_val), ptr(q_count), q_cap, ptr(min_scores), ptr(excl_start), ptr(excl_slot),
                                            ptr(covis10), int(cand_cap), ptr(cand), ptr(ncand), ptr(stats), ptr(common), ptr(score), ws.ptr, wb,
                                            _stream(q_word)))
        return dict(cand=cand, n_cand=ncand, stats=stats, common=common, score=score, workspace=ws.tensor)

    def detect_loop_candidates(self, bow, min_score, connected, covis10):
        """DetectLoopCandidates(pKF, minScore): the candidate slots in the reference's order. connected = GetConnectedKeyFrames() as slots."""
        return self.query(LOOP, [bow], covis10, [min_score], [list(connected)])["cand"][0]

    def detect_relocalization_candidates(self, bow, covis10):
        """DetectRelocalizationCandidates(F): the candidate slots in the reference's order."""
        return self.query(RELOC, [bow], covis10)["cand"][0]
