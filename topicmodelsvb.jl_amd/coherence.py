"""
Topic coherence on the device: whether the top words of a topic occur together in documents (the reference has no such function).

    codocfreq_raw(ctx, M, V, doc_ptr, terms, counts, top, max_bitset_bytes=0)   -> (status, dict | message): the ABI call itself
    coherence_from_counts(codf, M)                                              -> (umass[K], npmi[K], undefined_pairs[K]); host only
    coherence(model_or_top, corp, topn=10, ...)                                 -> CoherenceResult

codf[k][i][j] is the number of documents of `corp` that contain both the i-th and the j-th top word of topic k (only presence matters;
the diagonal is the document frequency).  The integers come from libtmvb_hip.so (tmvb_corpus_codocfreq, include/tmvb.h: a bit matrix
over the corpus, AND / popcount over pairs), are exact and additive over document shards; UMass (Mimno et al. 2011, as a mean over the
defined pairs) and NPMI with the document as the window (Lau et al. 2014) are fp64 host arithmetic on them (tmvb_coherence_from_counts).
There is no CPU fallback for the counts.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import CodfInfo  # noqa: F401 (re-exported)
from ._lib import CorpusError, _csr, _handle, check, lib, P_dbl, P_i32, P_i64
from .lda import _packed, call_context

CODF_CHUNK_DOCS = 4096              # TMVB_CODF_CHUNK_DOCS (include/tmvb.h): documents per workgroup of the pair pass
TOPN_MIN, TOPN_MAX = 2, 64


class CoherenceResult:
    """codf[K, N, N] (int64), df[K, N] (its diagonals), umass[K], npmi[K], undefined_pairs[K] (pairs UMass skipped: the higher-ranked word
    occurs in no document; umass is nan where every pair is undefined), diversity = distinct ids of top / (K N), ms = device time of the two
    kernels; mean_umass / mean_npmi: nan-aware means over topics."""

    def __init__(self, top, codf, umass, npmi, undefined_pairs, ms=None, n_slots=0, n_batches=0):
        self.top = np.asarray(top, dtype=np.int64)
        self.codf = np.asarray(codf, dtype=np.int64)
        self.df = np.ascontiguousarray(np.diagonal(self.codf, axis1=1, axis2=2))
        self.umass = np.asarray(umass, dtype=np.float64)
        self.npmi = np.asarray(npmi, dtype=np.float64)
        self.undefined_pairs = np.asarray(undefined_pairs, dtype=np.int64)
        self.diversity = len(np.unique(self.top)) / self.top.size
        self.ms = dict(ms or {})
        self.n_slots, self.n_batches = int(n_slots), int(n_batches)

    @staticmethod
    def _nanmean(x):
        ok = ~np.isnan(x)
        return float(x[ok].mean()) if ok.any() else float("nan")

    @property
    def mean_umass(self) -> float:
        return self._nanmean(self.umass)

    @property
    def mean_npmi(self) -> float:
        return self._nanmean(self.npmi)

    def __repr__(self):
        K, N = self.top.shape
        return f"CoherenceResult(K={K}, N={N}, mean_umass={self.mean_umass:.6g}, mean_npmi={self.mean_npmi:.6g}, diversity={self.diversity:.3g})"


def codocfreq_raw(ctx, M, V, doc_ptr, terms, counts, top, max_bitset_bytes=0):
    """The ABI call tmvb_corpus_codocfreq.  ctx: a DeviceContext, or None for a NULL context (the library then answers TMVB_ENODEVICE on a
    machine without a GPU); top: K x N 0-based term ids.  Returns (status, dict) or (status, message): nothing raises here."""
    L = lib()
    doc_ptr, terms, counts = _csr(doc_ptr, terms, counts)
    top = np.ascontiguousarray(top, dtype=np.int32)
    if top.ndim != 2:
        return 1, "codocfreq_raw: top must be a K x N array"
    K, N = top.shape
    codf = np.zeros((max(K, 1), max(N, 1), max(N, 1)), dtype=np.int64)
    info = CodfInfo()
    rc = L.tmvb_corpus_codocfreq(_handle(ctx), int(M), int(V), doc_ptr.ctypes.data_as(P_i64), terms.ctypes.data_as(P_i32),
                                 counts.ctypes.data_as(P_i32), K, N, top.ctypes.data_as(P_i32), int(max_bitset_bytes),
                                 codf.ctypes.data_as(P_i64), C.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"codf": codf[:K, :N, :N], "n_slots": int(info.n_slots), "n_batches": int(info.n_batches),
                "ms": {"bitset": float(info.ms_bitset), "pairs": float(info.ms_pairs)}}


def coherence_from_counts_raw(K, N, M, codf):
    """The ABI call tmvb_coherence_from_counts on a flat or shaped int64 array.  Returns (status, (umass, npmi, undefined_pairs)) or
    (status, message): nothing raises here."""
    L = lib()
    codf = np.ascontiguousarray(codf, dtype=np.int64)
    n = max(int(K), 1)
    umass, npmi, undef = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    rc = L.tmvb_coherence_from_counts(int(K), int(N), int(M), codf.ctypes.data_as(P_i64), umass.ctypes.data_as(P_dbl),
                                      npmi.ctypes.data_as(P_dbl), undef.ctypes.data_as(P_i32))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    K = int(K)
    return rc, (umass[:K], npmi[:K], undef[:K].astype(np.int64))


def coherence_from_counts(codf, M):
    """(umass[K], npmi[K], undefined_pairs[K]) of co-document counts codf[K, N, N] over M documents (the counts of several shards summed,
    with M the total): host arithmetic, needs no device."""
    codf = np.asarray(codf)
    if codf.ndim != 3 or codf.shape[1] != codf.shape[2]:
        raise ValueError(f"codf must be K x N x N, got {codf.shape}.")
    rc, res = coherence_from_counts_raw(codf.shape[0], codf.shape[1], M, codf)
    check(rc)
    return res


def _top_of(model_or_top, topn):
    """K x N 0-based ids: the first topn entries of every row of a model's `topics` (the mirror stores them 1-based, like the reference), or
    an explicit integer array taken as it is"""
    if hasattr(model_or_top, "topics"):
        topics = model_or_top.topics
        if topn > min(len(t) for t in topics):
            raise ValueError(f"topn = {topn} above the vocabulary size.")
        return np.array([np.asarray(t)[:topn] for t in topics], dtype=np.int64) - 1
    top = np.asarray(model_or_top)
    if top.ndim != 2 or not np.issubdtype(top.dtype, np.integer):
        raise ValueError("top must be a K x N array of 0-based integer term ids (or a model with a `topics` field).")
    if not TOPN_MIN <= top.shape[1] <= TOPN_MAX:
        raise ValueError(f"top must hold between {TOPN_MIN} and {TOPN_MAX} ids per topic, got {top.shape[1]}.")
    return top.astype(np.int64)


def coherence(model_or_top, corp, topn: int = 10, device_id: int = 0, max_bitset_bytes: int = 0) -> CoherenceResult:
    """Coherence of the topics of a trained model (LDA, fLDA, CTM, fCTM, CTPF or their gpu forms: the first `topn` ids of every row of
    `model.topics`) or of an explicit K x N array of 0-based term ids, against the reference corpus `corp` (a Corpus or a PackedCorpus; for a
    model it must have the model's vocabulary size, else CorpusError).  topn outside [2, 64] raises ValueError."""
    if not (isinstance(topn, (int, np.integer)) and TOPN_MIN <= topn <= TOPN_MAX):
        raise ValueError(f"topn must be an integer in [{TOPN_MIN}, {TOPN_MAX}].")
    pc = _packed(corp)
    if hasattr(model_or_top, "topics") and pc.V != model_or_top.V:
        raise CorpusError("coherence corpus and model must have identical vocabularies.")
    top = _top_of(model_or_top, int(topn))
    with call_context(device_id) as ctx:
        rc, res = codocfreq_raw(ctx, pc.M, pc.V, pc.doc_ptr, pc.terms, pc.counts, top, max_bitset_bytes)
    check(rc)
    umass, npmi, undef = coherence_from_counts(res["codf"], pc.M)
    return CoherenceResult(top, res["codf"], umass, npmi, undef, res["ms"], res["n_slots"], res["n_batches"])
