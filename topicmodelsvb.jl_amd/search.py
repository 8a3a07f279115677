"""
Search documents by words: which documents are about *mitochondria membrane transport* (the reference has no such function).

    search_raw(ctx, K, V, theta, beta, q_ptr, q_terms, q_counts, n=10, laplace_smooth=0.0, splits=0)  -> (status, dict | message): the ABI call
    pack_queries(model, queries, skip_unknown=False)                                                  -> (q_ptr, q_terms 0-based, q_counts)
    search(model, queries, topn=10, laplace_smooth=0.0, theta=None, skip_unknown=False)               -> SearchResult

The score is the query likelihood of LDA-based retrieval (Wei & Croft 2006): score(q, d) = sum_j c_j log(sum_k Theta[k, d] beta'[k, w_j]),
beta' = (beta + laplace_smooth) / (1 + laplace_smooth V) -- heldout_loglik with the roles turned round: one short "held-out document",
every training document's Theta.  Scores and selection come from libtmvb_hip.so (tmvb_topic_search, include/tmvb.h: probabilities on the
f32 MFMA, logarithm and sum in fp64, the n best per query under the total order (score descending, index ascending) selected in the
epilogue; neither the probability matrix nor the score matrix ever exists).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import SearchInfo, TopicModelError, _handle, check, lib, P_dbl, P_f32, P_i32, P_i64
from .lda import call_context
from .neighbors import TOPN_MAX, topic_proportions

TILE_COLS = 128                         # TMVB_SEARCH_TILE_COLS: query entries per column tile; also the most entries one query may have


class SearchResult:
    """idx[Q, n] (0-based documents, best first; -1 past count), score[Q, n] (fp32 log-likelihood of the query under the document; -inf where
    a word has probability 0, and past count), count[Q] = min(n, M), loglik_per_token[Q, n] = score / (the query's sum of counts), info =
    {"splits", "kp", "col_tiles", "ms": {"prep", "scan", "merge"}} (device time of the three kernels)."""

    def __init__(self, idx, score, count, tokens, info=None):
        self.idx = np.asarray(idx, dtype=np.int32)
        self.score = np.asarray(score, dtype=np.float32)
        self.count = np.asarray(count, dtype=np.int32)
        self.tokens = np.asarray(tokens, dtype=np.int64)
        self.loglik_per_token = self.score.astype(np.float64) / self.tokens[:, None].astype(np.float64)
        self.info = dict(info or {})

    def __repr__(self):
        return f"SearchResult(Q={self.idx.shape[0]}, n={self.idx.shape[1]})"


def search_raw(ctx, K, V, theta, beta, q_ptr, q_terms, q_counts, n=10, laplace_smooth=0.0, splits=0, Q=None):
    """The ABI call tmvb_topic_search.  ctx: a DeviceContext, or None for a NULL context (the library then answers TMVB_ENODEVICE on a machine
    without a GPU); theta: K x Md, beta: K x V; the queries as a CSR (q_terms 0-based).  Q: the number of queries, by default
    len(q_ptr) - 1.  Returns (status, dict) or (status, message): nothing raises here."""
    L = lib()
    f64 = lambda a: np.asfortranarray(np.asarray(a, dtype=np.float64))
    theta, beta = f64(theta), f64(beta)
    if theta.ndim != 2 or beta.ndim != 2:
        return 1, "search_raw: theta must be a K x Md array and beta a K x V array"
    Md = theta.shape[1]
    q_ptr = np.ascontiguousarray(q_ptr, dtype=np.int64)
    q_terms = np.ascontiguousarray(q_terms, dtype=np.int32)
    q_counts = np.ascontiguousarray(q_counts, dtype=np.int32)
    Q = len(q_ptr) - 1 if Q is None else int(Q)
    rows, cols = max(Q, 1), max(int(n), 1)
    idx = np.zeros((rows, cols), dtype=np.int32)
    score = np.zeros((rows, cols), dtype=np.float32)
    count = np.zeros(rows, dtype=np.int32)
    info = SearchInfo()
    rc = L.tmvb_topic_search(_handle(ctx), int(K), int(V), Md, theta.ctypes.data_as(P_dbl), beta.ctypes.data_as(P_dbl),
                             float(laplace_smooth), Q, q_ptr.ctypes.data_as(P_i64), q_terms.ctypes.data_as(P_i32),
                             q_counts.ctypes.data_as(P_i32), int(n), int(splits), idx.ctypes.data_as(P_i32), score.ctypes.data_as(P_f32),
                             count.ctypes.data_as(P_i32), C.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"idx": idx[:Q, :n], "score": score[:Q, :n], "count": count[:Q], "splits": int(info.splits), "kp": int(info.kp),
                "col_tiles": int(info.col_tiles), "ms": {"prep": float(info.ms_prep), "scan": float(info.ms_scan), "merge": float(info.ms_merge)}}


def _vocab_index(model):
    """name -> 1-based key of the model's vocabulary: model.corp.vocab where the corpus carries one, else the names "1" .. "V" that
    PackedCorpus.to_corpus gives"""
    vocab = getattr(getattr(model, "corp", None), "vocab", None)
    if vocab:
        return {str(name): int(key) for key, name in vocab.items()}
    return {str(v): v for v in range(1, int(model.V) + 1)}


def pack_queries(model, queries, skip_unknown: bool = False):
    """The queries as the CSR the ABI takes: (q_ptr int64[Q + 1], q_terms int32 0-based, q_counts int32).  Each query is a list of vocabulary
    strings (resolved through the model's vocabulary; an unknown word raises ValueError unless skip_unknown), a list of 1-based term ids,
    or a dict term -> count (terms as strings or 1-based ids).  Repeated terms are merged by summing their counts, in the order of their
    first occurrence.  A query without a term left, one of more than 128 distinct terms, an id outside [1, V] or a count below 1 raise
    ValueError."""
    if isinstance(queries, (str, bytes, dict)) or not hasattr(queries, "__len__"):
        raise ValueError("queries must be a list of queries (each a list of words, a list of 1-based term ids, or a dict term -> count).")
    V = int(model.V)
    names = None
    ptr, terms, counts = [0], [], []
    for qi, q in enumerate(queries):
        if isinstance(q, (str, bytes)):
            raise ValueError(f"query {qi + 1} is a string: a query is a list of words (split it first).")
        items = list(q.items()) if isinstance(q, dict) else [(t, 1) for t in q]
        merged = {}
        for t, c in items:
            if isinstance(t, (str, bytes)):
                if names is None:
                    names = _vocab_index(model)
                key = names.get(t.decode() if isinstance(t, bytes) else t)
                if key is None:
                    if skip_unknown:
                        continue
                    raise ValueError(f"query {qi + 1}: word {t!r} is not in the model's vocabulary.")
            elif isinstance(t, (int, np.integer)) and not isinstance(t, bool):
                key = int(t)
                if not 1 <= key <= V:
                    raise ValueError(f"query {qi + 1}: term id {key} outside [1, {V}].")
            else:
                raise ValueError(f"query {qi + 1}: a term must be a vocabulary string or a 1-based integer id, not {type(t).__name__}.")
            if not (isinstance(c, (int, np.integer)) and not isinstance(c, bool) and c >= 1):
                raise ValueError(f"query {qi + 1}: the count of term {t!r} must be a positive integer.")
            merged[key] = merged.get(key, 0) + int(c)
        if not merged:
            raise ValueError(f"query {qi + 1} is empty.")
        if len(merged) > TILE_COLS:
            raise ValueError(f"query {qi + 1} has {len(merged)} distinct terms (limit {TILE_COLS}).")
        terms.extend(k - 1 for k in merged)
        counts.extend(merged.values())
        ptr.append(len(terms))
    if len(ptr) == 1:
        raise ValueError("queries is empty.")
    return np.asarray(ptr, dtype=np.int64), np.asarray(terms, dtype=np.int32), np.asarray(counts, dtype=np.int32)


def search(model, queries, topn: int = 10, laplace_smooth: float = 0.0, theta=None, skip_unknown: bool = False, splits: int = 0,
           device_id: int = 0) -> SearchResult:
    """For each query the `topn` documents under which the query's words are most likely.  queries: see pack_queries.  Theta is
    topic_proportions(model) -- every training document of an LDA, fLDA, CTM or fCTM model or its gpu form -- unless `theta` is given: a
    K x M array, or a model over other documents (what predict returned), whose topic_proportions are then ranked.  The filtered models are
    scored through their topics alone, as in heldout_loglik.  CTPF raises TopicModelError, as heldout_loglik does."""
    if hasattr(model, "alef"):
        raise TopicModelError("search has no method for CTPF models: its topics are not distributions over the vocabulary (see heldout_loglik).")
    if not hasattr(model, "beta"):
        raise TopicModelError("search needs an LDA, fLDA, CTM or fCTM model (or its gpu form).")
    if not (isinstance(topn, (int, np.integer)) and 1 <= topn <= TOPN_MAX):
        raise ValueError(f"topn must be an integer in [1, {TOPN_MAX}].")
    if not laplace_smooth >= 0:
        raise ValueError("laplace_smooth parameter must be nonnegative.")
    q_ptr, q_terms, q_counts = pack_queries(model, queries, skip_unknown)
    if theta is None:
        th = topic_proportions(model)
    elif isinstance(theta, np.ndarray):
        th = np.asarray(theta, dtype=np.float64)
    else:
        th = topic_proportions(theta)
    if th.ndim != 2 or th.shape[0] != model.K:
        raise TopicModelError("theta and model must have the same number of topics.")
    with call_context(device_id) as ctx:
        rc, res = search_raw(ctx, model.K, model.V, th, model.beta, q_ptr, q_terms, q_counts, int(topn), float(laplace_smooth), splits)
    check(rc)
    tokens = np.add.reduceat(q_counts.astype(np.int64), q_ptr[:-1])
    return SearchResult(res["idx"], res["score"], res["count"], tokens,
                        {"splits": res["splits"], "kp": res["kp"], "col_tiles": res["col_tiles"], "ms": res["ms"]})
