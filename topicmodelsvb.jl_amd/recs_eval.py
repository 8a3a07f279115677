"""
Held-out recommendation metrics for CTPF (the reference stops at showdrecs / showurecs): hold out part of the (document, reader) entries,
train on the rest, ask where each held-out document lands in its user's ranking.

    split_readers(corp, frac=0.2, seed=0, mode="entry")           -> (observed PackedCorpus, HeldReaders): same terms, readers split
    rec_ranks_raw(ctx, K, xd, xq, excl, tgt, splits=0)            -> (status, dict | message): the ABI call tmvb_score_ranks itself
    rank_metrics(tgt_ptr, rank, n_cand, topn=(10, 20, 50, 100))   -> dict: recall / precision / ndcg @N, mrr, pct_rank, their means
    rec_eval(model, held, topn=(10, 20, 50, 100), by="user")      -> RecEvalResult
    rec_quality(corp, K, frac=0.2, seed=0, mode="entry", ...)     -> RecEvalResult: split, train gpuCTPF on the observed side, rec_eval

The rank of a held-out pair is a count -- how many candidates score higher under the order of reverse(sortperm(.)) -- taken in the epilogue
of the f32-MFMA score GEMM of libtmvb_hip.so (tmvb_score_ranks, include/tmvb.h): no score matrix, no sort.  The split and the metrics are
host code of the same library.  There is no CPU fallback for the ranks.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import ReaderSplit, RecRanksInfo  # noqa: F401 (re-exported)
from ._lib import TopicModelError, _copy, _handle, check, lib, P_dbl, P_f32, P_i32, P_i64
from .corpus import PackedCorpus
from .lda import _packed, call_context

ENTRY, DOCUMENT = 0, 1                  # TMVB_RSPLIT_* (include/tmvb.h)
MODES = {"entry": ENTRY, "document": DOCUMENT}
TILE_DB = 128                           # TMVB_NB_TILE_DB: database rows per tile of the scan kernel


def transpose_csr(ptr, idx, n_cols, vals=None):
    """rows x n_cols CSR -> its transpose (ptr[n_cols + 1], row ids ascending inside a column[, vals])"""
    ptr = np.asarray(ptr, dtype=np.int64); idx = np.asarray(idx, dtype=np.int64)
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    order = np.lexsort((rows, idx))
    tptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_cols))]).astype(np.int64)
    out = (tptr, rows[order].astype(np.int32))
    return out if vals is None else out + (np.asarray(vals)[order],)


class HeldReaders:
    """The held-out (document, reader) entries: by document (rdr_ptr[M + 1], readers, ratings, the order of the corpus kept) and by user
    (user_ptr[U + 1], docs ascending, user_ratings)."""

    def __init__(self, rdr_ptr, readers, ratings, U):
        self.rdr_ptr = np.ascontiguousarray(rdr_ptr, dtype=np.int64)
        self.readers = np.ascontiguousarray(readers, dtype=np.int32)
        self.ratings = np.ascontiguousarray(ratings, dtype=np.int32)
        self.M, self.U = len(self.rdr_ptr) - 1, int(U)
        self.user_ptr, self.docs, self.user_ratings = transpose_csr(self.rdr_ptr, self.readers, self.U, self.ratings)

    @property
    def n(self):
        return int(self.rdr_ptr[-1])

    def __repr__(self):
        return f"HeldReaders(M={self.M}, U={self.U}, n={self.n})"


def split_readers_raw(M, U, rdr_ptr, readers, ratings, frac=0.2, seed=0, doc_offset=0, mode=ENTRY):
    """The ABI call tmvb_readers_split (host only).  Returns (status, dict) or (status, message): nothing raises here."""
    L = lib()
    rdr_ptr = np.ascontiguousarray(rdr_ptr, dtype=np.int64)
    readers = np.ascontiguousarray(readers, dtype=np.int32)
    ratings = np.ascontiguousarray(ratings, dtype=np.int32)
    out = ReaderSplit()
    rc = L.tmvb_readers_split(int(M), int(U), rdr_ptr.ctypes.data_as(P_i64), readers.ctypes.data_as(P_i32), ratings.ctypes.data_as(P_i32),
                              frac, np.uint64(int(seed) % 2 ** 64).astype(np.int64), int(doc_offset), int(mode),
                              C.byref(out))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    try:
        M = int(out.M)
        res = {"M": M, "n_obs": int(out.n_obs), "n_held": int(out.n_held),
               "obs_ptr": _copy(out.obs_ptr, M + 1, np.int64), "obs_readers": _copy(out.obs_readers, out.n_obs, np.int32),
               "obs_ratings": _copy(out.obs_ratings, out.n_obs, np.int32),
               "held_ptr": _copy(out.held_ptr, M + 1, np.int64), "held_readers": _copy(out.held_readers, out.n_held, np.int32),
               "held_ratings": _copy(out.held_ratings, out.n_held, np.int32)}
    finally:
        L.tmvb_rsplit_free(C.byref(out))
    return rc, res


def split_readers(corp, frac: float = 0.2, seed: int = 0, mode: str = "entry", doc_offset: int = 0):
    """(observed, held): every (document, reader) entry of `corp` goes to the held-out side with probability `frac` (mode "entry",
    in-matrix), or every document with all of its readers does (mode "document", cold start).  `observed` is a PackedCorpus with the terms
    of `corp` and the readers that stayed; `held` a HeldReaders."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}.")
    pc = _packed(corp)
    rc, res = split_readers_raw(pc.M, pc.U, pc.rdr_ptr, pc.readers, pc.ratings, float(frac), seed, doc_offset, MODES[mode])
    check(rc)
    obs = PackedCorpus(pc.doc_ptr, pc.terms, pc.counts, pc.V, res["obs_ptr"], res["obs_readers"], res["obs_ratings"], pc.U)
    return obs, HeldReaders(res["held_ptr"], res["held_readers"], res["held_ratings"], pc.U)


def rec_ranks_raw(ctx, K, xd, xq, excl, tgt, splits=0):
    """The ABI call tmvb_score_ranks.  ctx: a DeviceContext, or None for a NULL context (the library then answers TMVB_ENODEVICE on a
    machine without a GPU); xd: K x Md, xq: K x Mq; excl / tgt: (ptr[Mq + 1], idx) of 0-based database ids.  Returns (status, dict) or
    (status, message): nothing raises here."""
    L = lib()
    xd = np.asfortranarray(np.asarray(xd, dtype=np.float64))
    xq = np.asfortranarray(np.asarray(xq, dtype=np.float64))
    if xd.ndim != 2 or xq.ndim != 2 or xq.shape[0] != xd.shape[0]:
        return 1, "rec_ranks_raw: xd and xq must be K x Md and K x Mq arrays"
    Md, Mq = xd.shape[1], xq.shape[1]
    eptr, tptr = (np.ascontiguousarray(a[0], dtype=np.int64) for a in (excl, tgt))
    eidx, tidx = (np.ascontiguousarray(a[1], dtype=np.int32) for a in (excl, tgt))
    if len(eptr) != Mq + 1 or len(tptr) != Mq + 1:
        return 1, "rec_ranks_raw: excl and tgt need Mq + 1 pointers"
    nT = max(int(tptr[-1]), 0) if Mq > 0 else 0
    if len(tidx) < nT or (Mq > 0 and len(eidx) < int(eptr[-1])):
        return 1, "rec_ranks_raw: fewer ids than the pointers say"
    rank = np.zeros(max(nT, 1), dtype=np.int32)
    score = np.zeros(max(nT, 1), dtype=np.float32)
    n_cand = np.zeros(max(Mq, 1), dtype=np.int32)
    info = RecRanksInfo()
    rc = L.tmvb_score_ranks(_handle(ctx), int(K), Md, xd.ctypes.data_as(P_dbl), Mq, xq.ctypes.data_as(P_dbl),
                            eptr.ctypes.data_as(P_i64), eidx.ctypes.data_as(P_i32), tptr.ctypes.data_as(P_i64), tidx.ctypes.data_as(P_i32),
                            int(splits), rank.ctypes.data_as(P_i32), n_cand.ctypes.data_as(P_i32), score.ctypes.data_as(P_f32), C.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"rank": rank[:nT], "score": score[:nT], "n_cand": n_cand[:Mq], "splits": int(info.splits), "kp": int(info.kp),
                "ms": {"prep": float(info.ms_prep), "pairs": float(info.ms_pairs), "scan": float(info.ms_scan), "fix": float(info.ms_fix)}}


def rank_metrics_raw(tgt_ptr, rank, n_cand, Ns):
    """The ABI call tmvb_rank_metrics (host only).  Returns (status, dict) or (status, message): nothing raises here."""
    L = lib()
    tptr = np.ascontiguousarray(tgt_ptr, dtype=np.int64)
    rank = np.ascontiguousarray(rank, dtype=np.int32)
    n_cand = np.ascontiguousarray(n_cand, dtype=np.int32)
    Ns = np.ascontiguousarray(np.atleast_1d(Ns), dtype=np.int32)
    Mq, nN = len(tptr) - 1, len(Ns)
    if Mq >= 1 and (len(n_cand) < Mq or len(rank) < int(tptr[-1])):
        return 1, "rank_metrics_raw: fewer ranks or candidate counts than the pointers say"
    rows, cols = max(Mq, 1), max(nN, 1)
    rec, pre, nd = (np.zeros((rows, cols)) for _ in range(3))
    mrr, pct = np.zeros(rows), np.zeros(rows)
    mean, counts = np.zeros(3 * cols + 2), np.zeros(2, dtype=np.int64)
    rc = L.tmvb_rank_metrics(Mq, tptr.ctypes.data_as(P_i64), rank.ctypes.data_as(P_i32), n_cand.ctypes.data_as(P_i32), nN,
                             Ns.ctypes.data_as(P_i32), rec.ctypes.data_as(P_dbl), pre.ctypes.data_as(P_dbl), nd.ctypes.data_as(P_dbl), mrr.ctypes.data_as(P_dbl),
                             pct.ctypes.data_as(P_dbl), mean.ctypes.data_as(P_dbl), counts.ctypes.data_as(P_i64))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"topn": Ns.copy(), "recall": rec[:Mq, :nN], "precision": pre[:Mq, :nN], "ndcg": nd[:Mq, :nN], "mrr": mrr[:Mq], "pct_rank": pct[:Mq],
                "mean_recall": mean[:nN].copy(), "mean_precision": mean[nN:2 * nN].copy(), "mean_ndcg": mean[2 * nN:3 * nN].copy(),
                "mean_mrr": float(mean[3 * nN]), "mean_pct_rank": float(mean[3 * nN + 1]), "n_queries": int(counts[0]), "n_targets": int(counts[1])}


def rank_metrics(tgt_ptr, rank, n_cand, topn=(10, 20, 50, 100)):
    """recall@N, precision@N, ndcg@N (Mq x len(topn)), mrr, pct_rank (Mq; NaN for a query without targets) and their means over the queries
    with targets, from the ranks of tmvb_score_ranks."""
    rc, res = rank_metrics_raw(tgt_ptr, rank, n_cand, topn)
    check(rc)
    return res


class RecEvalResult:
    """by ("user": documents ranked per user, urecs; "doc": users ranked per document, drecs); tgt_ptr / tgt_idx: the held-out ids per query;
    rank, score (per held-out pair, in that order), n_cand (per query); the per-query arrays recall / precision / ndcg [Mq, len(topn)], mrr,
    pct_rank [Mq] and their means over the queries with held-out entries; ms: device time of the four stages; splits."""

    def __init__(self, by, tgt_ptr, tgt_idx, raw, metrics):
        self.by = by
        self.tgt_ptr, self.tgt_idx = tgt_ptr, tgt_idx
        self.rank, self.score, self.n_cand = raw["rank"], raw["score"], raw["n_cand"]
        self.ms, self.splits = dict(raw["ms"]), raw["splits"]
        for k, v in metrics.items():
            setattr(self, k, v)

    def __repr__(self):
        r = ", ".join(f"recall@{int(n)}={v:.4f}" for n, v in zip(self.topn, self.mean_recall))
        return f"RecEvalResult(by={self.by!r}, queries={self.n_queries}, targets={self.n_targets}, {r}, pct_rank={self.mean_pct_rank:.4f})"


def _unique_rows(ptr, idx):
    """a CSR with each row's ids sorted ascending and repeated ids dropped"""
    ptr = np.asarray(ptr, dtype=np.int64); idx = np.asarray(idx, dtype=np.int64)
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    order = np.lexsort((idx, rows))
    rows, idx = rows[order], idx[order]
    keep = np.ones(len(idx), dtype=bool)
    keep[1:] = (rows[1:] != rows[:-1]) | (idx[1:] != idx[:-1])
    rows, idx = rows[keep], idx[keep]
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(ptr) - 1))]).astype(np.int64), idx.astype(np.int32)


def ctpf_factors(model):
    """(X, Y) in fp64 from the model's host state: X = gimel / dalet + zayin / het (K x M), Y = he / vav (K x U); scores = X' Y"""
    f = lambda n: np.asarray(getattr(model, n), dtype=np.float64)
    return f("gimel") / f("dalet")[:, None] + f("zayin") / f("het")[:, None], f("he") / f("vav")[:, None]


def rec_eval(model, held, topn=(10, 20, 50, 100), by: str = "user", splits: int = 0, device_id: int = 0) -> RecEvalResult:
    """Where the held-out entries land in the rankings of a trained CTPF / gpuCTPF `model` (trained on the observed side of split_readers):
    by="user" ranks, for each user, every document outside the library the model was trained on (urecs) and reports the ranks of the user's
    held-out documents; by="doc" swaps the roles (drecs)."""
    if not hasattr(model, "alef"):
        raise TopicModelError("rec_eval needs a CTPF model (or its gpu form).")
    if by not in ("user", "doc"):
        raise ValueError('by must be "user" or "doc".')
    if held.M != model.M or held.U != model.U:
        raise TopicModelError("held-out readers and model must cover the same documents and users.")
    X, Y = ctpf_factors(model)
    corp = model.corp
    if by == "user":
        xd, xq = X, Y
        excl = transpose_csr(corp.rdr_ptr, corp.readers, model.U)
        tgt = (held.user_ptr, held.docs)
    else:
        xd, xq = Y, X
        excl = (corp.rdr_ptr, corp.readers)
        tgt = (held.rdr_ptr, held.readers)
    excl, tgt = _unique_rows(*excl), _unique_rows(*tgt)
    with call_context(device_id, getattr(model, "ctx", None)) as ctx:
        rc, raw = rec_ranks_raw(ctx, model.K, xd, xq, excl, tgt, splits)
    check(rc)
    return RecEvalResult(by, tgt[0], tgt[1], raw, rank_metrics(tgt[0], raw["rank"], raw["n_cand"], topn))


def rec_quality(corp, K: int, frac: float = 0.2, seed: int = 0, mode: str = "entry", topn=(10, 20, 50, 100), by: str = "user", **train_kw) -> RecEvalResult:
    """The perplexity of CTPF: split_readers(corp, frac, seed, mode), gpuCTPF(observed, K).train(recs=False, **train_kw), rec_eval on the
    held-out side."""
    from .ctpf import gpuCTPF
    obs, held = split_readers(corp, frac, seed, mode)
    train_kw.setdefault("printelbo", False)
    g = gpuCTPF(obs, K)
    try:
        g.train(recs=False, **train_kw)
        return rec_eval(g, held, topn, by)
    finally:
        g.close()
