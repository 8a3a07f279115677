"""
Nearest documents in topic space: which documents are about the same things as this one (the reference stops at topicdist(model, d)).

    neighbors_raw(ctx, K, metric, xd, xq=None, q0=0, n=10, splits=0)    -> (status, dict | message): the ABI call itself
    topic_proportions(model)                                            -> float64[K, M]: topicdist of every document, vectorised
    docsim(model, docs=None, topn=10, metric="hellinger", queries=None) -> NeighborsResult

The scores and the selection come from libtmvb_hip.so (tmvb_topic_neighbors, include/tmvb.h: features in fp32, scores on the f32 MFMA -- bit
for bit the ascending fmaf chain --, the n best per query under the total order (score descending, index ascending) selected in the
epilogue; the score matrix never exists).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import NeighborsInfo  # noqa: F401 (re-exported)
from ._lib import CorpusError, TopicModelError, _handle, check, lib, P_dbl, P_f32, P_i32
from .lda import call_context

DOT, HELLINGER, COSINE = 0, 1, 2        # TMVB_NB_* (include/tmvb.h)
METRICS = {"dot": DOT, "hellinger": HELLINGER, "cosine": COSINE}
TOPN_MAX = 64                           # TMVB_NB_TOPN_MAX
TILE_DB = 128                           # TMVB_NB_TILE_DB: database rows per tile of the scan kernel


class NeighborsResult:
    """idx[Mq, n] (0-based database rows, best first; -1 past count), score[Mq, n] (fp32; -inf past count), count[Mq], distance[Mq, n]
    (hellinger: sqrt(max(0, 1 - score)); cosine: 1 - score; dot: none, the field is None; inf past count), ms = device time of the three
    kernels, splits = database splits used."""

    def __init__(self, idx, score, count, metric, ms=None, splits=1):
        self.idx = np.asarray(idx, dtype=np.int32)
        self.score = np.asarray(score, dtype=np.float32)
        self.count = np.asarray(count, dtype=np.int32)
        self.metric = metric
        self.ms = dict(ms or {})
        self.splits = int(splits)
        s = self.score.astype(np.float64)
        if metric == "hellinger":
            self.distance = np.sqrt(np.maximum(0.0, 1.0 - s))
        elif metric == "cosine":
            self.distance = 1.0 - s
        else:
            self.distance = None

    def __repr__(self):
        return f"NeighborsResult(Mq={self.idx.shape[0]}, n={self.idx.shape[1]}, metric={self.metric!r})"


def neighbors_raw(ctx, K, metric, xd, xq=None, q0=0, n=10, splits=0, Mq=None):
    """The ABI call tmvb_topic_neighbors.  ctx: a DeviceContext, or None for a NULL context (the library then answers TMVB_ENODEVICE on a
    machine without a GPU); xd: K x Md, xq: K x Mq, or None: the queries are then database rows [q0, q0 + Mq), each
    excluding itself (Mq: the keyword, by default all rows from q0 on).  Returns (status, dict) or (status, message): nothing raises here."""
    L = lib()
    xd = np.asfortranarray(np.asarray(xd, dtype=np.float64))
    if xd.ndim != 2:
        return 1, "neighbors_raw: xd must be a K x Md array"
    Md = xd.shape[1]
    if xq is None:
        Mq = Md - int(q0) if Mq is None else int(Mq)
        q_ptr = C.cast(None, P_dbl)
    else:
        xq = np.asfortranarray(np.asarray(xq, dtype=np.float64))
        if xq.ndim != 2 or xq.shape[0] != xd.shape[0]:
            return 1, "neighbors_raw: xq must be a K x Mq array"
        Mq = xq.shape[1]
        q_ptr = xq.ctypes.data_as(P_dbl)
    rows, cols = max(Mq, 1), max(int(n), 1)
    idx = np.zeros((rows, cols), dtype=np.int32)
    score = np.zeros((rows, cols), dtype=np.float32)
    count = np.zeros(rows, dtype=np.int32)
    info = NeighborsInfo()
    rc = L.tmvb_topic_neighbors(_handle(ctx), int(K), int(metric), Md, xd.ctypes.data_as(P_dbl), Mq, q_ptr,
                                int(q0), int(n), int(splits), idx.ctypes.data_as(P_i32), score.ctypes.data_as(P_f32),
                                count.ctypes.data_as(P_i32), C.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"idx": idx[:Mq, :n], "score": score[:Mq, :n], "count": count[:Mq], "splits": int(info.splits), "kp": int(info.kp),
                "ms": {"prep": float(info.ms_prep), "scan": float(info.ms_scan), "merge": float(info.ms_merge)}}


def topic_proportions(model) -> np.ndarray:
    """K x M: column d - 1 is topicdist(model, d) -- gamma / sum gamma (LDA, fLDA), additive_logistic(lambda + vsq / 2) (CTM, fCTM),
    gimel / sum gimel (CTPF), and their gpu forms."""
    if hasattr(model, "gimel"):
        g = np.asarray(model.gimel, dtype=np.float64)
        return g / g.sum(axis=0)
    if hasattr(model, "gamma"):
        g = np.asarray(model.gamma, dtype=np.float64)
        return g / g.sum(axis=0)
    if hasattr(model, "lam") and hasattr(model, "vsq"):
        x = np.asarray(model.lam, dtype=np.float64) + 0.5 * np.asarray(model.vsq, dtype=np.float64)
        x = np.exp(x - x.max(axis=0))
        return x / x.sum(axis=0)
    raise TopicModelError("topic_proportions needs an LDA, fLDA, CTM, fCTM or CTPF model (or its gpu form).")


def docsim(model, docs=None, topn: int = 10, metric: str = "hellinger", queries=None, device_id: int = 0) -> NeighborsResult:
    """For each document of `docs` (1-based indices like topicdist, an integer or a sequence; None: every document) the `topn` documents of
    `model` nearest in topic space, the document itself excluded.  queries: another model over other documents (what predict returned):
    the training documents nearest to each of ITS documents (docs then indexes the query model; nothing is excluded).  metric: "hellinger"
    (score = Bhattacharyya coefficient), "cosine" or "dot".  A contiguous range of documents goes down as (q0, Mq); anything else as
    explicit query rows, with the self match removed here."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}.")
    if not (isinstance(topn, (int, np.integer)) and 1 <= topn <= TOPN_MAX):
        raise ValueError(f"topn must be an integer in [1, {TOPN_MAX}].")
    xd = topic_proportions(model)
    K, Md = xd.shape
    src = xd
    if queries is not None:
        src = topic_proportions(queries)
        if src.shape[0] != K:
            raise TopicModelError("queries and model must have the same number of topics.")
    if docs is None:
        sel = np.arange(src.shape[1], dtype=np.int64)
    else:
        sel = np.atleast_1d(np.asarray(docs)).astype(np.int64) - 1
        if sel.ndim != 1 or sel.size == 0 or sel.min() < 0 or sel.max() >= src.shape[1]:
            raise CorpusError("document index outside corpus range.")
    contiguous = bool(np.all(np.diff(sel) == 1))
    n = int(topn)
    with call_context(device_id) as ctx:
        if queries is not None:
            rc, res = neighbors_raw(ctx, K, METRICS[metric], xd, src[:, sel], 0, n)
        elif contiguous:
            rc, res = neighbors_raw(ctx, K, METRICS[metric], xd, None, int(sel[0]), n, Mq=len(sel))
        elif n < TOPN_MAX:
            rc, res = neighbors_raw(ctx, K, METRICS[metric], xd, xd[:, sel], 0, n + 1)
            if rc == 0:
                res = _drop_self(res, sel, n)
        else:                                           # no slot to spare for the self match: the library excludes it, row by row
            parts = []
            for d in sel:
                rc, res = neighbors_raw(ctx, K, METRICS[metric], xd, None, int(d), n, Mq=1)
                if rc != 0:
                    break
                parts.append(res)
            if rc == 0:
                res = {"idx": np.concatenate([p["idx"] for p in parts]), "score": np.concatenate([p["score"] for p in parts]),
                       "count": np.concatenate([p["count"] for p in parts]), "splits": parts[0]["splits"],
                       "ms": {k: sum(p["ms"][k] for p in parts) for k in ("prep", "scan", "merge")}}
    check(rc)
    return NeighborsResult(res["idx"], res["score"], res["count"], metric, res["ms"], res["splits"])


def _drop_self(res, sel, n):
    """n + 1 neighbours of explicit rows of the database -> n, without each row itself (it is among the n + 1 unless n + 1 others come
    before it: then the last one goes)"""
    Mq = len(sel)
    idx = np.full((Mq, n), -1, dtype=np.int32)
    score = np.full((Mq, n), -np.inf, dtype=np.float32)
    count = np.zeros(Mq, dtype=np.int32)
    for q in range(Mq):
        keep = [j for j in range(int(res["count"][q])) if res["idx"][q, j] != sel[q]][:n]
        idx[q, :len(keep)] = res["idx"][q, keep]
        score[q, :len(keep)] = res["score"][q, keep]
        count[q] = len(keep)
    return {"idx": idx, "score": score, "count": count, "splits": res["splits"], "ms": res["ms"]}
