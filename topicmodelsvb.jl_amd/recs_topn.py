"""
Top-n recommendations for CTPF: for a set of users the n best documents outside each user's library, with the roles swapped the n best
users outside each document's readers -- what the reference's showurecs(model, users, M=15) / showdrecs(model, docs, U=15) read off a full
ranking.

    rec_topn_raw(ctx, K, xd, xq, excl, n, splits=0)                       -> (status, dict | message): the ABI call tmvb_score_topn itself
    recommend_topn(model, topn=15, by="user", ids=None, splits=0)         -> RecTopN

The lists come from libtmvb_hip.so (tmvb_score_topn, include/tmvb.h): the scores on the f32 MFMA, the n best per query under the order of
reverse(sortperm(.)) kept in the epilogue of the scan, the exclusion lists searched there for the entries that pass a query's threshold.
No M x U array, no sort.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CorpusError, RecTopNInfo, TopicModelError, _handle, check, lib, P_dbl, P_f32, P_i32, P_i64
from .lda import call_context
from .recs_eval import _unique_rows, ctpf_factors, transpose_csr

TOPN_MAX = 64                           # TMVB_NB_TOPN_MAX


def rec_topn_raw(ctx, K, xd, xq, excl, n, splits=0):
    """The ABI call tmvb_score_topn.  ctx: a DeviceContext, or None for a NULL context (the library then answers TMVB_ENODEVICE on a
    machine without a GPU); xd: K x Md, xq: K x Mq (the caller's own factors, e.g. rows of documents or users that were not in training);
    excl: (ptr[Mq + 1], idx) of 0-based database ids, ascending inside a query.  Returns (status, dict) or (status, message): nothing
    raises here."""
    L = lib()
    xd = np.asfortranarray(np.asarray(xd, dtype=np.float64))
    xq = np.asfortranarray(np.asarray(xq, dtype=np.float64))
    if xd.ndim != 2 or xq.ndim != 2 or xq.shape[0] != xd.shape[0]:
        return 1, "rec_topn_raw: xd and xq must be K x Md and K x Mq arrays"
    Md, Mq = xd.shape[1], xq.shape[1]
    eptr = np.ascontiguousarray(excl[0], dtype=np.int64)
    eidx = np.ascontiguousarray(excl[1], dtype=np.int32)
    if len(eptr) != Mq + 1:
        return 1, "rec_topn_raw: excl needs Mq + 1 pointers"
    if Mq > 0 and len(eidx) < int(eptr[-1]):
        return 1, "rec_topn_raw: fewer ids than the pointers say"
    rows, cols = max(Mq, 1), max(int(n), 1)
    idx = np.zeros((rows, cols), dtype=np.int32)
    score = np.zeros((rows, cols), dtype=np.float32)
    count = np.zeros(rows, dtype=np.int32)
    info = RecTopNInfo()
    rc = L.tmvb_score_topn(_handle(ctx), int(K), Md, xd.ctypes.data_as(P_dbl), Mq, xq.ctypes.data_as(P_dbl), eptr.ctypes.data_as(P_i64),
                           eidx.ctypes.data_as(P_i32), int(n), int(splits), idx.ctypes.data_as(P_i32), score.ctypes.data_as(P_f32),
                           count.ctypes.data_as(P_i32), C.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"idx": idx[:Mq, :n], "score": score[:Mq, :n], "count": count[:Mq], "splits": int(info.splits), "kp": int(info.kp),
                "ms_prep": float(info.ms_prep), "ms_scan": float(info.ms_scan), "ms_merge": float(info.ms_merge)}


class RecTopN:
    """by ("user": documents per user, the head of urecs; "doc": users per document, the head of drecs); ids: the queries, 1-based, in the
    order asked for; idx[len(ids), topn] (int32, 0-based database rows, best first; -1 past count), score[len(ids), topn] (fp32; -inf past
    count), count[len(ids)]; ms: device time of the three stages; splits."""

    def __init__(self, by, ids, raw):
        self.by, self.ids = by, ids
        self.idx, self.score, self.count = raw["idx"], raw["score"], raw["count"]
        self.ms = {k: raw["ms_" + k] for k in ("prep", "scan", "merge")}
        self.splits = raw["splits"]

    def __repr__(self):
        return f"RecTopN(by={self.by!r}, queries={self.idx.shape[0]}, topn={self.idx.shape[1]})"


def slice_csr(ptr, idx, sel):
    """rows `sel` (0-based, any order, repeats allowed) of a CSR, as a CSR of its own: the pointer starts at 0 again"""
    ptr = np.asarray(ptr, dtype=np.int64)
    sel = np.asarray(sel, dtype=np.int64)
    lens = ptr[sel + 1] - ptr[sel]
    out = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.repeat(ptr[sel] - out[:-1], lens) + np.arange(int(out[-1]), dtype=np.int64)
    return out, np.asarray(idx)[take].astype(np.int32)


def recommend_topn(model, topn: int = 15, by: str = "user", ids=None, splits: int = 0, device_id: int = 0) -> RecTopN:
    """The `topn` best recommendations of a CTPF / gpuCTPF `model`: by="user", for each user of `ids` the documents outside the user's
    library (the first entries of urecs[u]); by="doc", for each document of `ids` the users outside its readers (drecs[d]).  ids: 1-based
    like the reference's showurecs(model, users), an integer or a sequence; None: every user / document.  The call is made on the slice."""
    if not hasattr(model, "alef"):
        raise TopicModelError("recommend_topn needs a CTPF model (or its gpu form).")
    if by not in ("user", "doc"):
        raise ValueError('by must be "user" or "doc".')
    if not (isinstance(topn, (int, np.integer)) and 1 <= topn <= TOPN_MAX):
        raise ValueError(f"topn must be an integer in [1, {TOPN_MAX}].")
    X, Y = ctpf_factors(model)
    corp = model.corp
    if by == "user":
        xd, xq = X, Y
        excl = transpose_csr(corp.rdr_ptr, corp.readers, model.U)
    else:
        xd, xq = Y, X
        excl = (corp.rdr_ptr, corp.readers)
    excl = _unique_rows(*excl)
    if ids is None:
        sel = np.arange(xq.shape[1], dtype=np.int64)
    else:
        sel = np.atleast_1d(np.asarray(ids)).astype(np.int64) - 1
        if sel.ndim != 1 or sel.size == 0 or sel.min() < 0 or sel.max() >= xq.shape[1]:
            raise CorpusError("user index outside corpus range." if by == "user" else "document index outside corpus range.")
        xq, excl = xq[:, sel], slice_csr(excl[0], excl[1], sel)
    with call_context(device_id, getattr(model, "ctx", None)) as ctx:
        rc, raw = rec_topn_raw(ctx, model.K, xd, xq, excl, int(topn), splits)
    check(rc)
    return RecTopN(by, sel + 1, raw)
