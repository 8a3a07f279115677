"""
CTPF fold-in: users and documents that were not in training, without retraining.

    foldin_users_raw(ctx, K, M, gimel, zayin, dalet, het, vav, e, lib_ptr, lib_docs, lib_ratings, ...)  -> (status, dict | message): the ABI
                                                                                     call tmvb_ctpf_foldin_users (handle=: ..._users_on)
    foldin_libraries(libs, ratings, M)                                    -> (ptr, docs, ratings): the host-side preparation, 0-based and sorted
    foldin_users(model, libs, ratings=None, viter=10, vtol=None, he0=None)           -> FoldinUsers(he, sweeps, info)
    predict_ctpf(corp, train_model, viter=10, vtol=None)                             -> CTPF: gimel / zayin of new documents
    recommend_new_users(model, libs, ratings=None, topn=15, ...)                     -> RecTopN: documents for users who were not in training
    recommend_new_docs(model, corp, topn=15, ...)                                    -> RecTopN: users for documents that were not in training

The user side is a new operator (include/tmvb.h, "CTPF fold-in"): he[:, u] iterated to its fixed point with every document factor frozen, on
libtmvb_hip.so.  The document side is the existing E-step on frozen globals, by the pattern of predict.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CorpusError, FoldinInfo, TopicModelError, _handle, check, lib, P_dbl, P_i32, P_i64
from .ctpf import CTPF, gpuCTPF
from .lda import _F, _packed, call_context
from .recs_eval import _unique_rows
from .recs_topn import TOPN_MAX, RecTopN, rec_topn_raw

FOLDIN_REG_CAPACITY = 32                # TMVB_FOLDIN_REG_CAP: library entries one wave keeps in registers, K <= 256
FOLDIN_REG_CAPACITY_BIGK = 16           # TMVB_FOLDIN_REG_CAP_BIGK: K > 256


def foldin_reg_capacity(K: int) -> int:
    """the longest library that takes the one-wave register path at this K; a longer one takes the workgroup path"""
    return FOLDIN_REG_CAPACITY_BIGK if K > 256 else FOLDIN_REG_CAPACITY


def _opt(a, dt):
    return None if a is None else np.ascontiguousarray(a, dtype=dt)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def foldin_users_raw(ctx, K, M, gimel, zayin, dalet, het, vav, e, lib_ptr, lib_docs, lib_ratings, he0=None, viter=10, vtol=None, Un=None,
                     handle=None):
    """The ABI call tmvb_ctpf_foldin_users; with handle= (a gpuCTPF's) tmvb_ctpf_foldin_users_on, which takes K, M, the state and e from the
    handle.  ctx: a DeviceContext, or None for a NULL context.  gimel, zayin: K x M; lib_ptr[Un + 1], lib_docs 0-based and strictly ascending
    inside a user, lib_ratings >= 1; he0: K x Un or None (all ones).  An argument may be None: the library answers for it.  Returns
    (status, dict) or (status, message): nothing raises here."""
    L = lib()
    st = [None if a is None else np.asfortranarray(np.asarray(a, dtype=np.float64)) for a in (gimel, zayin, dalet, het, vav)]
    lp, ld, lr = _opt(lib_ptr, np.int64), _opt(lib_docs, np.int32), _opt(lib_ratings, np.int32)
    if Un is None:
        Un = 0 if lp is None else len(lp) - 1
    Un, K, M = int(Un), int(K), int(M)
    if handle is None and 1 <= K <= 512 and M > 0:          # the sizes the library will read; outside, it answers before reading
        for a, n in zip(st, (K * M, K * M, K, K, K)):
            if a is not None and a.size != n:
                return 1, "foldin_users_raw: gimel and zayin must be K x M, dalet, het and vav of length K"
    if lp is not None and Un >= 0:
        if len(lp) != Un + 1:
            return 1, "foldin_users_raw: lib_ptr needs Un + 1 pointers"
        nE = int(lp[-1])
        if nE > 0 and ((ld is not None and len(ld) < nE) or (lr is not None and len(lr) < nE)):
            return 1, "foldin_users_raw: fewer library entries than the pointers say"
    h0 = None if he0 is None else np.asfortranarray(np.asarray(he0, dtype=np.float64))
    if h0 is not None and h0.shape != (K, Un):
        return 1, "foldin_users_raw: he0 must be a K x Un array"
    vtol = 1.0 / max(K, 1) ** 2 if vtol is None else float(vtol)
    he = np.zeros((max(K, 1), max(Un, 1)), order="F")
    sweeps = np.zeros(max(Un, 1), dtype=np.int32)
    info = FoldinInfo()
    if handle is not None:
        rc = L.tmvb_ctpf_foldin_users_on(handle, Un, _ptr(lp, P_i64), _ptr(ld, P_i32), _ptr(lr, P_i32), _ptr(h0, P_dbl), int(viter), vtol,
                                         he.ctypes.data_as(P_dbl), sweeps.ctypes.data_as(P_i32), C.byref(info))
    else:
        rc = L.tmvb_ctpf_foldin_users(_handle(ctx), K, M, *[_ptr(a, P_dbl) for a in st], float(e), Un, _ptr(lp, P_i64), _ptr(ld, P_i32),
                                      _ptr(lr, P_i32), _ptr(h0, P_dbl), int(viter), vtol, he.ctypes.data_as(P_dbl), sweeps.ctypes.data_as(P_i32),
                                      C.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    Un = max(Un, 0)
    return rc, {"he": np.asfortranarray(he[:K, :Un]), "sweeps": sweeps[:Un], "kp": int(info.kp), "capacity": int(info.capacity),
                "n_reg": int(info.n_reg), "n_long": int(info.n_long), "ms_prep": float(info.ms_prep), "ms_sweeps": float(info.ms_sweeps)}


class FoldinUsers:
    """he: K x Un (fp64 copies of the device's fp32), column u = the user of libs[u]; sweeps[Un]; info: kp, capacity, n_reg / n_long (users
    on the register and on the workgroup path), ms_prep / ms_sweeps (device time of the table kernel and of the user kernels); lib_ptr /
    lib_docs / lib_ratings: the libraries as the device took them (0-based, ascending)."""

    def __init__(self, raw, libs):
        self.he, self.sweeps = raw["he"], raw["sweeps"]
        self.info = {k: raw[k] for k in ("kp", "capacity", "n_reg", "n_long", "ms_prep", "ms_sweeps")}
        self.lib_ptr, self.lib_docs, self.lib_ratings = libs

    def __repr__(self):
        return f"FoldinUsers(K={self.he.shape[0]}, users={self.he.shape[1]})"


def foldin_libraries(libs, ratings, M: int):
    """The host side of foldin_users: libraries as the ABI takes them.  libs: a list with one sequence of 1-based document ids per user, or a
    CSR pair -- a TUPLE (ptr[Un + 1], ids), the ids 1-based as well; ratings: None (every rating 1), or the same structure as libs (a list of
    sequences; for a CSR pair one flat array).  Returns (ptr int64, docs int32 0-based and ascending inside a user, ratings int32, each
    moved with its id).  An id outside [1, M], a repeated id inside a user or a rating below 1 raise CorpusError."""
    if isinstance(libs, tuple):
        if len(libs) != 2:
            raise CorpusError("a CSR pair is (ptr, ids).")
        ptr = np.asarray(libs[0], dtype=np.int64).ravel()
        ids = np.asarray(libs[1], dtype=np.int64).ravel()
        if len(ptr) < 1 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(ids):
            raise CorpusError("library pointers must be non-decreasing from 0 to the number of ids.")
        rat = np.ones(len(ids), dtype=np.int64) if ratings is None else np.asarray(ratings, dtype=np.int64).ravel()
    else:
        rows = [np.asarray(r, dtype=np.int64).ravel() for r in libs]
        ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        ids = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        if ratings is None:
            rat = np.ones(len(ids), dtype=np.int64)
        else:
            if len(ratings) != len(rows):
                raise CorpusError("ratings must hold one sequence per library.")
            rr = [np.asarray(r, dtype=np.int64).ravel() for r in ratings]
            if any(len(a) != len(b) for a, b in zip(rr, rows)):
                raise CorpusError("a library and its ratings must have the same length.")
            rat = np.concatenate(rr) if rr else np.zeros(0, dtype=np.int64)
    if len(rat) != len(ids):
        raise CorpusError("a library and its ratings must have the same length.")
    if len(ids) and (ids.min() < 1 or ids.max() > M):
        raise CorpusError("document index outside corpus range.")
    if len(rat) and rat.min() < 1:
        raise CorpusError("ratings must be positive integers.")
    user = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    order = np.lexsort((ids, user))
    ids, rat, user = ids[order], rat[order], user[order]
    if len(ids) > 1 and np.any((user[1:] == user[:-1]) & (ids[1:] == ids[:-1])):
        raise CorpusError("a library holds a document more than once.")
    return ptr, (ids - 1).astype(np.int32), rat.astype(np.int32)


def _check_ctpf(model, what):
    if not hasattr(model, "alef"):
        raise TopicModelError(f"{what} needs a CTPF model (or its gpu form).")


def _check_sweep_args(viter, vtol):
    if not (isinstance(viter, (int, np.integer)) and viter >= 0):
        raise ValueError("iteration parameter must be a nonnegative integer.")
    if vtol is not None and not (np.isfinite(vtol) and vtol >= 0):
        raise ValueError("tolerance parameter must be nonnegative.")


def foldin_users(model, libs, ratings=None, viter: int = 10, vtol: float | None = None, he0=None, device_id: int = 0) -> FoldinUsers:
    """he of users who were not in training, under the trained CTPF / gpuCTPF `model` with its document factors frozen (include/tmvb.h,
    "CTPF fold-in"): each user's column runs the sweeps of the definition there from he0 (default all ones) for at most viter sweeps, the
    exit rule of the document loop (src/CTPF.jl:354-361) on he with vtol (default 1 / K^2).  libs / ratings: see foldin_libraries (1-based
    ids, sorted here).  For a gpuCTPF the device-resident state of its handle is used (no K x M upload); for a CTPF the host arrays."""
    _check_ctpf(model, "foldin_users")
    _check_sweep_args(viter, vtol)
    K, M = model.K, model.M
    csr = foldin_libraries(libs, ratings, M)
    Un = len(csr[0]) - 1
    if he0 is not None:
        he0 = _F(he0, (K, Un))
        if not (np.all(np.isfinite(he0)) and np.all(he0 > 0)):
            raise TopicModelError("he0 must be positive and finite.")
    if isinstance(model, gpuCTPF):
        rc, raw = foldin_users_raw(None, K, M, None, None, None, None, None, model.e, *csr, he0=he0, viter=viter, vtol=vtol, handle=model.handle)
    else:
        with call_context(device_id, getattr(model, "ctx", None)) as ctx:
            rc, raw = foldin_users_raw(ctx, K, M, model.gimel, model.zayin, model.dalet, model.het, model.vav, model.e, *csr, he0=he0,
                                       viter=viter, vtol=vtol)
    check(rc)
    return FoldinUsers(raw, csr)


def predict_ctpf(corp, train_model, viter: int = 10, vtol: float | None = None, device_id: int = 0) -> CTPF:
    """gimel / zayin of documents that were not in training, by the pattern of predict (src/modelutils.jl:831-855; the reference has none for
    CTPF): a CTPF on `corp` with alef, he, the four rates and the hyperparameters of `train_model`, gimel = zayin = 1, and ONE E-step --
    the document loop of src/CTPF.jl:353-362 with (viter, vtol) --, no M-step.  A document without readers is the cold-start case (its zayin
    stays g); one with readers uses them.  corp must have train_model's V and U.  train_model is not modified."""
    _check_ctpf(train_model, "predict_ctpf")
    _check_sweep_args(viter, vtol)
    K = train_model.K
    pc = _packed(corp)
    if pc.V != train_model.V:
        raise CorpusError("predict corpus and train_model corpus must have identical vocabularies.")
    if pc.U != train_model.U:
        raise CorpusError("predict corpus and train_model corpus must have identical users.")
    host = CTPF(pc, K)
    for n in "abcdefgh":
        setattr(host, n, float(getattr(train_model, n)))
    host.alef = np.array(train_model.alef, dtype=np.float64, order="F"); host.alef_old = host.alef.copy(order="F")
    host.he = np.array(train_model.he, dtype=np.float64, order="F"); host.he_old = host.he.copy(order="F")
    for n in ("bet", "vav", "dalet", "het"):
        setattr(host, n, np.array(getattr(train_model, n), dtype=np.float64)); setattr(host, n + "_old", getattr(host, n).copy())
    g = gpuCTPF(None, K, device_id=device_id, _from=host)
    try:
        g.estep(viter, vtol)
        g.update_host()
        host.doc_sweeps = g.doc_sweeps().astype(np.int32)
    finally:
        g.close()
    for n in ("gimel", "gimel_old", "zayin", "zayin_old"):
        setattr(host, n, getattr(g, n))
    host.topics = train_model.topics
    return host


def _topn_arg(topn):
    if not (isinstance(topn, (int, np.integer)) and 1 <= topn <= TOPN_MAX):
        raise ValueError(f"topn must be an integer in [1, {TOPN_MAX}].")


def _host_state(model):
    if isinstance(model, gpuCTPF):
        model.update_host()


def recommend_new_users(model, libs, ratings=None, topn: int = 15, viter: int = 10, vtol: float | None = None, he0=None, splits: int = 0,
                        device_id: int = 0) -> RecTopN:
    """The `topn` best documents outside each new user's library: foldin_users, then tmvb_score_topn (recs_topn.rec_topn_raw) with
    xd = gimel / dalet + zayin / het, xq = he_new / vav and the libraries as exclusions.  Row u of the result belongs to libs[u]; the
    fold-in itself is kept as .foldin."""
    _check_ctpf(model, "recommend_new_users")
    _topn_arg(topn)
    fold = foldin_users(model, libs, ratings, viter, vtol, he0, device_id)
    _host_state(model)
    f = lambda n: np.asarray(getattr(model, n), dtype=np.float64)
    xd = f("gimel") / f("dalet")[:, None] + f("zayin") / f("het")[:, None]
    xq = fold.he / f("vav")[:, None]
    with call_context(device_id, getattr(model, "ctx", None)) as ctx:
        rc, raw = rec_topn_raw(ctx, model.K, xd, xq, (fold.lib_ptr, fold.lib_docs), int(topn), splits)
    check(rc)
    out = RecTopN("user", np.arange(1, xq.shape[1] + 1), raw)
    out.foldin = fold
    return out


def recommend_new_docs(model, corp, topn: int = 15, viter: int = 10, vtol: float | None = None, splits: int = 0, device_id: int = 0) -> RecTopN:
    """The `topn` best users outside each new document's readers: predict_ctpf, then tmvb_score_topn with xd = he / vav, xq = gimel / dalet +
    zayin / het of the new documents and their readers as exclusions.  Row d belongs to document d of corp; the predicted model is kept as
    .predicted."""
    _check_ctpf(model, "recommend_new_docs")
    _topn_arg(topn)
    _host_state(model)
    p = predict_ctpf(corp, model, viter, vtol, device_id)
    f = lambda n: np.asarray(getattr(model, n), dtype=np.float64)
    xd = f("he") / f("vav")[:, None]
    xq = p.gimel / f("dalet")[:, None] + p.zayin / f("het")[:, None]
    excl = _unique_rows(p.corp.rdr_ptr, p.corp.readers)
    with call_context(device_id, getattr(model, "ctx", None)) as ctx:
        rc, raw = rec_topn_raw(ctx, model.K, xd, xq, excl, int(topn), splits)
    check(rc)
    out = RecTopN("doc", np.arange(1, xq.shape[1] + 1), raw)
    out.predicted = p
    return out
