"""
Map documents in two dimensions: exact t-SNE over the topic kNN graph (the reference has no such function).

    map_affinity_raw(ctx, idx, d2, count, perplexity, Mc=None, symmetric=True)  -> (status, dict | message): the ABI call tmvb_map_affinity
    map_layout_raw(ctx, M, row_ptr, col, val, iters, ...)                       -> (status, dict | message): the ABI call tmvb_map_layout
    map_docs(model, perplexity=None, metric="hellinger", n_neighbors=None, iters=750, init="pca", seed=0, theta=None, check=50) -> DocMap

Everything on the device comes from libtmvb_hip.so (include/tmvb.h, "map documents in two dimensions": the neighbours from tmvb_topic_neighbors, the
entropy search in fp64, the repulsive term over ALL pairs in a fixed order -- no Barnes-Hut tree, no FFT grid --, fixed-order fp64 sums, so equal
inputs give equal bytes).  There is no CPU fallback.  The PCA start and DocMap.place's weighted means are host display code.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from ._abi import MapInfo, MapParams  # noqa: F401 (re-exported)
from ._lib import TopicModelError, _handle, lib, P_dbl, P_f32, P_i32, P_i64
from ._lib import check as _check
from .lda import call_context
from .neighbors import COSINE, HELLINGER, TOPN_MAX, neighbors_raw, topic_proportions

METRICS = {"hellinger": HELLINGER, "cosine": COSINE}
BISECT, RUN, SEG, SLOTS = 64, 256, 64, 64       # TMVB_MAP_BISECT, TMVB_MAP_RUN, TMVB_MAP_SEG, TMVB_MAP_SLOTS (include/tmvb.h)
RNG_MAP = 9                                     # TMVB_RNG_MAP (csrc/tmvb_philox.h)
STOPS = {0: "iters", 1: "min_grad_norm"}
DEFAULTS = dict(exaggeration=12.0, exag_iters=250, momentum0=0.5, momentum1=0.8, min_gain=0.01)


def default_eta(M, exaggeration=12.0):
    return max(M / exaggeration / 4.0, 50.0)


def map_affinity_raw(ctx, idx, d2, count, perplexity, Mc=None, symmetric=True):
    """The ABI call tmvb_map_affinity.  idx[M, n], d2[M, n] (fp32), count[M] as tmvb_topic_neighbors returns them; symmetric=False is the conditional
    form (rows = new points against Mc mapped ones; beta and p_cond only).  ctx None: a NULL context.  Returns (status, dict) or (status, message)."""
    L = lib()
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    d2 = np.ascontiguousarray(d2, dtype=np.float32)
    count = np.ascontiguousarray(count, dtype=np.int32)
    if idx.ndim != 2 or d2.shape != idx.shape or count.shape != idx.shape[:1]:
        return 1, "map_affinity_raw: idx and d2 must be M x n arrays, count an M array"
    M, n = idx.shape
    beta = np.zeros(max(M, 1))
    p = np.zeros((max(M, 1), max(n, 1)))
    cap = 2 * max(M, 1) * max(n, 1) if symmetric else 1
    row_ptr, col, val = np.zeros(max(M, 1) + 1, dtype=np.int64), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.float32)
    null = lambda t: ct.cast(None, t)
    rc = L.tmvb_map_affinity(_handle(ctx), M, M if Mc is None else int(Mc), n, idx.ctypes.data_as(P_i32), d2.ctypes.data_as(P_f32),
                             count.ctypes.data_as(P_i32), float(perplexity), beta.ctypes.data_as(P_dbl), p.ctypes.data_as(P_dbl),
                             row_ptr.ctypes.data_as(P_i64) if symmetric else null(P_i64), col.ctypes.data_as(P_i32) if symmetric else null(P_i32),
                             val.ctypes.data_as(P_f32) if symmetric else null(P_f32))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    out = {"beta": beta[:M], "p_cond": p[:M, :n]}
    if symmetric:
        nnz = int(row_ptr[M])
        out.update(row_ptr=row_ptr, col=col[:nnz].copy(), val=val[:nnz].copy())
    return rc, out


def _state(a, M, name):
    if a is None:
        return None, ct.cast(None, P_f32)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != (M, 2):
        raise ValueError(f"{name} must be an M x 2 array.")
    return a, a.ctypes.data_as(P_f32)


def map_layout_raw(ctx, M, row_ptr, col, val, iters, iter0=0, y=None, vel=None, gain=None, eta=None, exaggeration=12.0, exag_iters=250, momentum0=0.5,
                   momentum1=0.8, min_gain=0.01, check=0, min_grad_norm=0.0, seed=0, j_split=0, pieces=False):
    """The ABI call tmvb_map_layout on the CSR of map_affinity_raw.  y / vel / gain: the M x 2 state on entry (None: the seeded start, 0, 1).  pieces:
    also return rep, zrow, att, grad of the last gradient evaluation.  Returns (status, dict) or (status, message)."""
    L = lib()
    M = int(M)
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float32)
    if row_ptr.shape != (max(M, 0) + 1,) or col.shape != val.shape or col.ndim != 1 or (M >= 1 and col.shape[0] < row_ptr[-1]):
        return 1, "map_layout_raw: row_ptr must have M + 1 entries, col and val row_ptr[M]"
    try:
        y0, y0p = _state(y, M, "y")
        v0, v0p = _state(vel, M, "vel")
        g0, g0p = _state(gain, M, "gain")
    except ValueError as e:
        return 1, "map_layout_raw: " + str(e)
    P = MapParams(int(iters), int(iter0), int(exag_iters), int(check), int(j_split), 0, int(seed), float(exaggeration), float(min_grad_norm), float(momentum0),
                  float(momentum1), float(default_eta(M, exaggeration) if eta is None else eta), float(min_gain))
    rows = max(M, 1)
    yo, vo, go = (np.zeros((rows, 2), dtype=np.float32) for _ in range(3))
    cap = (max(int(iters), 0) // int(check) if int(check) > 0 else 0) + 2
    kl, kl_iter = np.zeros(cap), np.zeros(cap, dtype=np.int32)
    rep, zrow, att, grad = np.zeros((rows, 2)), np.zeros(rows), np.zeros((rows, 2)), np.zeros((rows, 2), dtype=np.float32)
    opt = (lambda a, t: a.ctypes.data_as(t)) if pieces else (lambda a, t: ct.cast(None, t))
    info = MapInfo()
    rc = L.tmvb_map_layout(_handle(ctx), M, row_ptr.ctypes.data_as(P_i64), col.ctypes.data_as(P_i32), val.ctypes.data_as(P_f32), ct.byref(P), y0p, v0p, g0p,
                           yo.ctypes.data_as(P_f32), vo.ctypes.data_as(P_f32), go.ctypes.data_as(P_f32), cap, kl.ctypes.data_as(P_dbl),
                           kl_iter.ctypes.data_as(P_i32), opt(rep, P_dbl), opt(zrow, P_dbl), opt(att, P_dbl), opt(grad, P_f32), ct.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    k = int(info.n_kl)
    out = {"y": yo[:M], "vel": vo[:M], "gain": go[:M], "kl": kl[:k].copy(), "kl_iter": kl_iter[:k].copy(), "iters": int(info.iters), "stop": int(info.stop),
           "j_split": int(info.j_split), "Z": float(info.Z), "grad_norm": float(info.grad_norm),
           "ms": {"repulsion": float(info.ms_rep), "attraction": float(info.ms_att), "update": float(info.ms_upd)}}
    if pieces:
        out.update(rep=rep[:M], zrow=zrow[:M], att=att[:M], grad=grad[:M])
    return rc, out


def features(theta, metric):
    """K x M fp64: sqrt(theta) for hellinger, theta / ||theta||_2 for cosine -- the features whose squared distance is 2 - 2 score"""
    x = np.asarray(theta, dtype=np.float64)
    return np.sqrt(x) if metric == "hellinger" else x / np.sqrt((x * x).sum(axis=0))


def pca_init(theta, metric):
    """M x 2 fp32: the two leading principal components of the features (K x K covariance, numpy.linalg.eigh), each component's sign fixed so that its
    largest-magnitude loading is positive, both scaled by one factor so that the first has standard deviation 1e-4."""
    f = features(theta, metric)
    f = f - f.mean(axis=1, keepdims=True)
    w, v = np.linalg.eigh(f @ f.T / f.shape[1])
    out = np.zeros((f.shape[1], 2))
    for c in range(min(2, f.shape[0])):
        a = v[:, -1 - c]
        a = a * np.sign(a[np.argmax(np.abs(a))])
        out[:, c] = a @ f
    s = out[:, 0].std()
    return (out * (1e-4 / s if s > 0 else 0.0)).astype(np.float32)


def _d2(score):
    with np.errstate(invalid="ignore"):
        d = np.maximum(np.float32(0.0), np.float32(2.0) - np.float32(2.0) * np.asarray(score, dtype=np.float32))
    return np.where(np.isfinite(d), d, np.float32(0.0)).astype(np.float32)


class DocMap:
    """xy[M, 2] (fp32), kl / kl_iters (the KL divergence after that many iterations), beta[M] (the precisions of the entropy search), iters, stop,
    ms = device time per stage (neighbours, and all repulsion / attraction / update kernels so far).  resume(iters) continues from the kept state;
    place(theta_new) puts unseen documents on the finished map."""

    def __init__(self, x, metric, n_neighbors, perplexity, csr, beta, params, device_id):
        self._x, self.metric, self.n_neighbors, self.perplexity = x, metric, int(n_neighbors), float(perplexity)
        self._csr, self.beta, self._params, self.device_id = csr, beta, dict(params), int(device_id)
        self._vel = self._gain = None
        self.xy = None
        self.kl, self.kl_iters = np.zeros(0), np.zeros(0, dtype=np.int32)
        self.iters, self.stop, self.ms = 0, 0, {}

    def __repr__(self):
        return f"DocMap(M={self._x.shape[1]}, metric={self.metric!r}, perplexity={self.perplexity:g}, iters={self.iters})"

    def _run(self, ctx, iters, y0):
        rc, res = map_layout_raw(ctx, self._x.shape[1], *self._csr, iters, self.iters, y0, self._vel, self._gain, **self._params)
        _check(rc)
        self.xy, self._vel, self._gain = res["y"], res["vel"], res["gain"]
        keep = self.kl_iters < (res["kl_iter"][0] if len(res["kl_iter"]) else 0)
        self.kl, self.kl_iters = np.concatenate([self.kl[keep], res["kl"]]), np.concatenate([self.kl_iters[keep], res["kl_iter"]])
        self.iters += res["iters"]
        self.stop = res["stop"]
        for k, v in res["ms"].items():
            self.ms[k] = self.ms.get(k, 0.0) + v
        return self

    def resume(self, iters: int) -> "DocMap":
        """`iters` more iterations from the kept state: the bytes of one longer run."""
        if not (isinstance(iters, (int, np.integer)) and iters >= 0):
            raise ValueError("iters must be a nonnegative integer.")
        with call_context(self.device_id) as ctx:
            return self._run(ctx, int(iters), self.xy)

    def place(self, theta_new) -> np.ndarray:
        """M' x 2: positions of unseen documents (K x M' topic proportions, or what predict returned) on the finished map, which does not move: the
        p_{j|i}-weighted mean (this map's perplexity, tmvb_map_affinity's conditional form) of the positions of their nearest mapped documents."""
        xq = theta_new if isinstance(theta_new, np.ndarray) else topic_proportions(theta_new)
        xq = np.asarray(xq, dtype=np.float64)
        if xq.ndim != 2 or xq.shape[0] != self._x.shape[0]:
            raise TopicModelError("theta_new must be a K x M' array of topic proportions.")
        K, M = self._x.shape
        n = min(self.n_neighbors, M)
        with call_context(self.device_id) as ctx:
            rc, nb = neighbors_raw(ctx, K, METRICS[self.metric], self._x, xq, 0, n)
            _check(rc)
            rc, af = map_affinity_raw(ctx, np.maximum(nb["idx"], 0), _d2(nb["score"]), nb["count"], self.perplexity, Mc=M, symmetric=False)
            _check(rc)
        pos = self.xy.astype(np.float64)[np.maximum(nb["idx"], 0)]              # M' x n x 2
        return (af["p_cond"][:, :, None] * pos).sum(axis=1)


def map_docs(model, perplexity=None, metric: str = "hellinger", n_neighbors=None, iters: int = 750, init="pca", seed: int = 0, theta=None, check: int = 50,
             device_id: int = 0, **params) -> DocMap:
    """A 2-D map of the documents of `model` (or of theta, K x M topic proportions): t-SNE on the n_neighbors nearest documents of each document under
    `metric` ("hellinger" or "cosine"), the repulsion computed exactly over all pairs.  n_neighbors defaults to min(64, M - 1), perplexity to
    min(20, n_neighbors / 3) and must be below n_neighbors.  init: "pca" (host), "random" (seeded, on the device) or an M x 2 array.  check: the KL
    divergence is evaluated every `check` iterations (0: only at the end).  Further keywords: eta, exaggeration, exag_iters, momentum0, momentum1,
    min_gain, min_grad_norm, j_split."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}.")
    bad = set(params) - {"eta", "exaggeration", "exag_iters", "momentum0", "momentum1", "min_gain", "min_grad_norm", "j_split"}
    if bad:
        raise TypeError(f"map_docs: unknown keyword {sorted(bad)[0]!r}.")
    x = topic_proportions(model) if theta is None else np.asarray(theta, dtype=np.float64)
    if x.ndim != 2:
        raise TopicModelError("theta must be a K x M array of topic proportions.")
    K, M = x.shape
    if M < 3:
        raise TopicModelError("a map needs at least 3 documents.")
    if n_neighbors is None:
        n_neighbors = min(TOPN_MAX, M - 1)
    if not (isinstance(n_neighbors, (int, np.integer)) and 2 <= n_neighbors <= min(TOPN_MAX, M - 1)):
        raise ValueError(f"n_neighbors must be an integer in [2, min({TOPN_MAX}, M - 1)].")
    if perplexity is None:
        perplexity = min(20.0, n_neighbors / 3.0)
    if not (np.isfinite(perplexity) and 1.0 <= perplexity < n_neighbors):
        raise ValueError("perplexity must lie in [1, n_neighbors).")
    if not (isinstance(iters, (int, np.integer)) and iters >= 0) or not (isinstance(check, (int, np.integer)) and check >= 0):
        raise ValueError("iters and check must be nonnegative integers.")
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError('init must be "pca", "random" or an M x 2 array.')
        y0 = pca_init(x, metric) if init == "pca" else None
    else:
        y0 = np.asarray(init, dtype=np.float32)
        if y0.shape != (M, 2):
            raise TopicModelError("init must be an M x 2 array.")
    with call_context(device_id) as ctx:
        rc, nb = neighbors_raw(ctx, K, METRICS[metric], x, None, 0, int(n_neighbors))
        _check(rc)
        rc, af = map_affinity_raw(ctx, np.maximum(nb["idx"], 0), _d2(nb["score"]), nb["count"], perplexity)
        _check(rc)
        m = DocMap(x, metric, n_neighbors, perplexity, (af["row_ptr"], af["col"], af["val"]), af["beta"], dict(params, check=int(check), seed=int(seed)), device_id)
        m.ms["neighbors"] = sum(nb["ms"].values())
        return m._run(ctx, int(iters), y0)
