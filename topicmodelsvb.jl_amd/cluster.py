"""
Cluster documents in topic space: k-means on the topic proportions (the reference has no such function).

    kmeans_raw(ctx, K, metric, x, C, init=None, seed=0, max_iter=100, tol=0.0)    -> (status, dict | message): the ABI call itself
    cluster_docs(model, k, metric="hellinger", init="k-means++", seed=0, max_iter=100, tol=0.0, theta=None) -> ClusterResult

Everything comes from libtmvb_hip.so (tmvb_topic_kmeans, include/tmvb.h: fp32 features, the assignment on the f32 MFMA with the arg-max
in its epilogue, fixed-order fp64 sums for the centroids and the inertia, k-means++ seeding on the device).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from ._abi import KMeansInfo  # noqa: F401 (re-exported)
from ._lib import CorpusError, TopicModelError, _handle, check, lib, P_dbl, P_f32, P_i32, P_i64
from .lda import call_context
from .neighbors import topic_proportions

EUCLID, HELLINGER, COSINE = 0, 1, 2     # TMVB_KM_* (include/tmvb.h)
METRICS = {"euclid": EUCLID, "hellinger": HELLINGER, "cosine": COSINE}
CMAX = 1024                             # TMVB_KM_CMAX
RUN = 256                               # TMVB_KM_RUN: members / documents per fixed-order partial sum
STOPS = {0: "max_iter", 1: "converged", 2: "tol"}


def kmeans_raw(ctx, K, metric, x, C, init=None, seed=0, max_iter=100, tol=0.0):
    """The ABI call tmvb_topic_kmeans.  ctx: a DeviceContext, or None for a NULL context (the library then answers TMVB_ENODEVICE on a
    machine without a GPU); x: K x M; init: K x C centroids in feature space, or None: k-means++ with `seed`.  Returns (status, dict) or
    (status, message): nothing raises here."""
    L = lib()
    x = np.asfortranarray(np.asarray(x, dtype=np.float64))
    if x.ndim != 2:
        return 1, "kmeans_raw: x must be a K x M array"
    M, nc, it = x.shape[1], max(int(C), 1), max(int(max_iter), 0)
    i_ptr = ct.cast(None, P_dbl)
    if init is not None:
        init = np.asfortranarray(np.asarray(init, dtype=np.float64))
        if init.ndim != 2 or init.shape != (x.shape[0], int(C)):
            return 1, "kmeans_raw: init must be a K x C array"
        i_ptr = init.ctypes.data_as(P_dbl)
    label = np.zeros(max(M, 1), dtype=np.int32)
    centroid = np.zeros((max(int(K), 1), nc), dtype=np.float64, order="F")
    count = np.zeros(nc, dtype=np.int64)
    dist2 = np.zeros(max(M, 1), dtype=np.float32)
    inertia = np.full(min(it, 10000) + 1, np.nan)
    seeds = np.zeros(nc, dtype=np.int32)
    info = KMeansInfo()
    rc = L.tmvb_topic_kmeans(_handle(ctx), int(K), int(metric), M, x.ctypes.data_as(P_dbl), int(C), i_ptr,
                             int(seed), int(max_iter), float(tol), label.ctypes.data_as(P_i32), centroid.ctypes.data_as(P_dbl),
                             count.ctypes.data_as(P_i64), dist2.ctypes.data_as(P_f32), inertia.ctypes.data_as(P_dbl), seeds.ctypes.data_as(P_i32), ct.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"label": label[:M], "centroid": centroid, "count": count, "dist2": dist2[:M], "inertia": inertia, "seeds": seeds, "iters": int(info.iters),
                "stop": int(info.stop), "n_empty": int(info.n_empty), "kp": int(info.kp), "moved_last": int(info.moved_last),
                "ms": {"prep": float(info.ms_prep), "seed": float(info.ms_seed), "assign": float(info.ms_assign), "update": float(info.ms_update)}}


class ClusterResult:
    """labels[M] (0-based), centroids[K, k] (feature space: sqrt of proportions for hellinger, unit vectors for cosine), profiles[K, k] (the
    centroids as topic proportions: c^2 / sum c^2 for hellinger, c / sum c otherwise), counts[k], dist2[M] (fp32, squared feature distance to
    the own centroid), distance[M] (hellinger: the Hellinger distance sqrt(dist2 / 2); euclid: sqrt(dist2); cosine: 1 - cosine = dist2 / 2),
    inertia[iters + 1], iters, stop (0 max_iter, 1 no label moved, 2 tol), n_empty, seeds[k] (document ids of the k-means++ picks, -1 when the
    centroids were given), ms = device time per stage."""

    def __init__(self, labels, centroids, counts, dist2, inertia, metric, iters=0, stop=0, n_empty=0, seeds=None, ms=None, device_id=0):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {sorted(METRICS)}.")
        self.labels = np.asarray(labels, dtype=np.int32)
        self.centroids = np.asarray(centroids, dtype=np.float64)
        self.counts = np.asarray(counts, dtype=np.int64)
        self.dist2 = np.asarray(dist2, dtype=np.float32)
        self.inertia = np.asarray(inertia, dtype=np.float64)
        self.metric = metric
        self.iters, self.stop, self.n_empty = int(iters), int(stop), int(n_empty)
        self.seeds = np.full(self.centroids.shape[1], -1, dtype=np.int32) if seeds is None else np.asarray(seeds, dtype=np.int32)
        self.ms = dict(ms or {})
        self.device_id = int(device_id)
        c = self.centroids * self.centroids if metric == "hellinger" else self.centroids
        self.profiles = c / c.sum(axis=0)
        d = self.dist2.astype(np.float64)
        self.distance = np.sqrt(0.5 * d) if metric == "hellinger" else np.sqrt(d) if metric == "euclid" else 0.5 * d

    def __repr__(self):
        return f"ClusterResult(M={len(self.labels)}, k={self.centroids.shape[1]}, metric={self.metric!r}, iters={self.iters}, stop={STOPS[self.stop]!r})"

    def assign(self, theta, device_id=None) -> "ClusterResult":
        """Assign-only on other documents: theta is K x M' topic proportions, or a model (what predict returned).  The centroids are
        this result's; labels, dist2 and counts are the new documents'."""
        x = theta if isinstance(theta, np.ndarray) else topic_proportions(theta)
        return _run(x, self.centroids.shape[1], self.metric, self.centroids, 0, 0, 0.0, self.device_id if device_id is None else device_id)

    def representatives(self, n: int = 5):
        """Per cluster the (up to) n members with the smallest dist2, 0-based document ids, nearest first; ties go to the lower id."""
        if not (isinstance(n, (int, np.integer)) and n >= 1):
            raise ValueError("n must be a positive integer.")
        order = np.lexsort((np.arange(len(self.labels)), self.dist2, self.labels))      # label, then dist2, then id
        starts = np.concatenate([[0], np.cumsum(np.bincount(self.labels, minlength=self.centroids.shape[1]))])
        return [order[starts[c]:min(starts[c] + int(n), starts[c + 1])].astype(np.int64) for c in range(self.centroids.shape[1])]


def _run(x, k, metric, init, seed, max_iter, tol, device_id):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise TopicModelError("theta must be a K x M array of topic proportions.")
    with call_context(device_id) as ctx:
        rc, res = kmeans_raw(ctx, x.shape[0], METRICS[metric], x, k, init, seed, max_iter, tol)
    if rc == 1 and res.startswith("kmeans_raw:"):
        raise TopicModelError(res)
    check(rc)
    return ClusterResult(res["label"], res["centroid"], res["count"], res["dist2"], res["inertia"][:res["iters"] + 1], metric, res["iters"], res["stop"],
                         res["n_empty"], res["seeds"], res["ms"], device_id)


def cluster_docs(model, k: int, metric: str = "hellinger", init="k-means++", seed: int = 0, max_iter: int = 100, tol: float = 0.0, theta=None,
                 device_id: int = 0) -> ClusterResult:
    """k-means of the documents of `model` in topic space into k clusters: on topic_proportions(model), or on theta (K x M, e.g.
    topic_proportions(predict(new_corp, model))) if given.  metric: "hellinger" (features sqrt(theta): squared distance = 2 H^2), "cosine"
    (spherical k-means) or "euclid".  init: "k-means++" (seeded by `seed`), a K x k array of centroids in feature space, or an earlier
    ClusterResult (its centroids).  Stops when no label moves, after max_iter updates, or when the inertia improves by no more than tol x
    itself."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}.")
    if not (isinstance(k, (int, np.integer)) and 1 <= k <= CMAX):
        raise ValueError(f"k must be an integer in [1, {CMAX}].")
    x = topic_proportions(model) if theta is None else np.asarray(theta, dtype=np.float64)
    if x.ndim != 2:
        raise TopicModelError("theta must be a K x M array of topic proportions.")
    if k > x.shape[1]:
        raise CorpusError("more clusters than documents.")
    if isinstance(init, ClusterResult):
        if init.metric != metric:
            raise TopicModelError("the initial ClusterResult was made under another metric.")
        c0 = init.centroids
    elif isinstance(init, str):
        if init != "k-means++":
            raise ValueError('init must be "k-means++", a K x k array or a ClusterResult.')
        c0 = None
    else:
        c0 = np.asarray(init, dtype=np.float64)
    if c0 is not None and c0.shape != (x.shape[0], int(k)):
        raise TopicModelError("init must be a K x k array of centroids.")
    return _run(x, int(k), metric, c0, seed, max_iter, tol, device_id)
