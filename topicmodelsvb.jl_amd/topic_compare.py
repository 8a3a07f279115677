"""
Compare topics: divergences between the rows of topic-word matrices, matching of the topics of two runs, relevant terms (the reference has no
such functions; gensim's LdaModel.diff and LDAvis are the models).

    topic_divergence_raw(ctx, metric, a, b=None, smooth=0.0, splits=0)   -> (status, dict | message): the ABI call tmvb_topic_divergence
    term_relevance_raw(ctx, beta, pw, pi, lam, n, dense=False, terms=True) -> (status, dict | message): the ABI call tmvb_term_relevance
    assignment_raw(cost)                                                  -> (status, row_to_col | message, total): tmvb_assignment (host only)
    topic_distances(a, b=None, metric="js", smooth=0.0)                   -> float64[KA, KB]
    compare_topics(a, b=None, metric="js")                                -> TopicComparison
    topic_stability(models, metric="js")                                  -> TopicStability
    relevant_terms(model, corp=None, lam=0.6, topn=10)                    -> RelevantTerms
    topic_map(model, metric="js")                                         -> TopicMap;  pcoa(D) -> float64[K, 2], plain NumPy

The divergences, the relevance scores with their selection and the per-term statistics come from libtmvb_hip.so (include/tmvb.h: fp64 throughout,
every sum in one fixed order).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from ._abi import RelevanceInfo, TopicDivInfo  # noqa: F401 (re-exported)
from ._lib import TopicModelError, _handle, check, lib, P_dbl, P_i32
from .lda import call_context
from .neighbors import topic_proportions

JS, HELLINGER, TV, KL = 0, 1, 2, 3      # TMVB_TD_* (include/tmvb.h)
METRICS = {"js": JS, "js_distance": JS, "hellinger": HELLINGER, "tv": TV, "kl": KL}
RUN = 256                               # TMVB_TD_RUN: terms per fixed-order partial sum
KMAX = 4096                             # TMVB_TD_KMAX


def topic_word_matrix(x) -> np.ndarray:
    """K x V float64, column-major: a K x V array as given; model.beta of an LDA, fLDA, CTM or fCTM model or its gpu form (what showtopics
    reads); for CTPF the expected topic weights alef / bet with every row normalised to a distribution."""
    if isinstance(x, np.ndarray) or isinstance(x, (list, tuple)):
        b = np.asarray(x, dtype=np.float64)
    elif hasattr(x, "beta"):
        b = np.asarray(x.beta, dtype=np.float64)
    elif hasattr(x, "alef") and hasattr(x, "bet"):
        b = np.asarray(x.alef, dtype=np.float64) / np.asarray(x.bet, dtype=np.float64)[:, None]
        b = b / b.sum(axis=1, keepdims=True)
    else:
        raise TopicModelError("a topic comparison needs an LDA, fLDA, CTM, fCTM or CTPF model (or its gpu form), or a K x V array.")
    if b.ndim != 2:
        raise TopicModelError("the topic-word matrix must be a K x V array.")
    return np.asfortranarray(b)


def topic_divergence_raw(ctx, metric, a, b=None, smooth=0.0, splits=0):
    """The ABI call tmvb_topic_divergence.  ctx: a DeviceContext, or None for a NULL context (the library then answers TMVB_ENODEVICE on a
    machine without a GPU); a: KA x V, b: KB x V or None.  Returns (status, dict) or (status, message): nothing raises here."""
    L = lib()
    a = np.asfortranarray(np.asarray(a, dtype=np.float64))
    if a.ndim != 2:
        return 1, "topic_divergence_raw: a must be a KA x V array"
    KA, V = a.shape
    KB, b_ptr = KA, ct.cast(None, P_dbl)
    if b is not None:
        b = np.asfortranarray(np.asarray(b, dtype=np.float64))
        if b.ndim != 2 or b.shape[1] != V:
            return 1, "topic_divergence_raw: b must be a KB x V array over the same vocabulary"
        KB, b_ptr = b.shape[0], b.ctypes.data_as(P_dbl)
    D = np.zeros((max(KA, 1), max(KB, 1)), dtype=np.float64)
    info = TopicDivInfo()
    rc = L.tmvb_topic_divergence(_handle(ctx), int(metric), V, KA, a.ctypes.data_as(P_dbl), KB, b_ptr, float(smooth), int(splits),
                                 D.ctypes.data_as(P_dbl), ct.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"D": D[:KA, :KB], "splits": int(info.splits), "runs": int(info.runs),
                "ms": {"prep": float(info.ms_prep), "pairs": float(info.ms_pairs), "merge": float(info.ms_merge)}}


def term_relevance_raw(ctx, beta, pw, pi, lam, n, dense=False, terms=True):
    """The ABI call tmvb_term_relevance.  beta: K x V, pw[V], pi[K].  dense: also return all K x V scores; terms: also distinct / saliency.
    Returns (status, dict) or (status, message): nothing raises here."""
    L = lib()
    beta = np.asfortranarray(np.asarray(beta, dtype=np.float64))
    if beta.ndim != 2:
        return 1, "term_relevance_raw: beta must be a K x V array"
    K, V = beta.shape
    pw = np.ascontiguousarray(pw, dtype=np.float64)
    pi = np.ascontiguousarray(pi, dtype=np.float64)
    if pw.shape != (V,) or pi.shape != (K,):
        return 1, "term_relevance_raw: pw must have V entries and pi K"
    rows, cols = max(K, 1), max(int(n), 1)
    idx = np.zeros((rows, cols), dtype=np.int32)
    score = np.zeros((rows, cols), dtype=np.float64)
    count = np.zeros(rows, dtype=np.int32)
    null = ct.cast(None, P_dbl)
    dn = np.zeros((rows, max(V, 1)), dtype=np.float64) if dense else None
    di, sa = (np.zeros(max(V, 1)), np.zeros(max(V, 1))) if terms else (None, None)
    info = RelevanceInfo()
    rc = L.tmvb_term_relevance(_handle(ctx), K, V, beta.ctypes.data_as(P_dbl), pw.ctypes.data_as(P_dbl), pi.ctypes.data_as(P_dbl), float(lam), int(n),
                               idx.ctypes.data_as(P_i32), score.ctypes.data_as(P_dbl), count.ctypes.data_as(P_i32),
                               dn.ctypes.data_as(P_dbl) if dense else null, di.ctypes.data_as(P_dbl) if terms else null,
                               sa.ctypes.data_as(P_dbl) if terms else null, ct.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"idx": idx[:K, :n], "score": score[:K, :n], "count": count[:K], "dense": dn[:K, :V] if dense else None,
                "distinct": di[:V] if terms else None, "saliency": sa[:V] if terms else None,
                "ms": {"score": float(info.ms_score), "select": float(info.ms_select), "terms": float(info.ms_terms)}}


def assignment_raw(cost):
    """The ABI call tmvb_assignment (host only): cost n x m with n <= m, finite or +inf.  Returns (status, row_to_col int32[n] | message, total)."""
    L = lib()
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    if cost.ndim != 2:
        return 1, "assignment_raw: cost must be an n x m array", float("nan")
    n, m = cost.shape
    out = np.full(max(n, 1), -1, dtype=np.int32)
    total = ct.c_double(float("nan"))
    rc = L.tmvb_assignment(n, m, cost.ctypes.data_as(P_dbl), out.ctypes.data_as(P_i32), ct.byref(total))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace"), float("nan")
    return rc, out[:n], float(total.value)


def _metric(metric):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}.")
    return METRICS[metric]


def _distances(a, b, metric, smooth, device_id):
    code = _metric(metric)
    with call_context(device_id) as ctx:
        rc, res = topic_divergence_raw(ctx, code, a, b, smooth)
    if rc == 1 and res.startswith("topic_divergence_raw:"):
        raise TopicModelError(res)
    check(rc)
    return np.sqrt(res["D"]) if metric == "js_distance" else res["D"]


def topic_distances(a, b=None, metric: str = "js", smooth: float = 0.0, device_id: int = 0) -> np.ndarray:
    """D[i, j] = the divergence of topic i of `a` from topic j of `b` (of `a` itself when b is None).  a, b: models or K x V arrays over one
    vocabulary.  metric: "js" (Jensen-Shannon divergence, nats), "js_distance" (its square root, a metric; the root is taken on the host),
    "hellinger", "tv", or "kl" (directed, KL(a_i || b_j); smooth > 0 adds that much to every entry before renormalising and keeps it finite)."""
    _metric(metric)
    return _distances(topic_word_matrix(a), None if b is None else topic_word_matrix(b), metric, smooth, device_id)


def _match(D):
    """rows of the smaller side -> columns of the larger: (match, transposed)"""
    KA, KB = D.shape
    cost = D if KA <= KB else D.T
    rc, m, _ = assignment_raw(cost)
    if rc != 0:
        check(rc)
    return m.astype(np.int64), KA > KB


class TopicComparison:
    """distance[KA, KB]; match: the minimum-cost one-to-one matching of the smaller model's topics into the larger's (tmvb_assignment) --
    match[i] = the topic of b matched to topic i of a when KA <= KB, else (transposed is True) match[j] = the topic of a matched to topic j
    of b; match_distance = the distances of the matched pairs, in the order of match; nearest[i] = the topic of b closest to topic i of a
    (lowest id on ties; not one-to-one); unmatched = the topics of the larger side that nobody was matched to."""

    def __init__(self, distance, metric, a=None, b=None):
        self.distance = np.asarray(distance, dtype=np.float64)
        self.metric = metric
        self._a, self._b, self.self_comparison = a, (a if b is None else b), b is None
        self.match, self.transposed = _match(self.distance)
        rows = np.arange(len(self.match))
        self.match_distance = self.distance.T[rows, self.match] if self.transposed else self.distance[rows, self.match]
        self.nearest = np.argmin(self.distance, axis=1)
        self.unmatched = np.setdiff1d(np.arange(max(self.distance.shape)), self.match)

    def __repr__(self):
        return f"TopicComparison(KA={self.distance.shape[0]}, KB={self.distance.shape[1]}, metric={self.metric!r})"

    def redundant(self, threshold: float):
        """The pairs (i, j, distance), i < j, of topics of ONE model closer than threshold, nearest first: candidates for a collapsed topic."""
        if not self.self_comparison:
            raise TopicModelError("redundant topics are pairs inside one model: compare_topics(model).")
        i, j = np.nonzero(np.triu(self.distance < threshold, k=1))
        order = np.lexsort((j, i, self.distance[i, j]))
        return [(int(i[q]), int(j[q]), float(self.distance[i[q], j[q]])) for q in order]

    def jaccard(self, topn: int = 10) -> np.ndarray:
        """J[i, j] = |A_i & B_j| / |A_i | B_j| of the topn first terms of model.topics (gensim's diff(distance="jaccard") is 1 - J)."""
        if not (isinstance(topn, (int, np.integer)) and topn >= 1):
            raise ValueError("topn must be a positive integer.")
        for m in (self._a, self._b):
            if not hasattr(m, "topics"):
                raise TopicModelError("jaccard needs models (their .topics), not arrays.")
        sa = [set(np.asarray(t[:topn]).tolist()) for t in self._a.topics]
        sb = [set(np.asarray(t[:topn]).tolist()) for t in self._b.topics]
        return np.array([[len(x & y) / len(x | y) for y in sb] for x in sa], dtype=np.float64)


def compare_topics(a, b=None, metric: str = "js", smooth: float = 0.0, device_id: int = 0) -> TopicComparison:
    """Topics of `a` against topics of `b` (another run, another K), or against each other when b is None."""
    D = topic_distances(a, b, metric, smooth, device_id)
    return TopicComparison(D, metric, a, b)


class TopicStability:
    """per_topic[K]: for each topic of the first run the mean, over the other runs, of the distance to its matched topic; score = their mean;
    matches[R - 1][K]: the matched topic in each other run; matched[R - 1][K]: those distances; distance: the stacked R K x R K matrix."""

    def __init__(self, per_topic, matches, matched, distance, metric):
        self.per_topic, self.matches, self.matched, self.distance, self.metric = per_topic, matches, matched, distance, metric
        self.score = float(np.mean(per_topic))

    def __repr__(self):
        return f"TopicStability(runs={len(self.matches) + 1}, K={len(self.per_topic)}, metric={self.metric!r}, score={self.score:.4g})"


def topic_stability(models, metric: str = "js", device_id: int = 0) -> TopicStability:
    """How stable are the topics of the first run across the others (other seeds, other K >= the first's)?  The rows of all runs are stacked
    and go through ONE device call; every other run is then matched to the first by tmvb_assignment."""
    _metric(metric)
    mats = [topic_word_matrix(m) for m in models]
    if len(mats) < 2:
        raise ValueError("topic_stability needs at least two runs.")
    K0, V = mats[0].shape
    if any(m.shape[1] != V for m in mats) or any(m.shape[0] < K0 for m in mats):
        raise TopicModelError("every run must be over the first run's vocabulary and have at least its number of topics.")
    if sum(m.shape[0] for m in mats) > KMAX:
        raise ValueError(f"more than {KMAX} topics in all.")
    D = _distances(np.vstack(mats), None, metric, 0.0, device_id)
    matches, matched, o = [], [], K0
    for m in mats[1:]:
        block = D[:K0, o:o + m.shape[0]]
        mt, _ = _match(block)
        matches.append(mt); matched.append(block[np.arange(K0), mt])
        o += m.shape[0]
    matched = np.array(matched)
    return TopicStability(matched.mean(axis=0), np.array(matches), matched, D, metric)


def topic_share(model) -> np.ndarray:
    """pi[K]: the token-weighted mean of topic_proportions(model) -- the share of the corpus' tokens that each topic accounts for."""
    theta = topic_proportions(model)
    c = np.asarray(model.C, dtype=np.float64)
    pi = theta @ c / c.sum()
    return pi / pi.sum()


def term_frequencies(corp, V=None) -> np.ndarray:
    """pw[V]: the share of the corpus' tokens that each term accounts for."""
    from .lda import _packed
    pc = _packed(corp)
    n = np.bincount(pc.terms, weights=pc.counts.astype(np.float64), minlength=int(V or pc.V))
    return n / n.sum()


class RelevantTerms:
    """idx[K, topn] (0-based term ids, most relevant first; -1 past count), score[K, topn], count[K], words[K][..] (the vocabulary's names, or the
    1-based keys as strings), saliency[V], distinctiveness[V], salient_idx[V] (terms by saliency descending, id ascending on ties), topic_share[K],
    pw[V], lam, ms = device time per stage."""

    def __init__(self, res, pi, pw, lam, vocab=None):
        self.idx, self.score, self.count = res["idx"], res["score"], res["count"]
        self.saliency, self.distinctiveness = res["saliency"], res["distinct"]
        self.salient_idx = np.lexsort((np.arange(len(self.saliency)), -self.saliency))
        self.topic_share, self.pw, self.lam, self.ms = pi, pw, float(lam), res["ms"]
        name = (lambda w: str(vocab[w + 1])) if vocab else (lambda w: str(w + 1))
        self.words = [[name(int(w)) for w in row[:c]] for row, c in zip(self.idx, self.count)]

    def __repr__(self):
        return f"RelevantTerms(K={self.idx.shape[0]}, topn={self.idx.shape[1]}, lam={self.lam})"


def relevant_terms(model, corp=None, lam: float = 0.6, topn: int = 10, device_id: int = 0) -> RelevantTerms:
    """The topn terms of every topic by relevance lam log(phi) + (1 - lam) log(phi / p_w) (Sievert & Shirley 2014; lam = 1 is the order of
    model.topics), with the distinctiveness and saliency of every term (Chuang et al. 2012).  p_w comes from the counts of `corp` when given,
    else it is the model's own marginal sum_k pi_k beta_k."""
    beta = topic_word_matrix(model)
    K, V = beta.shape
    if not (isinstance(lam, (int, float, np.floating, np.integer)) and 0.0 <= lam <= 1.0):
        raise ValueError("lam must lie in [0, 1].")
    if not (isinstance(topn, (int, np.integer)) and 1 <= topn <= V):
        raise ValueError("topn must be an integer in [1, V].")
    pi = topic_share(model) if not isinstance(model, np.ndarray) else np.full(K, 1.0 / K)
    if corp is not None:
        pw = term_frequencies(corp, V)
        if pw.shape != (V,):
            raise TopicModelError("corp and model must have the same vocabulary.")
    else:
        pw = pi @ beta
        pw = pw / pw.sum()
    with call_context(device_id) as ctx:
        rc, res = term_relevance_raw(ctx, beta, pw, pi, lam, int(topn))
    if rc == 1 and res.startswith("term_relevance_raw:"):
        raise TopicModelError(res)
    check(rc)
    return RelevantTerms(res, pi, pw, lam, getattr(getattr(model, "corp", None), "vocab", None))


def pcoa(D, dims: int = 2) -> np.ndarray:
    """Classical multidimensional scaling (principal coordinates) of a symmetric distance matrix, on the host: numpy.linalg.eigh of the
    double-centred squared distances, the `dims` largest eigenvalues (negative ones count as 0).  Each axis is signed so that its coordinate of
    largest magnitude is positive (the first such point on ties)."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or not np.all(np.isfinite(D)):
        raise ValueError("pcoa needs a square matrix of finite distances.")
    n = D.shape[0]
    J = np.eye(n) - np.full((n, n), 1.0 / n)
    S = 0.5 * (D + D.T)
    B = -0.5 * J @ (S * S) @ J
    vals, vecs = np.linalg.eigh(0.5 * (B + B.T))
    order = np.argsort(-vals, kind="stable")[:dims]
    xy = np.zeros((n, dims))
    for c, e in enumerate(order):
        xy[:, c] = vecs[:, e] * np.sqrt(max(vals[e], 0.0))
        p = int(np.argmax(np.abs(xy[:, c])))
        if xy[p, c] < 0:
            xy[:, c] = -xy[:, c]
    return xy


class TopicMap:
    """xy[K, 2]: the intertopic distance map (the left panel of LDAvis); share[K]: the topics' token shares, for bubble sizes; distance[K, K]."""

    def __init__(self, xy, share, distance, metric):
        self.xy, self.share, self.distance, self.metric = xy, share, distance, metric

    def __repr__(self):
        return f"TopicMap(K={self.xy.shape[0]}, metric={self.metric!r})"


def topic_map(model, metric: str = "js", device_id: int = 0) -> TopicMap:
    """Topics in the plane by classical MDS of their pairwise distances ("js" maps the Jensen-Shannon DISTANCE, the root of the divergence, as
    LDAvis does)."""
    D = topic_distances(model, None, "js_distance" if metric == "js" else metric, 0.0, device_id)
    K = D.shape[0]
    share = topic_share(model) if not isinstance(model, np.ndarray) else np.full(K, 1.0 / K)
    return TopicMap(pcoa(D), share, D, metric)
