"""
Topics by group and over time: how the topics differ between parts of the corpus -- years, journals, author classes, cluster_docs labels --
which topics rise or fall, and with which words topic k is written in part g (topics_over_time / topics_per_class elsewhere; the "hot and
cold topics" of Griffiths & Steyvers 2004).

    group_topics(model, groups, topn=10, order=None, corp=None)    -> GroupTopics: per group the topic masses and prevalence, the top words of
                                                                      every topic inside the group, its lexical shift from the pooled topic
                                                                      and its drift from the previous group; trend / hot / cold over the order
    time_bins(stamps, bins)                                        -> labels for group_topics from numeric stamps
    group_topics_raw(ctx, K, V, A, B, pc, group, G, ...)           -> the ABI call tmvb_group_topics itself (include/tmvb.h)
    group_index_raw(pc, group, G)                                  -> tmvb_group_index: the (group, term) index the kernel walks; host only

For every group g the device adds up S_g[k, w] = sum over the entries (w, c) of the documents of g of c r_k(d, w), with r the responsibilities
of tmvb_token_topics recomputed from the two factors (the engine keeps no phi).  All compute goes through libtmvb_hip.so; there is no CPU
fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import GroupTopicsInfo
from ._lib import TopicModelError, _csr, _handle, check, lib, P_dbl, P_i32, P_i64
from .lda import call_context
from .neighbors import topic_proportions
from .token_topics import EPSILON, _folded_in, token_factors

TOPN_MAX = 64                           # TMVB_GT_TOP_MAX
G_MAX = 65536                           # TMVB_GT_GMAX
SEG = 512                               # TMVB_GT_SEG


def _labels32(group, M):
    g = np.ascontiguousarray(group, dtype=np.int64)
    if g.shape != (M,):
        raise ValueError(f"group must hold one label per document ({M})")
    if g.size and (g.min() < -2 ** 31 or g.max() >= 2 ** 31):
        raise ValueError("a group id does not fit 32 bits")
    return g.astype(np.int32)


def group_topics_raw(ctx, K, V, A, B, pc, group, G, topn=10, eps=EPSILON, shift=True, drift=True, dense=False, max_chunk_groups=0):
    """The ABI call tmvb_group_topics: A K x M, B K x V, pc anything with doc_ptr / terms / counts, group[M] in [0, G) or -1.  Returns
    (status, dict) or (status, message): nothing raises here."""
    L = lib()
    try:
        f64 = lambda a: np.asfortranarray(np.asarray(a, dtype=np.float64))
        A, B = f64(A), f64(B)
        doc_ptr, terms, counts = _csr(pc.doc_ptr, pc.terms, pc.counts)
        M = len(doc_ptr) - 1
        K, V, G, n = int(K), int(V), int(G), int(topn)
        if A.shape != (K, M) or B.shape != (K, V):
            return 1, f"group_topics_raw: A must be of size ({K}, {M}) and B of size ({K}, {V})"
        g32 = _labels32(group, M)
        # sizes from the arguments alone, so that a bad argument reaches the library's own checks and not an allocation
        ok = 1 <= K <= 1024 and 1 <= G <= G_MAX and V >= 1 and K * V < 2 ** 31
        Gs, Ks, ns = (G, K, min(max(n, 1), TOPN_MAX)) if ok else (1, 1, 1)
        docs, tokens = np.zeros(Gs, dtype=np.int64), np.zeros(Gs, dtype=np.int64)
        mass = np.zeros((Gs, Ks), dtype=np.float64)
        top_idx, top_p = np.full((Gs, Ks, ns), -1, dtype=np.int32), np.zeros((Gs, Ks, ns), dtype=np.float64)
        sh = np.zeros((Gs, Ks), dtype=np.float64) if shift else None
        dr = np.zeros((Gs, Ks), dtype=np.float64) if drift else None
        dn = np.zeros((Gs, Ks, V if ok else 1), dtype=np.float64) if dense else None
    except (TypeError, ValueError, AttributeError, MemoryError) as e:
        return 1, f"group_topics_raw: {e}"
    info = GroupTopicsInfo()
    p = lambda a, ty: a.ctypes.data_as(ty) if a is not None else None
    rc = L.tmvb_group_topics(_handle(ctx), K, V, M, p(A, P_dbl), p(B, P_dbl), p(doc_ptr, P_i64), p(terms, P_i32), p(counts, P_i32), p(g32, P_i32), G,
                             float(eps), n, int(max_chunk_groups), p(docs, P_i64), p(tokens, P_i64), p(mass, P_dbl), p(top_idx, P_i32), p(top_p, P_dbl),
                             p(sh, P_dbl), p(dr, P_dbl), p(dn, P_dbl), C.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, {"docs": docs, "tokens": tokens, "mass": mass, "top_idx": top_idx, "top_p": top_p, "shift": sh, "drift": dr, "dense": dn,
                "info": {"nsel": int(info.nsel), "runs": int(info.runs), "segments": int(info.segments), "group_chunks": int(info.group_chunks),
                         "lanes_per_entry": int(info.lanes_per_entry), "ms_index": float(info.ms_index), "ms_accum": float(info.ms_accum),
                         "ms_select": float(info.ms_select), "ms_shift": float(info.ms_shift)}}


def group_index_raw(pc, group, G, V=None):
    """The host-only call tmvb_group_index: the selected entries in the order (group, term, document, position) and its runs.  Returns
    (status, dict(run_ptr, run_group, run_term, entry)) or (status, message)."""
    L = lib()
    try:
        doc_ptr, terms, _ = _csr(pc.doc_ptr, pc.terms, pc.counts)
        M = len(doc_ptr) - 1
        g32 = _labels32(group, M)
        V = int(pc.V if V is None else V)
        ok = M >= 1 and doc_ptr[0] == 0 and bool(np.all(np.diff(doc_ptr) >= 0)) and bool(np.all((g32 >= -1) & (g32 < int(G))))
        nsel = int(np.diff(doc_ptr)[g32 >= 0].sum()) if ok else 0
        run_ptr, entry = np.zeros(nsel + 1, dtype=np.int64), np.zeros(max(nsel, 1), dtype=np.int64)
        run_group, run_term = np.zeros(max(nsel, 1), dtype=np.int32), np.zeros(max(nsel, 1), dtype=np.int32)
    except (TypeError, ValueError, AttributeError) as e:
        return 1, f"group_index_raw: {e}"
    n_runs = C.c_int64(0)
    rc = L.tmvb_group_index(M, V, doc_ptr.ctypes.data_as(P_i64), terms.ctypes.data_as(P_i32), g32.ctypes.data_as(P_i32), int(G), C.byref(n_runs),
                            run_ptr.ctypes.data_as(P_i64), run_group.ctypes.data_as(P_i32), run_term.ctypes.data_as(P_i32), entry.ctypes.data_as(P_i64))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    r = int(n_runs.value)
    return rc, {"run_ptr": run_ptr[:r + 1], "run_group": run_group[:r], "run_term": run_term[:r], "entry": entry[:nsel]}


def time_bins(stamps, bins):
    """Labels for group_topics from numeric stamps (years, days, ...).  bins: an integer -- that many bins of equal width over [min, max] of the
    finite stamps -- or an ascending array of edges e_0 < ... < e_B.  Bin b is [e_b, e_b+1), the last one closed at e_B.  Returns a float array:
    the LEFT EDGE of every stamp's bin, NaN for a NaN stamp and for a stamp outside the edges (group_topics leaves those documents out)."""
    s = np.asarray(stamps, dtype=np.float64)
    if s.ndim != 1:
        raise ValueError("stamps must be a sequence of numbers.")
    if isinstance(bins, (int, np.integer)):
        fin = s[np.isfinite(s)]
        if bins < 1 or fin.size == 0:
            raise ValueError("bins must be a positive integer and at least one stamp finite.")
        lo, hi = float(fin.min()), float(fin.max())
        edges = np.linspace(lo, hi if hi > lo else lo + 1.0, int(bins) + 1)
    else:
        edges = np.asarray(bins, dtype=np.float64)
        if edges.ndim != 1 or edges.size < 2 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0):
            raise ValueError("bins must be an ascending array of at least two finite edges.")
    out = np.full(s.shape, np.nan)
    ok = np.isfinite(s) & (s >= edges[0]) & (s <= edges[-1])
    b = np.minimum(np.searchsorted(edges, s[ok], side="right") - 1, len(edges) - 2)
    out[ok] = edges[b]
    return out


def _is_missing(x):
    return x is None or (isinstance(x, (float, np.floating)) and x != x)


def _slopes(prev, present):
    """least-squares slope of every column of prev[G, K] against the row's position, over the rows marked present"""
    x = np.flatnonzero(present).astype(np.float64)
    if x.size < 2:
        return np.zeros(prev.shape[1])
    xc = x - x.mean()
    return (xc[:, None] * prev[present]).sum(axis=0) / (xc * xc).sum()


class GroupTopics:
    """labels[G] in the order of the groups; docs[G], tokens[G] (exact integers); mass[G, K] and prevalence[G, K] = mass / its row sum (NaN rows
    for a group without entries); theta_mean[G, K], the mean of topic_proportions over the group's documents; idx[G, K, topn] (0-based term
    ids, -1 for a group without entries), prob[G, K, topn], words[g][k] (the vocabulary's names, or the 1-based ids as strings); shift[G, K]
    and drift[G, K] (Jensen-Shannon divergence in nats from the pooled topic and from the previous group with entries; NaN where the group is
    empty, and for the first group's drift); trend[K], the least-squares slope of prevalence against the group's position (groups without
    entries left out); info: the library's tmvb_group_topics_info_t."""

    def __init__(self, labels, raw, theta_mean, vocab=None):
        self.labels = list(labels)
        self.docs, self.tokens, self.mass = raw["docs"], raw["tokens"], raw["mass"]
        self.idx, self.prob, self.info = raw["top_idx"], raw["top_p"], raw["info"]
        self.theta_mean = theta_mean
        present = self.tokens > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            self.prevalence = self.mass / self.mass.sum(axis=1, keepdims=True)
        self.prevalence[~present] = np.nan
        nan_rows = lambda a: None if a is None else np.where(present[:, None], a, np.nan)
        self.shift, self.drift = nan_rows(raw["shift"]), nan_rows(raw["drift"])
        if self.drift is not None and present.any():
            self.drift[int(np.argmax(present))] = np.nan
        self.trend = _slopes(self.prevalence, present)
        self._dense = raw["dense"]
        name = (lambda w: str(vocab[w + 1])) if vocab else (lambda w: str(w + 1))
        self.words = [[[name(int(w)) for w in row if w >= 0] for row in grp] for grp in self.idx]

    def hot(self, n: int = 5):
        """the n topics (0-based) whose prevalence rises fastest over the groups, steepest first (equal slopes: the lower topic first)"""
        return np.lexsort((np.arange(len(self.trend)), -self.trend))[:n]

    def cold(self, n: int = 5):
        """the n topics whose prevalence falls fastest"""
        return np.lexsort((np.arange(len(self.trend)), self.trend))[:n]

    def beta(self, g: int):
        """K x V: the topic-word matrix of group g (position in labels), S_g with every row normalised; needs dense=True"""
        if self._dense is None:
            raise ValueError("beta(g) needs group_topics(..., dense=True).")
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.mass[g][:, None] > 0, self._dense[g] / self.mass[g][:, None], 0.0)

    def __repr__(self):
        return f"GroupTopics(groups={len(self.labels)}, K={self.mass.shape[1]}, topn={self.idx.shape[2]})"


def _group_ids(groups, M, order):
    labels = list(groups)
    if len(labels) != M:
        raise ValueError(f"groups must hold one label per document ({M}).")
    present = [x for x in labels if not _is_missing(x)]
    if order is None:
        try:
            order = sorted(set(present))
        except TypeError:
            raise ValueError("the labels cannot be sorted: give order=.") from None
    order = list(order)
    pos = {lab: i for i, lab in enumerate(order)}
    if len(pos) != len(order) or not order:
        raise ValueError("order must hold every label once and at least one label.")
    if len(order) > G_MAX:
        raise ValueError(f"at most {G_MAX} groups.")
    missing = set(present) - set(pos)
    if missing:
        raise ValueError(f"labels not in order: {sorted(map(str, missing))[:5]}")
    return order, np.array([-1 if _is_missing(x) else pos[x] for x in labels], dtype=np.int32)


def group_topics(model, groups, topn: int = 10, order=None, corp=None, iter: int = 10, tol=None, dense: bool = False, device_id: int = 0) -> GroupTopics:
    """Topics by group.  groups: one hashable label per document of the model's corpus (None or NaN leaves the document out); order: the labels
    in the order the groups are to take (default: sorted), which is the order of drift and trend.  corp: a new corpus instead, folded in first
    with the family's own predict (iter / tol), as in token_topics.  LDA, CTM, CTPF and their gpu forms; fLDA / fCTM raise TopicModelError."""
    if not (isinstance(topn, (int, np.integer)) and 1 <= topn <= min(TOPN_MAX, model.V)):
        raise ValueError(f"topn must be an integer in [1, min({TOPN_MAX}, V)].")
    A, B = token_factors(model)                                     # raises for the filtered models before anything is folded in
    if corp is not None:
        model = _folded_in(model, corp, iter, tol, device_id)
        A, B = token_factors(model)
    labels, g = _group_ids(groups, model.M, order)
    with call_context(device_id) as ctx:
        rc, raw = group_topics_raw(ctx, model.K, model.V, A, B, model.corp, g, len(labels), topn=int(topn), dense=dense)
    check(rc)
    theta = topic_proportions(model)
    theta_mean = np.full((len(labels), model.K), np.nan)
    for i in range(len(labels)):
        if np.any(g == i):
            theta_mean[i] = theta[:, g == i].mean(axis=1)
    return GroupTopics(labels, raw, theta_mean, getattr(model.corp, "vocab", None))
