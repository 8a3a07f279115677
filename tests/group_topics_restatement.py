"""
NumPy restatement of tmvb_group_topics and tmvb_group_index (include/tmvb.h, "topics by group and over time"), in fp64 from the
definitions (a helper module of tests/test_group_topics_*.py: no fixtures, no test):

    index      np.lexsort on (position, document, term, group) of the entries of the documents with group >= 0; a run = one (group, term)
    S_g[k, w]  sum over the run's entries of c * r_k, r given per entry (the device's own phi bits, or tests/token_topics_restatement.py's)
    mass       row sums of S_g; beta_g = S_g / mass; selection by lexsort on (term id, -p); JS rows with math.fsum
    cut_mutant the library built with -DTMVB_MUTANT_GT_SEG_CUT=1: the last segment of every run longer than SEG is left out of S

Caps (u = 2^-53; every addend is nonnegative, so the bounds hold for every order of the additions):
    cap_S(n_run)    |S - S64| <= n_run u S          a sum of n_run nonnegative exact products: (n_run - 1) u relative to first order, for any tree
    cap_mass(n, V)  |mass - mass64| <= (n + V) u mass   the V run sums (each within n u, n the longest run of the row) added in any order: (V - 1) u more
    cap_js(V)       |JS - JS64| <= (V + 16) 2^-52, absolute: V addends whose absolute values total < ln 2 < 1 added in any order give at most
                    (V - 1) u x 1; an addend 0.5 (p log(2p / s) + q log(2q / s)) carries the roundings of s, the two quotients, the two logarithms
                    (1 ulp each, at arguments in (0, 2]: |log| error <= 2 u |log| + the quotient's u), the two products, the sum and the halving:
                    at most 8 u (p + q) per addend since |x log x| terms are bounded by the mass they weigh, and sum_w (p + q) = 2: 16 u in all;
                    V u + 16 u <= (V + 16) 2^-53, stated with 2^-52 for the first-order terms dropped.
"""
import math

import numpy as np

SEG = 512                               # TMVB_GT_SEG
U53 = 2.0 ** -53


def cap_S(n_run):
    return n_run * U53


def cap_mass(n_max, V):
    return (n_max + V) * U53


def cap_js(V):
    return (V + 16) * 2.0 ** -52


def index(doc_ptr, terms, group):
    """dict(entry, run_ptr, run_group, run_term, doc): the order tmvb_group_index returns"""
    doc_ptr, terms, group = np.asarray(doc_ptr, dtype=np.int64), np.asarray(terms, dtype=np.int64), np.asarray(group, dtype=np.int64)
    M = len(doc_ptr) - 1
    doc_of = np.repeat(np.arange(M), np.diff(doc_ptr))
    pos = np.arange(len(terms), dtype=np.int64)
    keep = group[doc_of] >= 0
    pos, d, w, g = pos[keep], doc_of[keep], terms[keep], group[doc_of][keep]
    o = np.lexsort((pos, d, w, g))
    pos, d, w, g = pos[o], d[o], w[o], g[o]
    new = np.ones(len(pos), dtype=bool)
    new[1:] = (g[1:] != g[:-1]) | (w[1:] != w[:-1])
    starts = np.flatnonzero(new)
    return {"entry": pos, "doc": d, "run_ptr": np.concatenate([starts, [len(pos)]]).astype(np.int64), "run_group": g[starts].astype(np.int32),
            "run_term": w[starts].astype(np.int32)}


def stats(r, doc_ptr, terms, counts, group, G, V, cut_mutant=False):
    """S[G, K, V] (fp64) from per-entry responsibilities r[nnz, K] (any float type, taken to fp64 exactly), with tokens[G], docs[G] and the
    longest run per group n_max[G].  Addends c * r are exact in fp64; a run is added by NumPy's sum in index order (under the exactness
    conditions of the GPU test every order gives the same bits; elsewhere the caps above absorb the order)."""
    ix = index(doc_ptr, terms, group)
    r = np.asarray(r).astype(np.float64)
    K = r.shape[1]
    counts, group = np.asarray(counts, dtype=np.int64), np.asarray(group, dtype=np.int64)
    S = np.zeros((G, K, V))
    n_max = np.zeros(G, dtype=np.int64)
    for u in range(len(ix["run_group"])):
        a, b = ix["run_ptr"][u], ix["run_ptr"][u + 1]
        if cut_mutant and b - a > SEG:
            b = a + ((b - a - 1) // SEG) * SEG                         # the last segment is left out
        e = ix["entry"][a:b]
        g, w = ix["run_group"][u], ix["run_term"][u]
        S[g, :, w] = (counts[e][:, None].astype(np.float64) * r[e]).sum(axis=0)
        n_max[g] = max(n_max[g], ix["run_ptr"][u + 1] - ix["run_ptr"][u])
    ptr = np.asarray(doc_ptr, dtype=np.int64)
    tokens, docs = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    for d in range(len(ptr) - 1):
        if group[d] >= 0:
            docs[group[d]] += 1
            tokens[group[d]] += int(counts[ptr[d]:ptr[d + 1]].sum())
    return {"S": S, "tokens": tokens, "docs": docs, "n_max": n_max}


def normalise(S, mass):
    """beta[G, K, V] = S / mass with 0 rows where mass is 0: the device's quotient when S and mass are the device's bits"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mass[..., None] > 0, S / mass[..., None], 0.0)


def select(beta, mass, n):
    """(idx[G, K, n], p[G, K, n]) under (p descending, term id ascending); -1 and 0 in the rows whose mass is 0"""
    G, K, V = beta.shape
    ids = np.broadcast_to(np.arange(V), beta.shape)
    order = np.lexsort((ids, -beta), axis=2)[:, :, :n]
    idx, p = order.astype(np.int32), np.take_along_axis(beta, order, axis=2)
    empty = ~(mass > 0)
    idx[empty] = -1
    p[empty] = 0.0
    return idx, p


def js_row(p, q):
    """the Jensen-Shannon divergence of two rows in nats: the addend of TMVB_TD_JS, summed with math.fsum, clamped at 0"""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    s = p + q
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.where(p > 0, p * np.log((2.0 * p) / s), 0.0)
        y = np.where(q > 0, q * np.log((2.0 * q) / s), 0.0)
    return max(0.0, math.fsum(0.5 * (x + y)))


def pooled(S):
    """the pooled row: the S_g added in ascending g, normalised by its row sums (fsum)"""
    pool = np.zeros(S.shape[1:])
    for g in range(S.shape[0]):
        pool = pool + S[g]
    tot = np.array([math.fsum(row) for row in pool])
    return normalise(pool[None], tot[None])[0]


def shift_drift(beta, present, pool):
    """shift[G, K] from the pooled row and drift[G, K] from the nearest lower group with entries; 0 where the definition says 0"""
    G, K, _ = beta.shape
    shift, drift = np.zeros((G, K)), np.zeros((G, K))
    prev = -1
    for g in range(G):
        if not present[g]:
            continue
        for k in range(K):
            shift[g, k] = js_row(beta[g, k], pool[k])
            if prev >= 0:
                drift[g, k] = js_row(beta[g, k], beta[prev, k])
        prev = g
    return shift, drift
