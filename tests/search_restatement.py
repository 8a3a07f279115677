"""
NumPy restatement of the word search (tmvb_topic_search, include/tmvb.h) -- the yardstick of tests/test_search_host.py and
tests/test_search_gpu.py; the reference has no such function.

  * `beta_prime`: (beta + s) / (1 + s V) in fp64;
  * `s64`: score(q, d) = sum_j c_j log(theta_d . beta'_{w_j}), everything in fp64, j in the query's own order;
  * `p_chain32` / `score_emulated`: the device's arithmetic said again -- features rounded once to fp32, the accumulator chain
    acc = float32(float64(acc) + float64(a) float64(b)) over k ascending, the fp64 log, the sum in j order in one fp64 accumulator, one
    rounding to fp32;
  * `cap`: C_q (K + 3) 2^-24 + |s64| 2^-24, C_q = the query's sum of counts.  First term: one rounding per feature and one per fmaf on a sum of
    nonnegative terms -- the relative error of p, which is the absolute error of log p, c_j times per entry; second term: the final rounding;
  * `np_topn`: the n best columns of every row under the total order (score descending, index ascending) by np.lexsort;
  * `make_queries`, `dirichlet_cols`, `dirichlet_beta`: the seeded inputs the two modules share.
"""
import numpy as np

TILE_COLS = 128


def cap_coeff(K):
    """the per-token part of the cap: (K + 3) 2^-24"""
    return (K + 3) * 2.0 ** -24


def beta_prime(beta, s):
    beta = np.asarray(beta, dtype=np.float64)
    return (beta + s) / (1.0 + s * beta.shape[1])


def dirichlet_cols(K, M, alpha, seed):
    """K x M fp64, columns ~ Dirichlet(alpha), renormalised in fp64"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = rng.standard_gamma(alpha, size=(K, M)) + 1e-300
    return g / g.sum(axis=0)


def dirichlet_beta(K, V, alpha, seed):
    """K x V fp64, rows ~ Dirichlet(alpha): right stochastic"""
    return np.ascontiguousarray(dirichlet_cols(V, K, alpha, seed).T)


def make_queries(lengths, V, seed, max_count=3):
    """a CSR of len(lengths) queries: q_ptr int64, q_terms int32 0-based (drawn with replacement: an id may repeat inside a query), q_counts
    int32 in [1, max_count]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    W = int(ptr[-1])
    return ptr, rng.integers(0, V, size=W).astype(np.int32), rng.integers(1, max_count + 1, size=W).astype(np.int32)


def slice_queries(q_ptr, q_terms, q_counts, sel):
    """the queries `sel` (any order) as their own CSR"""
    ptr = [0]
    t, c = [], []
    for q in sel:
        a, b = int(q_ptr[q]), int(q_ptr[q + 1])
        t.append(q_terms[a:b]); c.append(q_counts[a:b]); ptr.append(ptr[-1] + b - a)
    return np.asarray(ptr, dtype=np.int64), np.concatenate(t).astype(np.int32), np.concatenate(c).astype(np.int32)


def tokens(q_ptr, q_counts):
    return np.add.reduceat(np.asarray(q_counts, dtype=np.int64), np.asarray(q_ptr[:-1], dtype=np.int64))


def _segment_sum(logp, q_ptr, q_counts):
    """logp: Md x W fp64 -> Q x Md: sum over each query's entries in ascending j, one accumulator"""
    Q = len(q_ptr) - 1
    out = np.zeros((Q, logp.shape[0]))
    for q in range(Q):
        acc = np.zeros(logp.shape[0])
        for j in range(int(q_ptr[q]), int(q_ptr[q + 1])):
            acc = acc + float(q_counts[j]) * logp[:, j]
        out[q] = acc
    return out


def s64(theta, beta, s, q_ptr, q_terms, q_counts):
    """Q x Md fp64 scores; -inf where an entry has probability 0"""
    bp = beta_prime(beta, s)[:, q_terms]                              # K x W
    p = np.asarray(theta, dtype=np.float64).T @ bp                    # Md x W
    with np.errstate(divide="ignore"):
        return _segment_sum(np.log(p), q_ptr, q_counts)


def p_chain32(theta, beta, s, q_terms):
    """Md x W float32: the fp32 accumulator chain over k ascending from 0"""
    a = np.asarray(theta, dtype=np.float64).T.astype(np.float32)      # Md x K, each value rounded once
    b = beta_prime(beta, s)[:, q_terms].astype(np.float32)            # K x W, each value rounded once
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, k, None].astype(np.float64) * b[None, k, :].astype(np.float64)).astype(np.float32)
    return acc


def score_emulated(theta, beta, s, q_ptr, q_terms, q_counts):
    """Q x Md float32: the device's arithmetic said again in NumPy"""
    p = p_chain32(theta, beta, s, q_terms)
    with np.errstate(divide="ignore"):
        return _segment_sum(np.log(p.astype(np.float64)), q_ptr, q_counts).astype(np.float32)


def cap(K, S64, C):
    """Q x Md: C_q (K + 3) 2^-24 + |s64| 2^-24"""
    return np.asarray(C, dtype=np.float64)[:, None] * cap_coeff(K) + np.abs(S64) * 2.0 ** -24


def np_topn(S, n):
    """(idx[Q, n] int32, score[Q, n] of S's dtype, count[Q]): per row of S the n best columns, score descending, index ascending on equal
    scores (-inf is a score like any other); -1 / -inf past count"""
    Q, Md = S.shape
    idx = np.full((Q, n), -1, dtype=np.int32)
    score = np.full((Q, n), -np.inf, dtype=S.dtype)
    count = np.zeros(Q, dtype=np.int32)
    cols = np.arange(Md)
    for q in range(Q):
        order = np.lexsort((cols, -S[q]))[:n]
        idx[q, :len(order)] = order
        score[q, :len(order)] = S[q, order]
        count[q] = len(order)
    return idx, score, count
