"""
NumPy fp64 restatement of the topic comparison (include/tmvb.h, "compare topics"), written from the header: every formula in the stated order.
Python loops run over the runs of TMVB_TD_RUN terms; inside a run the terms of all pairs are formed at once and added by numpy.cumsum, which
accumulates sequentially in ascending order (numpy.sum would add pairwise).  Operands here are ROW-major K x V arrays (a[i, w]).

Also: the cap of the tests' tolerance with the sum S it scales with, a brute-force assignment over all injections, the relevance scores, their
selection by lexsort, distinctiveness and saliency, and the generators of the test inputs.
"""
import itertools

import numpy as np

JS, HELLINGER, TV, KL = 0, 1, 2, 3
RUN = 256
KMAX = 4096
U = 2.0 ** -53


def seq_sum(t):
    """the last axis added sequentially ascending from 0"""
    if t.shape[-1] == 0:
        return np.zeros(t.shape[:-1])
    return np.cumsum(t, axis=-1)[..., -1]


def prepare(metric, x, smooth=0.0):
    x = np.asarray(x, dtype=np.float64)
    if metric == HELLINGER:
        return np.sqrt(x)
    if metric == KL:
        return (x + smooth) / (1.0 + float(x.shape[1]) * smooth)
    return x


def terms(metric, p, q):
    """(term, sum of the absolute values of the addend's components) of prepared, broadcastable p and q"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if metric == JS:
            s = p + q
            x = np.where(p > 0, p * np.log((2.0 * p) / s), 0.0)
            y = np.where(q > 0, q * np.log((2.0 * q) / s), 0.0)
            return 0.5 * (x + y), 0.5 * (np.abs(x) + np.abs(y))
        if metric == HELLINGER:
            d = p - q
            t = 0.5 * (d * d)
            return t, t
        if metric == TV:
            t = 0.5 * np.abs(p - q)
            return t, t
        t = np.where(p > 0, p * np.log(p / q), 0.0)
        return t, np.abs(t)


def divergence(metric, a, b=None, smooth=0.0, drop_tail=False):
    """(D, sigma, S): the result, the sum before max(0, .) / sqrt, and S = the sum of the absolute values of the addends' components.
    drop_tail: the last, partial run is left out (what the negative control of the suite computes)."""
    A = prepare(metric, a, smooth)
    B = A if b is None else prepare(metric, b, smooth)
    V = A.shape[1]
    runs = V // RUN if drop_tail else (V + RUN - 1) // RUN
    sigma = np.zeros((A.shape[0], B.shape[0]))
    S = np.zeros_like(sigma)
    for r in range(runs):
        w0, w1 = r * RUN, min((r + 1) * RUN, V)
        t, s = terms(metric, A[:, None, w0:w1], B[None, :, w0:w1])
        sigma = sigma + seq_sum(t)
        S = S + s.sum(axis=-1)
    if metric in (JS, KL):
        D = np.maximum(0.0, sigma)
    elif metric == HELLINGER:
        D = np.sqrt(sigma)
    else:
        D = sigma
    return D, sigma, S


def cap_factor(V):
    """worst case of the blocked sequential sum -- a run of min(V, RUN) terms, then `runs` run sums -- plus 8 ulps for log, divide and products"""
    return (min(V, RUN) + (V + RUN - 1) // RUN + 8) * U


# ------------------------------------------------------------------------------------------------------------------ inputs
def exact_rows(K, V, seed):
    """rows of integers / 2^10 summing to 1: every partial sum of 0.5 |p - q| is a multiple of 2^-11 below 2, exact in any order"""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.full(V, 0.3)) if V > 1 else np.ones(1)
    return rng.multinomial(1024, w, size=K).astype(np.float64) / 1024.0


def dirichlet_rows(K, V, seed, shift=0):
    """row r at concentration (0.01, 0.1, 1)[(r + shift) % 3], a fifth of the entries set to exactly 0, renormalised"""
    rng = np.random.default_rng(seed)
    out = np.zeros((K, V))
    for r in range(K):
        c = (0.01, 0.1, 1.0)[(r + shift) % 3]
        x = rng.dirichlet(np.full(V, c)) if V > 1 else np.ones(1)
        z = rng.random(V) < 0.2
        z[int(np.argmax(x))] = False
        x = np.where(z, 0.0, x)
        out[r] = x / x.sum()
    return out


# ------------------------------------------------------------------------------------------------------------------ assignment
def brute_force_assignment(cost):
    """min over all injections rows -> columns of the total cost: (total, the set of optimal injections)"""
    cost = np.asarray(cost, dtype=np.float64)
    n, m = cost.shape
    best, arg = np.inf, []
    for cols in itertools.permutations(range(m), n):
        t = 0.0
        for i, j in enumerate(cols):
            t += cost[i, j]
        if t < best:
            best, arg = t, [cols]
        elif t == best:
            arg.append(cols)
    return best, arg


# ------------------------------------------------------------------------------------------------------------------ relevance
def relevance(beta, pw, lam):
    """(r[K, V], |lam log phi| + |(1 - lam) log(phi / pw)|)"""
    beta, pw = np.asarray(beta, dtype=np.float64), np.asarray(pw, dtype=np.float64)
    ok = (beta > 0) & (pw > 0)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = lam * np.log(beta)
        t2 = (1.0 - lam) * np.log(beta / pw[None, :])
    r = np.where(ok, (t1 + t2) + 0.0, -np.inf)
    return r, np.where(ok, np.abs(t1) + np.abs(t2), 0.0)


def select(dense, n):
    """(idx[K, n], score[K, n], count[K]) under (score descending, term id ascending)"""
    K, V = dense.shape
    idx = np.full((K, n), -1, dtype=np.int32)
    score = np.full((K, n), -np.inf)
    count = np.zeros(K, dtype=np.int32)
    for k in range(K):
        order = np.lexsort((np.arange(V), -dense[k]))[:n]
        fin = np.isfinite(dense[k, order])
        c = int(fin.sum())
        idx[k, :c], score[k, :c], count[k] = order[:c], dense[k, order[:c]], c
    return idx, score, count


def term_stats(beta, pw, pi):
    """(distinct[V], saliency[V], sum of |addends| of distinct): sums over k ascending from 0"""
    beta, pw, pi = (np.asarray(x, dtype=np.float64) for x in (beta, pw, pi))
    K, V = beta.shape
    den = np.zeros(V)
    for k in range(K):
        den = den + pi[k] * beta[k]
    d, S = np.zeros(V), np.zeros(V)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(K):
            P = (pi[k] * beta[k]) / den
            t = np.where((den > 0) & (P > 0), P * np.log(P / pi[k]), 0.0)
            d, S = d + t, S + np.abs(t)
    return d, pw * d, S


def relevance_inputs(K, V, seed):
    """beta with exact zeros and, for V >= 5, two duplicated columns (column 3 = column 1, column V - 1 = column 2, in beta and in pw alike: exact
    ties of the score), a zero of pw for V > 6, and pi.  Rows are divided by their sums last, which keeps equal entries equal."""
    rng = np.random.default_rng(seed)
    beta = rng.dirichlet(np.full(V, 0.2), size=K) if V > 1 else np.ones((K, 1))
    pw = rng.dirichlet(np.full(V, 0.5)) if V > 1 else np.ones(1)
    if V >= 5:
        beta[rng.random((K, V)) < 0.15] = 0.0
        beta[:, 0] = np.maximum(beta[:, 0], 1e-3)                  # no empty row
        for src, dst in ((1, 3), (2, V - 1)):
            beta[:, dst], pw[dst] = beta[:, src], pw[src]
        if V > 6:
            pw[5] = 0.0
    beta = beta / beta.sum(axis=1, keepdims=True)
    pw = pw / pw.sum()
    pi = rng.dirichlet(np.full(K, 2.0)) if K > 1 else np.ones(1)
    return beta, pw, pi
