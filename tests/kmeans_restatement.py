"""
NumPy restatement of tmvb_topic_kmeans (include/tmvb.h, "cluster documents in topic space"): the yardstick of tests/test_kmeans_host.py and
tests/test_kmeans_gpu.py -- the reference has no such function.  NumPy only; the Philox is the one tests/test_heldout_host.py holds to the
library's own.

  features32            the three transforms in fp64, ONE rounding to fp32 (COSINE: the norm in the device's order, lane-strided fma sums and
                        an xor butterfly; the fma is exact here only while every lane holds one term, K <= 64, and else a plain multiply-add
                        -- the floating tests do not need the last bit of a COSINE feature);
  chain32 / assign32    the fp32 fmaf chain over k ascending and the assignment rule on it: a + b_c, lowest c on equal s, dist2 = max(0,
                        fmaf(-2, s, n_d)).  fmaf is restated as a fp64 multiply-add rounded to fp32: exact whenever the fp64 sum is (always on
                        the integer cases, which are the ones compared bit for bit);
  blocked_sum           the fixed order of J: blocks of RUN ascending, each added sequentially, the block sums added sequentially;
  update32              the fixed-order mean of the members' fp32 rows: runs of RUN members, fp64;
  seeding               k-means++ exactly as the header states it, every fp64 operation in the stated order;
  lloyd64               Lloyd's loop in fp64 on the fp64 features from given c^0, recording per iteration the smallest gap between a document's
                        best and second-best score -- the admissibility measure of the free-running comparison;
  lloyd32               the contract's loop on the restated fp32 pieces (stops included).
"""
import numpy as np

EUCLID, HELLINGER, COSINE = 0, 1, 2
RUN = 256
RNG_KMEANS = 8
MASK = np.uint64(0xFFFFFFFF)


def cap(K):
    """bound on |s - s64| for features and centroids of norm <= 1 with nonnegative entries, u = 2^-24: the rounding of the features moves
    a = f.c by at most u |f||c| <= u (the centroid is taken as returned: it is the same number on both sides); the K fmaf of the chain add at
    most u each on partial sums <= 1; b_c = -n_c / 2 carries half of the K roundings of its own chain; the final add rounds a number of
    magnitude <= 1 once: (1 + K + K / 2 + 1) u = (1.5 K + 2) u to first order.  The terms of second order -- partial sums above 1 by K u, a
    centroid whose norm passes 1 by its own rounding -- stay below 2 u up to K = 1024: (1.5 K + 4) u."""
    return (1.5 * K + 4) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ Philox, uniforms
def uniforms(seed, n):
    """u_j = tmvb_u53(x[0], x[1]) of tmvb_rng(seed, j, TMVB_RNG_KMEANS, 0, 0), j = 0 .. n - 1"""
    from test_heldout_host import philox4x32_10
    j = np.arange(n, dtype=np.uint64)
    seed = np.uint64(int(seed) % 2 ** 64)
    ctr = np.stack([j & MASK, j >> np.uint64(32), np.full(n, RNG_KMEANS, dtype=np.uint64), np.zeros(n, dtype=np.uint64)], axis=1)
    key = np.stack([np.full(n, seed & MASK), np.full(n, seed >> np.uint64(32))], axis=1)
    w = philox4x32_10(ctr, key).astype(np.uint64)
    b = ((w[:, 0] << np.uint64(32)) | w[:, 1]) >> np.uint64(11)
    return b.astype(np.float64) * (1.0 / 9007199254740992.0)


# ------------------------------------------------------------------------------------------------------------------ features
def features64(x, metric):
    """K x M fp64 -> M x K fp64 features, nothing rounded to fp32"""
    x = np.asarray(x, dtype=np.float64).T
    if metric == HELLINGER:
        return np.sqrt(x)
    if metric == COSINE:
        return x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x.copy()


def cosine_norm_device_order(x):
    """M x K fp64 -> M: lane l adds x_k^2 over k = l, l + 64, ...; then v += v[lane ^ o] for o = 32, 16, .., 1"""
    M, K = x.shape
    v = np.zeros((M, 64))
    for k0 in range(0, K, 64):
        blk = x[:, k0:k0 + 64]
        v[:, :blk.shape[1]] = blk * blk + v[:, :blk.shape[1]]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return np.sqrt(v[:, 0])


def features32(x, metric):
    """K x M fp64 -> M x K fp32 features, each value rounded once"""
    x = np.asarray(x, dtype=np.float64).T
    if metric == HELLINGER:
        return np.sqrt(x).astype(np.float32)
    if metric == COSINE:
        return (x / cosine_norm_device_order(x)[:, None]).astype(np.float32)
    return x.astype(np.float32)


def fmaf32(a, b, c):
    """fp32 fmaf(a, b, c): the product of two fp32 is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def chain32(A, B):
    """A: m x K fp32, B: n x K fp32 -> m x n fp32: fmaf chain over k ascending from 0"""
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for k in range(A.shape[1]):
        acc = fmaf32(A[:, k:k + 1], B[None, :, k], acc)
    return acc


def norm32(F):
    """n = the fp32 fmaf chain of f^2 over k ascending"""
    F = np.asarray(F, dtype=np.float32)
    n = np.zeros(F.shape[0], dtype=np.float32)
    for k in range(F.shape[1]):
        n = fmaf32(F[:, k], F[:, k], n)
    return n


# ------------------------------------------------------------------------------------------------------------------ fixed-order sums
def seq_sum(v):
    """v[0] + v[1] + ... added one after the other in fp64 (np.cumsum is sequential)"""
    v = np.asarray(v, dtype=np.float64)
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def blocked_sum(v):
    v = np.asarray(v, dtype=np.float64)
    return seq_sum([seq_sum(v[i:i + RUN]) for i in range(0, len(v), RUN)])


# ------------------------------------------------------------------------------------------------------------------ assign, update
def assign32(F, Cf, no_bias=False):
    """(label int32, dist2 fp32, count int64, J, s fp32 [M, C]) of the assignment rule on fp32 features F[M, K] and centroids Cf[C, K]"""
    F, Cf = np.asarray(F, dtype=np.float32), np.asarray(Cf, dtype=np.float32)
    b = (np.float32(-0.5) * norm32(Cf)).astype(np.float32)
    s = chain32(F, Cf) if no_bias else (chain32(F, Cf) + b[None, :]).astype(np.float32)
    label = np.argmax(s, axis=1).astype(np.int32)                    # the first of equal maxima: the lowest c
    best = s[np.arange(len(F)), label]
    dist2 = np.maximum(np.float32(0), fmaf32(np.float32(-2), best, norm32(F)))
    return label, dist2, np.bincount(label, minlength=len(Cf)).astype(np.int64), blocked_sum(dist2), s


def update32(F, label, Cf, metric):
    """the centroids after one update: fixed-order fp64 mean of the members' fp32 rows; a cluster without members keeps its row of Cf"""
    F = np.asarray(F, dtype=np.float32)
    out = np.array(Cf, dtype=np.float32, copy=True)
    for c in range(len(out)):
        mem = np.flatnonzero(np.asarray(label) == c)
        if len(mem) == 0:
            continue
        runs = [np.cumsum(F[mem[i:i + RUN]].astype(np.float64), axis=0)[-1] for i in range(0, len(mem), RUN)]
        tot = np.cumsum(np.stack(runs), axis=0)[-1]
        out[c] = (tot / np.sqrt((tot * tot).sum()) if metric == COSINE else tot / float(len(mem))).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------------------ seeding
def seeding(F, C, seed):
    """the document ids of k-means++ on fp32 features F[M, K]"""
    F64 = np.asarray(F, dtype=np.float32).astype(np.float64)
    M = len(F64)
    u = uniforms(seed, C)
    N = np.cumsum(F64 * F64, axis=1)[:, -1]                          # every product exact, the sum sequential over k
    picks = [min(M - 1, int(np.floor(u[0] * M)))]
    m = None
    for j in range(1, C):
        s = picks[-1]
        dot = np.cumsum(F64 * F64[s][None, :], axis=1)[:, -1]
        D2 = np.maximum(0.0, (N + N[s]) - 2.0 * dot)
        m = D2 if m is None else np.minimum(m, D2)
        bsum = [seq_sum(m[i:i + RUN]) for i in range(0, M, RUN)]
        total = seq_sum(bsum)
        thr = u[j] * total
        pick, P = -1, 0.0
        if total > 0.0:
            for b, B in enumerate(bsum):
                if P + B > thr:
                    cum = P + np.cumsum(m[b * RUN:(b + 1) * RUN])
                    pick = b * RUN + int(np.flatnonzero(cum > thr)[0])
                    break
                P = P + B
        if pick < 0:
            pick = min(set(range(M)) - set(picks))
        picks.append(pick)
    return np.asarray(picks, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------ Lloyd
def scores64(F64, C64):
    return F64 @ C64.T - 0.5 * (C64 * C64).sum(axis=1)[None, :]


def lloyd64(F64, c0, metric, max_iter=100):
    """Lloyd's loop in fp64.  Returns dict(label, centroids, iters, stop, inertia[iters + 1], gaps[iters + 1], labels = the label vector of every
    iteration); gaps[t] = min over documents of (best - second best) score at iteration t (inf with one cluster)."""
    F64, c = np.asarray(F64, dtype=np.float64), np.array(c0, dtype=np.float64, copy=True)
    prev, t, stop, inertia, gaps, labels = None, 0, 0, [], [], []
    while True:
        s = scores64(F64, c)
        label = np.argmax(s, axis=1)
        top2 = np.sort(s, axis=1)[:, -2:]
        gaps.append(float((top2[:, -1] - top2[:, 0]).min()) if s.shape[1] > 1 else float("inf"))
        d2 = np.maximum(0.0, (F64 * F64).sum(axis=1) - 2.0 * s[np.arange(len(F64)), label])
        inertia.append(float(d2.sum()))
        labels.append(label)
        if prev is not None and np.array_equal(prev, label):
            stop = 1
            break
        if t == max_iter:
            break
        for k in range(len(c)):
            mem = label == k
            if mem.any():
                tot = F64[mem].sum(axis=0)
                c[k] = tot / np.sqrt((tot * tot).sum()) if metric == COSINE else tot / mem.sum()
        prev, t = label, t + 1
    return {"label": label.astype(np.int32), "centroids": c, "iters": t, "stop": stop, "inertia": np.asarray(inertia), "gaps": np.asarray(gaps), "labels": labels}


def lloyd32(F, c0, metric, max_iter=100, tol=0.0):
    """the contract's loop on the restated fp32 pieces"""
    c = np.array(c0, dtype=np.float32, copy=True)
    prev, t, stop, inertia = None, 0, 0, []
    while True:
        label, dist2, count, J, _ = assign32(F, c)
        inertia.append(J)
        if t >= 1 and np.array_equal(prev, label):
            stop = 1
            break
        if t == max_iter:
            stop = 0
            break
        if tol > 0.0 and t >= 1 and inertia[t - 1] - J <= tol * inertia[t - 1]:
            stop = 2
            break
        c = update32(F, label, c, metric)
        prev, t = label, t + 1
    return {"label": label, "centroids": c, "count": count, "dist2": dist2, "iters": t, "stop": stop, "inertia": np.asarray(inertia)}


# ------------------------------------------------------------------------------------------------------------------ inputs
def integer_cols(K, M, seed, levels=(0, 1, 2, 7)):
    """K x M fp64 drawn from few integer levels in [0, 7]: ties everywhere, every score an exact small number"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.choice(np.asarray(levels, dtype=np.float64), size=(K, M))


def dirichlet_cols(K, M, alpha, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    g = rng.standard_gamma(alpha, size=(K, M)) + 1e-300
    return g / g.sum(axis=0)


def planted_mixture(K, M, groups, seed, conc=30.0):
    """K x M topic proportions: document d ~ Dirichlet(conc * centre of group d mod groups + 0.02), the centres Dirichlet(0.3) draws"""
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = rng.dirichlet(np.full(K, 0.3), size=groups)
    g = rng.standard_gamma(conc * centres[np.arange(M) % groups] + 0.02) + 1e-300
    return np.ascontiguousarray((g / g.sum(axis=1, keepdims=True)).T)
