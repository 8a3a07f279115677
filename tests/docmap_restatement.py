"""
NumPy fp64 restatement of tmvb_map_affinity and tmvb_map_layout, written from include/tmvb.h ("map documents in two dimensions") alone: the entropy
search on its fixed schedule, the symmetrisation, the forces, the fp32 update bit for bit, the blocked sums bit for bit (np.cumsum is sequential),
the KL divergence and the Philox start.  The repulsion is restated in fp64 -- the device's fp32 chain is bounded against it, not reproduced.
"""
import numpy as np

BISECT, RUN, SEG, SLOTS = 64, 256, 64, 64
RNG_MAP = 9
U24 = 2.0 ** -24
REP_CAP = (RUN + 24) * U24          # |rep - rep64| <= REP_CAP sum_j |w dx|
Z_CAP = (RUN + 8) * U24             # |zrow - z64| <= Z_CAP sum_j q


# ------------------------------------------------------------------------------------------------------------------ Philox start
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    M0, M1, W0, W1, m32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & m32 for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & m32, int(k1) & m32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & m32, (k1 + W1) & m32
    return c0, c1, c2, c3


def init_y(M, seed):
    """y_ic = (float)(1e-4 (2 u - 1)), u = the 53-bit uniform of tmvb_rng(seed, i, TMVB_RNG_MAP, c, 0)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.arange(M, dtype=np.uint64)
    y = np.zeros((M, 2), dtype=np.float32)
    for c in range(2):
        x0, x1, _, _ = philox4x32_10(i, i >> np.uint64(32), np.full(M, RNG_MAP | (c << 8), dtype=np.uint64), np.zeros(M, dtype=np.uint64), seed, seed >> 32)
        u = ((x0 << np.uint64(32) | x1) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        y[:, c] = (1e-4 * (2.0 * u - 1.0)).astype(np.float32)
    return y


# ------------------------------------------------------------------------------------------------------------------ affinity
def row_entropy(delta, beta):
    e = np.exp(-beta * delta)
    S = e.sum()
    return np.log(S) + beta * (delta * e).sum() / S


def row_p(delta, beta):
    e = np.exp(-beta * delta)
    return e / e.sum()


def row_beta(delta, u):
    """the fixed schedule: BISECT evaluations, no early exit"""
    logu, beta, lo, hi = np.log(u), 1.0, 0.0, np.inf
    for _ in range(BISECT):
        if row_entropy(delta, beta) > logu:
            lo = beta
            beta = 2.0 * beta if np.isinf(hi) else 0.5 * (beta + hi)
        else:
            hi = beta
            beta = 0.5 * (lo + beta)
    return beta


def affinity(d2, count, u, beta=None):
    """beta[M], p_cond[M, n]; beta given: p_cond at THAT beta (rows with n_i <= u stay uniform)"""
    M, n = d2.shape
    out_b, p = np.zeros(M), np.zeros((M, n))
    for i in range(M):
        ni = int(count[i])
        if ni == 0:
            continue
        if ni <= u:
            p[i, :ni] = 1.0 / ni
            continue
        D = d2[i, :ni].astype(np.float64)
        delta = D - D.min()
        out_b[i] = row_beta(delta, u) if beta is None else beta[i]
        p[i, :ni] = row_p(delta, out_b[i])
    return out_b, p


def reachable(d2, count, u):
    """rows whose entropy can equal log u: more than u neighbours, fewer than u of them at the minimum distance"""
    out = np.zeros(len(count), dtype=bool)
    for i in range(len(count)):
        ni = int(count[i])
        if ni > u:
            D = d2[i, :ni]
            out[i] = (D == D.min()).sum() < u
    return out


def symmetrize(idx, p, count):
    """row_ptr, col (ascending in a row), val = float32((a + b) / (2 M))"""
    M = idx.shape[0]
    a = {}
    for i in range(M):
        for s in range(int(count[i])):
            a[(i, int(idx[i, s]))] = p[i, s]
    keys = sorted(set(a) | {(j, i) for (i, j) in a})
    row_ptr = np.zeros(M + 1, dtype=np.int64)
    col, val = np.zeros(len(keys), dtype=np.int32), np.zeros(len(keys), dtype=np.float32)
    for k, (i, j) in enumerate(keys):
        row_ptr[i + 1] += 1
        col[k] = j
        val[k] = np.float32((a.get((i, j), 0.0) + a.get((j, i), 0.0)) / (2.0 * M))
    return np.cumsum(row_ptr), col, val


# ------------------------------------------------------------------------------------------------------------------ sums
def seq_sum(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def blocked(v):
    """blocks of RUN rows, each added sequentially ascending from 0, the block sums added sequentially ascending from 0"""
    v = np.asarray(v, dtype=np.float64)
    return seq_sum([seq_sum(v[b:b + RUN]) for b in range(0, len(v), RUN)])


# ------------------------------------------------------------------------------------------------------------------ forces
def repulsion64(y, rows=None):
    """fp64 from the fp32 y, self term included in z: rep[r, 2], z[r], and the sums of the error model: sum |w dx| [r, 2], sum q [r]"""
    y = np.asarray(y, dtype=np.float64)
    rows = np.arange(len(y)) if rows is None else np.asarray(rows)
    rep, z, aw, sq = np.zeros((len(rows), 2)), np.zeros(len(rows)), np.zeros((len(rows), 2)), np.zeros(len(rows))
    for b in range(0, len(rows), 128):
        r = rows[b:b + 128]
        d = y[r][:, None, :] - y[None, :, :]
        q = 1.0 / (1.0 + (d * d).sum(axis=2))
        w = (q * q)[:, :, None] * d
        rep[b:b + 128], z[b:b + 128], aw[b:b + 128], sq[b:b + 128] = w.sum(axis=1), q.sum(axis=1), np.abs(w).sum(axis=1), q.sum(axis=1)
    return rep, z, aw, sq


def edges(row_ptr, col):
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr)), np.asarray(col[:row_ptr[-1]], dtype=np.int64)


def attraction64(y, row_ptr, col, val):
    """att[M, 2] and sum |terms| [M, 2] (the scale of the comparison)"""
    y = np.asarray(y, dtype=np.float64)
    i, j = edges(row_ptr, col)
    d = y[i] - y[j]
    t = (val[:len(i)].astype(np.float64) / (1.0 + (d * d).sum(axis=1)))[:, None] * d
    att, ab = np.zeros((len(y), 2)), np.zeros((len(y), 2))
    np.add.at(att, i, t)
    np.add.at(ab, i, np.abs(t))
    return att, ab


def kl64(y, row_ptr, col, val):
    y = np.asarray(y, dtype=np.float64)
    Z = repulsion64(y)[1].sum() - len(y)
    i, j = edges(row_ptr, col)
    d = y[i] - y[j]
    p = val[:len(i)].astype(np.float64)
    ok = p > 0
    return float((p[ok] * np.log(p[ok] * Z * (1.0 + (d[ok] * d[ok]).sum(axis=1)))).sum())


def gradient64(y, row_ptr, col, val, e=1.0):
    y = np.asarray(y, dtype=np.float64)
    dx, dy = y[:, 0][:, None] - y[:, 0][None, :], y[:, 1][:, None] - y[:, 1][None, :]
    q = 1.0 / (1.0 + dx * dx + dy * dy)
    w = q * q
    rep = np.stack([(w * dx).sum(axis=1), (w * dy).sum(axis=1)], axis=1)
    i, j = edges(row_ptr, col)
    t = (val[:len(i)].astype(np.float64) * q[i, j])[:, None] * (y[i] - y[j])
    att = np.stack([np.bincount(i, t[:, c], minlength=len(y)) for c in range(2)], axis=1)
    return 4.0 * (e * att - rep / (q.sum() - len(y)))


def grad32(att, rep, Z, e):
    """g = (float)(4.0 * (e * att - rep / Z)), every operation rounded on its own"""
    return (4.0 * (np.float64(e) * att - rep / np.float64(Z))).astype(np.float32)


def update32(g, y, vel, gain, mu, eta, min_gain):
    """the fp32 update and recentring, bit for bit: (y, vel, gain)"""
    g, y, vel, gain = (np.asarray(a, dtype=np.float32) for a in (g, y, vel, gain))
    mu, eta, min_gain = np.float32(mu), np.float32(eta), np.float32(min_gain)
    differ = ((vel > 0) & (g < 0)) | ((vel < 0) & (g > 0))
    gain = np.where(differ, gain + np.float32(0.2), gain * np.float32(0.8)).astype(np.float32)
    gain = np.maximum(gain, min_gain)
    vel = (mu * vel - (eta * gain) * g).astype(np.float32)
    y1 = (y + vel).astype(np.float32)
    mean = np.array([np.float32(blocked(y1[:, c]) / float(len(y1))) for c in range(2)], dtype=np.float32)
    return (y1 - mean).astype(np.float32), vel, gain


def layout64(y, row_ptr, col, val, iters, iter0=0, vel=None, gain=None, eta=200.0, exaggeration=12.0, exag_iters=250, momentum0=0.5, momentum1=0.8,
             min_gain=0.01):
    """the descent in fp64 throughout: (y, vel, gain)"""
    y = np.asarray(y, dtype=np.float64).copy()
    vel = np.zeros_like(y) if vel is None else np.asarray(vel, dtype=np.float64).copy()
    gain = np.ones_like(y) if gain is None else np.asarray(gain, dtype=np.float64).copy()
    for t in range(iter0, iter0 + iters):
        early = t < exag_iters
        g = gradient64(y, row_ptr, col, val, exaggeration if early else 1.0)
        differ = ((vel > 0) & (g < 0)) | ((vel < 0) & (g > 0))
        gain = np.maximum(np.where(differ, gain + 0.2, gain * 0.8), min_gain)
        vel = (momentum0 if early else momentum1) * vel - eta * gain * g
        y = y + vel
        y = y - y.mean(axis=0)
    return y, vel, gain


# ------------------------------------------------------------------------------------------------------------------ inputs
def knn(x, n, metric="hellinger"):
    """what tmvb_topic_neighbors returns, restated in fp64 (idx, d2 fp32, count): for the host tests"""
    f = np.sqrt(x) if metric == "hellinger" else x / np.sqrt((x * x).sum(axis=0))
    s = f.T @ f
    np.fill_diagonal(s, -np.inf)
    M = x.shape[1]
    idx = np.argsort(-s, axis=1, kind="stable")[:, :n].astype(np.int32)
    d2 = np.maximum(0.0, 2.0 - 2.0 * np.take_along_axis(s, idx, axis=1)).astype(np.float32)
    return idx, d2, np.full(M, n, dtype=np.int32)


def planted_theta(M=600, K=12, groups=5, seed=0, conc=200.0):
    """five groups: theta_d ~ Dirichlet(conc c_g + 0.05), c_g ~ Dirichlet(0.3); K x M and the group of every document"""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.dirichlet(np.full(K, 0.3), size=groups)
    g = np.arange(M) % groups
    th = np.stack([rng.dirichlet(conc * c[k] + 0.05) for k in g], axis=1)
    th = np.maximum(th, 1e-300)
    return th / th.sum(axis=0), g


def purity(xy, g):
    """share of points whose nearest 2-D neighbour is of their own group"""
    xy = np.asarray(xy, dtype=np.float64)
    d = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float((g[d.argmin(axis=1)] == g).mean())


def pca_init(theta, metric="hellinger"):
    f = np.sqrt(theta) if metric == "hellinger" else theta / np.sqrt((theta * theta).sum(axis=0))
    f = f - f.mean(axis=1, keepdims=True)
    w, v = np.linalg.eigh(f @ f.T / f.shape[1])
    out = np.zeros((f.shape[1], 2))
    for c in range(2):
        a = v[:, -1 - c]
        out[:, c] = (a * np.sign(a[np.argmax(np.abs(a))])) @ f
    return (out * (1e-4 / out[:, 0].std())).astype(np.float32)
