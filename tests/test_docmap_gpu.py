"""
tmvb_map_affinity and tmvb_map_layout on the device (include/tmvb.h, "map documents in two dimensions") against
tests/docmap_restatement.py.

  1. affinity       n in {1, 2, 63, 64} x M in {2, 65, 300}: quantised distances (exact ties), rows with several zeros, rows shorter than n, rows with
                    n_i <= u.  p_cond = the restatement at the DEVICE's beta (rel 1e-12); the entropy of every reachable row, recomputed in NumPy from
                    the device's beta, within 1e-10 of log u; beta against the restatement's beta within BETA_TOL (relative); the CSR structure exactly;
                    val bit for bit float32((a + b) / (2 M)) from the device's p_cond.
  2. forces         teacher-forced (iters = 1, state given), M in {2, 63, 64, 65, 255, 256, 257, 16383, 16385} (run and segment boundaries), y at the
                    early scale (1e-4) and a late one (+-50 with coincident points), j_split in {0, 1, 3}; at the two large sizes 512 sampled rows
                    (first, last, tile edges) against all j.
                    pieces:   |rep - rep64| <= REP_TOL 2^-24 sum_j |w dx|, |zrow - z64| <= Z_TOL 2^-24 sum_j q (the sums from the restatement);
                              att within 1e-12 of sum |terms|.
                    Z, grad:  Z = blocked(returned zrow) - M bit for bit; grad = float32(4 (e att - rep / Z)) from the returned pieces bit for bit.
                    KL:       the KL of the iters = 0 call on the same y = the restatement's KL of that y, evaluated with the device's own Z(y) (the Z the
                              iters = 1 call returns: the restatement's fp64 Z differs from the fp32 chain's by 1e-7), within 1e-12 of sum |terms|.
     Error model, per row and first order, units of 2^-24 relative: dx <= 1; d <= 4; q <= 4 + 2 (the reciprocal); w = q q <= 13; w dx before the fused
     add <= 14; a run of 256 sequential fp32 adds <= 255 of sum |terms|; the fp64 levels are negligible.  14 + 255 = 269 <= RUN + 24 and 6 + 255 = 261
     <= RUN + 8: the caps of the header hold with room (the derivation was checked and the constants kept).
  3. update         from the returned grad and the input state the restated fp32 update and recentring give y, vel, gain bit for bit: both sides of
                    exag_iters, gains at the floor, g = 0 (all points coincide).
  4. start          y0 = None, iters = 0: the Philox restatement bit for bit.
  5. free-running   ten iterations at M = 300 against the fp64 loop: max |y - y64| / spread(y64) <= FREE_TOL (ten, not 750: the descent amplifies
                    rounding differences).
  6. purity         identical bytes over two calls, j_split in {0, 1, 3} (M = 16 385 + 700: two segments), a + b split runs against one run with the
                    cut before, at and after exag_iters, DocMap.resume.
  7. end to end     map_docs on the planted groups (M = 600, 750 iterations): kl finite and lower at the end than at the first check after exag_iters,
                    nearest-neighbour purity >= 0.99, .place puts 50 fresh draws of each group next to a point of their own group; the trained golden
                    LDA / CTM / CTPF corpora: finite, centred, identical over two calls.

The floating tolerances were measured on one MI355X (TMVB_DOCMAP_RECORD=<file> records the worst of each; profiles/docmap_tolerances_measured.json) and
are frozen at <= 10 x the measurement; REP_TOL and Z_TOL also stay below the caps of the error model (tests/test_docmap_host.py asserts all of it).
"""
import functools
import json
import os

import numpy as np
import pytest

import docmap_restatement as dr
from docmap_restatement import RUN, SEG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured worst on one MI355X -> literal (profiles/docmap_tolerances_measured.json)
BETA_TOL = 2e-13            # relative; measured 4.2e-14
REP_TOL = 64.0              # units of 2^-24 sum |w dx|; measured 16.0; cap RUN + 24 = 280
Z_TOL = 100.0               # units of 2^-24 sum q; measured 26.5; cap RUN + 8 = 264
FREE_TOL = 5e-6             # max |y - y64| / spread after ten iterations; measured 1.06e-6
WORST = {"beta_rel": 0.0, "rep_units": 0.0, "z_units": 0.0, "free_rel": 0.0}

AFF_NS, AFF_MS = [1, 2, 63, 64], [2, 65, 300]
AFF_U = {1: 1.0, 2: 1.5, 63: 20.0, 64: 20.0}
FORCE_MS = [2, 63, 64, 65, 255, 256, 257, RUN * SEG - 1, RUN * SEG + 1]
SCALES = ["early", "late"]
SPLITS = [0, 1, 3]


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    out = os.environ.get("TMVB_DOCMAP_RECORD", "")
    if not out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"measured": WORST, "tolerance": {"beta_rel": BETA_TOL, "rep_units": REP_TOL, "z_units": Z_TOL, "free_rel": FREE_TOL},
                   "cap": {"rep_units": RUN + 24, "z_units": RUN + 8},
                   "what": "worst over every case of tests/test_docmap_gpu.py: |beta - beta64| / beta64; |rep - rep64| / (2^-24 sum |w dx|); |zrow - z64| / "
                           "(2^-24 sum q); max |y - y64| / (max y64 - min y64) after ten iterations at M = 300"}, f, indent=1)


def see(name, value, tol):
    """record, print, then assert: the figure is in the output whether or not the assertion holds"""
    WORST[name] = max(WORST[name], float(value))
    print(f"docmap {name}: {float(value):.4g} (tolerance {tol:g})")
    assert value <= tol, (name, float(value), tol)


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def affinity_inputs(M, n):
    rng = np.random.Generator(np.random.PCG64(1000 * M + n))
    full = min(n, M - 1)
    idx, d2, count = np.full((M, n), -1, dtype=np.int32), np.zeros((M, n), dtype=np.float32), np.zeros(M, dtype=np.int32)
    for i in range(M):
        ni = full if rng.random() < 0.7 else int(rng.integers(0, full + 1))          # rows shorter than n, some empty, some with n_i <= u
        others = np.delete(np.arange(M), i)
        idx[i, :ni] = rng.permutation(others)[:ni]
        d = rng.integers(0, 24, size=ni).astype(np.float32) / np.float32(16.0)        # quantised: exact ties
        if ni and rng.random() < 0.3:
            d[rng.permutation(ni)[:max(1, ni // 8)]] = 0.0                            # duplicates at distance 0
        if ni and rng.random() < 0.2:
            d = d + np.float32(0.37)                                                  # a minimum that is not 0
        d2[i, :ni] = d
        count[i] = ni
    return idx, d2, count


@functools.lru_cache(maxsize=None)
def affinity_reference(M, n):
    idx, d2, count = affinity_inputs(M, n)
    beta, _ = dr.affinity(d2, count, AFF_U[n])
    return beta, dr.symmetrize(idx, np.ones((M, n)), count)[:2], dr.reachable(d2, count, AFF_U[n])


def random_csr(M, n, seed):
    """a symmetric P with about 2 n entries per row, sum 1: (row_ptr, col, val)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = min(n, M - 1)
    i = np.repeat(np.arange(M, dtype=np.int64), n)
    j = (i + 1 + rng.integers(0, M - 1, size=len(i))) % M
    if M > 300:
        j[(np.arange(len(i)) % n == 0) & (i < 300)] = 7                               # a hub row: 300 edges, several per slot
        j[i == j] = 8
    v = rng.random(len(i))
    key, inv = np.unique(np.concatenate([i * M + j, j * M + i]), return_inverse=True)
    s = np.zeros(len(key))
    np.add.at(s, inv, np.concatenate([v, v]))
    val = (s / s.sum()).astype(np.float32)
    rows = key // M
    keep = rows != key % M
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=M))]).astype(np.int64)
    return row_ptr, (key % M)[keep].astype(np.int32), val[keep]


def state(M, scale, seed=3):
    rng = np.random.Generator(np.random.PCG64(10 * M + seed))
    if scale == "early":
        y = (1e-4 * rng.standard_normal((M, 2))).astype(np.float32)
    else:
        y = rng.uniform(-50.0, 50.0, size=(M, 2)).astype(np.float32)
        if M >= 4:
            y[M // 2] = y[1]                                                          # coincident points
            y[M - 1] = y[0]
    vel = (0.1 * np.abs(y).max() * rng.standard_normal((M, 2))).astype(np.float32)
    gain = rng.choice(np.array([0.01, 0.5, 1.0, 1.2, 3.0], dtype=np.float32), size=(M, 2))
    gain[0, 0] = np.float32(0.01)                                                     # at the floor
    return y, vel, gain


def sample_rows(M):
    if M <= 2048:
        return np.arange(M)
    rng = np.random.Generator(np.random.PCG64(M))
    edge = [0, 1, 255, 256, 257, 511, 512, 513, 7, M // 2, RUN * SEG - 2, RUN * SEG - 1, RUN * SEG, M - 2, M - 1]
    edge = [r for r in edge if 0 <= r < M]
    rest = [r for r in rng.permutation(M).tolist() if r not in set(edge)][:512 - len(set(edge))]
    return np.array(sorted(set(edge) | set(rest)))


@functools.lru_cache(maxsize=None)
def force_reference(M, scale):
    y, vel, gain = state(M, scale)
    csr = random_csr(M, 6, 5 * M + 1)
    rows = sample_rows(M)
    rep, z, aw, sq = dr.repulsion64(y, rows)
    att, ab = dr.attraction64(y, *csr)
    return y, vel, gain, csr, rows, rep, z, aw, sq, att, ab


def layout(tmvb, ctx, M, csr, iters, **kw):
    rc, res = tmvb.map_layout_raw(ctx, M, *csr, iters, **kw)
    assert rc == 0, res
    return res


def forced(tmvb, ctx, M, scale, split, e_side="early"):
    y, vel, gain, csr = force_reference(M, scale)[:4]
    return layout(tmvb, ctx, M, csr, 1, iter0=0 if e_side == "early" else 250, y=y, vel=vel, gain=gain, eta=50.0, j_split=split, pieces=True)


# ------------------------------------------------------------------------------------------------------------------ 1. affinity
@pytest.mark.parametrize("n", AFF_NS)
@pytest.mark.parametrize("M", AFF_MS)
def test_affinity(tmvb, ctx, M, n):
    idx, d2, count = affinity_inputs(M, n)
    u = AFF_U[n]
    beta64, (row_ptr, col), reach = affinity_reference(M, n)
    rc, res = tmvb.map_affinity_raw(ctx, idx, d2, count, u)
    assert rc == 0, res
    beta, p = res["beta"], res["p_cond"]
    _, p_at = dr.affinity(d2, count, u, beta=beta)
    np.testing.assert_allclose(p, p_at, rtol=1e-12, atol=1e-300)
    assert np.all(p[np.arange(n)[None, :] >= count[:, None]] == 0.0) and np.all(beta[count <= u] == 0.0)
    for i in np.flatnonzero(reach):
        D = d2[i, :count[i]].astype(np.float64)
        assert abs(dr.row_entropy(D - D.min(), beta[i]) - np.log(u)) <= 1e-10, (i, beta[i])
    if reach.any():
        see("beta_rel", np.max(np.abs(beta[reach] - beta64[reach]) / beta64[reach]), BETA_TOL)
    assert np.array_equal(res["row_ptr"], row_ptr) and np.array_equal(res["col"], col)
    assert res["val"].tobytes() == dr.symmetrize(idx, p, count)[2].tobytes()
    rc, cond = tmvb.map_affinity_raw(ctx, idx, d2, count, u, Mc=M, symmetric=False)           # the conditional form: the same rows
    assert rc == 0 and cond["p_cond"].tobytes() == p.tobytes() and cond["beta"].tobytes() == beta.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 2. forces
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("M", FORCE_MS)
def test_force_pieces(tmvb, ctx, M, scale, split):
    y, vel, gain, csr, rows, rep64, z64, aw, sq, att64, ab = force_reference(M, scale)
    r = forced(tmvb, ctx, M, scale, split)
    see("rep_units", np.max(np.abs(r["rep"][rows] - rep64) / (dr.U24 * aw + 1e-300)), REP_TOL)
    see("z_units", np.max(np.abs(r["zrow"][rows] - z64) / (dr.U24 * sq)), Z_TOL)
    assert np.all(np.abs(r["att"] - att64) <= 1e-12 * ab)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("M", FORCE_MS)
def test_force_z_and_gradient(tmvb, ctx, M, scale, split):
    for side, e in (("early", 12.0), ("late", 1.0)):
        r = forced(tmvb, ctx, M, scale, split, side)
        Z = dr.blocked(r["zrow"]) - float(M)
        assert r["Z"] == Z, (r["Z"], Z)
        assert r["grad"].tobytes() == dr.grad32(r["att"], r["rep"], Z, e).tobytes()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("M", FORCE_MS)
def test_kl_of_a_given_state(tmvb, ctx, M, scale):
    y, vel, gain, csr = force_reference(M, scale)[:4]
    Z = forced(tmvb, ctx, M, scale, 0)["Z"]                                           # the device's own Z(y)
    r = layout(tmvb, ctx, M, csr, 0, y=y, vel=vel, gain=gain, eta=50.0)
    assert list(r["kl_iter"]) == [0] and r["y"].tobytes() == y.tobytes() and r["gain"].tobytes() == gain.tobytes()
    i, j = dr.edges(csr[0], csr[1])
    d = y[i].astype(np.float64) - y[j].astype(np.float64)
    p = csr[2].astype(np.float64)
    t = p * np.log(p * Z * (1.0 + (d * d).sum(axis=1)))
    assert abs(r["kl"][0] - t.sum()) <= 1e-12 * np.abs(t).sum(), (r["kl"][0], t.sum())


# ------------------------------------------------------------------------------------------------------------------ 3. update
def assert_update(r, y, vel, gain, mu, eta, min_gain=0.01):
    y1, v1, g1 = dr.update32(r["grad"], y, vel, gain, mu, eta, min_gain)
    assert r["gain"].tobytes() == g1.tobytes()
    assert r["vel"].tobytes() == v1.tobytes()
    assert r["y"].tobytes() == y1.tobytes()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("M", [2, 65, 257, RUN * SEG + 1])
def test_update_bit_exact(tmvb, ctx, M, scale):
    y, vel, gain, csr = force_reference(M, scale)[:4]
    assert np.any(gain == np.float32(0.01))                                           # gains at the floor
    for side, mu in (("early", 0.5), ("late", 0.8)):                                  # both sides of exag_iters
        assert_update(forced(tmvb, ctx, M, scale, 0, side), y, vel, gain, mu, 50.0)


def test_update_with_a_zero_gradient(tmvb, ctx):
    M = 64
    y, vel, gain, csr = force_reference(M, "late")[:4]
    y = np.tile(y[:1], (M, 1))                                                        # every point in one place: no force at all
    r = layout(tmvb, ctx, M, csr, 1, y=y, vel=vel, gain=gain, eta=50.0, pieces=True)
    assert np.all(r["grad"] == 0.0) and r["Z"] == float(M) * (M - 1)
    assert_update(r, y, vel, gain, 0.5, 50.0)


# ------------------------------------------------------------------------------------------------------------------ 4. start
@pytest.mark.parametrize("seed", [0, 9, 2 ** 40 + 3])
def test_seeded_start(tmvb, ctx, seed):
    M = 300
    r = layout(tmvb, ctx, M, random_csr(M, 6, 1), 0, seed=seed)
    assert r["y"].tobytes() == dr.init_y(M, seed).tobytes()
    assert np.all(r["vel"] == 0.0) and np.all(r["gain"] == 1.0) and r["iters"] == 0 and np.abs(r["y"]).max() <= 1e-4


# ------------------------------------------------------------------------------------------------------------------ 5. free-running
def test_ten_iterations_against_the_fp64_loop(tmvb, ctx):
    M = 300
    csr = random_csr(M, 6, 11)
    y = state(M, "early", seed=5)[0]
    r = layout(tmvb, ctx, M, csr, 10, y=y, eta=50.0)
    y64 = dr.layout64(y, *csr, 10, eta=50.0)[0]
    see("free_rel", np.abs(r["y"] - y64).max() / (y64.max() - y64.min()), FREE_TOL)


# ------------------------------------------------------------------------------------------------------------------ 6. purity
def same(a, b, keys=("y", "vel", "gain")):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def test_two_calls_and_every_j_split_give_the_same_bytes(tmvb, ctx):
    M = RUN * SEG + 1 + 700                                                           # two segments, the second short
    csr = random_csr(M, 4, 2)
    y = state(M, "late")[0]
    runs = [layout(tmvb, ctx, M, csr, 2, y=y, eta=50.0, j_split=s, pieces=True) for s in (0, 0, 1, 3)]
    assert [r["j_split"] for r in runs[1:]] == [2, 1, 2]
    for r in runs[1:]:
        assert same(runs[0], r, ("y", "vel", "gain", "rep", "zrow", "att", "grad", "kl")) and r["Z"] == runs[0]["Z"]


@pytest.mark.parametrize("a", [3, 5, 7])
def test_split_runs_equal_one_run(tmvb, ctx, a):
    M, total = 300, 10
    csr = random_csr(M, 6, 4)
    kw = dict(eta=50.0, exag_iters=5, check=2)
    whole = layout(tmvb, ctx, M, csr, total, seed=3, **kw)
    first = layout(tmvb, ctx, M, csr, a, seed=3, **kw)
    second = layout(tmvb, ctx, M, csr, total - a, iter0=a, y=first["y"], vel=first["vel"], gain=first["gain"], **kw)
    assert same(whole, second)
    both = dict(zip(first["kl_iter"], first["kl"]))
    both.update(zip(second["kl_iter"], second["kl"]))
    assert all(both[int(t)] == k for t, k in zip(whole["kl_iter"], whole["kl"])) and list(whole["kl_iter"]) == [2, 4, 6, 8, 10]


# ------------------------------------------------------------------------------------------------------------------ 7. end to end
@pytest.fixture(scope="module")
def planted(tmvb):
    theta, g = dr.planted_theta(M=600)
    return theta, g, tmvb.map_docs(None, theta=theta, iters=750)


def test_planted_groups(tmvb, planted):
    theta, g, m = planted
    assert m.xy.shape == (600, 2) and m.iters == 750 and np.all(np.isfinite(m.kl)) and list(m.kl_iters) == list(range(50, 751, 50))
    assert m.kl[-1] < m.kl[list(m.kl_iters).index(300)]
    p = dr.purity(m.xy, g)
    print("docmap planted purity:", p)
    assert p >= 0.99
    assert np.abs(m.xy.astype(np.float64).mean(axis=0)).max() <= 1e-4 * np.abs(m.xy).max()


def test_resume_gives_the_bytes_of_one_run(tmvb, planted):
    theta, g, m = planted
    part = tmvb.map_docs(None, theta=theta, iters=200)
    part.resume(300)
    part.resume(250)
    assert part.iters == 750 and part.xy.tobytes() == m.xy.tobytes()
    assert list(part.kl_iters) == list(m.kl_iters) and part.kl.tobytes() == m.kl.tobytes()


def test_place_puts_fresh_draws_next_to_their_group(tmvb, planted):
    theta, g, m = planted
    before = m.xy.copy()
    rng = np.random.Generator(np.random.PCG64(0))
    c = rng.dirichlet(np.full(12, 0.3), size=5)                                       # the generator of planted_theta(seed = 0): the same c_g
    gn = np.repeat(np.arange(5), 50)
    new = np.stack([np.random.Generator(np.random.PCG64(77 + k)).dirichlet(200.0 * c[gk] + 0.05) for k, gk in enumerate(gn)], axis=1)
    new = np.maximum(new, 1e-300)
    xy = m.place(new / new.sum(axis=0))
    assert xy.shape == (250, 2) and m.xy.tobytes() == before.tobytes()
    d = ((xy[:, None, :] - m.xy[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
    assert np.array_equal(g[d.argmin(axis=1)], gn)


def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def check_model(tmvb, model):
    a, b = tmvb.map_docs(model, iters=300), tmvb.map_docs(model, iters=300)
    M = tmvb.topic_proportions(model).shape[1]
    assert a.xy.shape == (M, 2) and a.n_neighbors == M - 1 and np.all(np.isfinite(a.xy)) and np.all(np.isfinite(a.kl))
    assert np.abs(a.xy.astype(np.float64).mean(axis=0)).max() <= 1e-4 * np.abs(a.xy).max()
    assert a.xy.tobytes() == b.xy.tobytes() and a.kl.tobytes() == b.kl.tobytes()
    r = tmvb.map_docs(model, iters=20, init="random", metric="cosine", seed=4)
    assert np.all(np.isfinite(r.xy))


def test_map_docs_of_a_trained_lda(tmvb):
    g = load("lda_m40_v60_k7")
    K, V = int(g["K"]), int(g["V"])
    m = tmvb.LDA(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m)


def test_map_docs_of_a_trained_ctm(tmvb):
    g = load("ctm_m40_v60_k5")
    K, V = int(g["K"]), int(g["V"])
    m = tmvb.CTM(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train_ctm(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m)


def test_map_docs_of_a_trained_ctpf(tmvb):
    g = load("ctpf_m40_v60_u15_k4")
    K, V, U = int(g["K"]), int(g["V"]), int(g["U"])
    m = tmvb.CTPF(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V, g["rdr_ptr"], g["readers"], g["ratings"], U), K)
    m.alef = np.asfortranarray(g["alef0"]); m.alef_old = m.alef.copy(order="F")
    tmvb.gpu_train_ctpf(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m)
