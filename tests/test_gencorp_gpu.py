"""
gendoc / gencorp (src/modelutils.jl:594-649) on the device, through the C ABI (tmvb_lda_gencorp / tmvb_ctm_gencorp) and the Python mirror.

Structure, exact conservation between the diagnostics and the CSR, determinism (seed, prefix, doc_offset slice), and the distributions of
every stage: w | z (chi-square per topic), z | theta, theta (Dirichlet moments; logistic-normal mean and covariance), C_d (Poisson).
Statistical assertions: p >= 1e-6 each, counted by test_gencorp_stats.accept (at most 200 in the suite: 24 on the CPU side, 167 here).
All seeds below were fixed before the first GPU run.
"""
import numpy as np
import pytest
from scipy import special, stats

from test_gencorp_stats import (K_SMALL, M_SMALL, MEAN_C_SMALL, SMOOTHINGS, V_SMALL, abi_error_cases, assert_chi2, assert_z, smoothed,
                                zipf_gamma_beta)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()


def gen(tmvb, ctx, K, V, beta, M, mean_C, **kw):
    rc, res = tmvb.gencorp_raw(ctx, K, V, beta, M, mean_C, **kw)
    assert rc == 0, res
    return res


def check_structure(tmvb, res, V):
    M, ptr, terms, counts = res["M"], res["doc_ptr"], res["terms"], res["counts"]
    assert ptr.shape == (M + 1,) and ptr[0] == 0 and ptr[M] == res["nnz"] == len(terms) == len(counts)
    assert np.all(np.diff(ptr) >= 0)
    assert np.all(counts >= 1) and res["sum_counts"] == counts.sum(dtype=np.int64)
    if len(terms):
        assert terms.min() >= 0 and terms.max() < V
        inner = np.ones(len(terms), dtype=bool)
        inner[ptr[:-1][ptr[:-1] < len(terms)]] = False          # first entry of each non-empty document
        assert np.all(np.diff(terms.astype(np.int64))[inner[1:]] > 0), "terms must be strictly ascending inside a document"


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("doc_ptr", "terms", "counts")) and a["sum_counts"] == b["sum_counts"]


@pytest.fixture(scope="module")
def small_runs(tmvb, ctx):
    """The inputs of tests/test_gencorp_stats.py: K = 8, V = 2000, M = 20 000, mean C = 120, alpha = 1, for the three smoothings."""
    beta = zipf_gamma_beta(K_SMALL, V_SMALL, seed=20261016)
    return beta, {a: gen(tmvb, ctx, K_SMALL, V_SMALL, beta, M_SMALL, MEAN_C_SMALL, alpha=np.ones(K_SMALL), laplace_smooth=a,
                         seed=7001 + i, diagnostics=True) for i, a in enumerate(SMOOTHINGS)}


def test_structure_and_check_corp(tmvb, ctx, small_runs):
    beta, runs = small_runs
    for res in runs.values():
        check_structure(tmvb, res, V_SMALL)
    r = gen(tmvb, ctx, K_SMALL, V_SMALL, beta, 300, 40.0, alpha=np.ones(K_SMALL), seed=11)
    check_structure(tmvb, r, V_SMALL)
    pc = tmvb.PackedCorpus(r["doc_ptr"], r["terms"], r["counts"], V_SMALL)
    tmvb.check_corp(pc.to_corpus())


def test_empty_documents(tmvb, ctx):
    beta = zipf_gamma_beta(4, 300, seed=3)
    r = gen(tmvb, ctx, 4, 300, beta, 5000, 0.7, alpha=np.ones(4), seed=12, diagnostics=True)
    check_structure(tmvb, r, 300)
    n = np.diff(r["doc_ptr"])
    C = r["doc_topic"].sum(axis=1)
    assert (C == 0).sum() > 1000 and np.array_equal(n == 0, C == 0)


def test_conservation_between_diagnostics_and_csr(small_runs):
    _, runs = small_runs
    for res in runs.values():
        ptr, terms, counts = res["doc_ptr"], res["terms"], res["counts"]
        cs = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        C = cs[ptr[1:]] - cs[ptr[:-1]]
        assert np.array_equal(res["doc_topic"].sum(axis=1, dtype=np.int64), C)
        assert np.array_equal(res["doc_topic"].sum(axis=0, dtype=np.int64), res["topic_term"].sum(axis=1))
        assert np.array_equal(res["topic_term"].sum(axis=0), np.bincount(terms, weights=counts, minlength=V_SMALL).astype(np.int64))


def test_determinism_prefix_and_slice(tmvb, ctx):
    K, V = 6, 1500
    beta = zipf_gamma_beta(K, V, seed=21)
    alpha = np.array([0.05, 0.3, 1.0, 2.0, 0.007, 5.0])
    kw = dict(alpha=alpha, laplace_smooth=1e-5)
    a = gen(tmvb, ctx, K, V, beta, 1000, 90.0, seed=1234, **kw)
    b = gen(tmvb, ctx, K, V, beta, 1000, 90.0, seed=1234, **kw)
    assert same(a, b)
    assert a["terms"].tobytes() == b["terms"].tobytes() and a["counts"].tobytes() == b["counts"].tobytes()
    c = gen(tmvb, ctx, K, V, beta, 1000, 90.0, seed=1235, **kw)
    assert not same(a, c)
    d = gen(tmvb, ctx, K, V, beta, 1000, 90.0, seed=1234, diagnostics=True, **kw)
    assert same(a, d)
    pc = tmvb.PackedCorpus(a["doc_ptr"], a["terms"], a["counts"], V)
    # prefix
    p = gen(tmvb, ctx, K, V, beta, 500, 90.0, seed=1234, **kw)
    s = pc.shard(0, 500)
    assert np.array_equal(p["doc_ptr"], s.doc_ptr) and np.array_equal(p["terms"], s.terms) and np.array_equal(p["counts"], s.counts)
    # slice through doc_offset (this is also gendoc: one document at a time)
    for d0, m in ((137, 300), (999, 1), (0, 1)):
        q = gen(tmvb, ctx, K, V, beta, m, 90.0, seed=1234, doc_offset=d0, **kw)
        s = pc.shard(d0, d0 + m)
        assert np.array_equal(q["doc_ptr"], s.doc_ptr) and np.array_equal(q["terms"], s.terms) and np.array_equal(q["counts"], s.counts)
    # the CTM entry point: same properties
    mu, sigma = np.linspace(-1, 1, K), np.eye(K) + 0.3
    e = gen(tmvb, ctx, K, V, beta, 400, 60.0, mu=mu, sigma=sigma, seed=77)
    f = gen(tmvb, ctx, K, V, beta, 400, 60.0, mu=mu, sigma=sigma, seed=77, diagnostics=True)
    g = gen(tmvb, ctx, K, V, beta, 100, 60.0, mu=mu, sigma=sigma, seed=77, doc_offset=250)
    assert same(e, f)
    s = tmvb.PackedCorpus(e["doc_ptr"], e["terms"], e["counts"], V).shard(250, 350)
    assert np.array_equal(g["doc_ptr"], s.doc_ptr) and np.array_equal(g["terms"], s.terms) and np.array_equal(g["counts"], s.counts)


@pytest.mark.parametrize("a", SMOOTHINGS)
def test_term_given_topic_small(small_runs, a):
    beta, runs = small_runs
    tt = runs[a]["topic_term"]
    bt = smoothed(beta, a)
    for k in range(K_SMALL):
        assert_chi2(tt[k], tt[k].sum() * bt[k], f"w | z = {k}, a = {a}")


def test_zero_probability_terms_are_never_drawn(tmvb, ctx):
    """laplace_smooth = 0: a count of exactly 0 wherever beta is exactly 0 -- single terms, a whole 64-term stretch, the head and the tail of the vocabulary."""
    K, V = K_SMALL, V_SMALL
    beta = zipf_gamma_beta(K, V, seed=20261018)
    beta[:, 7] = 0.0; beta[3, 64:192] = 0.0; beta[5, 1990:] = 0.0; beta[6, :3] = 0.0; beta[2, ::2] = 0.0
    beta /= beta.sum(axis=1, keepdims=True)
    res = gen(tmvb, ctx, K, V, beta, 8000, MEAN_C_SMALL, alpha=np.ones(K), seed=7050, diagnostics=True)
    tt = res["topic_term"]
    assert (beta == 0).sum() > 1000 and tt.sum() > 900000
    assert np.all(tt[beta == 0] == 0), "a term of zero probability was drawn"
    assert np.all(tt[beta > 3e-4] > 0)                      # expected count above 30 each: the neighbours of the zeros are alive


def trained_shaped_beta(K, V, seed):
    """Most entries below 1e-6, like a trained topic matrix: Gamma(0.02) x Zipf."""
    return zipf_gamma_beta(K, V, seed, conc=0.02)


def test_term_given_topic_trained_shape(tmvb, ctx):
    K, V, M = 50, 25319, 40000
    beta = trained_shaped_beta(K, V, seed=20261017)
    assert (beta < 1e-6).mean() > 0.8
    res = gen(tmvb, ctx, K, V, beta, M, 128.4, alpha=np.ones(K), seed=7100, diagnostics=True)
    check_structure(tmvb, res, V)
    tt = res["topic_term"]
    for k in range(K):
        assert_chi2(tt[k], tt[k].sum() * beta[k], f"w | z = {k}, trained-shaped beta")
    assert np.all(tt[beta == 0] == 0)


def test_topic_given_theta(small_runs):
    _, runs = small_runs
    res = runs[0.0]
    theta = np.exp(res["log_theta"].astype(np.float64))
    C = res["doc_topic"].sum(axis=1).astype(np.float64)
    for k in range(K_SMALL):
        mean = (C * theta[:, k]).sum()
        var = (C * theta[:, k] * (1 - theta[:, k])).sum()
        assert_z(float(res["doc_topic"][:, k].sum()), mean, var, f"z | theta, topic {k}")


ALPHAS = {"ones": np.ones(8), "spread": np.array([0.05, 0.1, 0.2, 0.5, 1.0, 2.0, 3.5, 5.0]),
          "trained": np.array([0.007, 0.02, 0.05, 0.1, 0.3, 0.8, 1.5, 4.0])}


@pytest.mark.parametrize("name", list(ALPHAS))
def test_dirichlet_theta(tmvb, ctx, name):
    alpha = ALPHAS[name]
    K, V, M = len(alpha), 64, 50000
    beta = np.full((K, V), 1.0 / V)
    res = gen(tmvb, ctx, K, V, beta, M, 3.2, alpha=alpha, seed=7200 + list(ALPHAS).index(name), diagnostics=True)
    lt = res["log_theta"].astype(np.float64)
    assert np.all(np.isfinite(lt)) and np.all(lt <= 0)
    theta = np.exp(lt)
    assert np.abs(theta.sum(axis=1) - 1.0).max() < 1e-5
    a0 = alpha.sum()
    for i in range(K):
        assert_z(lt[:, i].mean(), special.digamma(alpha[i]) - special.digamma(a0),
                 (special.polygamma(1, alpha[i]) - special.polygamma(1, a0)) / M, f"mean log theta_{i}, alpha {name}")
        assert_z(theta[:, i].mean(), alpha[i] / a0, alpha[i] * (a0 - alpha[i]) / (a0 ** 2 * (a0 + 1) * M), f"mean theta_{i}, alpha {name}")


def trained_like_sigma(K, seed, cond=1e4):
    rng = np.random.Generator(np.random.PCG64(seed))
    q, _ = np.linalg.qr(rng.normal(size=(K, K)))
    s = (q * np.logspace(-np.log10(cond) / 2, np.log10(cond) / 2, K)) @ q.T
    return (s + s.T) / 2


@pytest.mark.parametrize("which", ["identity", "trained"])
def test_logistic_normal_theta(tmvb, ctx, which):
    K, V, M = 4, 64, 50000
    mu = np.array([0.5, -1.0, 0.0, 2.0])
    sigma = np.eye(K) if which == "identity" else trained_like_sigma(K, seed=31)
    if which == "trained":
        assert 5e3 < np.linalg.cond(sigma) < 2e4
    beta = np.full((K, V), 1.0 / V)
    res = gen(tmvb, ctx, K, V, beta, M, 3.2, mu=mu, sigma=sigma, seed=7300 + (which == "trained"), diagnostics=True)
    lt = res["log_theta"].astype(np.float64)
    assert np.all(np.isfinite(lt)) and np.abs(np.exp(lt).sum(axis=1) - 1.0).max() < 1e-5
    H = np.eye(K) - 1.0 / K
    y = lt - lt.mean(axis=1, keepdims=True)                   # centred log-ratios: H eta
    m, S = H @ mu, H @ sigma @ H.T
    for i in range(K):
        assert_z(y[:, i].mean(), m[i], S[i, i] / M, f"clr mean {i}, sigma {which}")
    Sh = np.cov(y, rowvar=False)
    for i in range(K):
        for j in range(i, K):
            assert_z(Sh[i, j], S[i, j], (S[i, i] * S[j, j] + S[i, j] ** 2) / (M - 1), f"clr cov ({i},{j}), sigma {which}")


@pytest.mark.parametrize("mean_C", [3.2, 128.4, 2500.0])
def test_poisson_lengths(tmvb, ctx, mean_C):
    K, V, M = 2, 50, 20000
    beta = np.full((K, V), 1.0 / V)
    res = gen(tmvb, ctx, K, V, beta, M, mean_C, alpha=np.ones(K), seed=7400 + int(mean_C), diagnostics=True)
    C = res["doc_topic"].sum(axis=1).astype(np.int64)
    assert res["sum_counts"] == C.sum()
    hi = int(max(C.max(), mean_C + 12 * np.sqrt(mean_C))) + 1
    pmf = stats.poisson.pmf(np.arange(hi + 1), mean_C)
    pmf[-1] += stats.poisson.sf(hi, mean_C)                   # the open tail rides in the last cell (pooled: its expectation is far below 5)
    assert_chi2(np.bincount(C, minlength=hi + 1), M * pmf, f"C_d ~ Poisson({mean_C})")
    assert_z(C.mean(), mean_C, mean_C / M, f"mean C_d, Poisson({mean_C})")
    # sample variance: Var(S^2) = (mu4 - sigma^4 (M - 3) / (M - 1)) / M with mu4 = lambda (1 + 3 lambda)
    assert_z(C.var(ddof=1), mean_C, (mean_C * (1 + 3 * mean_C) - mean_C ** 2 * (M - 3) / (M - 1)) / M, f"var C_d, Poisson({mean_C})")


def test_round_trip_trains(tmvb):
    """A corpus generated from known (alpha, beta) at K = 5 is a corpus like any other: gpuLDA accepts and trains on it (a use test)."""
    K, V = 5, 400
    template = tmvb.LDA(tmvb.syn_nsf(M=60, V=V, seed=2), K)
    template.alpha = np.array([0.3, 0.5, 0.2, 0.8, 0.4])
    template.beta = np.asfortranarray(zipf_gamma_beta(K, V, seed=41, conc=0.3))
    pc = tmvb.gencorp(template, 600, laplace_smooth=1e-5, seed=99)
    assert pc.M == 600 and pc.V == V
    tmvb.check_corp(pc.to_corpus())
    again = tmvb.gencorp(template, 600, laplace_smooth=1e-5, seed=99)
    assert np.array_equal(pc.terms, again.terms) and np.array_equal(pc.counts, again.counts)
    doc = tmvb.gendoc(template, laplace_smooth=1e-5, seed=99)
    assert np.array_equal(doc.terms - 1, pc.terms[pc.doc_ptr[0]:pc.doc_ptr[1]]) and np.array_equal(doc.counts, pc.counts[pc.doc_ptr[0]:pc.doc_ptr[1]])
    gm = tmvb.gpuLDA(pc, K)
    traj = gm.train(iter=30, tol=0.0, checkelbo=1, printelbo=False)
    assert len(traj) == 30 and np.all(np.isfinite(traj))
    # non-decreasing up to the fp32 evaluation of the ELBO (relative 1e-5, the bound smoke() uses for the same quantity)
    assert np.all(np.diff(traj) >= -1e-5 * np.abs(traj[:-1])), np.diff(traj)
    # a gpu model generates through its own context, from its host fields
    pc2 = tmvb.gencorp(gm, 50, seed=5)
    assert pc2.M == 50 and pc2.V == V
    ctm = tmvb.CTM(pc, K)
    pc3 = tmvb.gencorp(ctm, 50, seed=5)
    assert pc3.M == 50 and pc3.nnz > 0
    with pytest.raises(TypeError):
        tmvb.gencorp(tmvb.CTPF(tmvb.syn_citeu(M=40, V=100, U=20, seed=1), 3), 5)


@pytest.mark.parametrize("case", abi_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_abi_error_codes(tmvb, ctx, case):
    _, base, change, status, msg = case
    kw = dict(base, **change)
    rc, res = tmvb.gencorp_raw(ctx, kw.pop("K"), kw.pop("V"), kw.pop("beta"), kw.pop("M"), kw.pop("mean_C"), **kw)
    assert rc == status and msg in res["error"], (rc, res)


def test_null_context_with_a_device_is_einval(tmvb):
    rc, res = tmvb.gencorp_raw(None, 3, 6, np.full((3, 6), 1 / 6), 5, 2.0, alpha=np.ones(3))
    assert rc == 1 and "ctx is NULL" in res["error"]
