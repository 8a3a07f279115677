"""
Topic comparison on the device against tests/topic_compare_restatement.py (which tests/test_topic_compare_host.py holds to mpmath and math.fsum).

  1. exact        TV on rows of integers / 2^10 is exact in any order: D equals the restatement bit for bit over a pairwise cover of
                  KA, KB in {1, 2, 31, 32, 33, 65, 130} x V in {1, 2, 255, 256, 257, 513, 1000} x splits in {0, 1, all runs}, and at 4096 x 2.
                  Pins indexing, tiling and run edges (tests/test_topic_compare_mutant_gpu.py is its negative control).
  2. floating     JS, HELLINGER, KL (smooth 0 and 1e-3) on Dirichlet rows at concentrations 0.01, 0.1 and 1 with planted zeros, same shapes:
                  |D - restatement| <= (min(V, RUN) + runs + 8) 2^-53 S, S = the restatement's sum of the absolute values of the addends'
                  components -- the worst case of the blocked sequential sum plus a few ulps for log, divide and product: derived, not measured
                  (the host tests find the restatement's own sum within 0.17 of it).  HELLINGER: the cap applies to the sum before the root: the
                  root is correctly rounded and monotone, so D must lie in [sqrt(sum - cap), sqrt(sum + cap)].  +inf exactly where the
                  restatement has it.  TMVB_TOPICDIV_RECORD=1 writes the largest observed ratio per metric to
                  profiles/topic_compare_tolerances_measured.json.
  3. identities   bit for bit: zero where two rows are equal, D(a, b) = D(b, a)^T for JS / HELLINGER / TV, b = NULL symmetric.
  4. purity       identical bytes over two calls, over every splits, for row slices.
  5. relevance    dense within 8 * 2^-53 (|lam log phi| + |(1 - lam) log(phi / pw)|); idx / score / count = the lexsort of the device's OWN dense
                  bits (duplicated columns: exact ties; zeros: count < n); distinct and saliency within 8 K 2^-53 sum |addends|.
  6. Python       planted matching, topic_stability, redundant, and the trained golden LDA, CTM and CTPF models.
"""
import functools
import itertools
import json
import os

import numpy as np
import pytest

import topic_compare_restatement as tr
from topic_compare_restatement import HELLINGER, JS, KL, RUN, TV, U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KS = [1, 2, 31, 32, 33, 65, 130]
VS = [1, 2, 255, 256, 257, 513, 1000]
SPLITS = ["0", "1", "all"]
FLOATING = [("js", JS, 0.0), ("hellinger", HELLINGER, 0.0), ("kl", KL, 0.0), ("kl_smooth", KL, 1e-3)]
WORST = {name: 0.0 for name, _, _ in FLOATING}


def pairwise_cover(axes, ok=lambda p: True):
    """greedy: the admissible grid in its natural order, each time the point that covers most value pairs not covered yet"""
    grid = [p for p in itertools.product(*axes) if ok(p)]
    pairs = lambda p: {(i, p[i], j, p[j]) for i in range(len(p)) for j in range(i + 1, len(p))}
    todo = set().union(*(pairs(p) for p in grid))
    out = []
    while todo:
        best = max(grid, key=lambda p: len(pairs(p) & todo))
        out.append(best)
        todo -= pairs(best)
    return out


CASES = pairwise_cover([KS, KS, VS, SPLITS])
assert {(c[0], c[1]) for c in CASES} == set(itertools.product(KS, KS)) and len(CASES) < 70
BIG = (4096, 2, 257, "0")


def runs_of(V):
    return (V + RUN - 1) // RUN


def splits_of(s, V):
    return runs_of(V) if s == "all" else int(s)


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    if os.environ.get("TMVB_TOPICDIV_RECORD", "") != "1":
        return
    out = os.path.join(ROOT, "profiles", "topic_compare_tolerances_measured.json")
    with open(out, "w") as f:
        json.dump({"topic_divergence.sum_abs": {"measured": WORST, "cap": 1.0,
                                                "what": "per metric, the largest |D - restatement| / ((min(V, RUN) + runs + 8) 2^-53 S) over every case of "
                                                        "test_floating_divergences of tests/test_topic_compare_gpu.py (HELLINGER: |D^2 - sum| over the cap)"}},
                  f, indent=1, sort_keys=True)


def call(tmvb, ctx, metric, a, b=None, smooth=0.0, splits=0):
    rc, res = tmvb.topic_divergence_raw(ctx, metric, a, b, smooth, splits)
    assert rc == 0, res
    return res


# ------------------------------------------------------------------------------------------------------------------ 1. exact
@functools.lru_cache(maxsize=None)
def exact_case(KA, KB, V):
    a, b = tr.exact_rows(KA, V, 1000 * KA + V), tr.exact_rows(KB, V, 1000 * KB + V + 7)
    return a, b, tr.divergence(TV, a, b)[0]


@pytest.mark.parametrize("KA,KB,V,splits", CASES + [BIG])
def test_exact_total_variation(tmvb, ctx, KA, KB, V, splits):
    a, b, want = exact_case(KA, KB, V)
    assert np.all(a.sum(axis=1) == 1.0) and np.all(b.sum(axis=1) == 1.0)
    res = call(tmvb, ctx, TV, a, b, 0.0, splits_of(splits, V))
    assert res["runs"] == runs_of(V) and (splits == "0" or res["splits"] == splits_of(splits, V))
    assert res["D"].shape == (KA, KB)
    assert res["D"].tobytes() == want.tobytes(), float(np.abs(res["D"] - want).max())


# ------------------------------------------------------------------------------------------------------------------ 2. floating
@functools.lru_cache(maxsize=8)
def floating_case(metric, smooth, KA, KB, V):
    a, b = tr.dirichlet_rows(KA, V, 77 * KA + V, shift=V), tr.dirichlet_rows(KB, V, 91 * KB + V + 3, shift=KB)
    return (a, b) + tr.divergence(metric, a, b, smooth)


def check_floating(name, metric, V, D, want, sigma, S):
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(D), inf) and not np.isnan(D).any()
    assert metric == KL or not inf.any()
    cap = tr.cap_factor(V) * S
    fin = ~inf
    if metric == HELLINGER:
        lo, hi = np.nextafter(np.sqrt(np.maximum(0.0, sigma - cap)), -np.inf), np.nextafter(np.sqrt(sigma + cap), np.inf)
        ratio = np.abs(D * D - sigma) / np.where(cap > 0, cap, 1.0)
        print(f"{name} V {V}: largest |D^2 - sum| / cap = {float(ratio.max()):.4f}")
        WORST[name] = max(WORST[name], float(ratio.max()))
        assert np.all((D >= lo) & (D <= hi))
        return
    err = np.abs(D[fin] - want[fin])
    ratio = err / np.where(cap[fin] > 0, cap[fin], 1.0)
    print(f"{name} V {V}: largest |D - restatement| / cap = {float(ratio.max()) if ratio.size else 0.0:.4f}")
    if ratio.size:
        WORST[name] = max(WORST[name], float(ratio.max()))
    assert np.all(err <= cap[fin])
    assert np.all(D >= 0.0)


@pytest.mark.parametrize("name,metric,smooth", FLOATING)
@pytest.mark.parametrize("KA,KB,V,splits", CASES + [BIG])
def test_floating_divergences(tmvb, ctx, name, metric, smooth, KA, KB, V, splits):
    a, b, want, sigma, S = floating_case(metric, smooth, KA, KB, V)
    res = call(tmvb, ctx, metric, a, b, smooth, splits_of(splits, V))
    check_floating(name, metric, V, res["D"], want, sigma, S)
    if name == "kl" and V >= 255 and KA > 2 and KB > 2:
        assert np.isinf(want).any()                                  # the planted zeros do put +inf somewhere
    if name == "kl_smooth":
        assert np.all(np.isfinite(res["D"]))


# ------------------------------------------------------------------------------------------------------------------ 3. identities
IDENT = [(33, 65, 513), (130, 31, 1000), (2, 1, 257), (65, 65, 256)]


@pytest.mark.parametrize("KA,KB,V", IDENT)
@pytest.mark.parametrize("splits", ["0", "all"])
def test_bitwise_identities(tmvb, ctx, KA, KB, V, splits):
    sp = splits_of(splits, V)
    a, b = tr.dirichlet_rows(KA, V, 5 + KA, shift=1).copy(), tr.dirichlet_rows(KB, V, 9 + KB)
    if KA > 1:
        a[KA - 1] = a[0]                                             # two equal rows in different tiles (KA > 32) or lanes
    for metric, smooth in ((JS, 0.0), (HELLINGER, 0.0), (TV, 0.0), (KL, 0.0), (KL, 1e-3)):
        D = call(tmvb, ctx, metric, a, None, smooth, sp)["D"]
        assert np.all(np.diag(D) == 0.0), metric
        assert D[0, KA - 1] == 0.0 and D[KA - 1, 0] == 0.0, metric
        both = call(tmvb, ctx, metric, a, a, smooth, sp)["D"]          # b = NULL is b = a
        assert both.tobytes() == D.tobytes(), metric
        if metric != KL:
            assert D.tobytes() == D.T.copy().tobytes(), metric
            ab = call(tmvb, ctx, metric, a, b, smooth, sp)["D"]
            ba = call(tmvb, ctx, metric, b, a, smooth, sp)["D"]
            assert ab.tobytes() == ba.T.copy().tobytes(), metric


# ------------------------------------------------------------------------------------------------------------------ 4. purity
@pytest.mark.parametrize("name,metric,smooth", FLOATING + [("tv", TV, 0.0)])
def test_purity(tmvb, ctx, name, metric, smooth):
    KA, KB, V = 130, 65, 1000
    a, b = tr.dirichlet_rows(KA, V, 3, shift=2), tr.dirichlet_rows(KB, V, 4)
    first = call(tmvb, ctx, metric, a, b, smooth, 0)
    assert first["splits"] > 1                                        # 15 pair tiles do not fill a device: the library splits here
    for sp in (0, 1, 2, 3, runs_of(V)):
        res = call(tmvb, ctx, metric, a, b, smooth, sp)
        assert res["D"].tobytes() == first["D"].tobytes(), sp
    for i0, i1 in ((0, 1), (17, 83), (96, 130)):
        part = call(tmvb, ctx, metric, a[i0:i1], b, smooth, 0)["D"]
        assert part.tobytes() == first["D"][i0:i1].tobytes(), (i0, i1)
    self_full = call(tmvb, ctx, metric, a, None, smooth, 0)["D"]
    assert call(tmvb, ctx, metric, a[17:83], a, smooth, 1)["D"].tobytes() == self_full[17:83].tobytes()


# ------------------------------------------------------------------------------------------------------------------ 5. relevance
RK, RV, RN, RL = [1, 3, 50, 130], [1, 5, 257, 3000], ["1", "10", "V"], [0.0, 0.3, 0.6, 1.0]
RCASES = pairwise_cover([RK, RV, RN, RL], lambda p: p[2] != "10" or p[1] >= 10)
assert len(RCASES) < 40


@pytest.mark.parametrize("K,V,n,lam", RCASES)
def test_relevance(tmvb, ctx, K, V, n, lam):
    n = V if n == "V" else int(n)
    beta, pw, pi = tr.relevance_inputs(K, V, 100 * K + V)
    rc, res = tmvb.term_relevance_raw(ctx, beta, pw, pi, lam, n, dense=True)
    assert rc == 0, res
    want, mag = tr.relevance(beta, pw, lam)
    dense = res["dense"]
    assert np.array_equal(np.isneginf(dense), np.isneginf(want)) and not np.isnan(dense).any()
    fin = np.isfinite(want)
    assert np.all(np.abs(dense[fin] - want[fin]) <= 8 * U * mag[fin])
    idx, score, count = tr.select(dense, n)                          # the order is judged on the device's own bits
    assert np.array_equal(res["idx"], idx) and res["score"].tobytes() == score.tobytes() and np.array_equal(res["count"], count)
    if V >= 5:
        assert np.all(dense[:, 3] == dense[:, 1]) and np.all(dense[:, V - 1] == dense[:, 2])      # the duplicated columns tie exactly
    if V >= 257 and n == V:
        assert np.all(count < n) and np.all(res["idx"][:, -1] == -1) and np.all(np.isneginf(res["score"][:, -1]))
    d, s, S = tr.term_stats(beta, pw, pi)
    assert np.all(np.abs(res["distinct"] - d) <= 8 * K * U * S) and np.all(np.abs(res["saliency"] - s) <= 8 * K * U * pw * S)
    only = tmvb.term_relevance_raw(ctx, beta, pw, pi, lam, n, dense=False, terms=False)[1]            # the optional outputs change nothing
    assert np.array_equal(only["idx"], res["idx"]) and only["score"].tobytes() == res["score"].tobytes() and only["distinct"] is None


def test_relevance_ties_keep_ascending_ids(tmvb, ctx):
    K, V = 3, 257
    beta, pw, pi = tr.relevance_inputs(K, V, 8)
    rc, res = tmvb.term_relevance_raw(ctx, beta, pw, pi, 0.6, V, dense=True)
    assert rc == 0
    for k in range(K):
        row = res["idx"][k, :res["count"][k]].tolist()
        for lo, hi in ((1, 3), (2, V - 1)):
            if lo in row:
                assert row.index(hi) == row.index(lo) + 1             # equal scores: the lower id first, the higher right behind it


# ------------------------------------------------------------------------------------------------------------------ 6. Python layer
def planted(K, V, seed):
    rng = np.random.default_rng(seed)
    A = tr.dirichlet_rows(K, V, seed, shift=1)
    copies = []
    for r in range(3):
        perm = rng.permutation(K)
        B = A[perm] * (1.0 + 0.01 * rng.standard_normal((K, V)))
        copies.append((perm, B / B.sum(axis=1, keepdims=True)))
    return A, copies


def test_planted_matching_and_stability(tmvb):
    K = 20
    A, copies = planted(K, 500, 11)
    for metric in ("js", "hellinger", "tv", "js_distance"):
        perm, B = copies[0]
        c = tmvb.compare_topics(A, B, metric=metric)
        assert c.distance.shape == (K, K) and not c.transposed and len(c.unmatched) == 0
        assert np.array_equal(perm[c.match], np.arange(K))            # B[j] is A[perm[j]]: topic i of A sits at the j with perm[j] = i
        assert np.array_equal(c.nearest, c.match) and np.all(c.match_distance < 0.05)
    wide = tmvb.compare_topics(A[:12], copies[0][1])                  # the smaller K is matched into the larger, either way round
    assert np.array_equal(copies[0][0][wide.match], np.arange(12)) and len(wide.unmatched) == K - 12
    tall = tmvb.compare_topics(copies[0][1], A[:12])
    assert tall.transposed and np.array_equal(tall.match, wide.match) and np.array_equal(tall.unmatched, wide.unmatched)
    st = tmvb.topic_stability([A] + [B for _, B in copies])
    assert st.distance.shape == (4 * K, 4 * K) and st.per_topic.shape == (K,) and st.matches.shape == (3, K)
    for r, (perm, _) in enumerate(copies):
        assert np.array_equal(perm[st.matches[r]], np.arange(K))
    D1 = tmvb.topic_distances(A, copies[1][1])
    assert st.distance[:K, 2 * K:3 * K].tobytes() == D1.tobytes()      # one stacked call = the pairwise calls, bit for bit
    assert 0.0 < st.score < 0.01 and st.score == float(np.mean(st.per_topic))
    noise = tmvb.topic_stability([A, tr.dirichlet_rows(K, 500, 99)])
    assert noise.score > 10 * st.score


def test_redundant_finds_a_planted_duplicate(tmvb):
    A = tr.dirichlet_rows(15, 400, 21, shift=2).copy()
    A[7] = A[2] * (1.0 + 1e-3 * np.random.default_rng(1).standard_normal(400))
    A[7] /= A[7].sum()
    c = tmvb.compare_topics(A)
    found = c.redundant(1e-3)
    assert [(i, j) for i, j, _ in found] == [(2, 7)] and found[0][2] == c.distance[2, 7]
    assert np.all(np.diag(c.distance) == 0.0) and np.array_equal(c.match, np.arange(15))


def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def check_model(tmvb, model):
    """-> whether relevant_terms(lam = 1) could be held to model.topics (no tie of log beta among a topic's first n + 1 terms)"""
    beta = np.ascontiguousarray(tmvb.topic_word_matrix(model))
    K, V = beta.shape
    for name, metric in (("js", JS), ("hellinger", HELLINGER), ("tv", TV)):
        D = tmvb.topic_distances(model, metric=name)
        want, sigma, S = tr.divergence(metric, beta)
        if metric == TV:
            assert np.all(np.abs(D - want) <= tr.cap_factor(V) * S)
        else:
            check_floating(name, metric, V, D, want, sigma, S)
    n = 8
    rt = tmvb.relevant_terms(model, lam=0.6, topn=n)
    assert abs(rt.topic_share.sum() - 1.0) < 1e-12 and abs(rt.pw.sum() - 1.0) < 1e-12 and rt.idx.shape == (K, n)
    want, mag = tr.relevance(beta, rt.pw, 0.6)
    for k in range(K):
        c = rt.count[k]
        got = rt.idx[k, :c]
        tol = 8 * U * mag[k]
        assert np.all(np.abs(rt.score[k, :c] - want[k, got]) <= tol[got]) and np.all(np.diff(rt.score[k, :c]) <= 0)
        rest = np.setdiff1d(np.arange(V), got)
        if c == n and rest.size:
            assert np.all(want[k, rest] - tol[rest] <= rt.score[k, c - 1] + tol[got[-1]])
        assert rt.words[k] == [str(model.corp.vocab[w + 1]) if getattr(model.corp, "vocab", None) else str(w + 1) for w in got]
    d, s, S = tr.term_stats(beta, rt.pw, rt.topic_share)
    assert np.all(np.abs(rt.distinctiveness - d) <= 8 * K * U * S) and np.all(np.abs(rt.saliency - s) <= 8 * K * U * rt.pw * S)
    assert np.all(np.diff(rt.saliency[rt.salient_idx]) <= 0)
    with_corp = tmvb.relevant_terms(model, corp=model.corp, lam=0.6, topn=n)
    counts = np.bincount(model.corp.terms, weights=model.corp.counts, minlength=V)
    np.testing.assert_allclose(with_corp.pw, counts / counts.sum(), rtol=1e-15)
    tm = tmvb.topic_map(model)
    assert tm.xy.shape == (K, 2) and np.all(np.isfinite(tm.xy)) and tm.share.shape == (K,) and abs(tm.share.sum() - 1.0) < 1e-12
    j = tmvb.compare_topics(model).jaccard(topn=5)
    assert j.shape == (K, K) and np.all(np.diag(j) == 1.0) and np.all((j >= 0) & (j <= 1))
    # lam = 1 is the order of model.topics, wherever log beta separates the first n + 1 terms
    with np.errstate(divide="ignore"):
        logb = np.log(beta)
    head = [np.asarray(t[:n + 1]) - 1 for t in model.topics]
    if any(len(np.unique(logb[k, head[k]])) < n + 1 or not np.all(np.isfinite(logb[k, head[k]])) for k in range(K)):
        return False
    r1 = tmvb.relevant_terms(model, lam=1.0, topn=n)
    assert all(np.array_equal(r1.idx[k], head[k][:n]) for k in range(K))
    return True


def trained_models(tmvb):
    g = load("lda_m40_v60_k7")
    K, V = int(g["K"]), int(g["V"])
    m = tmvb.LDA(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    yield "lda", m
    g = load("ctm_m40_v60_k5")
    K, V = int(g["K"]), int(g["V"])
    m = tmvb.CTM(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train_ctm(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    yield "ctm", m
    g = load("ctpf_m40_v60_u15_k4")
    K, V, Us = int(g["K"]), int(g["V"]), int(g["U"])
    m = tmvb.CTPF(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V, g["rdr_ptr"], g["readers"], g["ratings"], Us), K)
    m.alef = np.asfortranarray(g["alef0"]); m.alef_old = m.alef.copy(order="F")
    tmvb.gpu_train_ctpf(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    yield "ctpf", m


def test_trained_golden_models(tmvb):
    admissible = {name: check_model(tmvb, m) for name, m in trained_models(tmvb)}
    print("lam = 1 held to model.topics on:", admissible)
    assert any(admissible.values())
