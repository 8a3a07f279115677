"""
Search by words on the device (tmvb_topic_search and its Python mirror) against the NumPy restatement of tests/search_restatement.py.

Shapes sit on the edges that can go wrong: Md of one row, two, one short of a database tile, a tile, one more, two tiles and two rows; query
lengths of one entry, two, five, one short of a column tile and a whole one (128: the longest query there is); Q of one query, three and
130 (more than one column tile even at length 1); K = 1 (one real feature in a padded group of four), 3, 50 (one K-chunk), 65 (two chunks of
32 and one of 4), 130, and 1024 once; n = 1, 10, 64.  A greedy pairwise cover of that grid holds every value and every pair of values.  Two
mixed packings fill a column tile to exactly 128 entries (the next query opens a tile) and to 129 (the last query that does not fit opens one).

TOL[K] is the per-token tolerance of |score - s64| <= TOL[K] C_q + |s64| 2^-24 (C_q = the query's sum of counts; the second term is the
final rounding to fp32).  Each literal is within [1, 10] x the worst per-token deviation max(0, |score - s64| - |s64| 2^-24) / C_q this
module measured on an MI355X (profiles/search_tolerances_measured.json; a run with TMVB_SEARCH_RECORD=<file> writes such a record at the
module's end) and never above the derivable cap (K + 3) 2^-24 (tests/test_search_host.py asserts both).
"""
import itertools
import json
import os

import numpy as np
import pytest

import search_restatement as sr

pytestmark = pytest.mark.gpu

T = 128                                 # TMVB_NB_TILE_DB = TMVB_SEARCH_TILE_COLS
MDS = [1, 2, T - 1, T, T + 1, 2 * T + 2]
LENS = [1, 2, 5, T - 1, T]
QS = [1, 3, 130]
KS = [1, 3, 50, 65, 130]
NS = [1, 10, 64]
FLOAT_KS = KS + [1024]
V = 200
SMOOTH = 1e-6
# about 5 x the worst per-token deviation per K over every floating case of this module on one MI355X (0, 3.1e-8, 1.6e-7, 8.9e-8, 8.1e-9, 9.7e-8:
# profiles/search_tolerances_measured.json), each under its cap (K + 3) 2^-24; K = 1: theta is exactly 1, p is the rounded beta' itself and the
# whole deviation is the final rounding.  (K >= 100 draws theta from Dirichlet(0.01): nearly one topic per document, hence the small figures.)
TOL = {1: 0.0, 3: 1.5e-7, 50: 8.0e-7, 65: 4.4e-7, 130: 4.0e-8, 1024: 4.8e-7}
WORST = {K: 0.0 for K in FLOAT_KS}


def pairwise_cover(axes):
    """greedy: the full grid in its natural order, each time the point that covers most value pairs not covered yet"""
    grid = list(itertools.product(*axes))
    pairs = lambda p: {(i, p[i], j, p[j]) for i in range(len(p)) for j in range(i + 1, len(p))}
    todo = set().union(*(pairs(p) for p in grid))
    out = []
    while todo:
        best = max(grid, key=lambda p: len(pairs(p) & todo))
        out.append(best)
        todo -= pairs(best)
    return out


CASES = pairwise_cover([MDS, LENS, QS, KS, NS]) + [(130, 5, 3, 1024, 10)]
assert all({c[i] for c in CASES[:-1]} == set(ax) for i, ax in enumerate([MDS, LENS, QS, KS, NS])) and len(CASES) < 60
# mixed packings: the first two queries fill a column tile to exactly 128 entries / overflow it at 129
PACKINGS = {"sum128": [T - 1, 1, 5, 2, T, 1], "sum129": [T - 1, 2, 5, 1, T - 1, 1, 1], "ragged": [3, 60, 60, 5, 1, 64, 64, 1, 127, 2]}


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    out = os.environ.get("TMVB_SEARCH_RECORD", "")
    if not out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"search.score_per_token": {"measured": {str(K): WORST[K] for K in FLOAT_KS}, "tolerance": {str(K): TOL[K] for K in FLOAT_KS},
                                              "cap": {str(K): sr.cap_coeff(K) for K in FLOAT_KS},
                                              "what": "per K, max over queries and returned slots of max(0, |score - s64| - |s64| 2^-24) / C_q, "
                                                      "every floating case of tests/test_search_gpu.py"}}, f, indent=1)


def run(tmvb, ctx, theta, beta, qs, n=10, s=SMOOTH, splits=0):
    rc, res = tmvb.search_raw(ctx, theta.shape[0], beta.shape[1], theta, beta, qs[0], qs[1], qs[2], n, s, splits)
    assert rc == 0, res
    return res


def same_bytes(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in ("idx", "score", "count"))


def inputs(K, Md, seed, alpha=None):
    """theta ~ Dirichlet(0.1) (0.01 from K = 100 on), beta rows ~ Dirichlet(0.05)"""
    alpha = (0.1 if K < 100 else 0.01) if alpha is None else alpha
    return sr.dirichlet_cols(K, Md, alpha, seed), sr.dirichlet_beta(K, V, 0.05, seed + 1)


# ------------------------------------------------------------------------------------------------------------------ 1. exact selection
def device_scores(tmvb, ctx, theta, beta, qs, s=SMOOTH):
    """Q x Md float32: every document's device score, from calls on database slices of at most 64 rows with n = 64 (every row is returned)"""
    Q, Md = len(qs[0]) - 1, theta.shape[1]
    out = np.full((Q, Md), np.nan, dtype=np.float32)
    for a in range(0, Md, 64):
        b = min(a + 64, Md)
        r = run(tmvb, ctx, theta[:, a:b], beta, qs, n=64, s=s)
        assert np.all(r["count"] == b - a)
        for q in range(Q):
            i = r["idx"][q, :b - a]
            assert sorted(i.tolist()) == list(range(b - a))
            out[q, a + i] = r["score"][q, :b - a]
    assert not np.isnan(out).any()
    return out


@pytest.mark.parametrize("Md,K,n,packing", [(2 * T + 2, 50, 10, "sum128"), (2 * T + 2, 3, 64, "sum129"), (T + 1, 65, 1, "ragged"), (T - 1, 130, 64, "sum128"),
                                            (3 * T + 5, 1, 10, "sum129")])
def test_exact_selection_on_the_device_scores(tmvb, ctx, Md, K, n, packing):
    """independent of any libm: a database of few distinct rows, so ties are everywhere; the full call's lists must be the lexsort of the
    device's own score bits, taken from calls on database slices -- and duplicated rows carry identical bits wherever they lie"""
    distinct, beta = inputs(K, 7, seed=11 * K + Md)
    rng = np.random.Generator(np.random.PCG64(Md + K))
    which = rng.integers(0, 7, size=Md)
    theta = distinct[:, which]
    qs = sr.make_queries(PACKINGS[packing], V, seed=5 * K + n)
    S = device_scores(tmvb, ctx, theta, beta, qs)
    for w in range(7):
        rows = np.flatnonzero(which == w)
        assert np.all(S[:, rows].view(np.uint32) == S[:, rows[:1]].view(np.uint32)), w
    idx, score, count = sr.np_topn(S, n)
    for splits in (0, 1):
        res = run(tmvb, ctx, theta, beta, qs, n=n, splits=splits)
        assert np.array_equal(res["count"], count) and np.all(count == min(n, Md))
        assert np.array_equal(res["idx"], idx), np.argwhere(res["idx"] != idx)[:5]
        assert res["score"].tobytes() == score.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 2. p is the neighbours scan's p
@pytest.mark.parametrize("K,Md", [(3, 40), (50, 2 * T + 2), (130, T + 1)])
def test_single_entry_scores_are_the_log_of_the_neighbours_dot(tmvb, ctx, K, Md):
    theta, beta = inputs(K, Md, seed=21 * K)
    terms = np.arange(0, V, 7, dtype=np.int32)
    qs = (np.arange(len(terms) + 1, dtype=np.int64), terms, np.ones(len(terms), dtype=np.int32))
    res = run(tmvb, ctx, theta, beta, qs, n=64)
    rc, nb = tmvb.neighbors_raw(ctx, K, 0, theta, sr.beta_prime(beta, SMOOTH)[:, terms], 0, 64)          # TMVB_NB_DOT: returns p
    assert rc == 0, nb
    met = 0
    for q in range(len(terms)):
        p_of = dict(zip(nb["idx"][q, :nb["count"][q]].tolist(), nb["score"][q, :nb["count"][q]].tolist()))
        have = [(j, p_of[int(d)]) for j, d in enumerate(res["idx"][q, :res["count"][q]]) if int(d) in p_of]
        assert len(have) >= min(Md, 64) // 2, (q, len(have))           # the two lists differ only where the rounded log merges neighbours
        p = np.asarray([v for _, v in have], dtype=np.float32)
        got = res["score"][q, [j for j, _ in have]]
        # along the search list p falls wherever the score falls (the logarithm is monotone).  Where the rounded log merges neighbours the
        # scores tie, the index decides, and p may rise inside the tie by less than the rounding merged: the 1-ulp check below holds it
        assert np.all(np.diff(p)[np.diff(got) < 0] < 0), q
        want = np.log(p.astype(np.float64)).astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)), q   # 1 fp32 ulp
        met += len(have)
    assert met > 0


# ------------------------------------------------------------------------------------------------------------------ 3. floating data
def assert_floating(res, S64, C, n, tol, tag=None):
    """the four checks of every query; returns the worst per-token deviation max(0, |score - s64| - |s64| 2^-24) / C_q"""
    Q, Md = S64.shape
    idx, score, count = res["idx"], res["score"].astype(np.float64), res["count"]
    assert np.all(count == min(n, Md)), tag
    worst = 0.0
    for q in range(Q):
        c = int(count[q])
        i, s = idx[q, :c], score[q, :c]
        assert np.all(idx[q, c:] == -1) and np.all(np.isneginf(score[q, c:]))
        assert len(set(i.tolist())) == c and i.min() >= 0 and i.max() < Md, (tag, q)                    # distinct and valid
        assert np.all(np.diff(s) <= 0) and np.all(np.diff(i)[np.diff(s) == 0] > 0), (tag, q)            # the total order
        dev = np.abs(s - S64[q, i])
        rnd = np.abs(S64[q, i]) * 2.0 ** -24
        bound = tol * C[q] + rnd
        worst = max(worst, float(np.maximum(0.0, dev - rnd).max()) / C[q])
        assert np.all(dev <= bound), (tag, q, float((dev - bound).max()), float(bound.max()))
        rest = np.ones(Md, dtype=bool)
        rest[i] = False
        if rest.any():                                                                                  # completeness
            last = S64[q, i[-1]]
            assert S64[q, rest].max() <= last + 2 * (tol * C[q] + abs(last) * 2.0 ** -24), (tag, q, S64[q, rest].max() - last)
    return worst


def floating_case(tmvb, ctx, Md, lengths, K, n, seed):
    theta, beta = inputs(K, Md, seed)
    qs = sr.make_queries(lengths, V, seed + 2)
    S64 = sr.s64(theta, beta, SMOOTH, *qs)
    res = run(tmvb, ctx, theta, beta, qs, n=n)
    assert res["kp"] == (K + 3) // 4 * 4
    worst = assert_floating(res, S64, sr.tokens(qs[0], qs[2]), n, TOL[K], tag=(Md, lengths[:3], K, n))
    print(f"search Md = {Md} Q = {len(lengths)} K = {K} n = {n}: worst per-token deviation = {worst:.3e} (tolerance {TOL[K]:.3e}, cap {sr.cap_coeff(K):.3e})")
    WORST[K] = max(WORST[K], worst)
    assert TOL[K] <= sr.cap_coeff(K)
    return res


@pytest.mark.parametrize("Md,L,Q,K,n", CASES, ids=lambda v: str(v))
def test_floating_scores(tmvb, ctx, Md, L, Q, K, n):
    res = floating_case(tmvb, ctx, Md, [L] * Q, K, n, seed=1000 * Md + 10 * K + L)
    assert res["col_tiles"] == -(-Q // (T // L))


@pytest.mark.parametrize("packing", sorted(PACKINGS))
def test_floating_scores_of_mixed_packings(tmvb, ctx, packing):
    lengths = PACKINGS[packing]
    res = floating_case(tmvb, ctx, 2 * T + 2, lengths, 50, 10, seed=77)
    assert res["col_tiles"] == {"sum128": 4, "sum129": 4, "ragged": 5}[packing]


# ------------------------------------------------------------------------------------------------------------------ 4. against the held-out scorer
@pytest.mark.parametrize("K,L", [(3, 2), (50, 5), (130, T)])
def test_against_heldout_loglik(tmvb, ctx, K, L):
    Md = T + 1
    theta, beta = inputs(K, Md, seed=41 * K)
    qs = sr.make_queries([L], V, seed=43 * K)
    res = run(tmvb, ctx, theta, beta, qs, n=64)
    pc = tmvb.PackedCorpus(np.arange(Md + 1, dtype=np.int64) * L, np.tile(qs[1], Md), np.tile(qs[2], Md), V)    # the query as every document's held-out words
    rc, ho = tmvb.heldout_loglik_raw(ctx, K, V, theta, beta, pc, SMOOTH)
    assert rc == 0, ho
    C = float(qs[2].sum())
    i = res["idx"][0]
    ll = ho.ll[i]
    assert np.all(ho.tokens == int(C))
    bound = 2 * (TOL[K] * C + np.abs(ll) * 2.0 ** -24)
    print(f"search against heldout_loglik K = {K} L = {L}: worst |score - ll| / bound = {float((np.abs(res['score'][0].astype(np.float64) - ll) / bound).max()):.3f}")
    assert np.all(np.abs(res["score"][0].astype(np.float64) - ll) <= 2 * (TOL[K] * C + np.abs(ll) * 2.0 ** -24))


# ------------------------------------------------------------------------------------------------------------------ 5. purity
@pytest.mark.parametrize("K,packing", [(50, "sum128"), (65, "sum129"), (3, "ragged")])
def test_splits_calls_slices_and_permutations_give_identical_bytes(tmvb, ctx, K, packing):
    Md, n = 2 * T + 2, 10
    theta, beta = inputs(K, Md, seed=51 * K)
    lengths = PACKINGS[packing] + [1] * 130                           # the single-entry tail alone fills more than one column tile
    qs = sr.make_queries(lengths, V, seed=53 * K)
    Q = len(lengths)
    base = run(tmvb, ctx, theta, beta, qs, n=n, splits=1)
    assert base["splits"] == 1 and base["ms"]["scan"] > 0 and base["ms"]["prep"] > 0 and base["ms"]["merge"] == 0
    used = set()
    for splits in (0, 1, 2, 3, 1):                                    # splits, and the same call twice
        r = run(tmvb, ctx, theta, beta, qs, n=n, splits=splits)
        used.add(r["splits"])
        assert same_bytes(r, base), splits
    assert {1, 2, 3} <= used
    part = lambda r, sel: {f: r[f][sel] for f in ("idx", "score", "count")}
    for a, b in ((0, 1), (1, 3), (2, Q), (Q - 1, Q), (5, 70)):        # query slices, among them batches of one
        r = run(tmvb, ctx, theta, beta, sr.slice_queries(*qs, range(a, b)), n=n)
        assert same_bytes(r, part(base, slice(a, b))), (a, b)
    perm = np.random.Generator(np.random.PCG64(K)).permutation(Q)     # the same query in another column position and tile
    r = run(tmvb, ctx, theta, beta, sr.slice_queries(*qs, perm), n=n)
    assert same_bytes(r, part(base, perm))


# ------------------------------------------------------------------------------------------------------------------ 6. zero probability
@pytest.mark.parametrize("Md,n", [(130, 64), (40, 64), (2 * T + 2, 10)])
def test_zero_probability_documents_come_last_in_index_order(tmvb, ctx, Md, n):
    K, G = 3, V // 3
    beta = np.zeros((K, V))
    for g in range(K):
        beta[g, g * G:(g + 1) * G] = 1.0 / G                          # disjoint vocabularies: exact zeros
    beta[K - 1, K * G:] = 0.0
    beta[K - 1, (K - 1) * G:] = 1.0 / (V - (K - 1) * G)
    rng = np.random.Generator(np.random.PCG64(Md))
    theta = np.zeros((K, Md))
    kind = rng.integers(0, 4, size=Md)                                # 0, 1, 2: all mass on that topic; 3: a mixture of all
    for d in range(Md):
        theta[:, d] = rng.dirichlet(np.ones(K)) if kind[d] == 3 else np.eye(K)[kind[d]]
    qs = (np.array([0, 2, 3, 5], dtype=np.int64), np.array([1, 2, G + 1, 3, 2 * G + 4], dtype=np.int32), np.array([1, 2, 1, 1, 3], dtype=np.int32))
    S64 = sr.s64(theta, beta, 0.0, *qs)
    res = run(tmvb, ctx, theta, beta, qs, n=n, s=0.0)
    assert np.all(res["count"] == min(n, Md))
    for q, topics in enumerate(([0], [1], [0, 2])):
        finite = np.flatnonzero(np.isfinite(S64[q]))
        assert set(finite.tolist()) == {d for d in range(Md) if kind[d] == 3 or (len(topics) == 1 and kind[d] == topics[0])}
        c = int(res["count"][q])
        i, s = res["idx"][q, :c], res["score"][q, :c]
        k = min(c, len(finite))
        assert np.all(np.isfinite(s[:k])) and set(i[:k].tolist()) <= set(finite.tolist())
        assert np.all(np.isneginf(s[k:]))
        rest = np.setdiff1d(np.arange(Md), finite)
        assert np.array_equal(i[k:], rest[:c - k])                     # the unsupported documents: after all finite ones, ascending index
    if Md < n:
        assert np.all(res["idx"][:, Md:] == -1) and np.all(np.isneginf(res["score"][:, Md:]))


# ------------------------------------------------------------------------------------------------------------------ 7. plumbing
GROUPS, PER_GROUP, PV = 3, 67, 90


def planted_corpus(tmvb, per_group, seed):
    """documents of GROUPS groups, group g first: generated by gencorp from a model whose topics have disjoint vocabularies and whose alpha puts
    a document of group g on topic g almost entirely"""
    host = tmvb.LDA(tmvb.syn_nsf(M=30, V=PV, seed=9), GROUPS)
    beta = np.zeros((GROUPS, PV))
    for g in range(GROUPS):
        beta[g, g * (PV // GROUPS):(g + 1) * (PV // GROUPS)] = 1.0 / (PV // GROUPS)
    host.beta = np.asfortranarray(beta)
    ptr, terms, counts = [np.zeros(1, dtype=np.int64)], [], []
    for g in range(GROUPS):
        host.alpha = np.where(np.arange(GROUPS) == g, 60.0, 0.05)
        pc = tmvb.gencorp(host, per_group, laplace_smooth=1e-4, seed=seed + g)
        ptr.append(pc.doc_ptr[1:] + ptr[-1][-1]); terms.append(pc.terms); counts.append(pc.counts)
    pc = tmvb.PackedCorpus(np.concatenate(ptr), np.concatenate(terms), np.concatenate(counts), PV)
    assert pc.M == GROUPS * per_group and np.all(pc.N > 0)
    return pc, np.repeat(np.arange(GROUPS), per_group)


def test_end_to_end_planted_groups(tmvb):
    pc, group = planted_corpus(tmvb, PER_GROUP, seed=100)
    fresh, fresh_group = planted_corpus(tmvb, 8, seed=200)
    W = PV // GROUPS
    ids = [[g * W + 1, g * W + 4, g * W + 9] for g in range(GROUPS)]                    # 1-based ids of three words of each group
    lda = tmvb.LDA(pc, GROUPS)
    tmvb.gpu_train(lda, iter=40, tol=0.0, checkelbo=float("inf"), printelbo=False)
    ctm = tmvb.CTM(pc, GROUPS)
    tmvb.gpu_train_ctm(ctm, iter=40, tol=0.0, checkelbo=float("inf"), printelbo=False)
    for model, pred in ((lda, tmvb.predict), (ctm, tmvb.predict_ctm)):
        r = tmvb.search(model, ids, topn=5, laplace_smooth=1e-6)
        assert r.idx.shape == (GROUPS, 5) and np.all(r.count == 5) and r.tokens.tolist() == [3, 3, 3]
        assert np.array_equal(group[r.idx], np.repeat(np.arange(GROUPS)[:, None], 5, axis=1)), type(model).__name__
        assert np.all(np.diff(r.score, axis=1) <= 0) and np.allclose(r.loglik_per_token, r.score.astype(np.float64) / 3.0, rtol=0, atol=0)
        assert r.info["col_tiles"] == 1 and r.info["ms"]["scan"] > 0
        # the three forms of a query say the same thing: words (a PackedCorpus names its terms "1" .. "V"), 1-based ids, term -> count
        words = tmvb.search(model, [[str(t) for t in q] for q in ids], topn=5, laplace_smooth=1e-6)
        dicts = tmvb.search(model, [{t: 1 for t in q} for q in ids], topn=5, laplace_smooth=1e-6)
        twice = tmvb.search(model, [q + q[:1] for q in ids], topn=5, laplace_smooth=1e-6)       # a repeated word is merged: count 2, first position
        dict2 = tmvb.search(model, [{str(q[0]): 2, q[1]: 1, q[2]: 1} for q in ids], topn=5, laplace_smooth=1e-6)
        for other in (words, dicts):
            assert np.array_equal(other.idx, r.idx) and other.score.tobytes() == r.score.tobytes()
        assert np.array_equal(twice.idx, dict2.idx) and twice.score.tobytes() == dict2.score.tobytes() and twice.tokens.tolist() == [4, 4, 4]
        with pytest.raises(ValueError, match="not in the model's vocabulary"):
            tmvb.search(model, [["1", "no such word"]], topn=5)
        skipped = tmvb.search(model, [[str(t) for t in q] + ["no such word"] for q in ids], topn=5, laplace_smooth=1e-6, skip_unknown=True)
        assert np.array_equal(skipped.idx, r.idx) and skipped.score.tobytes() == r.score.tobytes()
        # unseen documents: theta = what predict returned
        f = tmvb.search(model, ids, topn=5, laplace_smooth=1e-6, theta=pred(fresh, model))
        assert f.idx.shape == (GROUPS, 5) and f.idx.max() < fresh.M
        assert np.array_equal(fresh_group[f.idx], np.repeat(np.arange(GROUPS)[:, None], 5, axis=1)), type(model).__name__
        P = tmvb.topic_proportions(model)
        g = tmvb.search(model, ids, topn=5, laplace_smooth=1e-6, theta=P)
        assert np.array_equal(g.idx, r.idx) and g.score.tobytes() == r.score.tobytes()
