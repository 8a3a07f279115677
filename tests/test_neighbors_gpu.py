"""
Nearest documents in topic space on the device (tmvb_topic_neighbors and its Python mirror) against the NumPy checker of
tests/test_neighbors_host.py: the selection bit for bit where the scores are exact, and within a tolerance frozen from its own MI355X
measurement where they are not.

Exact cases: DOT on integer features in [0, 15], K <= 64 (every dot product is an integer below 2^24: fp32 and fp64 agree), drawn from few
levels so that ties are everywhere; idx, score and count must equal the lexsort of the fp64 score matrix.  The database's LAST row is all
15 where every other entry is at most 14, and every row's first feature is at least 1: the last row is the single best match of every
query, so a scan that loses the last rows of the database cannot pass by luck (tests/test_neighbors_mutant_gpu.py relies on it).
Shapes, T = TMVB_NB_TILE_DB = 128 database rows per tile and 128 queries per workgroup: Md around one row, one 32-row MFMA block, one tile and
two tiles with a partial third; Mq of one row, past one MFMA block, past one wave's 64 rows; K = 1 (one real feature in a padded group of
four), 2, 3, 50 (the SYN-NSF size), 64 (the largest exact K: a full single K-chunk); n = 1, 10, 64.  A greedy pairwise cover of that grid, built
below, holds every value of every parameter and every pair of values.

Floating cases: HELLINGER and COSINE on Dirichlet columns; K = 1, 3 (one padded group), 50 (one chunk), 65 (68 floats: two chunks of 32 and
one of 4), 130, 1024 (the largest K: 32 chunks).  TOL[K] bounds |score - s64|, s64 the fp64 dot product of the fp64 features: each literal is
within [1, 10] x the worst deviation this module measured on an MI355X (profiles/neighbors_tolerances_measured.json; the run with
TMVB_NEIGHBORS_RECORD=<file> writes such a record at the module's end) and never above the derivable cap (K + 3) 2^-24
(tests/test_neighbors_host.py asserts both).
"""
import itertools
import json
import os

import numpy as np
import pytest

from test_neighbors_host import COSINE, DOT, HELLINGER, T, cap, dirichlet_cols, integer_rows, np_scores64, np_topn

pytestmark = pytest.mark.gpu

MDS = [1, 2, 31, 32, 33, T, T + 1, 2 * T + 2]
MQS = [1, 33, 65]
KS = [1, 2, 3, 50, 64]
NS = [1, 10, 64]
FLOAT_KS = [1, 3, 50, 65, 130, 1024]
# about 4 x the worst |score - s64| per K over every floating case of this module on one MI355X (1.2e-7, 3.0e-7, 3.5e-7, 5.3e-7, 1.3e-6), K = 3
# held under its cap of 3.58e-7; K = 1: every feature and every score is exactly 1
TOL = {1: 0.0, 3: 3.5e-7, 50: 1.2e-6, 65: 1.4e-6, 130: 2.1e-6, 1024: 5.2e-6}
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


CASES = pairwise_cover([MDS, MQS, KS, NS])
assert all({c[i] for c in CASES} == set(ax) for i, ax in enumerate([MDS, MQS, KS, NS])) and len(CASES) < 60


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    out = os.environ.get("TMVB_NEIGHBORS_RECORD", "")
    if not out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"neighbors.score_abs": {"measured": {str(K): WORST[K] for K in FLOAT_KS}, "tolerance": {str(K): TOL[K] for K in FLOAT_KS},
                                           "cap": {str(K): cap(K) for K in FLOAT_KS},
                                           "what": "per K, max over queries and returned slots of |score - fp64 dot product of the fp64 features|, "
                                                   "every floating case of tests/test_neighbors_gpu.py"}}, f, indent=1)


def run(tmvb, ctx, K, metric, xd, xq=None, q0=0, n=10, splits=0, Mq=None):
    rc, res = tmvb.neighbors_raw(ctx, K, metric, xd, xq, q0, n, splits, Mq=Mq)
    assert rc == 0, res
    return res


def exact_rows(K, M, seed):
    """integer features in [0, 14] from few levels, first feature >= 1; the caller plants the all-15 row"""
    x = integer_rows(K, M, seed, levels=(0, 1, 2, 14))
    x[0] = np.maximum(x[0], 1.0)
    return x


def assert_exact(res, S, n, self_of=None, tag=None):
    idx, score, count = np_topn(S, n, self_of)
    assert res["idx"].dtype == np.int32 and res["score"].dtype == np.float32 and res["idx"].shape == idx.shape
    assert np.array_equal(res["count"], count), (tag, res["count"], count)
    assert np.array_equal(res["idx"], idx), (tag, np.argwhere(res["idx"] != idx)[:5])
    assert res["score"].tobytes() == score.astype(np.float32).tobytes(), tag


# ------------------------------------------------------------------------------------------------------------------ exact selection
@pytest.mark.parametrize("Md,Mq,K,n", CASES, ids=lambda v: str(v))
def test_exact_selection(tmvb, ctx, Md, Mq, K, n):
    xd = exact_rows(K, Md, seed=1000 * Md + K)
    xd[:, -1] = 15.0
    xq = exact_rows(K, Mq, seed=77 * Mq + K)
    S = np_scores64(xd, xq, DOT)
    assert S.max() < 2 ** 24
    if Md > 1:
        assert np.all(S[:, -1] > S[:, :-1].max(axis=1))                                  # the last row is every query's single best match
    assert_exact(run(tmvb, ctx, K, DOT, xd, xq, n=n), S, n, tag="explicit queries")
    m = min(Mq, Md)                                                                      # queries that are database rows: at most Md of them
    for q0 in sorted({q for q in (0, T - 1, Md - m) if 0 <= q and q + m <= Md}):
        sel = np.arange(q0, q0 + m)
        res = run(tmvb, ctx, K, DOT, xd, None, q0, n, Mq=m)
        assert_exact(res, np_scores64(xd, xd[:, sel], DOT), n, self_of=sel, tag=f"self-exclusion at q0 = {q0}")
        if n > Md - 1:                                                                   # more slots than candidates
            assert np.all(res["count"] == Md - 1) and np.all(res["idx"][:, Md - 1:] == -1) and np.all(np.isneginf(res["score"][:, Md - 1:]))


def rows_of_score(scores, K=64):
    """K x M integer features in [0, 15] with column sums `scores`: against the all-ones query, row i scores scores[i] exactly"""
    x = np.zeros((K, len(scores)))
    for i, s in enumerate(scores):
        full, rest = divmod(int(s), 15)
        x[:full, i] = 15.0
        if rest:
            x[full, i] = rest
    assert np.array_equal(x.sum(axis=0), scores)
    return x


@pytest.mark.parametrize("order", ["ascending", "descending", "identical"])
@pytest.mark.parametrize("n", [1, 64])
def test_adversarial_visiting_order(tmvb, ctx, order, n):
    """one query against a database sorted by score: ascending (every row beats the threshold it meets), descending (none after the first n
    does), all rows identical (the index decides everything)"""
    Md, K = 3 * T + 5, 64
    s = np.arange(Md, dtype=np.float64)
    xd = rows_of_score({"ascending": s, "descending": s[::-1].copy(), "identical": np.full(Md, 100.0)}[order], K)
    xq = np.ones((K, 1))
    S = np_scores64(xd, xq, DOT)
    for splits in (0, 1):
        res = run(tmvb, ctx, K, DOT, xd, xq, n=n, splits=splits)
        assert_exact(res, S, n, tag=(order, splits))
    want = {"ascending": np.arange(Md - 1, Md - 1 - n, -1), "descending": np.arange(n), "identical": np.arange(n)}[order]
    assert np.array_equal(res["idx"][0], want)


# ------------------------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("Md", [300, 2 * T + 2])
def test_splits_calls_and_query_shards_give_identical_bits(tmvb, ctx, Md):
    K, n = 50, 10
    for metric, xd in ((DOT, exact_rows(8, Md, seed=5)), (HELLINGER, dirichlet_cols(K, Md, 0.1, seed=6))):
        Kx = xd.shape[0]
        base = run(tmvb, ctx, Kx, metric, xd, None, 0, n, splits=1)
        assert base["splits"] == 1 and base["ms"]["scan"] > 0 and base["ms"]["prep"] > 0 and base["ms"]["merge"] == 0
        used = set()
        for splits in (1, 2, 3, 7, 0):
            r = run(tmvb, ctx, Kx, metric, xd, None, 0, n, splits=splits)
            used.add(r["splits"])
            for f in ("idx", "score", "count"):
                assert r[f].tobytes() == base[f].tobytes(), (metric, splits, f)
        assert {1, 2, 3} <= used                                     # the database has three tiles: at most three splits
        xq = xd[:, ::3]
        eb = run(tmvb, ctx, Kx, metric, xd, xq, n=n, splits=1)
        for splits in (2, 3, 7, 0):
            r = run(tmvb, ctx, Kx, metric, xd, xq, n=n, splits=splits)
            assert all(r[f].tobytes() == eb[f].tobytes() for f in ("idx", "score", "count")), (metric, splits)
        for q0, m in ((0, 1), (T - 1, 2), (Md - 70, 70), (130, 65)):
            r = run(tmvb, ctx, Kx, metric, xd, None, q0, n, Mq=m)
            for f in ("idx", "score", "count"):
                assert r[f].tobytes() == base[f][q0:q0 + m].tobytes(), (metric, q0, m, f)


# ------------------------------------------------------------------------------------------------------------------ floating metrics
def assert_floating(res, S64, n, tol, self_of=None, tag=None):
    """the four checks of every query; returns the worst |score - s64|"""
    Mq, Md = S64.shape
    idx, score, count = res["idx"], res["score"].astype(np.float64), res["count"]
    cand = Md - (0 if self_of is None else 1)
    assert np.all(count == min(n, cand)), tag
    worst = 0.0
    for q in range(Mq):
        c = int(count[q])
        i, s = idx[q, :c], score[q, :c]
        assert np.all(idx[q, c:] == -1) and np.all(np.isneginf(score[q, c:]))
        assert len(set(i.tolist())) == c and i.min() >= 0 and i.max() < Md, (tag, q)                    # distinct and valid
        assert self_of is None or self_of[q] not in i, (tag, q)                                         # not the query itself
        assert np.all(np.diff(s) <= 0) and np.all(np.diff(i)[np.diff(s) == 0] > 0), (tag, q)            # the total order
        dev = float(np.abs(s - S64[q, i]).max())
        worst = max(worst, dev)
        assert dev <= tol, (tag, q, dev, tol)
        rest = np.ones(Md, dtype=bool)
        rest[i] = False
        if self_of is not None:
            rest[self_of[q]] = False
        if rest.any():                                                                                  # completeness
            assert S64[q, rest].max() <= S64[q, i[-1]] + 2 * tol, (tag, q, S64[q, rest].max() - S64[q, i[-1]])
    return worst


@pytest.mark.parametrize("alpha", [0.1, 1.0])
@pytest.mark.parametrize("metric", [HELLINGER, COSINE], ids=["hellinger", "cosine"])
@pytest.mark.parametrize("K", FLOAT_KS)
def test_floating_metrics(tmvb, ctx, K, metric, alpha):
    Md, n = 2 * T + 2, 10
    xd = dirichlet_cols(K, Md, alpha, seed=31 * K + int(10 * alpha))
    S64 = np_scores64(xd, xd, metric)
    res = run(tmvb, ctx, K, metric, xd, None, 0, n)
    assert res["kp"] == (K + 3) // 4 * 4
    worst = assert_floating(res, S64, n, TOL[K], self_of=np.arange(Md), tag=(K, metric, alpha, "all pairs"))
    xq = dirichlet_cols(K, 65, alpha, seed=32 * K + int(10 * alpha))
    res = run(tmvb, ctx, K, metric, xd, xq, n=n)
    worst = max(worst, assert_floating(res, np_scores64(xd, xq, metric), n, TOL[K], tag=(K, metric, alpha, "explicit queries")))
    print(f"neighbors K = {K} metric = {metric} alpha = {alpha}: worst |score - s64| = {worst:.3e} (tolerance {TOL[K]:.3e}, cap {cap(K):.3e})")
    WORST[K] = max(WORST[K], worst)
    assert TOL[K] <= cap(K)


# ------------------------------------------------------------------------------------------------------------------ end to end
GROUPS, PER_GROUP, V = 3, 67, 90


def planted_corpus(tmvb, per_group, seed):
    """documents of GROUPS groups, group g first: generated by gencorp from a model whose topics have disjoint vocabularies and whose alpha puts
    a document of group g on topic g almost entirely"""
    host = tmvb.LDA(tmvb.syn_nsf(M=30, V=V, seed=9), GROUPS)
    beta = np.zeros((GROUPS, V))
    for g in range(GROUPS):
        beta[g, g * (V // GROUPS):(g + 1) * (V // GROUPS)] = 1.0 / (V // GROUPS)
    host.beta = np.asfortranarray(beta)
    ptr, terms, counts = [np.zeros(1, dtype=np.int64)], [], []
    for g in range(GROUPS):
        host.alpha = np.where(np.arange(GROUPS) == g, 60.0, 0.05)
        pc = tmvb.gencorp(host, per_group, laplace_smooth=1e-4, seed=seed + g)
        ptr.append(pc.doc_ptr[1:] + ptr[-1][-1]); terms.append(pc.terms); counts.append(pc.counts)
    pc = tmvb.PackedCorpus(np.concatenate(ptr), np.concatenate(terms), np.concatenate(counts), V)
    assert pc.M == GROUPS * per_group and np.all(pc.N > 0)
    return pc, np.repeat(np.arange(GROUPS), per_group)


def test_end_to_end_planted_groups(tmvb):
    pc, group = planted_corpus(tmvb, PER_GROUP, seed=100)
    fresh, fresh_group = planted_corpus(tmvb, 8, seed=200)
    lda = tmvb.LDA(pc, GROUPS)
    tmvb.gpu_train(lda, iter=40, tol=0.0, checkelbo=float("inf"), printelbo=False)
    ctm = tmvb.CTM(pc, GROUPS)
    tmvb.gpu_train_ctm(ctm, iter=40, tol=0.0, checkelbo=float("inf"), printelbo=False)
    for model, pred in ((lda, tmvb.predict), (ctm, tmvb.predict_ctm)):
        r = tmvb.docsim(model, topn=5)
        assert r.idx.shape == (pc.M, 5) and np.all(r.count == 5) and r.metric == "hellinger"
        assert np.array_equal(group[r.idx], np.repeat(group[:, None], 5, axis=1)), type(model).__name__
        assert np.all(r.idx != np.arange(pc.M)[:, None])
        assert np.all((r.distance >= 0) & (r.distance <= 1)) and np.all(np.diff(r.distance, axis=1) >= 0)
        q = tmvb.docsim(model, topn=5, queries=pred(fresh, model))
        assert q.idx.shape == (fresh.M, 5)
        assert np.array_equal(group[q.idx], np.repeat(fresh_group[:, None], 5, axis=1)), type(model).__name__
        # a contiguous range, a single document and a scattered list are the rows of the all-documents call
        for docs in (range(60, 71), 7, [200, 3, 68]):
            part = tmvb.docsim(model, docs=docs, topn=5)
            rows = np.atleast_1d(np.asarray(docs)) - 1
            assert np.array_equal(part.idx, r.idx[rows]) and part.score.tobytes() == r.score[rows].tobytes()
        c = tmvb.docsim(model, docs=[1, 100], topn=3, metric="cosine")
        assert np.array_equal(group[c.idx], np.repeat(group[[0, 99], None], 3, axis=1)) and np.all(np.diff(c.distance, axis=1) >= 0)


def test_end_to_end_ctpf_and_flda(tmvb):
    pf = tmvb.syn_citeu(M=60, V=150, U=20, seed=5)
    f = tmvb.CTPF(pf, 3)
    tmvb.gpu_train_ctpf(f, iter=3, tol=0.0, checkelbo=float("inf"), printelbo=False)
    pc = tmvb.syn_nsf(M=120, V=300, seed=4)
    m = tmvb.fLDA(pc, 3)
    tmvb.gpu_train_flda(m, iter=4, tol=0.0, checkelbo=float("inf"), printelbo=False)
    for model in (f, m):
        P = tmvb.topic_proportions(model)
        r = tmvb.docsim(model, topn=5)
        res = {"idx": r.idx, "score": r.score, "count": r.count}
        worst = assert_floating(res, np_scores64(P, P, HELLINGER), 5, TOL[3], self_of=np.arange(P.shape[1]), tag=type(model).__name__)
        WORST[3] = max(WORST[3], worst)
