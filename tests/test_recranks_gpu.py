"""
The ranks of held-out pairs on the device (tmvb_score_ranks and its Python mirror) against the NumPy checkers of tests/test_recranks_host.py:
bit for bit where the scores are exact, exactly the ranks of the returned fp32 scores where every score is returned, and inside the interval
that the fp64 scores allow where they are not.

Exact cases: integer features from the levels (0, 1, 2, 14), K <= 64 (every dot product is an integer below 2^24: fp32 and fp64 agree), ties
everywhere; rank, n_cand and score must equal NumPy's.  The database's LAST row is all 15 and is neither a target nor excluded: it comes
before every target of every query, so a scan that loses the last rows of the database cannot pass by luck
(tests/test_recranks_mutant_gpu.py relies on it).  Shapes, T = 128 database rows per tile and 128 queries per workgroup: Md around one row,
one 32-row MFMA block, one tile and two tiles with a partial third; Mq of one row, past one MFMA block, past one wave's 64 rows, past one
workgroup; K = 1, 2, 3, 50, 64; exclusions none / random / every non-target; targets for some queries only / one each / random.  A greedy
pairwise cover of that grid, built below, holds every value of every parameter and every pair of values.  (With Md = 1 the only row is the
planted one and no query has a target; with Md = 2 row 0 is the only possible target.)
"""
import itertools
import json
import os

import numpy as np
import pytest

from test_recranks_host import (FLOAT_KS, T, all_targets_case, bounds_case, csr_of, eps_of, exact_case, np_rank_bounds, np_ranks)

pytestmark = pytest.mark.gpu

MDS = [1, 2, 31, 32, 33, T, T + 1, 2 * T + 2]
MQS = [1, 33, 65, 129]
KS = [1, 2, 3, 50, 64]
EXCL = ["none", "random", "all"]
TGT = ["some_none", "one_each", "random"]
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


CASES = pairwise_cover([MDS, MQS, KS, EXCL, TGT])
assert all({c[i] for c in CASES} == set(ax) for i, ax in enumerate([MDS, MQS, KS, EXCL, TGT])) and len(CASES) < 70


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    out = os.environ.get("TMVB_RECRANKS_RECORD", "")
    if not out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"recranks.score_rel": {"measured": {str(K): WORST[K] for K in FLOAT_KS}, "cap": {str(K): eps_of(K) for K in FLOAT_KS},
                                          "what": "per K, max over the returned scores of |score - s64| / s64, s64 the fp64 dot product of the fp64 "
                                                  "factors; the floating cases of tests/test_recranks_gpu.py.  For information: the cap is the test."}}, f, indent=1)


def run(tmvb, ctx, xd, xq, excl, tgt, splits=0):
    rc, res = tmvb.rec_ranks_raw(ctx, xd.shape[0], xd, xq, excl, tgt, splits)
    assert rc == 0, res
    return res


def assert_exact(res, S, excl, tgt, tag=None):
    rank, n_cand = np_ranks(S, excl, tgt)
    q_of = np.repeat(np.arange(S.shape[0]), np.diff(tgt[0]))
    assert res["rank"].dtype == np.int32 and res["score"].dtype == np.float32 and res["rank"].shape == rank.shape
    assert np.array_equal(res["n_cand"], n_cand), (tag, res["n_cand"], n_cand)
    assert res["score"].tobytes() == S[q_of, tgt[1]].astype(np.float32).tobytes(), tag
    assert np.array_equal(res["rank"], rank), (tag, np.argwhere(res["rank"] != rank)[:5].ravel(), res["rank"][:8], rank[:8])


# ------------------------------------------------------------------------------------------------------------------ exact ranks
@pytest.mark.parametrize("Md,Mq,K,excl_mode,tgt_mode", CASES, ids=lambda v: str(v))
def test_exact_ranks(tmvb, ctx, Md, Mq, K, excl_mode, tgt_mode):
    xd, xq, excl, tgt = exact_case(Md, Mq, K, excl_mode, tgt_mode)
    S = xq.T @ xd
    assert S.max() < 2 ** 24 and (Md == 1 or np.all(S[:, -1] > S[:, :-1].max(axis=1)))
    assert Md - 1 not in tgt[1] and Md - 1 not in excl[1]
    assert Md <= 2 or tgt[0][-1] > 0
    res = run(tmvb, ctx, xd, xq, excl, tgt)
    assert res["kp"] == (K + 3) // 4 * 4
    assert_exact(res, S, excl, tgt, tag=(Md, Mq, K, excl_mode, tgt_mode))
    assert np.all(res["rank"] >= 1)                                  # the planted row comes before every target


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
def test_adversarial_database_orders(tmvb, ctx, order):
    """one query against a database sorted by score: ascending, descending, all rows identical (the index decides everything)"""
    Md, K = 3 * T + 5, 64
    s = np.arange(Md, dtype=np.float64)
    xd = rows_of_score({"ascending": s, "descending": s[::-1].copy(), "identical": np.full(Md, 100.0)}[order], K)
    xq = np.ones((K, 1))
    S = xq.T @ xd
    targets = np.array([0, 1, 31, 32, T - 1, T, 200, 3 * T, Md - 1])
    excluded = np.array([2, 5, 64, T + 1, 201, 3 * T + 1, Md - 2])
    excl, tgt = csr_of([excluded]), csr_of([targets])
    for splits in (0, 1, 3):
        res = run(tmvb, ctx, xd, xq, excl, tgt, splits=splits)
        assert_exact(res, S, excl, tgt, tag=(order, splits))
    cand = np.setdiff1d(np.arange(Md), excluded)
    want = {"ascending": [np.count_nonzero(cand > t) for t in targets], "descending": [np.count_nonzero(cand < t) for t in targets],
            "identical": [np.count_nonzero(cand > t) for t in targets]}[order]           # equal scores: the candidates with a larger index come before
    assert res["rank"].tolist() == want


# ------------------------------------------------------------------------------------------------------------------ floating data
@pytest.mark.parametrize("K", FLOAT_KS)
def test_pair_and_scan_scores_agree_bit_for_bit(tmvb, ctx, K, monkeypatch):
    """every database row a target of every query: the ranks must be exactly the NumPy ranks of the fp32 scores the call returns -- which fails
    if the pair kernel and the scan kernel round one pair differently.  With 96 target slots in LDS the 5 x 200 targets of the one query tile
    take 11 passes, and a query's list is cut across passes."""
    xd, xq, excl, tgt = all_targets_case(K)
    Md, Mq = xd.shape[1], xq.shape[1]
    res = run(tmvb, ctx, xd, xq, excl, tgt)
    S32 = res["score"].reshape(Mq, Md)
    rank, n_cand = np_ranks(S32, excl, tgt)
    assert np.array_equal(res["rank"], rank), (K, np.argwhere(res["rank"] != rank)[:5].ravel())
    assert np.all(res["n_cand"] == Md) and sorted(res["rank"][:Md].tolist()) == list(range(Md))          # a query's ranks are a permutation
    monkeypatch.setenv("TMVB_RK_TARGET_SLOTS", "96")
    for splits in (0, 1):
        sliced = run(tmvb, ctx, xd, xq, excl, tgt, splits=splits)
        assert sliced["rank"].tobytes() == res["rank"].tobytes() and sliced["score"].tobytes() == res["score"].tobytes(), (K, splits)
    S64 = xq.T @ xd
    pos = S64 > 0
    WORST[K] = max(WORST[K], float((np.abs(S32 - S64)[pos] / S64[pos]).max()))


@pytest.mark.parametrize("K", FLOAT_KS)
def test_floating_ranks_against_fp64(tmvb, ctx, K):
    xd, xq, excl, tgt = bounds_case(K)
    S64 = xq.T @ xd
    eps = eps_of(K)
    res = run(tmvb, ctx, xd, xq, excl, tgt)
    q_of = np.repeat(np.arange(xq.shape[1]), np.diff(tgt[0]))
    s64 = S64[q_of, tgt[1]]
    dev = np.abs(res["score"].astype(np.float64) - s64)
    rel = float((dev[s64 > 0] / s64[s64 > 0]).max())
    print(f"recranks K = {K}: worst |score - s64| / s64 = {rel:.3e} (cap {eps:.3e})")
    WORST[K] = max(WORST[K], rel)
    assert np.all(dev <= eps * s64), (K, rel, eps)
    lo, hi = np_rank_bounds(S64, excl, tgt, eps)
    assert np.all((lo <= res["rank"]) & (res["rank"] <= hi)), (K, np.argwhere((res["rank"] < lo) | (res["rank"] > hi))[:5].ravel())
    assert np.array_equal(res["n_cand"], xd.shape[1] - np.diff(excl[0]))


# ------------------------------------------------------------------------------------------------------------------ purity
def test_splits_calls_and_query_slices_give_identical_bits(tmvb, ctx):
    for xd, xq, excl, tgt in (exact_case(2 * T + 2, 129, 50, "random", "random"), bounds_case(65, Md=300, Mq=140)):
        base = run(tmvb, ctx, xd, xq, excl, tgt, splits=1)
        assert base["splits"] == 1 and all(base["ms"][k] > 0 for k in ("prep", "pairs", "scan", "fix"))
        used = set()
        for splits in (1, 3, 0, 2):
            r = run(tmvb, ctx, xd, xq, excl, tgt, splits=splits)
            used.add(r["splits"])
            for f in ("rank", "score", "n_cand"):
                assert r[f].tobytes() == base[f].tobytes(), (splits, f)
        assert {1, 2, 3} <= used                                     # the database has three tiles: at most three splits
        Mq = xq.shape[1]
        for a, b in ((0, 1), (T - 1, T + 1), (5, 70), (Mq - 3, Mq)):  # queries [a, b) of a call equal the call on that slice
            cut = lambda c: (c[0][a:b + 1] - c[0][a], c[1][c[0][a]:c[0][b]])
            r = run(tmvb, ctx, xd, xq[:, a:b], cut(excl), cut(tgt))
            assert r["rank"].tobytes() == base["rank"][tgt[0][a]:tgt[0][b]].tobytes() and r["n_cand"].tobytes() == base["n_cand"][a:b].tobytes()
            assert r["score"].tobytes() == base["score"][tgt[0][a]:tgt[0][b]].tobytes()


# ------------------------------------------------------------------------------------------------------------------ with a trained model
def test_rec_eval_with_a_trained_model(tmvb):
    from test_recranks_host import RECS
    pf = tmvb.syn_citeu(M=40, V=60, U=15, seed=5)
    obs, held = tmvb.split_readers(pf, frac=0.3, seed=2)
    assert 0 < held.n < pf.nR
    g = tmvb.gpuCTPF(obs, 4)
    g.train(iter=5, tol=0.0, checkelbo=float("inf"), printelbo=False, recs=False)
    topn = (1, 5, 10, 100)
    X, Y = RECS.ctpf_factors(g)
    eps = eps_of(4)
    g.recommend(scores=False)
    for by, xd, xq, counts in (("user", X, Y, [len(r) for r in g.urecs]), ("doc", Y, X, [len(r) for r in g.drecs])):
        r = tmvb.rec_eval(g, held, topn=topn, by=by)
        assert r.by == by and r.n_targets == held.n == len(r.rank) and r.n_queries == np.count_nonzero(np.diff(r.tgt_ptr))
        assert np.array_equal(r.n_cand, counts), by                  # urec_count / drec_count of recommend() on the same handle
        excl = RECS._unique_rows(*(RECS.transpose_csr(obs.rdr_ptr, obs.readers, obs.U) if by == "user" else (obs.rdr_ptr, obs.readers)))
        lo, hi = np_rank_bounds(xq.T @ xd, excl, (r.tgt_ptr, r.tgt_idx), eps)
        assert np.all((lo <= r.rank) & (r.rank <= hi)), by
        has = np.diff(r.tgt_ptr) > 0
        for m in (r.recall, r.precision, r.ndcg, r.mrr, r.pct_rank):
            assert np.all((m[has] >= 0) & (m[has] <= 1)) and np.all(np.isnan(m[~has]))
        assert np.all(np.diff(r.recall[has], axis=1) >= 0)           # recall is non-decreasing in N
        assert np.all(r.recall[has, -1] == 1.0) and max(counts) <= topn[-1]                              # ... and 1 at N >= n_cand
        assert all(v > 0 for v in r.ms.values())
    g.close()
    q = tmvb.rec_quality(pf, 4, frac=0.3, seed=2, topn=topn, iter=5, tol=0.0, checkelbo=float("inf"))
    assert q.n_targets == held.n and np.array_equal(q.tgt_idx, tmvb.rec_eval.__globals__["_unique_rows"](held.user_ptr, held.docs)[1])
    assert 0.0 <= q.mean_pct_rank <= 1.0 and q.mean_recall[-1] == 1.0
