"""
The n best rows outside each query's exclusion list on the device (tmvb_score_topn and its Python mirror) against the NumPy checker of
tests/test_rectopn_host.py: bit for bit where the scores are exact, exactly the head of the returned fp32 scores of tmvb_score_ranks where
they are not, and the head of urecs / drecs of tmvb_ctpf_recommend on a handle.

Exact cases: the integer features of exact_case, K <= 64 (every dot product is an integer below 2^24: fp32 and fp64 agree), ties everywhere;
idx, the bits of score and count must equal NumPy's.  The database's LAST row is all 15 and comes before every other row of every query:
where it is not excluded it must be idx[q][0].  Shapes, T = 128 database rows per tile and 128 queries per workgroup: Md around one row, one
32-row MFMA block, one tile and two tiles with a partial third; Mq of one row, past one MFMA block, past one wave's 64 rows, past one
workgroup; K = 1, 2, 3, 50, 64; n = 1, 15, 63, 64 (one slot, the reference's 15, one lane short of a wave, a whole wave); exclusions none /
random (query 0 always lists the planted row) / all but three rows (count < n, padding; the planted row always listed) / all (count 0, a row
of -1 / -inf).  A greedy pairwise cover of that grid, built below, holds every value of every parameter and every pair of values.
"""
import numpy as np
import pytest

from test_recranks_gpu import pairwise_cover, rows_of_score
from test_recranks_host import FLOAT_KS, T, csr_of, eps_of, float_factors
from test_rectopn_host import EXCL, np_topn, topn_case

pytestmark = pytest.mark.gpu

MDS = [1, 2, 31, 32, 33, T, T + 1, 2 * T + 2]
MQS = [1, 33, 65, 129]
KS = [1, 2, 3, 50, 64]
NS = [1, 15, 63, 64]
CASES = pairwise_cover([MDS, MQS, KS, NS, EXCL])
assert all({c[i] for c in CASES} == set(ax) for i, ax in enumerate([MDS, MQS, KS, NS, EXCL])) and len(CASES) < 70


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()


def run(tmvb, ctx, xd, xq, excl, n, splits=0):
    rc, res = tmvb.rec_topn_raw(ctx, xd.shape[0], xd, xq, excl, n, splits)
    assert rc == 0, res
    return res


def same_bytes(a, b, tag=None):
    for f in ("idx", "score", "count"):
        assert a[f].tobytes() == b[f].tobytes(), (tag, f)


def assert_exact(res, S, excl, n, tag=None):
    idx, score, count = np_topn(S, excl, n)
    assert res["idx"].dtype == np.int32 and res["score"].dtype == np.float32 and res["count"].dtype == np.int32
    assert res["idx"].shape == idx.shape and res["score"].shape == score.shape
    assert np.array_equal(res["count"], count), (tag, res["count"][:8], count[:8])
    assert np.array_equal(res["idx"], idx), (tag, np.argwhere(res["idx"] != idx)[:5].tolist(), res["idx"][0, :8], idx[0, :8])
    assert res["score"].tobytes() == score.tobytes(), tag


# ------------------------------------------------------------------------------------------------------------------ exact lists
@pytest.mark.parametrize("Md,Mq,K,n,excl_mode", CASES, ids=lambda v: str(v))
def test_exact_topn(tmvb, ctx, Md, Mq, K, n, excl_mode):
    xd, xq, excl = topn_case(Md, Mq, K, excl_mode)
    S = xq.T @ xd
    assert S.max() < 2 ** 24 and (Md == 1 or np.all(S[:, -1] > S[:, :-1].max(axis=1)))
    res = run(tmvb, ctx, xd, xq, excl, n)
    assert res["kp"] == (K + 3) // 4 * 4
    assert_exact(res, S, excl, n, tag=(Md, Mq, K, n, excl_mode))
    lens = np.diff(excl[0])
    assert np.array_equal(res["count"], np.minimum(n, Md - lens))
    planted_out = np.array([lens[q] > 0 and excl[1][excl[0][q + 1] - 1] == Md - 1 for q in range(Mq)])
    assert np.all(res["idx"][~planted_out, 0] == Md - 1) and not np.any(res["idx"][planted_out] == Md - 1)
    if excl_mode == "all":
        assert np.all(res["count"] == 0) and np.all(res["idx"] == -1) and np.all(np.isneginf(res["score"]))
    if excl_mode == "all-but-three":
        assert np.all(res["count"] == min(n, 3, Md - 1)) and (n <= 3 or np.all(res["idx"][:, -1] == -1))
    if excl_mode == "random":
        assert planted_out[0]


@pytest.mark.parametrize("order", ["ascending", "descending", "identical"])
@pytest.mark.parametrize("n", [15, 64])
def test_adversarial_database_orders(tmvb, ctx, order, n):
    """one all-ones query against a database sorted by score: ascending (every row of every tile passes the threshold), descending, all rows
    identical -- the index decides everything, across tile and split boundaries"""
    Md, K = 3 * T + 5, 64
    s = np.arange(Md, dtype=np.float64)
    xd = rows_of_score({"ascending": s, "descending": s[::-1].copy(), "identical": np.full(Md, 100.0)}[order], K)
    xq = np.ones((K, 1))
    S = xq.T @ xd
    best = {"ascending": np.arange(Md - 5, Md), "descending": np.arange(5), "identical": np.arange(Md - 5, Md)}[order]
    excluded = np.union1d([2, 5, 64, T + 1, 201, 3 * T + 1, Md - 2], best)
    excl = csr_of([excluded])
    first = None
    for splits in (0, 1, 3):
        res = run(tmvb, ctx, xd, xq, excl, n, splits=splits)
        assert_exact(res, S, excl, n, tag=(order, n, splits))
        first = first or res
        same_bytes(res, first, (order, n, splits))
    cand = np.setdiff1d(np.arange(Md), excluded)
    want = {"ascending": cand[::-1][:n], "descending": cand[:n], "identical": cand[::-1][:n]}[order]     # equal scores: the highest indices first
    assert res["idx"][0].tolist() == want.tolist() and res["count"][0] == n


# ------------------------------------------------------------------------------------------------------------------ floating data
@pytest.mark.parametrize("K", FLOAT_KS)
def test_floating_lists_are_the_head_of_the_returned_score_bits(tmvb, ctx, K):
    """tmvb_score_ranks with every row outside a query's exclusion list as a target returns the fp32 score and the rank of every candidate: the
    list must be exactly the n best of those bits under the order -- nothing left out --, the rank reported there for idx[q][j] must be j, and
    every score within the derived bound of the fp64 dot product"""
    Md, Mq, n = 2 * T + 2, 65, 15
    xd, xq = float_factors(K, Md, Mq)
    rng = np.random.Generator(np.random.PCG64(11 * K))
    ex = [np.flatnonzero(rng.random(Md) < 0.3) for _ in range(Mq)]
    excl, tgt = csr_of(ex), csr_of([np.setdiff1d(np.arange(Md), e) for e in ex])
    rc, ranks = tmvb.rec_ranks_raw(ctx, K, xd, xq, excl, tgt)
    assert rc == 0, ranks
    S32 = np.full((Mq, Md), -np.inf, dtype=np.float32)
    R = np.full((Mq, Md), -1, dtype=np.int64)
    q_of = np.repeat(np.arange(Mq), np.diff(tgt[0]))
    S32[q_of, tgt[1]] = ranks["score"]
    R[q_of, tgt[1]] = ranks["rank"]
    res = run(tmvb, ctx, xd, xq, excl, n)
    idx, score, count = np_topn(S32, excl, n)
    assert np.all(count == n) and np.array_equal(res["count"], count)
    assert np.array_equal(res["idx"], idx), (K, np.argwhere(res["idx"] != idx)[:5].tolist())
    assert res["score"].tobytes() == score.tobytes(), K
    assert np.array_equal(R[np.arange(Mq)[:, None], res["idx"]], np.tile(np.arange(n), (Mq, 1))), K
    s64 = (xq.T @ xd)[np.arange(Mq)[:, None], res["idx"]]
    dev = np.abs(res["score"].astype(np.float64) - s64)
    rel = float((dev[s64 > 0] / s64[s64 > 0]).max())
    print(f"rectopn K = {K}: worst |score - s64| / s64 = {rel:.3e} (cap {eps_of(K):.3e})")
    assert np.all(dev <= eps_of(K) * s64), (K, rel, eps_of(K))


# ------------------------------------------------------------------------------------------------------------------ purity
def test_splits_calls_and_query_slices_give_identical_bits(tmvb, ctx):
    Md, Mq, n = 4 * T + 7, 129, 15
    fx, fq = float_factors(65, Md, Mq)
    rng = np.random.Generator(np.random.PCG64(21))
    fex = csr_of([np.flatnonzero(rng.random(Md) < 0.3) for _ in range(Mq)])
    for xd, xq, excl in (topn_case(4 * T + 7, 129, 50, "random"), (fx, fq, fex)):
        base = run(tmvb, ctx, xd, xq, excl, n, splits=1)
        assert base["splits"] == 1 and base["ms_prep"] > 0 and base["ms_scan"] > 0 and base["ms_merge"] == 0
        used = set()
        for splits in (0, 1, 2, 5, 1):                               # ... and the same call twice
            r = run(tmvb, ctx, xd, xq, excl, n, splits=splits)
            used.add(r["splits"])
            same_bytes(r, base, splits)
            assert r["splits"] == 1 or r["ms_merge"] > 0
        assert {1, 2, 5} <= used                                     # the database has five tiles: at most five splits
        for a, b in ((0, 40), (40, 129)):                            # queries [a, b) of a call equal the call on that slice
            r = run(tmvb, ctx, xd, xq[:, a:b], (excl[0][a:b + 1] - excl[0][a], excl[1][excl[0][a]:excl[0][b]]), n)
            same_bytes(r, {f: base[f][a:b] for f in ("idx", "score", "count")}, (a, b))


# ------------------------------------------------------------------------------------------------------------------ on a handle
def test_recommend_topn_is_the_head_of_recommend(tmvb):
    """A gpuCTPF whose state is small integers (rates 1): every score is an exact integer in any summation order and any precision, so the
    lists must equal the first 15 entries of urecs / drecs of recommend() on the same handle, tie order included."""
    M, U, K, V = 150, 70, 6, 40
    rng = np.random.Generator(np.random.PCG64(9))
    readers = [np.sort(rng.choice(np.arange(1, U), size=rng.integers(0, 13), replace=False)) for _ in range(M)]   # user 0 has no library
    readers[7] = np.arange(1, U)                                     # the document everyone else reads: user 0 is all it can be recommended to
    readers[0] = readers[0][:0]                                      # ... and a document nobody reads
    rdr_ptr = np.concatenate([[0], np.cumsum([len(r) for r in readers])]).astype(np.int64)
    rd = np.concatenate(readers).astype(np.int32)
    doc_ptr = np.arange(0, 3 * M + 1, 3, dtype=np.int64)
    terms = np.concatenate([np.sort(rng.choice(V, size=3, replace=False)) for _ in range(M)]).astype(np.int32)
    pc = tmvb.PackedCorpus(doc_ptr, terms, np.ones(3 * M, dtype=np.int32), V, rdr_ptr, rd, np.ones(len(rd), dtype=np.int32), U)
    g = tmvb.gpuCTPF(pc, K)
    try:
        ints = lambda *shape: np.asfortranarray(rng.integers(1, 7, size=shape).astype(np.float64))
        g.he, g.gimel, g.zayin = ints(K, U), ints(K, M), ints(K, M)
        g.bet = np.ones(K); g.vav = np.ones(K); g.dalet = np.ones(K); g.het = np.ones(K)
        g.update_buffer()
        g.recommend()
        S = (g.gimel + g.zayin).T @ g.he                              # M x U, integers
        assert np.array_equal(g.scores, S) and S.max() < 2 ** 24
        assert np.bincount(rd, minlength=U)[0] == 0 and len(g.urecs[0]) == M and g.drecs[7].tolist() == [1] and len(g.drecs[0]) == U
        for by, recs, Sq in (("user", g.urecs, S.T), ("doc", g.drecs, S)):
            r = g.recommend_topn(topn=15, by=by)
            assert r.by == by and r.idx.shape == (len(recs), 15) and np.array_equal(r.ids, np.arange(1, len(recs) + 1))
            for q, full in enumerate(recs):
                head = np.asarray(full[:15]) - 1
                assert r.count[q] == len(head) and np.array_equal(r.idx[q, :len(head)], head), (by, q, r.idx[q], head)
                assert np.all(r.idx[q, len(head):] == -1) and np.all(np.isneginf(r.score[q, len(head):]))
                assert np.array_equal(r.score[q, :len(head)], Sq[q, head].astype(np.float32))
        assert r.count[7] == 1 and r.idx[7, 0] == 0                   # by="doc" ran last: document 7 is left with user 0
        sel = g.recommend_topn(topn=15, by="user", ids=[3, 1, 70])
        whole = g.recommend_topn(topn=15, by="user")
        assert sel.ids.tolist() == [3, 1, 70] and sel.idx.shape == (3, 15)
        for f in ("idx", "score", "count"):
            assert getattr(sel, f).tobytes() == getattr(whole, f)[[2, 0, 69]].tobytes(), f
        assert np.array_equal(sel.idx[1, :15], np.asarray(g.urecs[0][:15]) - 1)
        free = tmvb.recommend_topn(g, topn=64, by="doc", ids=5)       # the function form, on the handle's context
        assert free.idx.shape == (1, 64) and np.array_equal(free.idx[0, :free.count[0]], (np.asarray(g.drecs[4]) - 1)[:64])
    finally:
        g.close()
