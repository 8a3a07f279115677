"""
Held-out recommendation metrics (tmvb_readers_split, tmvb_score_ranks, tmvb_rank_metrics; include/tmvb.h), the part that needs no GPU -- and the
NumPy checkers and the inputs of tests/test_recranks_gpu.py: the reference has no such functions, so the yardsticks are restatements written here.

  * `np_philox` / `np_split`: Philox4x32-10 and the draw rule in NumPy; the library's split must equal it bit for bit;
  * `np_ranks`: rank = #{e not excluded, e != t : s_e > s_t or (s_e == s_t and e > t)} from a score matrix; `np_rank_bounds`: the interval
    [lo, hi] a rank must lie in when every score is known to a relative eps only; `np_metrics`: the metrics on the ranks;
  * every row of the three error tables comes back with its status and message from a NULL context, valid arguments without a device give
    TMVB_ENODEVICE;
  * the floating cases of the GPU file are built here and the condition that makes their interval check meaningful (at least 95 % of the pairs
    have lo == hi) is asserted on the fp64 reference alone;
  * the header, the structures, SOURCES, the Julia shim, the mutant's flag, the call scope and the kernel-resource table.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tmvb_amd  # noqa: E402
from test_call_scope_host import test_units_own_no_device_scratch as _units_own_no_device_scratch  # noqa: E402

# the mirror module of the feature: a tree without it fails here, at import, and with it every test of this module and of the two GPU modules
RECS = sys.modules[tmvb_amd.pkg.__name__ + ".recs_eval"]
T = RECS.TILE_DB
ENTRY, DOCUMENT = RECS.ENTRY, RECS.DOCUMENT
EINVAL, ESHAPE, ENODEVICE = 1, 2, 7
FLOAT_KS = [3, 50, 65, 130, 512]


def eps_of(K):
    """relative bound on |score - s64| for nonnegative factors: one rounding per factor (two per product) and one per fmaf, each at most
    2^-24 relative, every term positive"""
    return (K + 3) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ NumPy checkers
def np_philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of counters: -> uint32[..., 4]"""
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(mask) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & mask, int(k1) & mask
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(mask), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(mask)]
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def np_held_flags(rdr_ptr, frac, seed, doc_offset, mode):
    """bool[nR]: which entries the draw rule holds out"""
    rdr_ptr = np.asarray(rdr_ptr, dtype=np.int64)
    M, n = len(rdr_ptr) - 1, int(rdr_ptr[-1])
    thr = int(np.floor(frac * 4294967296.0))
    seed = int(seed) % 2 ** 64
    doc = np.repeat(np.arange(M, dtype=np.int64), np.diff(rdr_ptr)) + doc_offset
    j = np.arange(n, dtype=np.int64) - np.repeat(rdr_ptr[:-1], np.diff(rdr_ptr))
    if mode == DOCUMENT:
        w = np_philox(doc & 0xFFFFFFFF, doc >> 32, 7, 0, seed, seed >> 32)[:, 0]
    else:
        w = np_philox(doc & 0xFFFFFFFF, doc >> 32, 6, j >> 2, seed, seed >> 32)[np.arange(n), j & 3]
    return w.astype(np.int64) < thr


def np_ranks(S, excl, tgt):
    """ranks (int32, the order of tgt's ids) and n_cand from the score matrix S[Mq, Md] under the order of reverse(sortperm(.))"""
    Mq, Md = S.shape
    (eptr, eidx), (tptr, tidx) = excl, tgt
    rank = np.zeros(int(tptr[-1]), dtype=np.int32)
    n_cand = np.zeros(Mq, dtype=np.int32)
    ids = np.arange(Md)
    for q in range(Mq):
        cand = np.ones(Md, dtype=bool)
        cand[eidx[eptr[q]:eptr[q + 1]]] = False
        n_cand[q] = cand.sum()
        for g in range(tptr[q], tptr[q + 1]):
            t = tidx[g]
            before = (S[q] > S[q, t]) | ((S[q] == S[q, t]) & (ids > t))
            rank[g] = np.count_nonzero(before & cand)
    return rank, n_cand


def np_rank_bounds(S64, excl, tgt, eps):
    """(lo, hi) per target: lo = #{cand: s_e (1 - eps) > s_t (1 + eps)}, hi = #{cand: s_e (1 + eps) >= s_t (1 - eps)} - 1 (the target itself)"""
    Mq, Md = S64.shape
    (eptr, eidx), (tptr, tidx) = excl, tgt
    lo = np.zeros(int(tptr[-1]), dtype=np.int64); hi = lo.copy()
    for q in range(Mq):
        cand = np.ones(Md, dtype=bool)
        cand[eidx[eptr[q]:eptr[q + 1]]] = False
        for g in range(tptr[q], tptr[q + 1]):
            st = S64[q, tidx[g]]
            lo[g] = np.count_nonzero(cand & (S64[q] * (1 - eps) > st * (1 + eps)))
            hi[g] = np.count_nonzero(cand & (S64[q] * (1 + eps) >= st * (1 - eps))) - 1
    return lo, hi


def np_metrics(tptr, rank, n_cand, Ns):
    Mq = len(tptr) - 1
    out = {k: np.full((Mq, len(Ns)), np.nan) for k in ("recall", "precision", "ndcg")}
    out["mrr"] = np.full(Mq, np.nan); out["pct_rank"] = np.full(Mq, np.nan)
    for q in range(Mq):
        r = np.asarray(rank[tptr[q]:tptr[q + 1]], dtype=np.float64)
        if len(r) == 0:
            continue
        for a, N in enumerate(Ns):
            hit = r < N
            out["recall"][q, a] = hit.sum() / len(r)
            out["precision"][q, a] = hit.sum() / N
            out["ndcg"][q, a] = (1.0 / np.log2(r[hit] + 2.0)).sum() / (1.0 / np.log2(np.arange(min(len(r), N)) + 2.0)).sum()
        out["mrr"][q] = 1.0 / (r.min() + 1.0)
        out["pct_rank"][q] = r.mean() / max(int(n_cand[q]) - 1, 1)
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs of the GPU file
def integer_rows(K, M, seed, levels=(0, 1, 2, 14)):
    """K x M fp64 from few integer levels, first feature >= 1: ties everywhere; the caller plants the all-15 row"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.choice(np.asarray(levels, dtype=np.float64), size=(K, M))
    x[0] = np.maximum(x[0], 1.0)
    return x


def csr_of(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if len(rows) and ptr[-1] else np.zeros(0, dtype=np.int32)
    return ptr, idx.astype(np.int32)


def lists_of(Mq, Md, excl_mode, tgt_mode, seed):
    """(excl, tgt) over the rows [0, Md - 1): the last database row is neither a target nor excluded"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = np.arange(Md - 1)
    tg, ex = [], []
    for q in range(Mq):
        if len(pool) == 0 or (tgt_mode == "some_none" and q % 2 == 1):
            t = pool[:0]
        elif tgt_mode == "one_each":
            t = rng.choice(pool, size=1)
        elif tgt_mode == "some_none":
            t = rng.choice(pool, size=min(len(pool), 3), replace=False)
        else:
            t = pool[rng.random(len(pool)) < 0.3]
        t = np.sort(t)
        rest = np.setdiff1d(pool, t)
        e = {"none": rest[:0], "random": rest[rng.random(len(rest)) < 0.4], "all": rest}[excl_mode]
        tg.append(t); ex.append(e)
    return csr_of(ex), csr_of(tg)


def exact_case(Md, Mq, K, excl_mode, tgt_mode):
    xd = integer_rows(K, Md, seed=1000 * Md + K)
    xd[:, -1] = 15.0
    xq = integer_rows(K, Mq, seed=77 * Mq + K)
    excl, tgt = lists_of(Mq, Md, excl_mode, tgt_mode, seed=13 * Md + 7 * Mq + K)
    return xd, xq, excl, tgt


def gamma_factors(K, M, seed, active=None, nonzero=None):
    """K x M Gamma(0.3) factors; with active / nonzero: each row keeps `nonzero` entries among the first `active` dimensions (few non-zeros
    per row: the scores spread widely, so few pairs lie within the rounding error of one another)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_gamma(0.3, size=(K, M)) + 1e-12
    if active is not None:
        keep = np.zeros((K, M), dtype=bool)
        for m in range(M):
            keep[rng.choice(active, size=nonzero, replace=False), m] = True
        x = np.where(keep, x, 0.0)
    return x


def float_factors(K, Md, Mq):
    kw = dict(active=48, nonzero=12) if K == 512 else {}
    return gamma_factors(K, Md, seed=31 * K + 1, **kw), gamma_factors(K, Mq, seed=31 * K + 2, **kw)


def bounds_case(K, Md=300, Mq=20):
    """the inputs of the floating ranks against fp64: 8 targets per query, random exclusions"""
    xd, xq = float_factors(K, Md, Mq)
    rng = np.random.Generator(np.random.PCG64(5 * K))
    tg, ex = [], []
    for q in range(Mq):
        t = np.sort(rng.choice(Md, size=8, replace=False))
        rest = np.setdiff1d(np.arange(Md), t)
        tg.append(t); ex.append(rest[rng.random(len(rest)) < 0.2])
    return xd, xq, csr_of(ex), csr_of(tg)


def all_targets_case(K, Md=200, Mq=5):
    """every database row a target of every query, no exclusions: the call returns the whole fp32 score matrix"""
    xd, xq = float_factors(K, Md, Mq)
    return xd, xq, csr_of([[] for _ in range(Mq)]), csr_of([np.arange(Md) for _ in range(Mq)])


@pytest.mark.parametrize("K", FLOAT_KS)
def test_the_floating_cases_leave_few_ambiguous_pairs(K):
    xd, xq, excl, tgt = bounds_case(K)
    S64 = xq.T @ xd
    lo, hi = np_rank_bounds(S64, excl, tgt, eps_of(K))
    assert np.all(lo <= hi)
    sharp = np.count_nonzero(lo == hi) / len(lo)
    print(f"K = {K}: {100 * (1 - sharp):.2f} % of the pairs are ambiguous at eps = {eps_of(K):.3e}")
    assert sharp >= 0.95, (K, sharp)
    r, _ = np_ranks(S64, excl, tgt)                                   # the fp64 ranks lie inside their own interval
    assert np.all((lo <= r) & (r <= hi))


def test_the_restatement_against_brute_force():
    rng = np.random.Generator(np.random.PCG64(3))
    S = rng.integers(0, 3, size=(4, 9)).astype(np.float64)           # three levels: ties in every row
    excl, tgt = csr_of([[0, 4], [], [8], [1, 2, 3]]), csr_of([[1, 7], [0, 8], [], [0]])
    rank, n_cand = np_ranks(S, excl, tgt)
    assert n_cand.tolist() == [7, 9, 8, 6]
    for q in range(4):
        ex = set(excl[1][excl[0][q]:excl[0][q + 1]].tolist())
        order = sorted((e for e in range(9) if e not in ex), key=lambda e: (S[q, e], e), reverse=True)   # reverse(sortperm(.))
        for g in range(tgt[0][q], tgt[0][q + 1]):
            assert rank[g] == order.index(tgt[1][g])


def test_integer_scores_are_exact_in_fp32():
    xd, xq, _, _ = exact_case(258, 65, 64, "none", "random")
    S = xq.T @ xd
    assert S.max() <= 64 * 15 * 15 < 2 ** 24 and np.array_equal(S, S.astype(np.float32).astype(np.float64)) and np.array_equal(S, np.rint(S))
    assert np.all(S[:, -1] > S[:, :-1].max(axis=1))                  # the last row comes before every other row of every query


# ------------------------------------------------------------------------------------------------------------------ the split
def _corpus(tmvb, M=60, U=25, seed=3):
    return tmvb.syn_citeu(M=M, V=50, U=U, seed=seed)


@pytest.mark.parametrize("mode", [ENTRY, DOCUMENT], ids=["entry", "document"])
@pytest.mark.parametrize("frac,seed,off", [(0.3, 0, 0), (0.5, 2 ** 40 + 17, 5), (0.07, -3, 2 ** 33)])
def test_split_is_bit_exact_against_the_numpy_philox(tmvb, mode, frac, seed, off):
    pc = _corpus(tmvb)
    rc, res = tmvb.split_readers_raw(pc.M, pc.U, pc.rdr_ptr, pc.readers, pc.ratings, frac, seed, off, mode)
    assert rc == 0, res
    held = np_held_flags(pc.rdr_ptr, frac, seed, off, mode)
    doc = np.repeat(np.arange(pc.M), np.diff(pc.rdr_ptr))
    for side, m in (("obs", ~held), ("held", held)):
        assert np.array_equal(res[side + "_readers"], pc.readers[m]) and np.array_equal(res[side + "_ratings"], pc.ratings[m])       # order kept
        assert np.array_equal(np.diff(res[side + "_ptr"]), np.bincount(doc[m], minlength=pc.M)) and res[side + "_ptr"][0] == 0
    assert res["n_obs"] + res["n_held"] == pc.nR and res["n_held"] == held.sum() and 0 < res["n_held"] < pc.nR


def test_split_partition_fractions_shards_modes_and_seeds(tmvb):
    pc = _corpus(tmvb, M=80)
    pc.ratings = (1 + np.arange(pc.nR) % 5).astype(np.int32)
    go = lambda **kw: tmvb.split_readers_raw(pc.M, pc.U, pc.rdr_ptr, pc.readers, pc.ratings, **kw)[1]
    for frac, n_held in ((0.0, 0), (1.0, pc.nR)):
        for mode in (ENTRY, DOCUMENT):
            r = go(frac=frac, seed=1, mode=mode)
            assert r["n_held"] == n_held and r["n_obs"] == pc.nR - n_held
    whole = go(frac=0.4, seed=9, mode=ENTRY)
    # obs + held reproduces the input: merged back by the flags the restatement gives
    held = np_held_flags(pc.rdr_ptr, 0.4, 9, 0, ENTRY)
    back = np.empty(pc.nR, dtype=np.int32); back[held] = whole["held_readers"]; back[~held] = whole["obs_readers"]
    assert np.array_equal(back, pc.readers)
    for mode in (ENTRY, DOCUMENT):                                   # documents [d0, d0 + m) of a large call equal the call (m, doc_offset = d0)
        w = go(frac=0.4, seed=9, mode=mode)
        for d0, d1 in ((0, 13), (13, 50), (50, 80)):
            sh = pc.shard(d0, d1)
            rc, part = tmvb.split_readers_raw(sh.M, sh.U, sh.rdr_ptr, sh.readers, sh.ratings, 0.4, 9, d0, mode)
            assert rc == 0
            for side in ("obs", "held"):
                a, b = w[side + "_ptr"][d0], w[side + "_ptr"][d1]
                assert np.array_equal(part[side + "_readers"], w[side + "_readers"][a:b]) and np.array_equal(part[side + "_ratings"], w[side + "_ratings"][a:b])
                assert np.array_equal(part[side + "_ptr"], w[side + "_ptr"][d0:d1 + 1] - a)
    doc = go(frac=0.4, seed=9, mode=DOCUMENT)                        # DOCUMENT mode never splits a document
    no, nh = np.diff(doc["obs_ptr"]), np.diff(doc["held_ptr"])
    assert np.all((no == 0) | (nh == 0)) and np.array_equal(no + nh, np.diff(pc.rdr_ptr)) and 0 < doc["n_held"] < pc.nR
    assert not np.array_equal(go(frac=0.4, seed=10, mode=ENTRY)["held_ptr"], whole["held_ptr"])          # two seeds differ
    assert np.array_equal(go(frac=0.4, seed=9, mode=ENTRY)["held_readers"], whole["held_readers"])       # one seed does not


def test_split_readers_mirror(tmvb):
    pc = _corpus(tmvb)
    obs, held = tmvb.split_readers(pc, 0.3, seed=4)
    assert obs.M == pc.M and obs.U == pc.U and np.array_equal(obs.terms, pc.terms) and np.array_equal(obs.doc_ptr, pc.doc_ptr)
    assert obs.nR + held.n == pc.nR and held.M == pc.M and held.U == pc.U
    for u in range(pc.U):                                            # the by-user transpose: the documents of u, ascending
        docs = held.docs[held.user_ptr[u]:held.user_ptr[u + 1]]
        want = [d for d in range(pc.M) if u in held.readers[held.rdr_ptr[d]:held.rdr_ptr[d + 1]]]
        assert docs.tolist() == want
    with pytest.raises(ValueError, match="mode"):
        tmvb.split_readers(pc, mode="rows")
    with pytest.raises(ValueError, match="frac"):
        tmvb.split_readers(pc, frac=1.5)


def split_error_cases():
    ptr, rd, ra = np.array([0, 2, 3]), np.array([0, 1, 2]), np.array([1, 1, 2])
    b = dict(M=2, U=3, rdr_ptr=ptr, readers=rd, ratings=ra, frac=0.5, seed=0, doc_offset=0, mode=ENTRY)
    return [
        ("frac above 1", dict(b, frac=1.0001), EINVAL, "frac must lie in [0, 1]"),
        ("frac negative", dict(b, frac=-0.1), EINVAL, "frac must lie in [0, 1]"),
        ("frac nan", dict(b, frac=float("nan")), EINVAL, "frac must lie in [0, 1]"),
        ("doc_offset negative", dict(b, doc_offset=-1), EINVAL, "doc_offset must be nonnegative"),
        ("unknown mode", dict(b, mode=2), EINVAL, "unknown mode 2"),
        ("M zero", dict(b, M=0), EINVAL, "M must be a positive integer"),
        ("U zero", dict(b, U=0), EINVAL, "U must be a positive integer"),
        ("pointer not from 0", dict(b, rdr_ptr=np.array([1, 2, 3])), ESHAPE, "rdr_ptr must start at 0"),
        ("pointer decreases", dict(b, rdr_ptr=np.array([0, 3, 2])), ESHAPE, "rdr_ptr decreases at document 1"),
        ("reader out of range", dict(b, readers=np.array([0, 3, 2])), ESHAPE, "holds reader 3 outside [0, 3)"),
        ("reader negative", dict(b, readers=np.array([0, 1, -1])), ESHAPE, "holds reader -1 outside [0, 3)"),
        ("rating zero", dict(b, ratings=np.array([1, 0, 1])), ESHAPE, "holds a rating below 1"),
    ]


@pytest.mark.parametrize("case", split_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_split_argument_errors(tmvb, case):
    _, kw, status, msg = case
    rc, res = tmvb.split_readers_raw(**kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_split_null_arguments_through_the_abi(tmvb):
    L = tmvb.lib()
    ptr = np.array([0, 1], dtype=np.int64); rd = np.zeros(1, dtype=np.int32); ra = np.ones(1, dtype=np.int32)
    out = RECS.ReaderSplit()
    a = [ptr.ctypes.data_as(C.POINTER(C.c_int64)), rd.ctypes.data_as(C.POINTER(C.c_int32)), ra.ctypes.data_as(C.POINTER(C.c_int32))]
    for hole in range(4):
        p = [None if q == hole else v for q, v in enumerate(a + [C.byref(out)])]
        rc = L.tmvb_readers_split(C.c_int64(1), C.c_int64(1), p[0], p[1], p[2], C.c_double(0.5), C.c_int64(0), C.c_int64(0), C.c_int32(0), p[3])
        assert rc == EINVAL and ("NULL" in L.tmvb_last_error().decode()), hole


# ------------------------------------------------------------------------------------------------------------------ the metrics
def test_rank_metrics_against_the_numpy_restatement(tmvb):
    rng = np.random.Generator(np.random.PCG64(8))
    sizes = rng.integers(0, 7, size=40)
    sizes[[3, 17]] = 0
    tptr = np.concatenate([[0], np.cumsum(sizes)])
    n_cand = rng.integers(8, 300, size=40)
    rank = np.concatenate([rng.choice(n_cand[q], size=sizes[q], replace=False) for q in range(40)]).astype(np.int32)
    Ns = [1, 5, 10, 100]
    got = tmvb.rank_metrics(tptr, rank, n_cand, Ns)
    want = np_metrics(tptr, rank, n_cand, Ns)
    has = sizes > 0
    for k in ("recall", "precision", "ndcg", "mrr", "pct_rank"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-14, atol=0, equal_nan=True)
        assert np.array_equal(np.isnan(got[k]).reshape(40, -1).all(axis=1), ~has), k
        np.testing.assert_allclose(np.atleast_1d(got["mean_" + k]), np.atleast_1d(want[k][has].mean(axis=0)), rtol=1e-13)
    assert got["n_queries"] == has.sum() and got["n_targets"] == sizes.sum()
    assert np.all(np.diff(got["recall"][has], axis=1) >= 0)


def test_rank_metrics_known_answers(tmvb):
    m = tmvb.rank_metrics([0, 1], [0], [50], [1, 10])                # a single target at rank 0
    assert m["recall"].tolist() == [[1.0, 1.0]] and m["precision"].tolist() == [[1.0, 0.1]] and m["ndcg"].tolist() == [[1.0, 1.0]]
    assert m["mrr"].tolist() == [1.0] and m["pct_rank"].tolist() == [0.0]
    m = tmvb.rank_metrics([0, 3], [20, 30, 48], [50], [5, 20])       # all targets beyond every N
    assert not m["recall"].any() and not m["precision"].any() and not m["ndcg"].any()
    assert m["mrr"][0] == 1.0 / 21.0 and m["pct_rank"][0] == (98.0 / 3.0) / 49.0
    m = tmvb.rank_metrics([0, 4], [0, 1, 2, 7], [9], [2])            # T > N: the ideal list is cut at N
    assert m["recall"][0, 0] == 0.5 and m["precision"][0, 0] == 1.0 and m["ndcg"][0, 0] == 1.0
    m = tmvb.rank_metrics([0, 2], [0, 3], [9], [2])
    assert m["ndcg"][0, 0] == 1.0 / (1.0 + 1.0 / np.log2(3.0))
    m = tmvb.rank_metrics([0, 1, 1], [0], [1, 1], [1])               # n_cand = 1: the percentile's denominator is max(n_cand - 1, 1)
    assert m["pct_rank"][0] == 0.0 and np.isnan(m["pct_rank"][1]) and m["n_queries"] == 1 and m["mean_mrr"] == 1.0
    m = tmvb.rank_metrics([0, 0], [], [4], [3])                      # nobody has targets
    assert m["n_queries"] == 0 and m["n_targets"] == 0 and np.isnan(m["mean_mrr"]) and np.isnan(m["mean_recall"]).all()


@pytest.mark.parametrize("kw,status,msg", [
    (dict(tgt_ptr=[0, 1], rank=[5], n_cand=[5], Ns=[1]), ESHAPE, "rank 5 outside [0, 5)"),
    (dict(tgt_ptr=[0, 1], rank=[-1], n_cand=[5], Ns=[1]), ESHAPE, "rank -1 outside [0, 5)"),
    (dict(tgt_ptr=[1, 1], rank=[0], n_cand=[5], Ns=[1]), ESHAPE, "tgt_ptr must start at 0"),
    (dict(tgt_ptr=[0, 2, 1], rank=[0, 1], n_cand=[5, 5], Ns=[1]), ESHAPE, "tgt_ptr decreases at query 1"),
    (dict(tgt_ptr=[0, 1], rank=[0], n_cand=[5], Ns=[0]), EINVAL, "N = 0 below 1"),
    (dict(tgt_ptr=[0, 1], rank=[0], n_cand=[5], Ns=[3, -2]), EINVAL, "N = -2 below 1"),
    (dict(tgt_ptr=[0, 1], rank=[0], n_cand=[5], Ns=[]), EINVAL, "at least one cut-off"),
    (dict(tgt_ptr=[0], rank=[], n_cand=[], Ns=[1]), EINVAL, "Mq must be a positive integer"),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_rank_metrics_errors(tmvb, kw, status, msg):
    rc, res = tmvb.rank_metrics_raw(**kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


# ------------------------------------------------------------------------------------------------------------------ tmvb_score_ranks: errors
def _base():
    return dict(K=3, xd=np.arange(15, dtype=np.float64).reshape(3, 5), xq=np.ones((3, 2)), excl=([0, 1, 1], [2]), tgt=([0, 1, 2], [1, 3]), splits=0)


def rank_error_cases():
    b = _base()
    return [
        ("K above 1024", dict(b, K=1025, xd=np.ones((1025, 5)), xq=np.ones((1025, 2))), EINVAL, "K = 1025"),
        ("splits negative", dict(b, splits=-1), EINVAL, "splits = -1"),
        ("splits above Md", dict(b, splits=6), EINVAL, "splits = 6"),
        ("nan in the database", dict(b, xd=np.where(np.arange(15).reshape(3, 5) == 7, np.nan, 1.0)), ESHAPE, "non-finite entry (database row 2)"),
        ("inf in the queries", dict(b, xq=np.array([[1.0, 1.0], [1.0, np.inf], [0.0, 0.0]])), ESHAPE, "non-finite entry (query row 1)"),
        ("excl pointer not from 0", dict(b, excl=([1, 1, 1], [2])), ESHAPE, "excl_ptr must start at 0"),
        ("tgt pointer decreases", dict(b, tgt=([0, 2, 1], [1, 3])), ESHAPE, "tgt_ptr decreases at query 1"),
        ("target out of range", dict(b, tgt=([0, 1, 2], [1, 5])), ESHAPE, "query 1 holds target id 5 outside [0, 5)"),
        ("exclusion negative", dict(b, excl=([0, 1, 1], [-1])), ESHAPE, "query 0 holds excluded id -1 outside [0, 5)"),
        ("targets not ascending", dict(b, tgt=([0, 2, 2], [3, 1])), ESHAPE, "the target ids of query 0 are not strictly ascending"),
        ("exclusions repeated", dict(b, excl=([0, 2, 2], [2, 2])), ESHAPE, "the excluded ids of query 0 are not strictly ascending"),
        ("shared id", dict(b, excl=([0, 1, 1], [1])), ESHAPE, "id 1 of query 0 is both excluded and a target"),
    ]


def call(tmvb, ctx, kw):
    return tmvb.rec_ranks_raw(ctx, kw["K"], kw["xd"], kw["xq"], kw["excl"], kw["tgt"], kw["splits"])


@pytest.mark.parametrize("case", rank_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_score_ranks_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call(tmvb, None, kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_score_ranks_shape_errors_through_the_abi(tmvb):
    """K = 0, Md = 0, Mq = 0 and Md = 2^31 cannot be said with an array: the C call itself (no entry is read before these are judged)"""
    L = tmvb.lib()
    PD, P32, P64, PF = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    x = np.ones(8); ptr = np.zeros(3, dtype=np.int64); idx = np.zeros(2, dtype=np.int32); out = np.zeros(4, dtype=np.int32)
    a = [x.ctypes.data_as(PD), x.ctypes.data_as(PD), ptr.ctypes.data_as(P64), idx.ctypes.data_as(P32), ptr.ctypes.data_as(P64), idx.ctypes.data_as(P32),
         out.ctypes.data_as(P32), out.ctypes.data_as(P32)]

    def go(K, Md, Mq, p=a):
        rc = L.tmvb_score_ranks(None, C.c_int32(K), C.c_int64(Md), p[0], C.c_int64(Mq), p[1], p[2], p[3], p[4], p[5], C.c_int32(0), p[6], p[7], None, None)
        return rc, L.tmvb_last_error().decode()

    for K, Md, Mq, msg in ((0, 2, 2, "K = 0"), (-1, 2, 2, "K = -1"), (2, 0, 1, "Md and Mq must be positive"), (2, 2, 0, "Md and Mq must be positive"),
                           (2, -4, 1, "Md and Mq must be positive"), (2, 2 ** 31, 1, "2^31 or more")):
        rc, err = go(K, Md, Mq)
        assert rc == EINVAL and msg in err, (K, Md, Mq, rc, err)
    for hole in (0, 1, 2, 4, 6, 7):                                  # xd, xq, excl_ptr, tgt_ptr, rank, n_cand (the id arrays may be NULL when empty)
        rc, err = go(2, 2, 2, [None if q == hole else v for q, v in enumerate(a)])
        assert rc == EINVAL and "NULL argument" in err, (hole, rc, err)
    ptr1 = np.array([0, 1, 1], dtype=np.int64)                       # ... and not when the pointers say there are ids
    rc, err = go(2, 2, 2, a[:4] + [ptr1.ctypes.data_as(P64), None] + a[6:])
    assert rc == EINVAL and "NULL argument" in err
    rc, err = go(2, 2, 2, a[:2] + [ptr1.ctypes.data_as(P64), None] + a[4:])
    assert rc == EINVAL and "NULL argument" in err


def test_valid_arguments_without_a_device_are_enodevice(tmvb):
    """No silent CPU path: the arguments pass, then a NULL context on a machine without a GPU is TMVB_ENODEVICE -- the last row of the table."""
    if tmvb.lib().tmvb_device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_recranks_gpu.py covers the live path")
    xd, xq, excl, tgt = exact_case(33, 5, 3, "random", "random")
    for kw in (_base(), dict(_base(), splits=5), dict(K=3, xd=xd, xq=xq, excl=excl, tgt=tgt, splits=0)):
        rc, res = call(tmvb, None, kw)
        assert rc == ENODEVICE and "no HIP device" in res, (rc, res)
    pf = tmvb.syn_citeu(M=12, V=30, U=6, seed=1)
    obs, held = tmvb.split_readers(pf, 0.3)
    with pytest.raises(tmvb.EngineError):
        tmvb.rec_eval(tmvb.CTPF(obs, 3), held)


def test_rec_eval_mirror_errors(tmvb):
    pf = tmvb.syn_citeu(M=12, V=30, U=6, seed=1)
    obs, held = tmvb.split_readers(pf, 0.3)
    with pytest.raises(tmvb.TopicModelError, match="CTPF"):
        tmvb.rec_eval(tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3), held)
    with pytest.raises(ValueError, match="by must be"):
        tmvb.rec_eval(tmvb.CTPF(obs, 3), held, by="rows")
    with pytest.raises(tmvb.TopicModelError, match="same documents and users"):
        tmvb.rec_eval(tmvb.CTPF(tmvb.syn_citeu(M=13, V=30, U=6, seed=1), 3), held)
    m = tmvb.CTPF(obs, 3)
    X, Y = RECS.ctpf_factors(m)
    assert X.shape == (3, 12) and Y.shape == (3, 6) and X.dtype == np.float64
    assert np.array_equal(X, m.gimel / m.dalet[:, None] + m.zayin / m.het[:, None]) and np.array_equal(Y, m.he / m.vav[:, None])


# ------------------------------------------------------------------------------------------------------------------ static checks
def test_the_new_unit_owns_no_device_scratch():
    _units_own_no_device_scratch("tmvb_recranks.hip")


def test_header_structures_sources_and_exports(tmvb):
    syms = tmvb.exported_symbols()
    lib = C.CDLL(tmvb.LIB_PATH)
    for s in ("tmvb_readers_split", "tmvb_rsplit_free", "tmvb_score_ranks", "tmvb_rank_metrics"):
        assert s in syms and hasattr(lib, s), s
    for name in ("split_readers", "split_readers_raw", "rec_ranks_raw", "rank_metrics", "rank_metrics_raw", "rec_eval", "rec_quality", "RecEvalResult", "HeldReaders"):
        assert name in tmvb.__all__ and getattr(tmvb, name) is not None
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    define = lambda n: int(re.search(r"#define " + n + r" (\d+)", hdr).group(1))
    assert (define("TMVB_RSPLIT_ENTRY"), define("TMVB_RSPLIT_DOCUMENT")) == (ENTRY, DOCUMENT) == (0, 1) and define("TMVB_NB_TILE_DB") == T
    for struct, cls in (("tmvb_recranks_info_t", RECS.RecRanksInfo), ("tmvb_rsplit_t", RECS.ReaderSplit)):
        fields = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", hdr).group(1)
        assert re.findall(r"\b(\w+)\s*[;,]", fields) == [f[0] for f in cls._fields_], struct
    csrc = os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc")
    assert "tmvb_recranks.hip" in tmvb._lib.SOURCES
    assert all(u in open(os.path.join(ROOT, "Makefile")).read() for u in tmvb._lib.SOURCES)                  # the Makefile's list is whole again
    philox = open(os.path.join(csrc, "tmvb_philox.h")).read()
    assert "TMVB_RNG_RSPLIT_ENTRY = 6" in philox and "TMVB_RNG_RSPLIT_DOCUMENT = 7" in philox and "TMVB_RNG_SPLIT = 5" in philox
    assert "TMVB_MUTANT_RK_DROP_TAIL" in open(os.path.join(csrc, "tmvb_internal.h")).read()
    assert "tmvb_recranks.hip -DTMVB_MUTANT_RK_DROP_TAIL=1" in open(os.path.join(ROOT, "tools", "build_mutants.sh")).read()
    # the staging and layout code is shared, not copied
    for unit in ("tmvb_recranks.hip", "tmvb_neighbors.hip"):
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "tmvb_nbtile.h"' in src and "__builtin_amdgcn_mfma_f32_32x32x2f32(a0.x" not in src and "nb_perm(int k)" not in src, unit


def test_julia_shim_binds_the_entry_points():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    for s in (":tmvb_readers_split", ":tmvb_rsplit_free", ":tmvb_score_ranks", ":tmvb_rank_metrics", "mutable struct TmvbReaderSplit", "mutable struct TmvbRecRanksInfo"):
        assert s in src, s
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    for struct, jl in (("tmvb_recranks_info_t", "TmvbRecRanksInfo"), ("tmvb_rsplit_t", "TmvbReaderSplit")):
        names = re.findall(r"\b(\w+)\s*[;,]", re.search(r"typedef struct \{([^}]*)\} " + struct + ";", hdr).group(1))
        body = src[src.index("mutable struct " + jl):]
        body = body[:body.index(jl + "() =")]
        assert re.findall(r"(\w+)::", body) == names, struct


def test_the_kernels_are_in_the_resource_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    names = ("rk_feature_kernel", "rk_pairs_kernel", "rk_sort_kernel", "rk_scan_kernel", "rk_fix_kernel")
    assert all(kr.BENCHED.get(k) == 0 for k in names)
    recorded = open(os.path.join(ROOT, "profiles", "recranks_kernel_resources.txt")).read()
    assert all(k in recorded for k in names)
    lib = os.path.join(ROOT, "topicmodelsvb.jl_amd", "libtmvb_hip.so")
    if not (os.path.exists(lib) and os.path.exists(kr.READELF)):
        pytest.skip("needs the built library and llvm-readelf")
    rows = [r for r in kr.kernels(lib) if r["demangled"].startswith(names)]
    assert len(rows) == 5 and all(r["scratch"] == 0 and r["vgpr_spills"] == 0 for r in rows), rows
