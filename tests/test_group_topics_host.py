"""
CPU tests of the grouped word-topic statistics (include/tmvb.h: tmvb_group_topics, tmvb_group_index; topicmodelsvb.jl_amd/group_topics.py):

  * the two symbols are exported and in the ABI table;
  * tmvb_group_index equals the lexsort restatement bit for bit: random corpora with empty documents, -1 labels, an empty group, repeated ids and
    unused terms, the seven presentations of tests/presentations.py, and one corpus large enough for the threaded counting sort;
  * every argument error of tmvb_group_topics is TMVB_EINVAL and comes before the device (2^31 - 2 or more entries included, for both entry
    points, judged on doc_ptr[M] alone); a NULL context without a device is TMVB_ENODEVICE;
  * time_bins at edges and NaN; trend, hot and cold on a planted prevalence table;
  * the restatement itself: JS rows against mpmath at 50 digits, additivity of S over a document split, the mutant's cut;
  * the new translation unit takes its device memory and events from tmvb_call and restates neither the responsibilities nor the JS addend.
"""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest

import group_topics_restatement as gr
import presentations as pr
import token_topics_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE = 1, 7


def random_corpus(seed, M=60, V=40, G=5, max_len=30):
    """empty documents, -1 labels, group G - 2 without a document, repeated ids inside documents, the upper fifth of the vocabulary unused"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len, size=M)
    lens[rng.integers(0, M, size=3)] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(ptr[-1])
    terms = rng.integers(0, V - V // 5, size=n).astype(np.int32)
    for d in range(0, M, 7):                               # repeats
        if lens[d] >= 3:
            terms[ptr[d] + 2] = terms[ptr[d]]
    counts = rng.integers(1, 6, size=n).astype(np.int32)
    group = rng.integers(-1, G, size=M).astype(np.int32)
    group[group == G - 2] = 0
    return types.SimpleNamespace(doc_ptr=ptr, terms=terms, counts=counts, V=V), group


def assert_index(tmvb, pc, group, G):
    rc, got = tmvb.group_index_raw(pc, group, G)
    assert rc == 0, got
    ref = gr.index(pc.doc_ptr, pc.terms, group)
    for k in ("entry", "run_ptr", "run_group", "run_term"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    return got


# ------------------------------------------------------------------------------------------------------------------ symbols
def test_the_symbols_are_new(tmvb):
    L = tmvb.lib()
    assert hasattr(L, "tmvb_group_topics") and hasattr(L, "tmvb_group_index")
    assert {"tmvb_group_topics", "tmvb_group_index"} <= set(tmvb.exported_symbols())
    import sys
    abi = sys.modules[tmvb.__name__ + "._abi"]
    assert "tmvb_group_topics" in abi.PROTOTYPES and "tmvb_group_index" in abi.PROTOTYPES and "tmvb_group_topics_info_t" in abi.STRUCTS
    assert len(abi.PROTOTYPES["tmvb_group_topics"][1]) == 23 and len(abi.PROTOTYPES["tmvb_group_index"][1]) == 11
    for name in ("group_topics", "group_topics_raw", "group_index_raw", "GroupTopics", "time_bins"):
        assert getattr(tmvb, name) is not None and name in tmvb.__all__
    hdr = open(os.path.join(ROOT, "include", "tmvb.h")).read()
    assert re.search(r"#define TMVB_GT_SEG (\d+)", hdr).group(1) == str(gr.SEG)


# ------------------------------------------------------------------------------------------------------------------ the index
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_index_equals_the_lexsort_on_random_corpora(tmvb, seed):
    pc, group = random_corpus(seed, G=5 + seed)
    got = assert_index(tmvb, pc, group, 5 + seed)
    assert len(got["entry"]) == int(np.diff(pc.doc_ptr)[group >= 0].sum()) and (5 + seed - 2) not in got["run_group"]
    assert np.any(np.diff(got["run_ptr"]) > 1)


def test_index_edge_shapes(tmvb):
    pc, group = random_corpus(9)
    got = assert_index(tmvb, pc, np.full(len(group), -1, dtype=np.int32), 3)           # nothing selected
    assert len(got["entry"]) == 0 and got["run_ptr"].tolist() == [0]
    assert_index(tmvb, pc, np.zeros(len(group), dtype=np.int32), 1)                    # one group
    one = types.SimpleNamespace(doc_ptr=np.array([0, 4]), terms=np.array([3, 3, 0, 3], dtype=np.int32), counts=np.ones(4, dtype=np.int32), V=5)
    got = assert_index(tmvb, one, np.array([0], dtype=np.int32), 65536)
    assert got["entry"].tolist() == [2, 0, 1, 3] and got["run_ptr"].tolist() == [0, 1, 4] and got["run_term"].tolist() == [0, 3]


@pytest.mark.parametrize("name", pr.NAMES)
def test_index_on_the_seven_presentations(tmvb, name):
    p = pr.present(pr.canonical(), name)
    rng = np.random.default_rng(5)
    group = rng.integers(-1, 4, size=p.M).astype(np.int32)
    pc = types.SimpleNamespace(doc_ptr=p.doc_ptr, terms=p.terms, counts=p.counts, V=p.V)
    got = assert_index(tmvb, pc, group, 4)
    if name in ("P5", "P6"):                               # repeated ids: several entries of one document in one run, in position order
        d = np.searchsorted(p.doc_ptr, got["entry"], side="right") - 1
        same = (d[1:] == d[:-1]) & (p.terms[got["entry"]][1:] == p.terms[got["entry"]][:-1])
        assert same.any() and np.all(got["entry"][1:][same] > got["entry"][:-1][same])


def test_index_at_a_size_that_uses_the_threads(tmvb):
    rng = np.random.default_rng(6)
    M, V, G = 9000, 3000, 37
    lens = rng.integers(100, 140, size=M)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert ptr[-1] >= 2 ** 20
    pc = types.SimpleNamespace(doc_ptr=ptr, terms=rng.integers(0, V, size=int(ptr[-1])).astype(np.int32), counts=None, V=V)
    pc.counts = np.ones(int(ptr[-1]), dtype=np.int32)
    group = rng.integers(0, G, size=M).astype(np.int32)    # every document selected: nsel >= 2^20
    assert_index(tmvb, pc, group, G)


def test_index_argument_errors(tmvb):
    pc, group = random_corpus(2)
    bad = lambda **kw: types.SimpleNamespace(**{**pc.__dict__, **kw})
    t6 = pc.terms.copy(); t6[6] = pc.V
    for name, (rc, msg) in {
        "G = 0": tmvb.group_index_raw(pc, np.full(len(group), -1), 0),
        "G = 65537": tmvb.group_index_raw(pc, group, 65537),
        "group = G": tmvb.group_index_raw(pc, np.where(np.arange(len(group)) == 3, 5, group), 5),
        "group = -2": tmvb.group_index_raw(pc, np.where(np.arange(len(group)) == 3, -2, group), 5),
        "term = V": tmvb.group_index_raw(bad(terms=t6), group, 5),
        "doc_ptr starts at 1": tmvb.group_index_raw(bad(doc_ptr=np.concatenate([[1], pc.doc_ptr[1:]])), group, 5),
        "V = 0": tmvb.group_index_raw(pc, group, 5, V=0),
    }.items():
        assert rc == EINVAL and isinstance(msg, str) and msg, (name, rc, msg)
    L = tmvb.lib()
    assert L.tmvb_group_index(1, 1, None, None, None, 1, None, None, None, None, None) == EINVAL and b"NULL" in L.tmvb_last_error()


# ------------------------------------------------------------------------------------------------------------------ argument errors
@pytest.fixture(scope="module")
def small():
    K, M, V = 3, 4, 6
    pc = types.SimpleNamespace(doc_ptr=np.array([0, 2, 2, 5, 6]), terms=np.array([0, 5, 1, 2, 3, 4]), counts=np.array([1, 2, 1, 1, 3, 1]), V=V)
    return K, V, np.ones((K, M)), np.ones((K, V)), pc, np.array([0, 1, -1, 1])


def test_argument_errors_come_before_the_device(tmvb, small):
    K, V, A, B, pc, grp = small
    # a NULL context: whatever passes the checks ends in ENODEVICE or EINVAL(ctx); topn = 2 where the case does not set it (V = 6 < the default 10)
    raw = lambda *a, **kw: tmvb.group_topics_raw(None, *a, **{"topn": 2, **kw})
    last = ENODEVICE if tmvb.lib().tmvb_device_count() < 1 else EINVAL
    bad = lambda **kw: types.SimpleNamespace(**{**pc.__dict__, **kw})
    cases = {
        "K = 0": raw(0, V, np.ones((0, 4)), np.ones((0, V)), pc, grp, 2),
        "K = 1025": raw(1025, V, np.ones((1025, 4)), np.ones((1025, V)), pc, grp, 2),
        "G = 0": raw(K, V, A, B, pc, np.full(4, -1), 0),
        "G = 65537": raw(K, V, A, B, pc, grp, 65537),
        "n = 0": raw(K, V, A, B, pc, grp, 2, topn=0),
        "n = V + 1": raw(K, V, A, B, pc, grp, 2, topn=V + 1),
        "n = 65": raw(K, 100, A, np.ones((K, 100)), pc, grp, 2, topn=65),
        "eps below 2^-100": raw(K, V, A, B, pc, grp, 2, eps=2.0 ** -101),
        "eps = 0": raw(K, V, A, B, pc, grp, 2, eps=0.0),
        "eps above 1": raw(K, V, A, B, pc, grp, 2, eps=1.5),
        "eps NaN": raw(K, V, A, B, pc, grp, 2, eps=float("nan")),
        "max_chunk_groups < 0": raw(K, V, A, B, pc, grp, 2, max_chunk_groups=-1),
        "term = V": raw(K, V, A, B, bad(terms=np.array([0, 5, 1, 2, 3, 6])), grp, 2),
        "term < 0": raw(K, V, A, B, bad(terms=np.array([0, 5, -1, 2, 3, 4])), grp, 2),
        "count = 0": raw(K, V, A, B, bad(counts=np.array([1, 2, 0, 1, 3, 1])), grp, 2),
        "count = 2^29": raw(K, V, A, B, bad(counts=np.array([1, 2, 2 ** 29, 1, 3, 1])), grp, 2),
        "doc_ptr decreases": raw(K, V, A, B, bad(doc_ptr=np.array([0, 2, 1, 5, 6])), grp, 2),
        "doc_ptr starts at 1": raw(K, V, A, B, bad(doc_ptr=np.array([1, 2, 2, 5, 6])), grp, 2),
        "group = G": raw(K, V, A, B, pc, np.array([0, 2, -1, 1]), 2),
        "group = -2": raw(K, V, A, B, pc, np.array([0, -2, -1, 1]), 2),
        "negative A": raw(K, V, np.where(np.arange(12).reshape(3, 4) == 7, -1e-300, A), B, pc, grp, 2),
        "NaN A": raw(K, V, np.where(np.arange(12).reshape(3, 4) == 0, np.nan, A), B, pc, grp, 2),
        "A beyond fp32": raw(K, V, np.where(np.arange(12).reshape(3, 4) == 0, 1e39, A), B, pc, grp, 2),
        "negative B": raw(K, V, A, np.where(np.arange(18).reshape(3, 6) == 17, -1.0, B), pc, grp, 2),
        "NaN B": raw(K, V, A, np.where(np.arange(18).reshape(3, 6) == 4, np.nan, B), pc, grp, 2),
        "infinite B": raw(K, V, A, np.where(np.arange(18).reshape(3, 6) == 4, np.inf, B), pc, grp, 2),
        "A of the wrong shape": raw(K, V, np.ones((K, 5)), B, pc, grp, 2),
        "group of the wrong length": raw(K, V, A, B, pc, grp[:3], 2),
    }
    for name, (rc, msg) in cases.items():
        assert rc == EINVAL and isinstance(msg, str) and msg, (name, rc, msg)
        assert "ctx is NULL" not in msg and "no HIP device" not in msg, (name, msg)
    # the edges of the legal ranges pass every check and reach the context test
    for kw in (dict(eps=2.0 ** -100), dict(eps=1.0), dict(topn=V), dict(topn=1), dict(shift=False, drift=False), dict(dense=True), dict(max_chunk_groups=1)):
        rc, msg = raw(K, V, A, B, pc, grp, 2, **kw)
        assert rc == last and ("no HIP device" in msg or "ctx is NULL" in msg), (kw, rc, msg)
    rc, msg = raw(K, V, A, B, bad(counts=np.array([1, 2, 2 ** 29 - 1, 1, 3, 1])), grp, 2)
    assert rc == last, msg
    # a NaN in the column of A of a document that is left out is not read
    rc, msg = raw(K, V, np.where(np.arange(12).reshape(3, 4) == 2, np.nan, A), B, pc, grp, 2)
    assert rc == last, msg


def test_size_and_null_errors_of_the_abi_itself(tmvb, small):
    K, V, A, B, pc, grp = small
    L = tmvb.lib()
    f = lambda a, t: np.ascontiguousarray(a, dtype=t)
    Af, Bf = np.asfortranarray(A), np.asfortranarray(B)
    ptr, terms, counts, g32 = f(pc.doc_ptr, np.int64), f(pc.terms, np.int32), f(pc.counts, np.int32), f(grp, np.int32)
    docs, tokens, mass = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros((2, K))
    idx, p = np.zeros((2, K, 1), np.int32), np.zeros((2, K, 1))
    P = {np.dtype(np.float64): C.POINTER(C.c_double), np.dtype(np.int64): C.POINTER(C.c_int64), np.dtype(np.int32): C.POINTER(C.c_int32)}
    ptrs = lambda *arrs: [a.ctypes.data_as(P[a.dtype]) if a is not None else None for a in arrs]

    def call(K_=K, V_=V, M_=4, drop=None):
        args = [Af, Bf, ptr, terms, counts, g32, docs, tokens, mass, idx, p]
        if drop is not None:
            args[drop] = None
        a = ptrs(*args)
        return L.tmvb_group_topics(None, K_, V_, M_, a[0], a[1], a[2], a[3], a[4], a[5], 2, 1e-30, 1, 0, a[6], a[7], a[8], a[9], a[10], None, None, None, None)

    assert call(K_=1024, V_=2 ** 21) == EINVAL and b"K V is 2^31 or more" in L.tmvb_last_error()          # judged before B is read
    assert call(M_=0) == EINVAL and call(V_=0) == EINVAL and call(M_=-1) == EINVAL
    for drop in range(11):
        assert call(drop=drop) == EINVAL and b"NULL argument" in L.tmvb_last_error(), drop
    last = ENODEVICE if L.tmvb_device_count() < 1 else EINVAL
    assert call() == last and (b"no HIP device" in L.tmvb_last_error() or b"ctx is NULL" in L.tmvb_last_error())
    assert docs.tolist() == [1, 2] and tokens.tolist() == [3, 1]                                           # host integers, filled with the checks


def test_too_many_entries_are_refused_before_an_entry_is_read(tmvb):
    """2^31 - 2 or more entries in one call: judged on doc_ptr[M] alone, so M = 1 with doc_ptr = [0, 2^31 - 2] and one-element arrays needs no memory"""
    L = tmvb.lib()
    K, V = 2, 3
    ptr, terms, counts, g32 = np.array([0, 2 ** 31 - 2], np.int64), np.zeros(1, np.int32), np.ones(1, np.int32), np.zeros(1, np.int32)
    A, B = np.ones((K, 1), order="F"), np.ones((K, V), order="F")
    docs, tokens, mass, idx, p = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros((1, K)), np.zeros((1, K, 1), np.int32), np.zeros((1, K, 1))
    d, i64, i32 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    for n_entries in (2 ** 31 - 2, 2 ** 31 - 1, 2 ** 33):
        ptr[1] = n_entries
        rc = L.tmvb_group_topics(None, K, V, 1, d(A), d(B), i64(ptr), i32(terms), i32(counts), i32(g32), 1, 1e-30, 1, 0, i64(docs), i64(tokens), d(mass), i32(idx),
                                 d(p), None, None, None, None)
        assert rc == EINVAL and f"{n_entries} entries in one call (limit 2^31 - 2)".encode() in L.tmvb_last_error(), (n_entries, L.tmvb_last_error())
        n_runs, run_ptr, run_group, run_term, entry = C.c_int64(-1), np.zeros(2, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int64)
        rc = L.tmvb_group_index(1, V, i64(ptr), i32(terms), i32(g32), 1, C.byref(n_runs), i64(run_ptr), i32(run_group), i32(run_term), i64(entry))
        assert rc == EINVAL and f"tmvb_group_index: {n_entries} entries in one call (limit 2^31 - 2)".encode() in L.tmvb_last_error(), (n_entries, L.tmvb_last_error())
        assert n_runs.value == -1 and docs[0] == 0 and tokens[0] == 0                   # nothing was written
    ptr[1] = 1                                             # the same arrays with one entry pass every check and reach the context test / build the index
    rc = L.tmvb_group_topics(None, K, V, 1, d(A), d(B), i64(ptr), i32(terms), i32(counts), i32(g32), 1, 1e-30, 1, 0, i64(docs), i64(tokens), d(mass), i32(idx), d(p),
                             None, None, None, None)
    assert rc == (ENODEVICE if L.tmvb_device_count() < 1 else EINVAL) and (b"no HIP device" in L.tmvb_last_error() or b"ctx is NULL" in L.tmvb_last_error())
    n_runs = C.c_int64(-1)
    run_ptr, run_group, run_term, entry = np.zeros(2, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int64)
    assert L.tmvb_group_index(1, V, i64(ptr), i32(terms), i32(g32), 1, C.byref(n_runs), i64(run_ptr), i32(run_group), i32(run_term), i64(entry)) == 0
    assert n_runs.value == 1 and run_ptr.tolist() == [0, 1] and entry.tolist() == [0]


# ------------------------------------------------------------------------------------------------------------------ time_bins, trend
def test_time_bins_at_edges_and_nan(tmvb):
    s = [1990.0, 1994.999, 1995.0, 2000.0, float("nan"), 1989.9, 2000.1, 1999.0]
    out = tmvb.time_bins(s, [1990, 1995, 2000])
    assert out[:4].tolist() == [1990.0, 1990.0, 1995.0, 1995.0] and out[7] == 1995.0                       # the last bin is closed above
    assert np.isnan(out[4]) and np.isnan(out[5]) and np.isnan(out[6])
    out = tmvb.time_bins([0.0, 1.0, 2.0, 3.0, 4.0, float("nan")], 2)
    assert out[:5].tolist() == [0.0, 0.0, 2.0, 2.0, 2.0] and np.isnan(out[5])
    assert tmvb.time_bins([5.0, 5.0], 3).tolist() == [5.0, 5.0]                                            # one distinct stamp: the first bin
    for bad in ([2.0, 1.0], [1.0], [[1.0, 2.0]], [1.0, float("inf")], 0):
        with pytest.raises(ValueError):
            tmvb.time_bins([1.0], bad)
    with pytest.raises(ValueError):
        tmvb.time_bins([float("nan")], 2)


def planted(prev, tokens):
    G, K = prev.shape
    mass = prev * tokens[:, None]
    return {"docs": (tokens > 0).astype(np.int64), "tokens": tokens, "mass": mass, "top_idx": np.full((G, K, 2), -1, dtype=np.int32),
            "top_p": np.zeros((G, K, 2)), "shift": np.ones((G, K)), "drift": np.ones((G, K)), "dense": None, "info": {}}


def test_trend_hot_and_cold_on_a_planted_table(tmvb):
    G, K = 6, 4
    x = np.arange(G, dtype=np.float64)
    prev = np.stack([0.1 + 0.05 * x, 0.4 - 0.06 * x, np.full(G, 0.2), 0.3 + 0.01 * x], axis=1)           # slopes 0.05, -0.06, 0, 0.01; rows sum to 1
    assert np.allclose(prev.sum(axis=1), 1.0)
    tokens = np.array([100, 200, 0, 50, 400, 10], dtype=np.int64)                                          # group 2 has no entries: left out of the fit
    gt = tmvb.GroupTopics(list("abcdef"), planted(prev, tokens), np.zeros((G, K)))
    assert np.allclose(gt.trend, [0.05, -0.06, 0.0, 0.01], atol=1e-12)
    assert gt.hot(2).tolist() == [0, 3] and gt.cold(2).tolist() == [1, 2] and gt.hot(10).tolist() == [0, 3, 2, 1]
    assert np.all(np.isnan(gt.prevalence[2])) and np.all(np.isnan(gt.shift[2])) and np.all(np.isnan(gt.drift[2]))
    assert np.all(np.isnan(gt.drift[0])) and not np.any(np.isnan(gt.drift[[1, 3, 4, 5]])) and not np.any(np.isnan(gt.shift[[0, 1, 3, 4, 5]]))
    assert np.allclose(gt.prevalence[[0, 1, 3, 4, 5]], prev[[0, 1, 3, 4, 5]], rtol=1e-13)
    assert gt.words[0] == [[], [], [], []]
    with pytest.raises(ValueError):
        gt.beta(0)
    one = tmvb.GroupTopics(["a"], planted(prev[:1], tokens[:1]), np.zeros((1, K)))
    assert one.trend.tolist() == [0.0] * K


def test_labels_and_order(tmvb):
    mod = __import__("sys").modules[tmvb.__name__ + ".group_topics"]
    labels, g = mod._group_ids(["b", None, "a", float("nan"), "b"], 5, None)
    assert labels == ["a", "b"] and g.tolist() == [1, -1, 0, -1, 1]
    labels, g = mod._group_ids([2, 1, 2], 3, [2, 3, 1])
    assert labels == [2, 3, 1] and g.tolist() == [0, 2, 0]
    for groups, order in ((["a", "b"], ["a"]), (["a", "b"], ["a", "a", "b"]), ([None, None], None), (["a", 1], None)):
        with pytest.raises(ValueError):
            mod._group_ids(groups, 2, order)
    with pytest.raises(ValueError):
        mod._group_ids(["a"], 2, None)


@pytest.mark.parametrize("name", ["flda_m40_v60_k5", "fctm_m30_v50_k4"])
def test_filtered_models_raise(tmvb, name):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    m = types.SimpleNamespace(**{k: g[k] for k in g.files})
    m.V, m.M = int(g["V"]), len(g["doc_ptr"]) - 1
    with pytest.raises(tmvb.TopicModelError, match="tau"):
        tmvb.group_topics(m, [0] * m.M)


# ------------------------------------------------------------------------------------------------------------------ the restatement itself
def test_js_rows_against_mpmath():
    import mpmath                                         # a missing mpmath fails this test; it does not skip it
    mpmath.mp.dps = 50
    rng = np.random.default_rng(7)
    for V in (5, 60, 700):
        p, q = rng.gamma(0.3, size=V), rng.gamma(0.3, size=V)
        p[rng.random(V) < 0.2] = 0.0
        q[rng.random(V) < 0.2] = 0.0
        p, q = p / p.sum(), q / q.sum()
        ref = mpmath.mpf(0)
        for a, b in zip(p, q):
            a, b = mpmath.mpf(float(a)), mpmath.mpf(float(b))
            s = a + b
            ref += (a * mpmath.log(2 * a / s) if a > 0 else 0) / 2 + (b * mpmath.log(2 * b / s) if b > 0 else 0) / 2
        got = gr.js_row(p, q)
        print(f"js_row V = {V}: {got:.17g} against mpmath {float(ref):.17g}, |difference| / cap = {abs(got - float(ref)) / gr.cap_js(V):.3f}")
        assert abs(got - float(ref)) <= gr.cap_js(V) and 0.0 < got < math.log(2.0)
    assert gr.js_row([0.5, 0.5, 0.0], [0.5, 0.5, 0.0]) == 0.0
    assert abs(gr.js_row([1.0, 0.0], [0.0, 1.0]) - math.log(2.0)) <= 2.0 ** -52


def test_s_is_additive_over_a_document_split_and_the_mutant_cuts_the_last_segment():
    pc, group = random_corpus(3, M=50, V=30, G=4)
    K, M = 5, 50
    rng = np.random.default_rng(8)
    A, B = rng.integers(1, 3, size=(K, M)).astype(np.float64), rng.integers(1, 3, size=(K, pc.V)).astype(np.float64)
    r = tr.responsibilities(A, B, pc.doc_ptr, pc.terms, None, 2.0 ** -100).astype(np.float32)               # fp32 values of at least 1 / 20, counts below 6: every sum is exact in fp64
    whole = gr.stats(r, pc.doc_ptr, pc.terms, pc.counts, group, 4, pc.V)
    cut = 23
    first, second = np.where(np.arange(M) < cut, group, -1), np.where(np.arange(M) >= cut, group, -1)
    a, b = gr.stats(r, pc.doc_ptr, pc.terms, pc.counts, first, 4, pc.V), gr.stats(r, pc.doc_ptr, pc.terms, pc.counts, second, 4, pc.V)
    assert np.array_equal(a["S"] + b["S"], whole["S"]) and np.array_equal(a["tokens"] + b["tokens"], whole["tokens"])
    assert np.array_equal(a["docs"] + b["docs"], whole["docs"]) and whole["docs"].sum() == int((group >= 0).sum())
    assert np.allclose(whole["S"].sum(axis=(1, 2)), whole["tokens"], rtol=1e-6)                             # sum_k r = 1 up to fp32 rounding
    assert np.array_equal(gr.stats(r, pc.doc_ptr, pc.terms, pc.counts, group, 4, pc.V, cut_mutant=True)["S"], whole["S"])          # no run longer than SEG here
    # the mutant: a run of 2 SEG + 1 entries of one term keeps 2 SEG of them; a run of SEG entries is whole
    n = 2 * gr.SEG + 1
    ptr = np.arange(n + 1, dtype=np.int64)
    ones = np.ones((n, 1), dtype=np.float32)
    full = gr.stats(ones, ptr, np.zeros(n, np.int32), np.ones(n, np.int32), np.zeros(n, np.int32), 1, 2)
    mut = gr.stats(ones, ptr, np.zeros(n, np.int32), np.ones(n, np.int32), np.zeros(n, np.int32), 1, 2, cut_mutant=True)
    assert full["S"][0, 0, 0] == n and mut["S"][0, 0, 0] == 2 * gr.SEG and full["n_max"][0] == n
    short = gr.stats(ones[:gr.SEG], ptr[:gr.SEG + 1], np.zeros(gr.SEG, np.int32), np.ones(gr.SEG, np.int32), np.zeros(gr.SEG, np.int32), 1, 2, cut_mutant=True)
    assert short["S"][0, 0, 0] == gr.SEG


def test_selection_breaks_ties_towards_the_lower_term():
    beta = np.array([[[0.25, 0.5, 0.25, 0.0], [0.0, 0.0, 0.0, 0.0]]])
    idx, p = gr.select(beta, np.array([[1.0, 0.0]]), 3)
    assert idx.tolist() == [[[1, 0, 2], [-1, -1, -1]]] and p.tolist() == [[[0.5, 0.25, 0.25], [0.0, 0.0, 0.0]]]


# ------------------------------------------------------------------------------------------------------------------ the unit's device scratch
def test_the_unit_owns_no_device_scratch_and_restates_nothing():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_group_topics.hip")).read()
    assert '#include "tmvb_call.h"' in src and '#include "tmvb_token_phi.h"' in src and '#include "tmvb_divergence_terms.h"' in src
    for pat in (r"hipMalloc\(", r"hipFree\(", r"hipEventCreate\(", r"hipEventDestroy\(", r"struct \w*_pool", r"auto cleanup", r"#define [A-Z]+_(HIP|TRY)"):
        assert not re.search(pat, src), f"tmvb_group_topics.hip: {pat} -- device memory and events of a call come from tmvb_call (csrc/tmvb_call.h)"
    assert "getenv" not in src and "atomic" not in src.replace("No atomics", "")
    assert "__fmaf_rn" not in src and "__fdiv_rn" not in src and "log(" not in src          # the responsibilities and the JS addend live in the shared headers
    for unit, fn in (("tmvb_token_topics.hip", "tt_responsibilities("), ("tmvb_topic_compare.hip", "td_term<METRIC>(")):
        u = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", unit)).read()
        assert fn in u and "__fdiv_rn" not in u and "log((2.0 * p)" not in u
