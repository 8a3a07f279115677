"""
Nearest documents in topic space (tmvb_topic_neighbors, include/tmvb.h), the part that needs no GPU -- and the NumPy checker of
tests/test_neighbors_gpu.py: the reference has no such function, so the yardstick is a restatement written here.

  * `np_features`: the three transforms in fp64 (nothing rounded to fp32); `np_scores64`: their fp64 dot products; `np_topn`: the n best
    columns of every row of a score matrix under the total order (score descending, index ascending) by np.lexsort, a self column taken out
    first; `np_topn` equals a brute-force sort of Python tuples on tiny cases, ties included;
  * every argument error comes back with its status and message from a NULL context, valid arguments without a device give TMVB_ENODEVICE;
  * topic_proportions equals the three topicdist functions document by document for each model class; NeighborsResult's distances;
  * the header, the structure, SOURCES, the Julia shim, the mutant's flag, the kernel-resource table, and the tolerance literals of the GPU
    test against their recorded MI355X measurement (profiles/neighbors_tolerances_measured.json) and against the derivable cap.

Exact cases (DOT on integer features in [0, 15], K <= 64): every product is an integer below 2^8 and every partial sum one below 2^14, so
the fp32 fmaf chain and fp64 agree exactly and idx, score and count are compared bit for bit.
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tmvb_amd  # noqa: E402

# the mirror module of the feature: a tree without it fails here, at import, and with it every test of this module and of the two GPU modules
NEIGHBORS = sys.modules[tmvb_amd.pkg.__name__ + ".neighbors"]
T = NEIGHBORS.TILE_DB                       # TMVB_NB_TILE_DB; test_header_structure_sources_and_exports holds it to the header
DOT, HELLINGER, COSINE = NEIGHBORS.DOT, NEIGHBORS.HELLINGER, NEIGHBORS.COSINE
EINVAL, ESHAPE, ENODEVICE = 1, 2, 7


def cap(K):
    """the derivable bound on |score - s64| for unit-norm nonnegative features: one rounding per feature (two factors of a product) and one
    per fmaf, each at most 2^-24 relative, on terms whose sum is at most 1"""
    return (K + 3) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ NumPy checker
def np_features(x, metric):
    """K x M fp64 -> M x K fp64 features"""
    x = np.asarray(x, dtype=np.float64).T
    if metric == HELLINGER:
        return np.sqrt(x)
    if metric == COSINE:
        return x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x.copy()


def np_scores64(xd, xq, metric):
    """Mq x Md fp64 scores"""
    return np_features(xq, metric) @ np_features(xd, metric).T


def np_topn(S, n, self_of=None):
    """(idx[Mq, n] int32, score[Mq, n] of S's dtype, count[Mq]): per row of S the n best columns, score descending, index ascending on equal
    scores; column self_of[q] is no candidate of row q; -1 / -inf past count"""
    Mq, Md = S.shape
    idx = np.full((Mq, n), -1, dtype=np.int32)
    score = np.full((Mq, n), -np.inf, dtype=S.dtype)
    count = np.zeros(Mq, dtype=np.int32)
    cols = np.arange(Md)
    for q in range(Mq):
        order = np.lexsort((cols, -S[q]))
        if self_of is not None:
            order = order[order != self_of[q]]
        order = order[:n]
        idx[q, :len(order)] = order
        score[q, :len(order)] = S[q, order]
        count[q] = len(order)
    return idx, score, count


def integer_rows(K, M, seed, levels=(0, 1, 2, 15)):
    """K x M fp64 with entries drawn from few integer levels in [0, 15]: ties everywhere"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.choice(np.asarray(levels, dtype=np.float64), size=(K, M))


def dirichlet_cols(K, M, alpha, seed):
    """K x M fp64, columns ~ Dirichlet(alpha), renormalised in fp64 (a column's sum is within a few ulp of 1)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = rng.standard_gamma(alpha, size=(K, M)) + 1e-300
    return g / g.sum(axis=0)


@pytest.mark.parametrize("Mq,Md,n,seed", [(1, 1, 1, 1), (3, 5, 2, 2), (4, 9, 9, 3), (5, 7, 12, 4), (6, 6, 3, 5)])
def test_the_restatement_against_brute_force(Mq, Md, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    S = rng.integers(0, 3, size=(Mq, Md)).astype(np.float64)         # three levels: ties in every row
    for self_of in (None, np.arange(Mq) % Md):
        idx, score, count = np_topn(S, n, self_of)
        for q in range(Mq):
            cand = [(-S[q, e], e) for e in range(Md) if self_of is None or e != self_of[q]]
            best = sorted(cand)[:n]
            assert count[q] == len(best) == min(n, len(cand))
            assert idx[q, :count[q]].tolist() == [e for _, e in best]
            assert score[q, :count[q]].tolist() == [-s for s, _ in best]
            assert np.all(idx[q, count[q]:] == -1) and np.all(np.isneginf(score[q, count[q]:]))
    assert len(np.unique(S)) <= 3


def test_integer_scores_are_exact_in_fp32():
    xd = integer_rows(64, 50, 1)
    S = np_scores64(xd, xd, DOT)
    assert S.max() <= 64 * 15 * 15 < 2 ** 24 and np.array_equal(S, S.astype(np.float32).astype(np.float64))
    assert np.array_equal(S, np.rint(S))


# ------------------------------------------------------------------------------------------------------------------ argument errors
def _base():
    return dict(K=3, metric=DOT, xd=np.arange(15, dtype=np.float64).reshape(3, 5), xq=None, q0=0, n=2, splits=0, Mq=None)


def _dist(cols):
    return np.asarray(cols, dtype=np.float64).T


def error_cases():
    b = _base()
    p = _dist([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    return [
        ("K above 1024", dict(b, K=1025, xd=np.ones((1025, 2))), EINVAL, "K = 1025"),
        ("n zero", dict(b, n=0), EINVAL, "n = 0"),
        ("n sixty-five", dict(b, n=65), EINVAL, "n = 65"),
        ("Mq zero", dict(b, Mq=0), EINVAL, "Md and Mq must be positive"),
        ("Mq negative", dict(b, Mq=-2), EINVAL, "Md and Mq must be positive"),
        ("splits negative", dict(b, splits=-1), EINVAL, "splits = -1"),
        ("splits above Md", dict(b, splits=6), EINVAL, "splits = 6"),
        ("q0 negative", dict(b, q0=-1, Mq=2), EINVAL, "q0 must be nonnegative"),
        ("q0 + Mq above Md", dict(b, q0=3, Mq=3), EINVAL, "queries [3, 6) are not rows of a database of 5"),
        ("q0 with explicit queries", dict(b, xq=np.ones((3, 2)), q0=1), EINVAL, "q0 must be 0 with explicit queries"),
        ("unknown metric", dict(b, metric=3), EINVAL, "unknown metric 3"),
        ("negative metric", dict(b, metric=-1), EINVAL, "unknown metric -1"),
        ("nan in the database", dict(b, xd=np.where(np.arange(15).reshape(3, 5) == 7, np.nan, 1.0)), ESHAPE, "non-finite entry (database row 2)"),
        ("inf in the queries", dict(b, xq=np.array([[1.0], [np.inf], [0.0]])), ESHAPE, "non-finite entry (query row 0)"),
        ("hellinger negative entry", dict(b, metric=HELLINGER, xd=_dist([[0.5, 0.5, 0.0], [1.5, -0.5, 0.0]])), ESHAPE, "not a probability vector (database row 1)"),
        ("hellinger sum off by 2e-6", dict(b, metric=HELLINGER, xd=p, xq=_dist([[0.5, 0.25, 0.250002]])), ESHAPE, "not a probability vector (query row 0)"),
        ("cosine negative entry", dict(b, metric=COSINE, xd=_dist([[1.0, 2.0, 3.0], [1.0, -2.0, 3.0]])), ESHAPE, "negative entry (database row 1)"),
        ("cosine zero row", dict(b, metric=COSINE, xd=_dist([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])), ESHAPE, "all-zero row (database row 0)"),
    ]


def call(tmvb, ctx, kw):
    return tmvb.neighbors_raw(ctx, kw["K"], kw["metric"], kw["xd"], kw["xq"], kw["q0"], kw["n"], kw["splits"], Mq=kw["Mq"])


@pytest.mark.parametrize("case", error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call(tmvb, None, kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_shape_errors_through_the_abi(tmvb):
    """K = 0, Md = 0 and Md = 2^31 cannot be said with an array: the C call itself (no entry is read before these are judged)"""
    L = tmvb.lib()
    PD, P32, PF = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    x = np.ones(8); idx = np.zeros(8, dtype=np.int32); sc = np.zeros(8, dtype=np.float32); cnt = np.zeros(8, dtype=np.int32)
    a = (x.ctypes.data_as(PD), idx.ctypes.data_as(P32), sc.ctypes.data_as(PF), cnt.ctypes.data_as(P32))

    def go(K, Md, Mq, xd=a[0], out=a[1:]):
        rc = L.tmvb_topic_neighbors(None, C.c_int32(K), C.c_int32(DOT), C.c_int64(Md), xd, C.c_int64(Mq), None, C.c_int64(0), C.c_int32(1), C.c_int32(0),
                                    out[0], out[1], out[2], None)
        return rc, L.tmvb_last_error().decode()

    for K, Md, Mq, msg in ((0, 2, 2, "K = 0"), (-1, 2, 2, "K = -1"), (2, 0, 1, "Md and Mq must be positive"), (2, -4, 1, "Md and Mq must be positive"),
                           (2, 2 ** 31, 1, "2^31 or more")):
        rc, err = go(K, Md, Mq)
        assert rc == EINVAL and msg in err, (K, Md, Mq, rc, err)
    for hole in range(4):                                            # xd, idx, score, count
        p = [None if q == hole else v for q, v in enumerate(a)]
        rc, err = go(2, 2, 2, p[0], p[1:])
        assert rc == EINVAL and "NULL argument" in err, (hole, rc, err)


def test_valid_arguments_without_a_device_are_enodevice(tmvb):
    """No silent CPU path: the arguments pass, then a NULL context on a machine without a GPU is TMVB_ENODEVICE."""
    if tmvb.lib().tmvb_device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_neighbors_gpu.py covers the live path")
    p = _dist([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    for kw in (_base(), dict(_base(), metric=HELLINGER, xd=p, xq=p[:, :2]), dict(_base(), metric=COSINE, q0=2, Mq=3, splits=5),
               dict(_base(), metric=HELLINGER, xd=_dist([[0.5, 0.25, 0.2500009]]))):
        rc, res = call(tmvb, None, kw)
        assert rc == ENODEVICE and "no HIP device" in res, (rc, res)
    m = tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3)
    with pytest.raises(tmvb.EngineError):
        tmvb.docsim(m, topn=2)


# ------------------------------------------------------------------------------------------------------------------ the Python mirror
def test_topic_proportions_against_topicdist_for_each_model_class(tmvb):
    rng = np.random.Generator(np.random.PCG64(11))
    pc = tmvb.syn_nsf(M=9, V=30, seed=2)
    pf = tmvb.syn_citeu(M=9, V=30, U=5, seed=3)
    K = 4
    for cls, fn, fields in ((tmvb.LDA, tmvb.topicdist, ("gamma",)), (tmvb.fLDA, tmvb.topicdist, ("gamma",)), (tmvb.CTM, tmvb.topicdist_ctm, ("lam", "vsq")),
                            (tmvb.fCTM, tmvb.topicdist_ctm, ("lam", "vsq")), (tmvb.CTPF, tmvb.topicdist_ctpf, ("gimel",))):
        m = cls(pf if cls is tmvb.CTPF else pc, K)
        for f in fields:
            v = rng.normal(0.0, 30.0, size=(K, m.M)) if f == "lam" else rng.gamma(0.3, size=(K, m.M)) + 1e-3
            setattr(m, f, np.asfortranarray(v))
        P = tmvb.topic_proportions(m)
        assert P.shape == (K, m.M) and P.dtype == np.float64
        want = np.stack(fn(m, range(1, m.M + 1)), axis=1)
        assert np.array_equal(P, want), cls.__name__                 # the same operations, vectorised: the same bits
        np.testing.assert_allclose(P.sum(axis=0), 1.0, rtol=0, atol=1e-14)
    with pytest.raises(tmvb.TopicModelError):
        tmvb.topic_proportions(object())


def test_result_distances_and_mirror_errors(tmvb):
    s = np.array([[1.0, 0.75, 1.0000001, -np.inf]], dtype=np.float32)
    i = np.array([[4, 2, 9, -1]], dtype=np.int32)
    h = tmvb.NeighborsResult(i, s, [3], "hellinger")
    assert h.distance[0, 0] == 0.0 and h.distance[0, 1] == 0.5 and h.distance[0, 2] == 0.0 and np.isposinf(h.distance[0, 3])
    c = tmvb.NeighborsResult(i, s, [3], "cosine")
    assert c.distance[0, 1] == 0.25 and np.isposinf(c.distance[0, 3]) and c.distance.dtype == np.float64
    assert tmvb.NeighborsResult(i, s, [3], "dot").distance is None
    assert h.idx.dtype == np.int32 and h.score.dtype == np.float32 and h.count.tolist() == [3]
    m = tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3)
    with pytest.raises(ValueError, match="metric"):
        tmvb.docsim(m, metric="euclid")
    for topn in (0, 65, 2.5):
        with pytest.raises(ValueError, match="topn"):
            tmvb.docsim(m, topn=topn)
    for docs in (0, 7, [1, 9], []):
        with pytest.raises(tmvb.CorpusError, match="outside corpus range"):
            tmvb.docsim(m, docs=docs)
    with pytest.raises(tmvb.TopicModelError, match="same number of topics"):
        tmvb.docsim(m, queries=tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 4))


# ------------------------------------------------------------------------------------------------------------------ static checks
def test_header_structure_sources_and_exports(tmvb):
    assert "tmvb_topic_neighbors" in tmvb.exported_symbols() and hasattr(C.CDLL(tmvb.LIB_PATH), "tmvb_topic_neighbors")
    assert tmvb.lib().tmvb_abi_version() == 2
    for name in ("docsim", "neighbors_raw", "topic_proportions", "NeighborsResult"):
        assert name in tmvb.__all__ and getattr(tmvb, name) is not None
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    define = lambda n: int(re.search(r"#define " + n + r" (\d+)", hdr).group(1))
    assert (define("TMVB_NB_DOT"), define("TMVB_NB_HELLINGER"), define("TMVB_NB_COSINE")) == (DOT, HELLINGER, COSINE) == (0, 1, 2)
    assert define("TMVB_NB_TOPN_MAX") == NEIGHBORS.TOPN_MAX == 64
    assert define("TMVB_NB_TILE_DB") == T and T % 32 == 0
    fields = re.search(r"typedef struct \{([^}]*)\} tmvb_neighbors_info_t;", hdr).group(1)
    assert re.findall(r"\b(\w+)\s*[;,]", fields) == [f[0] for f in NEIGHBORS.NeighborsInfo._fields_]
    assert "tmvb_neighbors.hip" in tmvb._lib.SOURCES
    assert "TMVB_MUTANT_NB_DROP_TAIL" in open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_internal.h")).read()
    assert "tmvb_neighbors.hip -DTMVB_MUTANT_NB_DROP_TAIL=1" in open(os.path.join(ROOT, "tools", "build_mutants.sh")).read()
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_neighbors.hip")).read()
    assert "atomicAdd(s_cnt" in src and len(re.findall(r"\batomic\w+\(", src)) == 1     # the one atomic is the LDS append counter


def test_julia_shim_binds_the_entry_point():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    for s in (":tmvb_topic_neighbors", "function docsim(", "mutable struct TmvbNeighborsInfo"):
        assert s in src, s
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    names = re.findall(r"\b(\w+)\s*[;,]", re.search(r"typedef struct \{([^}]*)\} tmvb_neighbors_info_t;", hdr).group(1))
    body = src[src.index("mutable struct TmvbNeighborsInfo"):]
    body = body[:body.index("TmvbNeighborsInfo() =")]
    assert re.findall(r"(\w+)::", body) == names


def test_the_kernels_are_in_the_resource_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    names = ("nb_feature_kernel", "nb_scan_kernel", "nb_merge_kernel")
    assert all(kr.BENCHED.get(k) == 0 for k in names)
    lib = os.path.join(ROOT, "topicmodelsvb.jl_amd", "libtmvb_hip.so")
    if not (os.path.exists(lib) and os.path.exists(kr.READELF)):
        pytest.skip("needs the built library and llvm-readelf")
    rows = [r for r in kr.kernels(lib) if r["demangled"].startswith(names)]
    assert len(rows) == 3 and all(r["scratch"] == 0 and r["vgpr_spills"] == 0 for r in rows), rows
    recorded = open(os.path.join(ROOT, "profiles", "neighbors_kernel_resources.txt")).read()
    assert all(k in recorded for k in names)


def test_the_gpu_tolerances_are_frozen_from_their_measurement():
    """a tolerance is at least 1 x and at most 10 x the worst deviation measured on the MI355X -- and here never above the
    derivable cap (K + 3) 2^-24."""
    import test_neighbors_gpu as g
    ev = json.load(open(os.path.join(ROOT, "profiles", "neighbors_tolerances_measured.json")))["neighbors.score_abs"]
    assert sorted(int(k) for k in ev["measured"]) == sorted(g.TOL) == sorted(g.FLOAT_KS)
    for K, tol in g.TOL.items():
        measured = ev["measured"][str(K)]
        assert measured >= 0.0 and measured <= tol <= 10.0 * measured, (K, tol, measured)
        assert tol <= cap(K), (K, tol, cap(K))
