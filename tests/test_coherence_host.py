"""
Topic coherence (tmvb_corpus_codocfreq / tmvb_coherence_from_counts, include/tmvb.h), the part that needs no GPU -- and the NumPy checker of
tests/test_coherence_gpu.py: the reference has no such function, so the yardstick is a restatement written here.

  * `np_codf`: a dense boolean matrix B[M, T] from the CSR, B.T @ B in int64; `np_scores`: the UMass / NPMI formulas of the header in fp64,
    every topic's terms summed exactly (math.fsum);
  * tmvb_coherence_from_counts equals `np_scores` on random consistent count tables (rows with df = 0, pairs with D_ij = 0 and D_ij = M) and
    gives the closed-form answers of a planted corpus;
  * every argument error of both entry points comes back with its status and message from a NULL context, valid arguments without a device
    give TMVB_ENODEVICE;
  * the Python mirror's own errors, the header, SOURCES, the Julia shim and the kernel-resource table.

Tolerances: counts are compared exactly.  Scores at rel 1e-12, no absolute slack: both sides take fp64 logarithms of the same integers (each
within an ulp, 1.1e-16 relative) and sum at most 2 016 of them, the checker exactly and the library with a compensated sum.
"""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tmvb_amd  # noqa: E402

# the mirror module of the feature: a tree without it fails here, at import, and with it every test of this module and of the two GPU modules
COHERENCE = sys.modules[tmvb_amd.pkg.__name__ + ".coherence"]
CHUNK_DOCS = COHERENCE.CODF_CHUNK_DOCS      # TMVB_CODF_CHUNK_DOCS; test_header_structure_sources_and_exports holds it to the header

EINVAL, ESHAPE, ENODEVICE = 1, 2, 7
SCORE_RTOL = 1e-12


# ------------------------------------------------------------------------------------------------------------------ NumPy checker
def np_codf(M, V, doc_ptr, terms, top):
    """codf[K, N, N] int64: documents that contain both top[k, i] and top[k, j]; only presence matters"""
    top = np.asarray(top, dtype=np.int64)
    ids, inv = np.unique(top, return_inverse=True)
    slot = np.full(V, -1, dtype=np.int64); slot[ids] = np.arange(len(ids))
    doc = np.repeat(np.arange(M), np.diff(np.asarray(doc_ptr, dtype=np.int64)))
    s = slot[np.asarray(terms, dtype=np.int64)]
    B = np.zeros((M, len(ids)), dtype=bool)
    B[doc[s >= 0], s[s >= 0]] = True
    G = B.T.astype(np.int64) @ B.astype(np.int64)
    sl = inv.reshape(top.shape)
    return np.stack([G[np.ix_(r, r)] for r in sl])


def np_scores(codf, M):
    """(umass[K], npmi[K], undefined_pairs[K]) by the formulas of include/tmvb.h, pairs i > j, fp64"""
    codf = np.asarray(codf, dtype=np.int64)
    K, N, _ = codf.shape
    umass, npmi, undef = np.zeros(K), np.zeros(K), np.zeros(K, dtype=np.int64)
    for k in range(K):
        D = codf[k]
        u, n = [], []
        for i in range(1, N):
            for j in range(i):
                Dij, Di, Dj = np.float64(D[i, j]), np.float64(D[i, i]), np.float64(D[j, j])
                if D[j, j] == 0:
                    undef[k] += 1
                else:
                    u.append(float(np.log((Dij + 1.0) / Dj)))
                if D[i, j] == 0:
                    n.append(-1.0)
                elif D[i, j] == M:
                    n.append(0.0)
                else:
                    n.append(float(np.log(Dij * np.float64(M) / (Di * Dj)) / -np.log(Dij / np.float64(M))))
        umass[k] = math.fsum(u) / len(u) if u else float("nan")
        npmi[k] = math.fsum(n) / len(n)
    return umass, npmi, undef


def assert_scores(got, want):
    """umass, npmi at rel 1e-12 (nan where nan), undefined_pairs exactly"""
    for g, w in zip(got[:2], want[:2]):
        assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
        ok = ~np.isnan(w)
        np.testing.assert_allclose(np.asarray(g)[ok], w[ok], rtol=SCORE_RTOL, atol=0.0)
    assert np.array_equal(got[2], want[2])


def random_corpus(M, V, seed, per_doc=8, everywhere=(), nowhere=()):
    """CSR with about per_doc distinct ids per document, 5 % of the documents drawn empty; the ids of `everywhere` are appended to EVERY document
    (so with them no document is empty), the ids of `nowhere` occur in none.  Returns (doc_ptr, terms, counts)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.poisson(per_doc, size=M)
    lens[rng.random(M) < 0.05] = 0
    pool = np.setdiff1d(np.arange(V), np.asarray(list(everywhere) + list(nowhere), dtype=np.int64))
    docs = []
    for d in range(M):
        t = rng.choice(pool, size=min(int(lens[d]), len(pool)), replace=False)
        docs.append(np.concatenate([t, np.asarray(everywhere, dtype=np.int64)]))
    doc_ptr = np.concatenate([[0], np.cumsum([len(t) for t in docs])]).astype(np.int64)
    terms = (np.concatenate(docs) if docs else np.zeros(0)).astype(np.int32)
    counts = rng.integers(1, 5, size=len(terms)).astype(np.int32)
    return doc_ptr, terms, counts


def planted(blocks, N):
    """K = len(blocks) blocks of N terms; blocks[k] documents hold exactly the N terms of block k.  Returns (M, V, doc_ptr, terms, counts)."""
    K, M = len(blocks), int(sum(blocks))
    terms = np.concatenate([np.tile(np.arange(k * N, (k + 1) * N), m) for k, m in enumerate(blocks)] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    doc_ptr = (np.arange(M + 1) * N).astype(np.int64)
    return M, K * N, doc_ptr, terms, np.ones(len(terms), dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------ scoring
@pytest.mark.parametrize("K,N,M,seed", [(1, 2, 5, 1), (3, 10, 40, 2), (4, 64, 200, 3), (6, 7, 1, 4)])
def test_scores_against_numpy_on_random_count_tables(tmvb, K, N, M, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    B = rng.random((K, M, N)) < rng.random((K, 1, N))              # every column its own density
    B[:, :, 0] = True                                              # D_ij = M for pairs of these two
    if N > 3:
        B[:, :, 1] = True
        B[:, :, 2] = False                                         # df = 0: undefined as j, D_ij = 0 everywhere
    if N > 5:
        B[:, :, 4] = ~B[:, :, 3]                                   # D_ij = 0 between two words that both occur
    codf = np.einsum("kmi,kmj->kij", B.astype(np.int64), B.astype(np.int64))
    assert (codf == M).any() and (N <= 3 or ((codf == 0).any() and (np.diagonal(codf, axis1=1, axis2=2) == 0).any()))
    want = np_scores(codf, M)
    assert_scores(tmvb.coherence_from_counts(codf, M), want)
    assert np.all(want[1] >= -1.0) and np.all(want[1] <= 1.0)


def test_closed_form_answers_on_a_planted_corpus(tmvb):
    N, blocks = 5, [7, 3, 0, 12]
    M, V, doc_ptr, terms, counts = planted(blocks, N)
    K = len(blocks)
    top = np.arange(K * N).reshape(K, N)
    codf = np_codf(M, V, doc_ptr, terms, top)
    for k, m in enumerate(blocks):
        assert np.all(codf[k] == m)
    umass, npmi, undef = tmvb.coherence_from_counts(codf, M)
    pairs = N * (N - 1) // 2
    for k, m in enumerate(blocks):
        if m == 0:
            assert undef[k] == pairs and math.isnan(umass[k]) and npmi[k] == -1.0
        else:
            assert undef[k] == 0
            assert umass[k] == pytest.approx(math.log((m + 1) / m), rel=SCORE_RTOL, abs=0.0)
            assert npmi[k] == pytest.approx(1.0, rel=SCORE_RTOL, abs=0.0)
    # rows that take terms from two blocks: the cross pairs never co-occur -> NPMI -1 on them, 1 on the others
    mixed = np.array([[0, 1, 2, N, N + 1]])
    c2 = np_codf(M, V, doc_ptr, terms, mixed)
    u2, n2, d2 = tmvb.coherence_from_counts(c2, M)
    cross, same = 3 * 2, 3 + 1
    assert n2[0] == pytest.approx((same - cross) / (same + cross), rel=SCORE_RTOL, abs=0.0) and d2[0] == 0
    assert_scores((u2, n2, d2), np_scores(c2, M))
    # K = 1, M_1 = M: every pair has D_ij = M -> NPMI 0
    M1, V1, p1, t1, _ = planted([9], N)
    c1 = np_codf(M1, V1, p1, t1, np.arange(N).reshape(1, N))
    u1, n1, d1 = tmvb.coherence_from_counts(c1, M1)
    assert n1[0] == 0.0 and d1[0] == 0 and u1[0] == pytest.approx(math.log(10 / 9), rel=SCORE_RTOL, abs=0.0)


def test_the_checker_counts_presence_only():
    """a repeated id counts its document once, order inside a document does not matter, empty documents count for nothing"""
    doc_ptr = [0, 4, 4, 6, 7]
    terms = [2, 0, 2, 1, 1, 0, 2]
    top = [[0, 1, 2]]
    want = np.array([[[2, 2, 1], [2, 2, 1], [1, 1, 2]]])
    assert np.array_equal(np_codf(4, 3, doc_ptr, terms, top), want)


# ------------------------------------------------------------------------------------------------------------------ argument errors
def _codf_base():
    return dict(M=3, V=6, doc_ptr=[0, 2, 2, 5], terms=[0, 5, 1, 2, 3], counts=[1, 4, 2, 1, 9], top=[[0, 1, 2], [5, 3, 0]], max_bitset_bytes=0)


def codocfreq_error_cases():
    b = _codf_base()
    return [
        ("K zero", dict(b, top=np.zeros((0, 3), dtype=np.int32)), EINVAL, "K = 0"),
        ("K above 1024", dict(b, top=np.tile([[0, 1, 2]], (1025, 1))), EINVAL, "K = 1025"),
        ("N one", dict(b, top=[[0], [1]]), EINVAL, "N = 1"),
        ("N sixty-five", dict(b, V=100, top=[list(range(65))]), EINVAL, "N = 65"),
        ("N above V", dict(b, top=[[0, 1, 2, 3, 4, 5, 6]]), EINVAL, "N = 7 top words of a vocabulary of 6"),
        ("M zero", dict(b, M=0), EINVAL, "M must be a positive integer"),
        ("M negative", dict(b, M=-3), EINVAL, "M must be a positive integer"),
        ("V zero", dict(b, V=0), EINVAL, "V must be a positive integer"),
        ("max_bitset_bytes negative", dict(b, max_bitset_bytes=-1), EINVAL, "max_bitset_bytes"),
        ("budget below one topic", dict(b, max_bitset_bytes=23), EINVAL, "one topic needs 24 bytes"),
        ("doc_ptr does not start at 0", dict(b, doc_ptr=[1, 2, 2, 5]), ESHAPE, "doc_ptr"),
        ("doc_ptr decreases", dict(b, doc_ptr=[0, 3, 2, 5]), ESHAPE, "doc_ptr"),
        ("term equal to V", dict(b, terms=[0, 6, 1, 2, 3]), ESHAPE, "term"),
        ("term negative", dict(b, terms=[0, 5, -1, 2, 3]), ESHAPE, "term"),
        ("count zero", dict(b, counts=[1, 4, 0, 1, 9]), ESHAPE, "count"),
        ("top id equal to V", dict(b, top=[[0, 1, 6], [5, 3, 0]]), ESHAPE, "top[0][2] = 6 outside"),
        ("top id negative", dict(b, top=[[0, 1, 2], [5, -1, 0]]), ESHAPE, "top[1][1] = -1 outside"),
        ("duplicate id in a row", dict(b, top=[[0, 1, 2], [5, 3, 5]]), ESHAPE, "term 5 is repeated in row 1"),
    ]


def _scores_base():
    return dict(K=1, N=3, M=10, codf=[[[5, 2, 1], [2, 4, 0], [1, 0, 3]]])


def scores_error_cases():
    b = _scores_base()
    return [
        ("K zero", dict(b, K=0), EINVAL, "K = 0"),
        ("K above 1024", dict(b, K=1025, codf=np.zeros((1025, 3, 3))), EINVAL, "K = 1025"),
        ("N one", dict(b, N=1, codf=[[[5]]]), EINVAL, "N = 1"),
        ("N sixty-five", dict(b, N=65, codf=np.zeros((1, 65, 65))), EINVAL, "N = 65"),
        ("M zero", dict(b, M=0), EINVAL, "M must be a positive integer"),
        ("not symmetric", dict(b, codf=[[[5, 2, 1], [2, 4, 0], [2, 0, 3]]]), ESHAPE, "not symmetric at (2, 0)"),
        ("off-diagonal above its own diagonal", dict(b, codf=[[[5, 2, 4], [2, 4, 0], [4, 0, 3]]]), ESHAPE, "exceeds a document frequency"),
        ("off-diagonal above the other diagonal", dict(b, codf=[[[5, 2, 1], [2, 1, 0], [1, 0, 3]]]), ESHAPE, "exceeds a document frequency"),
        ("diagonal above M", dict(b, M=4), ESHAPE, "is no document frequency of 4 documents"),
        ("negative entry", dict(b, codf=[[[5, 2, -1], [2, 4, 0], [-1, 0, 3]]]), ESHAPE, "negative"),
    ]


def call_codf(tmvb, ctx, kw):
    return tmvb.codocfreq_raw(ctx, kw["M"], kw["V"], kw["doc_ptr"], kw["terms"], kw["counts"], kw["top"], kw["max_bitset_bytes"])


@pytest.mark.parametrize("case", codocfreq_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_codocfreq_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call_codf(tmvb, None, kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


@pytest.mark.parametrize("case", scores_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_from_counts_argument_errors(tmvb, case):
    _, kw, status, msg = case
    rc, res = tmvb.coherence_from_counts_raw(kw["K"], kw["N"], kw["M"], kw["codf"])
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_null_arguments_are_einval(tmvb):
    L = tmvb.lib()
    P64, P32, PD = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    b = _codf_base()
    ptr = np.array(b["doc_ptr"], dtype=np.int64); t = np.array(b["terms"], dtype=np.int32); c = np.array(b["counts"], dtype=np.int32)
    top = np.array(b["top"], dtype=np.int32); codf = np.zeros((2, 3, 3), dtype=np.int64)
    full = [ptr.ctypes.data_as(P64), t.ctypes.data_as(P32), c.ctypes.data_as(P32), top.ctypes.data_as(P32), codf.ctypes.data_as(P64)]
    for hole in range(5):
        a = [p if q != hole else None for q, p in enumerate(full)]
        rc = L.tmvb_corpus_codocfreq(None, C.c_int64(3), C.c_int64(6), a[0], a[1], a[2], C.c_int32(2), C.c_int32(3), a[3], C.c_int64(0), a[4], None)
        assert rc == EINVAL and "NULL argument" in L.tmvb_last_error().decode(), hole
    u, n, d = np.zeros(2), np.zeros(2), np.zeros(2, dtype=np.int32)
    full = [codf.ctypes.data_as(P64), u.ctypes.data_as(PD), n.ctypes.data_as(PD), d.ctypes.data_as(P32)]
    for hole in range(4):
        a = [p if q != hole else None for q, p in enumerate(full)]
        rc = L.tmvb_coherence_from_counts(C.c_int32(2), C.c_int32(3), C.c_int64(3), a[0], a[1], a[2], a[3])
        assert rc == EINVAL and "NULL argument" in L.tmvb_last_error().decode(), hole


def test_valid_arguments_without_a_device_are_enodevice(tmvb):
    """No silent CPU path: the arguments pass, then a NULL context on a machine without a GPU is TMVB_ENODEVICE."""
    if tmvb.lib().tmvb_device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_coherence_gpu.py covers the live path")
    rc, res = call_codf(tmvb, None, _codf_base())
    assert rc == ENODEVICE and "no HIP device" in res
    pc = tmvb.PackedCorpus([0, 2, 2, 5], [0, 5, 1, 2, 3], [1, 4, 2, 1, 9], 6)
    with pytest.raises(tmvb.EngineError):
        tmvb.coherence(np.array([[0, 1, 2]]), pc)


def test_python_mirror_argument_errors(tmvb):
    pc = tmvb.PackedCorpus([0, 2, 2, 5], [0, 5, 1, 2, 3], [1, 4, 2, 1, 9], 6)
    other = tmvb.PackedCorpus([0, 2, 2, 5], [0, 5, 1, 2, 3], [1, 4, 2, 1, 9], 7)
    m = tmvb.LDA(pc, 3)
    with pytest.raises(tmvb.CorpusError, match="identical vocabularies"):
        tmvb.coherence(m, other, topn=3)
    for topn in (1, 65, 0, -2, 2.5):
        with pytest.raises(ValueError, match="topn"):
            tmvb.coherence(m, pc, topn=topn)
    with pytest.raises(ValueError, match="topn = 7 above the vocabulary size"):
        tmvb.coherence(m, pc, topn=7)
    with pytest.raises(ValueError):
        tmvb.coherence(np.array([[0.5, 1.0]]), pc)
    with pytest.raises(ValueError):
        tmvb.coherence(np.arange(65).reshape(1, 65), pc)
    with pytest.raises(ValueError, match="K x N x N"):
        tmvb.coherence_from_counts(np.zeros((2, 3, 4), dtype=np.int64), 5)
    with pytest.raises(tmvb.TopicModelError, match="not symmetric"):
        tmvb.coherence_from_counts([[[5, 2], [1, 4]]], 10)
    # the result object: df is the diagonal, the means skip nan, diversity counts distinct ids
    r = tmvb.CoherenceResult([[0, 1], [1, 2]], [[[3, 1], [1, 2]], [[0, 0], [0, 4]]], [-0.5, float("nan")], [0.25, -1.0], [0, 1])
    assert np.array_equal(r.df, [[3, 2], [0, 4]]) and r.diversity == 0.75
    assert r.mean_umass == -0.5 and r.mean_npmi == pytest.approx(-0.375)
    assert math.isnan(tmvb.CoherenceResult([[0, 1]], [[[0, 0], [0, 0]]], [float("nan")], [-1.0], [1]).mean_umass)


# ------------------------------------------------------------------------------------------------------------------ static checks
def test_header_structure_sources_and_exports(tmvb):
    syms = tmvb.exported_symbols()
    L = C.CDLL(tmvb.LIB_PATH)
    for s in ("tmvb_corpus_codocfreq", "tmvb_coherence_from_counts"):
        assert s in syms and hasattr(L, s)
    assert tmvb.lib().tmvb_abi_version() == 2
    for name in ("coherence", "coherence_from_counts", "codocfreq_raw", "CoherenceResult"):
        assert name in tmvb.__all__ and getattr(tmvb, name) is not None
    raw = open(os.path.join(ROOT, "include", "tmvb.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    mod = COHERENCE
    chunk = int(re.search(r"#define TMVB_CODF_CHUNK_DOCS (\d+)", hdr).group(1))
    assert chunk == mod.CODF_CHUNK_DOCS and chunk % 64 == 0
    assert int(re.search(r"#define TMVB_CODF_DEFAULT_BITSET_BYTES (\d+)", hdr).group(1)) == 2 ** 30
    # N = 64 rows of a chunk leave room for at least two workgroups in a CU's 160 KB of LDS
    assert 2 * 64 * (chunk // 64) * 8 <= 160 * 1024
    fields = re.search(r"typedef struct \{([^}]*)\} tmvb_codf_info_t;", hdr).group(1)
    assert re.findall(r"\b(\w+)\s*[;,]", fields) == [f[0] for f in mod.CodfInfo._fields_]
    assert "tmvb_coherence.hip" in tmvb._lib.SOURCES
    internal = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_internal.h")).read()
    assert "TMVB_MUTANT_CODF_DROP_TAIL" in internal
    assert "TMVB_MUTANT_CODF_DROP_TAIL=1" in open(os.path.join(ROOT, "tools", "build_mutants.sh")).read()


def test_julia_shim_binds_the_entry_points():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    for s in (":tmvb_corpus_codocfreq", ":tmvb_coherence_from_counts", "function coherence(", "mutable struct TmvbCodfInfo"):
        assert s in src, s
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    names = re.findall(r"\b(\w+)\s*[;,]", re.search(r"typedef struct \{([^}]*)\} tmvb_codf_info_t;", hdr).group(1))
    body = src[src.index("mutable struct TmvbCodfInfo"):]
    body = body[:body.index("TmvbCodfInfo() =")]
    assert re.findall(r"(\w+)::", body) == names


def test_both_kernels_are_in_the_resource_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    assert kr.BENCHED.get("codf_bitset_kernel") == 0 and kr.BENCHED.get("codf_pairs_kernel") == 0
    lib = os.path.join(ROOT, "topicmodelsvb.jl_amd", "libtmvb_hip.so")
    if not (os.path.exists(lib) and os.path.exists(kr.READELF)):
        pytest.skip("needs the built library and llvm-readelf")
    rows = [r for r in kr.kernels(lib) if r["demangled"].startswith(("codf_bitset_kernel", "codf_pairs_kernel"))]
    assert len(rows) == 2 and all(r["scratch"] == 0 and r["vgpr_spills"] == 0 for r in rows), rows
    pairs = [r for r in rows if r["demangled"].startswith("codf_pairs_kernel")][0]
    assert pairs["lds"] == 64 * 64 * 8
