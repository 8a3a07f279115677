"""
Search by words (tmvb_topic_search, include/tmvb.h), the part that needs no GPU:

  * the restatement of tests/search_restatement.py: its top-n against a brute-force sort of Python tuples, and its emulation of the device's
    fp32 accumulator chain inside the derivable cap C_q (K + 3) 2^-24 + |s64| 2^-24 at K = 3, 50, 130 and 1024;
  * the header, the structure, SOURCES, the exported symbol, the ctypes binding, the Julia shim (through the functions of
    tests/test_julia_shim_static.py), the mutant's flag and the kernel-resource table;
  * every argument error comes back with its status and message from a NULL context, valid arguments without a device give TMVB_ENODEVICE;
    the Python mirror's own errors (unknown word, CTPF, empty query, ...) and the packing of the three query forms;
  * the tolerance literals of the GPU module against their recorded MI355X measurement (profiles/search_tolerances_measured.json) and the cap.
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

import search_restatement as sr  # noqa: E402
import tmvb_amd  # noqa: E402

# the mirror module of the feature: a tree without it fails here, at import, and with it every test of this module and of the two GPU modules
SEARCH = sys.modules[tmvb_amd.pkg.__name__ + ".search"]
EINVAL, ESHAPE, ENODEVICE = 1, 2, 7


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("Q,Md,n,seed", [(1, 1, 1, 1), (3, 5, 2, 2), (4, 9, 9, 3), (5, 7, 12, 4)])
def test_the_restatement_top_n_against_brute_force(Q, Md, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    S = rng.integers(0, 3, size=(Q, Md)).astype(np.float64)          # three levels: ties in every row
    S[S == 0] = -np.inf                                              # -inf is a score like any other
    idx, score, count = sr.np_topn(S, n)
    for q in range(Q):
        best = sorted((-S[q, e], e) for e in range(Md))[:n]
        assert count[q] == len(best) == min(n, Md)
        assert idx[q, :count[q]].tolist() == [e for _, e in best] and score[q, :count[q]].tolist() == [-s for s, _ in best]
        assert np.all(idx[q, count[q]:] == -1) and np.all(np.isneginf(score[q, count[q]:]))


@pytest.mark.parametrize("K,alpha", [(3, 0.1), (50, 0.1), (130, 0.03), (1024, 0.01)])
def test_the_emulated_fp32_chain_stays_inside_the_cap(K, alpha):
    """Dirichlet theta, Dirichlet beta rows and laplace_smooth = 1e-6: every p is at least about 1e-6, nothing underflows in fp32"""
    V, Md = 200, 130
    theta = sr.dirichlet_cols(K, Md, alpha, seed=K)
    beta = sr.dirichlet_beta(K, V, 0.05, seed=K + 1)
    qs = sr.make_queries([1, 2, 5, 127, 128, 3, 1], V, seed=K + 2)
    S64 = sr.s64(theta, beta, 1e-6, *qs)
    E = sr.score_emulated(theta, beta, 1e-6, *qs)
    assert sr.p_chain32(theta, beta, 1e-6, qs[1]).min() > 5e-7 and np.all(np.isfinite(S64))
    ratio = np.abs(E.astype(np.float64) - S64) / sr.cap(K, S64, sr.tokens(qs[0], qs[2]))
    print(f"K = {K}: worst |emulation - s64| / cap = {ratio.max():.3f}")
    assert ratio.max() <= 1.0, (K, ratio.max())
    assert ratio.max() > 0.0                                         # the two are not the same computation


def test_the_restatement_on_a_case_by_hand():
    theta = np.array([[0.5, 1.0], [0.5, 0.0]])                       # K = 2, two documents
    beta = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5]])
    qs = (np.array([0, 2, 3], dtype=np.int64), np.array([0, 2, 1], dtype=np.int32), np.array([2, 1, 3], dtype=np.int32))
    S = sr.s64(theta, beta, 0.0, *qs)
    assert np.isclose(S[0, 0], 2 * np.log(0.25) + np.log(0.25)) and np.isneginf(S[0, 1])      # document 1 gives word 2 probability 0
    assert np.allclose(S[1], 3 * np.log(0.5))
    assert np.array_equal(sr.score_emulated(theta, beta, 0.0, *qs), S.astype(np.float32))     # powers of two: fp32 is exact
    assert sr.tokens(qs[0], qs[2]).tolist() == [3, 3]
    bp = sr.beta_prime(beta, 0.5)
    assert np.allclose(bp.sum(axis=1), 1.0) and np.isclose(bp[0, 2], 0.5 / 2.5)


# ------------------------------------------------------------------------------------------------------------------ static checks
def test_header_structure_sources_and_exports(tmvb):
    assert "tmvb_topic_search" in tmvb.exported_symbols() and hasattr(C.CDLL(tmvb.LIB_PATH), "tmvb_topic_search")
    for name in ("search", "search_raw", "pack_queries", "SearchResult", "SearchInfo"):
        assert name in tmvb.__all__ and getattr(tmvb, name) is not None
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    define = lambda n: int(re.search(r"#define " + n + r" (\d+)", hdr).group(1))
    assert define("TMVB_SEARCH_TILE_COLS") == SEARCH.TILE_COLS == sr.TILE_COLS == define("TMVB_NB_TILE_DB") == 128
    fields = re.search(r"typedef struct \{([^}]*)\} tmvb_search_info_t;", hdr).group(1)
    assert re.findall(r"\b(\w+)\s*[;,]", fields) == [f[0] for f in tmvb.SearchInfo._fields_] == ["splits", "kp", "col_tiles", "ms_prep", "ms_scan", "ms_merge"]
    assert C.sizeof(tmvb.SearchInfo) == 24
    assert "tmvb_search.hip" in tmvb._lib.SOURCES and "tmvb_search.hip" in open(os.path.join(ROOT, "Makefile")).read()
    assert "TMVB_MUTANT_SEARCH_DROP_LAST_ENTRY" in open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_internal.h")).read()
    assert "tmvb_search.hip -DTMVB_MUTANT_SEARCH_DROP_LAST_ENTRY=1" in open(os.path.join(ROOT, "tools", "build_mutants.sh")).read()
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_search.hip")).read()
    assert "atomicAdd(s_cnt" in src and len(re.findall(r"\batomic\w+\(", src)) == 1     # the one atomic is the LDS append counter
    assert "#ifdef TMVB_MUTANT_SEARCH_DROP_LAST_ENTRY" in src


def test_the_ctypes_binding_matches_the_header(tmvb):
    import test_julia_shim_static as js
    ret, params = js.header_protos()["tmvb_topic_search"]
    fn = tmvb.lib().tmvb_topic_search
    assert ret == "int" and fn.restype is C.c_int and len(fn.argtypes) == len(params) == 17
    scalar = {C.c_int32: "i32", C.c_int64: "i64", C.c_double: "f64", C.c_float: "f32"}
    for q, (want, at) in enumerate(zip(params, fn.argtypes)):
        if want[0] != "ptr":
            assert scalar[at] == want[0], (q, want, at)
        elif want[1] == "opaque":                                    # tmvb_ctx* travels as void*, the info struct by its own type
            assert at is C.c_void_p or at._type_ is tmvb.SearchInfo, (q, at)
        else:
            assert scalar[at._type_] == want[1], (q, want, at)


def test_julia_shim_binds_the_entry_point():
    import test_julia_shim_static as js
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    for s in (":tmvb_topic_search", "function search(", "mutable struct TmvbSearchInfo"):
        assert s in src, s
    ret, params = js.header_protos()["tmvb_topic_search"]
    calls = [c for c in js.ccalls(src) if c[0] == "tmvb_topic_search"]
    assert len(calls) == 1
    _, jret, types, args = calls[0]
    assert jret == "Cint" and len(types) == len(args) == len(params) == 17
    for q, (c, t) in enumerate(zip(params, types)):
        assert js.compatible(c, js.jl_class(t)), (q, c, t)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    names = re.findall(r"\b(\w+)\s*[;,]", re.search(r"typedef struct \{([^}]*)\} tmvb_search_info_t;", hdr).group(1))
    body = src[src.index("mutable struct TmvbSearchInfo"):]
    body = body[:body.index("TmvbSearchInfo() =")]
    assert re.findall(r"(\w+)::", body) == names


def test_the_kernels_are_in_the_resource_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    names = ("sr_feature_kernel", "sr_scan_kernel", "sr_merge_kernel")
    assert all(kr.BENCHED.get(k) == 0 for k in names)
    recorded = open(os.path.join(ROOT, "profiles", "search_kernel_resources.txt")).read()
    assert all(k in recorded for k in names)
    lib = os.path.join(ROOT, "topicmodelsvb.jl_amd", "libtmvb_hip.so")
    if not (os.path.exists(lib) and os.path.exists(kr.READELF)):
        pytest.skip("needs the built library and llvm-readelf")
    rows = [r for r in kr.kernels(lib) if r["demangled"].startswith(names)]
    assert len(rows) == 3 and all(r["scratch"] == 0 and r["vgpr_spills"] == 0 for r in rows), rows


def test_the_worst_case_lds_fits_the_compute_unit():
    """the p tile or the operand staging, the lists, the thresholds, the insertion buffer and the segment tables"""
    worst = max(max(2 * 128 * (kc + 2) * 4, 128 * 128 * 4) + 128 * n * 8 + 128 * 8 + 1024 * 12 + 3 * 128 * 4 + 16 for kc in (4, 32, 64) for n in (1, 64))
    assert worst == 147984 <= 160 * 1024
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_search.hip")).read()
    assert "#define SR_CAND 1024" in src and "3 * SR_TC * sizeof(int) + 16" in src


# ------------------------------------------------------------------------------------------------------------------ argument errors
def _base():
    theta = np.array([[0.5, 0.25, 0.2, 1.0], [0.25, 0.25, 0.3, 0.0], [0.25, 0.5, 0.5, 0.0]])         # K = 3, Md = 4
    beta = np.full((3, 5), 0.2)                                                                      # V = 5
    return dict(K=3, V=5, theta=theta, beta=beta, q_ptr=[0, 2, 3], q_terms=[0, 4, 2], q_counts=[1, 2, 1], n=2, s=0.0, splits=0, Q=None)


def error_cases():
    b = _base()
    bad_theta = b["theta"].copy(); bad_theta[2, 1] = 0.500002
    neg_theta = b["theta"].copy(); neg_theta[:, 2] = [1.5, -0.5, 0.0]
    nan_theta = b["theta"].copy(); nan_theta[0, 3] = np.nan
    bad_beta = b["beta"].copy(); bad_beta[1, 0] = 0.3
    neg_beta = b["beta"].copy(); neg_beta[0, :2] = [-0.1, 0.5]
    long_q = list(range(129))
    return [
        ("K above 1024", dict(b, K=1025, theta=np.full((1025, 2), 1.0 / 1025), beta=np.full((1025, 5), 0.2)), EINVAL, "K = 1025"),
        ("n zero", dict(b, n=0), EINVAL, "n = 0"),
        ("n sixty-five", dict(b, n=65), EINVAL, "n = 65"),
        ("Q zero", dict(b, Q=0), EINVAL, "Md, V and Q must be positive"),
        ("Q negative", dict(b, Q=-3), EINVAL, "Md, V and Q must be positive"),
        ("V zero", dict(b, V=0), EINVAL, "Md, V and Q must be positive"),
        ("splits negative", dict(b, splits=-1), EINVAL, "splits = -1"),
        ("splits above Md", dict(b, splits=5), EINVAL, "splits = 5"),
        ("smoothing negative", dict(b, s=-1e-9), EINVAL, "laplace_smooth parameter must be nonnegative."),
        ("smoothing nan", dict(b, s=float("nan")), EINVAL, "laplace_smooth parameter must be nonnegative."),
        ("smoothing inf", dict(b, s=float("inf")), EINVAL, "laplace_smooth parameter must be nonnegative."),
        ("q_ptr not from zero", dict(b, q_ptr=[1, 2, 3]), ESHAPE, "q_ptr must start at 0"),
        ("q_ptr decreasing", dict(b, q_ptr=[0, 3, 2]), ESHAPE, "q_ptr decreases at query 1"),
        ("empty query", dict(b, q_ptr=[0, 3, 3]), ESHAPE, "query 1 is empty"),
        ("empty first query", dict(b, q_ptr=[0, 0, 3]), ESHAPE, "query 0 is empty"),
        ("query of 129 entries", dict(b, V=200, beta=np.full((3, 200), 0.005), q_ptr=[0, 1, 130], q_terms=[0] + long_q, q_counts=[1] * 130), ESHAPE,
         "query 1 has 129 entries (limit 128)"),
        ("term id V", dict(b, q_terms=[0, 5, 2]), ESHAPE, "query 0 holds term 5 outside [0, 5)"),
        ("term id negative", dict(b, q_terms=[0, 4, -1]), ESHAPE, "query 1 holds term -1 outside [0, 5)"),
        ("count zero", dict(b, q_counts=[1, 0, 1]), ESHAPE, "query 0 holds a count below 1"),
        ("count negative", dict(b, q_counts=[1, 2, -4]), ESHAPE, "query 1 holds a count below 1"),
        ("beta row sum", dict(b, beta=bad_beta), ESHAPE, "beta must be a right stochastic matrix."),
        ("beta negative entry", dict(b, beta=neg_beta), ESHAPE, "beta must be a right stochastic matrix."),
        ("theta sum off by 2e-6", dict(b, theta=bad_theta), ESHAPE, "not a probability vector (document 1)"),
        ("theta negative entry", dict(b, theta=neg_theta), ESHAPE, "not a probability vector (document 2)"),
        ("theta nan", dict(b, theta=nan_theta), ESHAPE, "not a probability vector (document 3)"),
    ]


def call(tmvb, ctx, kw):
    return tmvb.search_raw(ctx, kw["K"], kw["V"], kw["theta"], kw["beta"], kw["q_ptr"], kw["q_terms"], kw["q_counts"], kw["n"], kw["s"], kw["splits"], Q=kw["Q"])


@pytest.mark.parametrize("case", error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call(tmvb, None, kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_shape_errors_through_the_abi(tmvb):
    """K = 0, Md = 0, Md = 2^31, 2^31 - 1 entries and NULL cannot be said with an array: the C call itself (no entry is read before these are judged)"""
    L = tmvb.lib()
    PD, P32, P64, PF = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    x = np.full(8, 0.5); ptr = np.array([0, 1], dtype=np.int64); t = np.zeros(8, dtype=np.int32); c = np.ones(8, dtype=np.int32)
    idx = np.zeros(8, dtype=np.int32); sc = np.zeros(8, dtype=np.float32); cnt = np.zeros(8, dtype=np.int32)
    a = [x.ctypes.data_as(PD), x.ctypes.data_as(PD), ptr.ctypes.data_as(P64), t.ctypes.data_as(P32), c.ctypes.data_as(P32), idx.ctypes.data_as(P32),
         sc.ctypes.data_as(PF), cnt.ctypes.data_as(P32)]

    def go(K, Md, p=a, Q=1):
        rc = L.tmvb_topic_search(None, K, 2, Md, p[0], p[1], 0.0, Q, p[2], p[3], p[4], 1, 0, p[5], p[6], p[7], None)
        return rc, L.tmvb_last_error().decode()

    for K, Md, msg in ((0, 2, "K = 0"), (-1, 2, "K = -1"), (2, 0, "Md, V and Q must be positive"), (2, -4, "Md, V and Q must be positive"),
                       (2, 2 ** 31, "2^31 or more")):
        rc, err = go(K, Md)
        assert rc == EINVAL and msg in err, (K, Md, rc, err)
    for hole in range(8):                                            # theta, beta, q_ptr, q_terms, q_counts, idx, score, count
        rc, err = go(2, 2, [None if q == hole else v for q, v in enumerate(a)])
        assert rc == EINVAL and "NULL argument" in err, (hole, rc, err)
    big = np.array([0, 100, 2 ** 31 - 1], dtype=np.int64)            # 2^31 - 1 entries: judged on q_ptr alone... after the per-query limit
    rc, err = go(2, 2, a[:2] + [big.ctypes.data_as(P64)] + a[3:], Q=2)
    assert rc == ESHAPE and "query 1 has" in err, (rc, err)


def test_the_entry_limit_is_judged_on_q_ptr_alone(tmvb):
    """2^31 - 1 entries in queries of legal length: TMVB_EINVAL before any entry is read (q_terms holds 8 ids, nothing more)"""
    L = tmvb.lib()
    Q = (2 ** 31 - 1 + 127) // 128
    ptr = np.minimum(np.arange(Q + 1, dtype=np.int64) * 128, 2 ** 31 - 1)
    assert ptr[-1] == 2 ** 31 - 1 and np.all(np.diff(ptr) >= 1)
    x = np.full(8, 0.5); t = np.zeros(8, dtype=np.int32); c = np.ones(8, dtype=np.int32)
    idx = np.zeros(8, dtype=np.int32); sc = np.zeros(8, dtype=np.float32); cnt = np.zeros(8, dtype=np.int32)
    P = lambda arr, ty: arr.ctypes.data_as(C.POINTER(ty))
    rc = L.tmvb_topic_search(None, 2, 2, 2, P(x, C.c_double), P(x, C.c_double), 0.0, Q, P(ptr, C.c_int64), P(t, C.c_int32), P(c, C.c_int32), 1, 0,
                             P(idx, C.c_int32), P(sc, C.c_float), P(cnt, C.c_int32), None)
    err = L.tmvb_last_error().decode()
    assert rc == EINVAL and "entries in one call" in err, (rc, err)


def test_valid_arguments_without_a_device_are_enodevice(tmvb):
    """No silent CPU path: the arguments pass, then a NULL context on a machine without a GPU is TMVB_ENODEVICE."""
    if tmvb.lib().tmvb_device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_search_gpu.py covers the live path")
    b = _base()
    ok_theta = b["theta"].copy(); ok_theta[2, 1] = 0.5000009          # inside the 1e-6 rule
    for kw in (b, dict(b, s=0.5, splits=4, n=64), dict(b, theta=ok_theta), dict(b, q_ptr=[0, 3], q_terms=[4, 4, 0], q_counts=[1, 7, 1])):
        rc, res = call(tmvb, None, kw)
        assert rc == ENODEVICE and "no HIP device" in res, (rc, res)
    m = tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3)
    with pytest.raises(tmvb.EngineError):
        tmvb.search(m, [[1, 2]], topn=2)


# ------------------------------------------------------------------------------------------------------------------ the Python mirror
def test_pack_queries_three_forms_merging_and_errors(tmvb):
    corp = tmvb.Corpus([tmvb.Document(terms=[1, 2, 3], counts=[1, 1, 1]), tmvb.Document(terms=[2, 4], counts=[2, 1])], vocab=["alpha", "beta", "gamma", "delta"])
    m = tmvb.LDA(corp, 2)
    assert m.corp.vocab == {1: "alpha", 2: "beta", 3: "gamma", 4: "delta"}
    ptr, terms, counts = tmvb.pack_queries(m, [["gamma", "alpha", "gamma"], [4, 2, 4, 4], {"beta": 3, 1: 2}, np.array([3])])
    assert ptr.tolist() == [0, 2, 4, 6, 7] and ptr.dtype == np.int64
    assert terms.tolist() == [2, 0, 3, 1, 1, 0, 2] and terms.dtype == np.int32          # 0-based, first-occurrence order
    assert counts.tolist() == [2, 1, 3, 1, 3, 2, 1] and counts.dtype == np.int32        # repeated terms merged by summing
    assert tmvb.pack_queries(m, [["alpha", "nope", "delta"]], skip_unknown=True)[1].tolist() == [0, 3]
    packed = tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3)                               # a PackedCorpus names its terms "1" .. "V"
    assert tmvb.pack_queries(packed, [["20", "1"]])[1].tolist() == [19, 0]
    for queries, msg in (([["alpha", "nope"]], "not in the model's vocabulary"), ([[]], "query 1 is empty"), ([["alpha"], {}], "query 2 is empty"),
                         ([["nope"]], "not in the model's vocabulary"), ([[0]], "term id 0 outside"), ([[5]], "term id 5 outside"), ([], "queries is empty"),
                         ("alpha", "must be a list of queries"), (["alpha"], "is a string"), ([{"alpha": 0}], "positive integer"),
                         ([{"alpha": 1.5}], "positive integer"), ([[1.0]], "vocabulary string or a 1-based integer id")):
        with pytest.raises(ValueError, match=msg):
            tmvb.pack_queries(m, queries)
    with pytest.raises(ValueError, match="query 1 is empty"):
        tmvb.pack_queries(m, [["nope"]], skip_unknown=True)
    big = tmvb.LDA(tmvb.syn_nsf(M=6, V=300, seed=1), 3)
    assert len(tmvb.pack_queries(big, [list(range(1, 129))])[1]) == 128
    with pytest.raises(ValueError, match="129 distinct terms"):
        tmvb.pack_queries(big, [list(range(1, 130))])


def test_mirror_errors_and_result(tmvb):
    m = tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3)
    with pytest.raises(tmvb.TopicModelError, match="CTPF"):
        tmvb.search(tmvb.CTPF(tmvb.syn_citeu(M=6, V=20, U=4, seed=1), 3), [[1]])
    with pytest.raises(tmvb.TopicModelError, match="needs an LDA"):
        tmvb.search(object(), [[1]])
    for topn in (0, 65, 2.5):
        with pytest.raises(ValueError, match="topn"):
            tmvb.search(m, [[1]], topn=topn)
    for s in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="laplace_smooth"):
            tmvb.search(m, [[1]], laplace_smooth=s)
    with pytest.raises(ValueError, match="query 1 is empty"):
        tmvb.search(m, [[]])
    with pytest.raises(tmvb.TopicModelError, match="same number of topics"):
        tmvb.search(m, [[1]], theta=np.full((4, 5), 0.25))
    r = tmvb.SearchResult([[4, 2, -1]], [[-6.0, -9.0, -np.inf]], [2], [3], {"splits": 1})
    assert r.idx.dtype == np.int32 and r.score.dtype == np.float32 and r.count.tolist() == [2] and r.info == {"splits": 1}
    assert r.loglik_per_token.tolist() == [[-2.0, -3.0, -np.inf]] and r.loglik_per_token.dtype == np.float64


# ------------------------------------------------------------------------------------------------------------------ frozen tolerances
def test_the_gpu_tolerances_are_frozen_from_their_measurement():
    """a tolerance is at least 1 x and at most 10 x the worst deviation measured on the MI355X -- and here never above the
    derivable cap (K + 3) 2^-24."""
    import test_search_gpu as g
    ev = json.load(open(os.path.join(ROOT, "profiles", "search_tolerances_measured.json")))["search.score_per_token"]
    assert sorted(int(k) for k in ev["measured"]) == sorted(g.TOL) == sorted(g.FLOAT_KS)
    for K, tol in g.TOL.items():
        measured = ev["measured"][str(K)]
        assert measured >= 0.0 and measured <= tol <= 10.0 * measured, (K, tol, measured)
        assert tol <= sr.cap_coeff(K), (K, tol, sr.cap_coeff(K))
