"""
Clustering documents in topic space (tmvb_topic_kmeans, include/tmvb.h), the part that needs no GPU:

  * tests/kmeans_restatement.py against hand-worked cases: the uniforms against the library's own Philox, the assignment rule with ties and a
    duplicate centroid, the blocked sum against a case where the order shows, the fixed-order mean, k-means++ on a case small enough to walk by
    hand and on identical documents, the fp32 loop against the fp64 loop;
  * every argument error comes back with its status and message from a NULL context (they are judged before the device), valid arguments
    without a device give TMVB_ENODEVICE;
  * ClusterResult's arithmetic: profiles, distance, representatives;
  * the floating inputs of the free-running GPU comparison are ADMISSIBLE by the restatement alone: every iteration of the fp64 loop leaves a gap of
    at least 8 cap(K) between every document's best and second-best score, the loop runs at least 4 iterations and labels still move after the
    first; the fp32 restatement of the contract reaches the same labels in the same number of iterations;
  * the header, the structure, SOURCES, the Philox stage, the Julia shim, the mutant's flag, and the tolerance literals of the GPU test against
    their recorded MI355X measurement (profiles/kmeans_tolerances_measured.json) and against cap(K).
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
import kmeans_restatement as kr  # noqa: E402

# the mirror module of the feature: a tree without it fails here, at import
CLUSTER = sys.modules[tmvb_amd.pkg.__name__ + ".cluster"]
EUCLID, HELLINGER, COSINE = CLUSTER.EUCLID, CLUSTER.HELLINGER, CLUSTER.COSINE
EINVAL, ESHAPE, ENODEVICE = 1, 2, 7


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_uniforms_against_the_library_philox(tmvb):
    L = tmvb.lib()
    P = C.POINTER(C.c_uint32)
    for seed in (0, 9, 2 ** 40 + 3):
        u = kr.uniforms(seed, 5)
        for j in range(5):
            c = np.array([j, 0, kr.RNG_KMEANS, 0], dtype=np.uint32)
            k = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
            out = np.zeros(4, dtype=np.uint32)
            assert L.tmvb_philox4x32_10(c.ctypes.data_as(P), k.ctypes.data_as(P), out.ctypes.data_as(P)) == 0
            assert u[j] == float(((int(out[0]) << 32) | int(out[1])) >> 11) / 2.0 ** 53 and 0.0 <= u[j] < 1.0


def test_assignment_rule_by_hand():
    F = np.array([[1, 0], [0, 1], [1, 1], [3, 3], [0, 0]], dtype=np.float32)
    Cf = np.array([[1, 0], [0, 1], [2, 2], [1, 0]], dtype=np.float32)                # the last repeats the first; b = -0.5, -0.5, -4, -0.5
    label, dist2, count, J, s = kr.assign32(F, Cf)
    assert s.tolist() == [[0.5, -0.5, -2, 0.5], [-0.5, 0.5, -2, -0.5], [0.5, 0.5, 0, 0.5], [2.5, 2.5, 8, 2.5], [-0.5, -0.5, -4, -0.5]]
    assert label.tolist() == [0, 1, 0, 2, 0]                                         # the lowest c on equal s
    assert dist2.tolist() == [0, 0, 1, 2, 1] and count.tolist() == [3, 1, 1, 0] and J == 4.0
    assert kr.assign32(F, Cf, no_bias=True)[0].tolist() == [2, 2, 2, 2, 0]           # the dot product alone: what the mutant selects


def test_blocked_sum_has_the_stated_order():
    v = np.zeros(2 * kr.RUN + 1)
    v[0], v[1:kr.RUN], v[kr.RUN] = 2.0 ** 53, 1.0, 2.0 ** 53
    assert kr.blocked_sum(v) == 2.0 ** 54                            # block 0: 2^53 swallows every 1 that follows it
    w = np.random.Generator(np.random.PCG64(1)).lognormal(0.0, 12.0, size=3 * kr.RUN + 17)
    tot = 0.0
    for i in range(0, len(w), kr.RUN):
        blk = 0.0
        for a in w[i:i + kr.RUN]:
            blk += float(a)
        tot += blk
    assert kr.blocked_sum(w) == tot and tot != float(np.cumsum(w)[-1])                # the order shows: one sequential sum gives other bits
    assert kr.blocked_sum(np.arange(1000.0)) == 499500.0 and kr.blocked_sum([]) == 0.0


def test_fixed_order_mean_by_hand():
    F = np.array([[1, 2], [3, 4], [5, 9], [0, 0]], dtype=np.float32)
    old = np.array([[9, 9], [8, 8], [7, 7]], dtype=np.float32)
    new = kr.update32(F, [0, 2, 0, 2], old, EUCLID)
    assert new.tolist() == [[3, 5.5], [8, 8], [1.5, 2]]                              # the empty cluster keeps its centroid
    cos = kr.update32(F[:3], [0, 2, 0], old, COSINE)
    assert np.allclose(cos[0], np.array([6, 11]) / np.sqrt(157.0), rtol=1e-7, atol=0) and cos[1].tolist() == [8, 8]
    assert np.array_equal(cos[2], np.array([0.6, 0.8], dtype=np.float32))
    big = np.ones((2 * kr.RUN + 3, 1), dtype=np.float32)
    assert kr.update32(big, np.zeros(len(big), dtype=int), np.zeros((1, 1), dtype=np.float32), EUCLID).tolist() == [[1.0]]


def test_seeding_by_hand():
    F = np.array([[0.0], [1.0], [3.0], [3.0]], dtype=np.float32)
    for seed in range(6):
        u = kr.uniforms(seed, 3)
        first = int(np.floor(u[0] * 4))
        picks = [first]
        for j in (1, 2):
            m = np.min([(F[:, 0].astype(float) - float(F[p, 0])) ** 2 for p in picks], axis=0)
            cum = np.cumsum(m)
            hit = np.flatnonzero(cum > u[j] * cum[-1])
            picks.append(int(hit[0]) if cum[-1] > 0 and len(hit) else min(set(range(4)) - set(picks)))
        assert kr.seeding(F, 3, seed).tolist() == picks and len(set(picks)) == 3
    same = np.ones((5, 2), dtype=np.float32)
    first = int(np.floor(kr.uniforms(1, 1)[0] * 5))
    assert kr.seeding(same, 4, 1).tolist() == [first] + [d for d in range(5) if d != first][:3]       # total == 0: the lowest id not yet chosen


def test_cosine_norm_in_the_device_order_is_the_norm():
    x = kr.dirichlet_cols(130, 7, 0.5, 3).T
    assert np.allclose(kr.cosine_norm_device_order(x), np.sqrt((x * x).sum(axis=1)), rtol=1e-15, atol=0)
    assert np.array_equal(kr.cosine_norm_device_order(x[:, :1]), np.abs(x[:, 0]))


# ------------------------------------------------------------------------------------------------------------------ admissible inputs
def test_the_free_running_inputs_are_admissible():
    import test_kmeans_gpu as g
    assert [c[:3] for c in g.FREE] == [(3, 257, 4), (50, 700, 7), (65, 300, 6), (130, 260, 5)]
    for K, M, Cn, G, gs in g.FREE:
        assert Cn > G
        x = g.free_input(K, M, G, gs)
        F32, F64 = kr.features32(x, HELLINGER), kr.features64(x, HELLINGER)
        seeds = kr.seeding(F32, Cn, gs)
        ref = kr.lloyd64(F64, F32[seeds].astype(np.float64), HELLINGER)
        assert ref["stop"] == 1 and ref["iters"] >= 4 and ref["gaps"].min() >= 8 * kr.cap(K), (K, ref["iters"], ref["gaps"].min() / kr.cap(K))
        assert any(not np.array_equal(ref["labels"][t], ref["labels"][t - 1]) for t in range(2, len(ref["labels"])))      # members still change after iteration 1
        r32 = kr.lloyd32(F32, F32[seeds], HELLINGER)
        assert r32["iters"] == ref["iters"] and r32["stop"] == 1 and np.array_equal(r32["label"], ref["label"])
        assert np.all(np.abs(r32["centroids"] - ref["centroids"]) <= 2.0 ** -23)
        assert np.all(np.abs(r32["inertia"] - ref["inertia"]) <= 2 * M * kr.cap(K))


# ------------------------------------------------------------------------------------------------------------------ argument errors
def _dist(cols):
    return np.asarray(cols, dtype=np.float64).T


def _base():
    return dict(K=3, metric=EUCLID, x=np.arange(15, dtype=np.float64).reshape(3, 5), C=2, init=None, seed=0, max_iter=10, tol=0.0)


def error_cases():
    b = _base()
    p = _dist([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    return [
        ("K above 1024", dict(b, K=1025, x=np.ones((1025, 2))), EINVAL, "K = 1025"),
        ("C zero", dict(b, C=0), EINVAL, "C = 0"),
        ("C above M", dict(b, C=6), EINVAL, "C = 6"),
        ("C above the cap", dict(b, C=1025, x=np.ones((3, 1030))), EINVAL, "C = 1025"),
        ("max_iter negative", dict(b, max_iter=-1), EINVAL, "max_iter = -1"),
        ("max_iter above 10000", dict(b, max_iter=10001), EINVAL, "max_iter = 10001"),
        ("tol negative", dict(b, tol=-1e-3), EINVAL, "tol must be"),
        ("tol nan", dict(b, tol=float("nan")), EINVAL, "tol must be"),
        ("tol inf", dict(b, tol=float("inf")), EINVAL, "tol must be"),
        ("unknown metric", dict(b, metric=3), EINVAL, "unknown metric 3"),
        ("negative metric", dict(b, metric=-1), EINVAL, "unknown metric -1"),
        ("nan in x", dict(b, x=np.where(np.arange(15).reshape(3, 5) == 7, np.nan, 1.0)), ESHAPE, "non-finite entry (row 2)"),
        ("inf in init", dict(b, init=np.array([[1.0, 0.0], [np.inf, 0.0], [0.0, 1.0]])), ESHAPE, "non-finite entry (init centroid 0)"),
        ("hellinger negative entry", dict(b, metric=HELLINGER, x=_dist([[0.5, 0.5, 0.0], [1.5, -0.5, 0.0]])), ESHAPE, "negative entry (row 1)"),
        ("hellinger sum off by 2e-6", dict(b, metric=HELLINGER, x=_dist([[0.5, 0.25, 0.25], [0.5, 0.25, 0.250002]])), ESHAPE, "not a probability vector (row 1)"),
        ("hellinger negative init", dict(b, metric=HELLINGER, x=p, init=np.array([[1.0, 0.5], [0.0, -0.5], [0.0, 0.5]])), ESHAPE, "negative entry (init centroid 1)"),
        ("cosine negative entry", dict(b, metric=COSINE, x=_dist([[1.0, 2.0, 3.0], [1.0, -2.0, 3.0]])), ESHAPE, "negative entry (row 1)"),
        ("cosine zero row", dict(b, metric=COSINE, x=_dist([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])), ESHAPE, "all-zero row (row 0)"),
        ("cosine zero init", dict(b, metric=COSINE, x=p, init=np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0]])), ESHAPE, "all-zero row (init centroid 1)"),
    ]


def call(tmvb, ctx, kw):
    return tmvb.kmeans_raw(ctx, kw["K"], kw["metric"], kw["x"], kw["C"], kw["init"], kw["seed"], kw["max_iter"], kw["tol"])


@pytest.mark.parametrize("case", error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call(tmvb, None, kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_shape_errors_through_the_abi(tmvb):
    """K = 0, M = 0, M = 2^31 and the NULL arguments cannot be said with an array: the C call itself (no entry is read before these are judged)"""
    L = tmvb.lib()
    PD, P32, P64, PF = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    x = np.ones(8); lab = np.zeros(8, dtype=np.int32); cen = np.zeros(8); cnt = np.zeros(8, dtype=np.int64); d2 = np.zeros(8, dtype=np.float32)
    J = np.zeros(8); sd = np.zeros(8, dtype=np.int32)
    a = [x.ctypes.data_as(PD), lab.ctypes.data_as(P32), cen.ctypes.data_as(PD), cnt.ctypes.data_as(P64), d2.ctypes.data_as(PF), J.ctypes.data_as(PD),
         sd.ctypes.data_as(P32)]

    def go(K, M, p=a):
        rc = L.tmvb_topic_kmeans(None, C.c_int32(K), C.c_int32(EUCLID), C.c_int64(M), p[0], C.c_int32(2), None, C.c_int64(0), C.c_int32(3), C.c_double(0.0),
                                 p[1], p[2], p[3], p[4], p[5], p[6], None)
        return rc, L.tmvb_last_error().decode()

    for K, M, msg in ((0, 2, "K = 0"), (-1, 2, "K = -1"), (2, 0, "M = 0"), (2, -4, "M = -4"), (2, 2 ** 31, "M = 2147483648")):
        rc, err = go(K, M)
        assert rc == EINVAL and msg in err, (K, M, rc, err)
    for hole in range(7):
        rc, err = go(2, 4, [None if q == hole else v for q, v in enumerate(a)])
        assert rc == EINVAL and "NULL argument" in err, (hole, rc, err)


def test_valid_arguments_without_a_device_are_enodevice(tmvb):
    """No silent CPU path: the arguments pass, then a NULL context on a machine without a GPU is TMVB_ENODEVICE."""
    if tmvb.lib().tmvb_device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_kmeans_gpu.py covers the live path")
    p = _dist([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    for kw in (_base(), dict(_base(), metric=HELLINGER, x=p, C=3, max_iter=0), dict(_base(), metric=COSINE, x=p, init=np.sqrt(p[:, :2]), tol=1e-4),
               dict(_base(), x=-np.arange(15.0).reshape(3, 5), init=-np.ones((3, 2)))):
        rc, res = call(tmvb, None, kw)
        assert rc == ENODEVICE and "no HIP device" in res, (rc, res)
    m = tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3)
    with pytest.raises(tmvb.EngineError):
        tmvb.cluster_docs(m, 2)


# ------------------------------------------------------------------------------------------------------------------ the Python mirror
def test_cluster_result_arithmetic(tmvb):
    labels = [1, 0, 1, 1, 0, 1]
    d2 = np.array([0.5, 0.02, 0.125, 0.125, 0.0, 2.0], dtype=np.float32)
    cen = np.array([[0.6, 0.0], [0.8, 1.0]])
    h = tmvb.ClusterResult(labels, cen, [2, 4], d2, [3.0, 2.77], "hellinger", iters=1, stop=1)
    assert np.allclose(h.profiles, [[0.36, 0.0], [0.64, 1.0]], rtol=1e-15) and h.distance[0] == 0.5 and h.distance[4] == 0.0 and h.distance[5] == 1.0
    c = tmvb.ClusterResult(labels, cen, [2, 4], d2, [3.0], "cosine")
    assert np.allclose(c.profiles, [[0.6 / 1.4, 0.0], [0.8 / 1.4, 1.0]], rtol=1e-15) and c.distance[0] == 0.25 and c.distance.dtype == np.float64
    e = tmvb.ClusterResult(labels, cen, [2, 4], d2, [3.0], "euclid")
    assert e.distance[0] == np.sqrt(0.5) and np.array_equal(e.profiles, c.profiles)
    assert h.labels.dtype == np.int32 and h.counts.dtype == np.int64 and h.dist2.dtype == np.float32 and np.all(h.seeds == -1)
    reps = h.representatives(3)
    assert [r.tolist() for r in reps] == [[4, 1], [2, 3, 0]]                          # nearest first; the tie of 2 and 3 goes to the lower id
    assert [r.tolist() for r in h.representatives(1)] == [[4], [2]]
    empty = tmvb.ClusterResult([0, 0], np.ones((2, 3)), [2, 0, 0], np.zeros(2, dtype=np.float32), [0.0], "euclid").representatives(2)
    assert [r.tolist() for r in empty] == [[0, 1], [], []]
    with pytest.raises(ValueError, match="n must be"):
        h.representatives(0)
    with pytest.raises(ValueError, match="metric"):
        tmvb.ClusterResult(labels, cen, [2, 4], d2, [3.0], "manhattan")


def test_mirror_errors(tmvb):
    m = tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3)
    with pytest.raises(ValueError, match="metric"):
        tmvb.cluster_docs(m, 2, metric="dot")
    for k in (0, 1025, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            tmvb.cluster_docs(m, k)
    with pytest.raises(tmvb.CorpusError, match="more clusters than documents"):
        tmvb.cluster_docs(m, 7)
    with pytest.raises(ValueError, match="init must be"):
        tmvb.cluster_docs(m, 2, init="random")
    with pytest.raises(tmvb.TopicModelError, match="K x k"):
        tmvb.cluster_docs(m, 2, init=np.ones((3, 3)))
    other = tmvb.ClusterResult([0], np.ones((3, 2)), [1, 0], np.zeros(1, dtype=np.float32), [0.0], "cosine")
    with pytest.raises(tmvb.TopicModelError, match="another metric"):
        tmvb.cluster_docs(m, 2, init=other)
    with pytest.raises(tmvb.TopicModelError):
        tmvb.cluster_docs(object(), 2)


# ------------------------------------------------------------------------------------------------------------------ static checks
def test_header_structure_sources_and_exports(tmvb):
    assert "tmvb_topic_kmeans" in tmvb.exported_symbols() and hasattr(C.CDLL(tmvb.LIB_PATH), "tmvb_topic_kmeans")
    assert tmvb.lib().tmvb_abi_version() == 2                        # a new function does not break an existing caller
    for name in ("cluster_docs", "kmeans_raw", "ClusterResult"):
        assert name in tmvb.__all__ and getattr(tmvb, name) is not None
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    define = lambda n: int(re.search(r"#define " + n + r"\s+(\d+)", hdr).group(1))
    assert (define("TMVB_KM_EUCLID"), define("TMVB_KM_HELLINGER"), define("TMVB_KM_COSINE")) == (EUCLID, HELLINGER, COSINE) == (0, 1, 2)
    assert define("TMVB_KM_CMAX") == CLUSTER.CMAX == 1024 and define("TMVB_KM_RUN") == CLUSTER.RUN == kr.RUN == 256
    fields = re.search(r"typedef struct \{([^}]*)\} tmvb_kmeans_info_t;", hdr).group(1)
    assert re.findall(r"\b(\w+)\s*[;,]", fields) == [f[0] for f in CLUSTER.KMeansInfo._fields_]
    assert C.sizeof(CLUSTER.KMeansInfo) == 40
    assert "tmvb_kmeans.hip" in tmvb._lib.SOURCES
    csrc = os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc")
    assert re.search(r"TMVB_RNG_KMEANS = %d\b" % kr.RNG_KMEANS, open(os.path.join(csrc, "tmvb_philox.h")).read())
    assert "TMVB_MUTANT_KM_NO_BIAS" in open(os.path.join(csrc, "tmvb_internal.h")).read()
    assert "tmvb_kmeans.hip -DTMVB_MUTANT_KM_NO_BIAS=1" in open(os.path.join(ROOT, "tools", "build_mutants.sh")).read()
    assert "tmvb_topic_kmeans" in open(os.path.join(csrc, "tmvb_call.h")).read().split("#pragma once")[0]
    src = open(os.path.join(csrc, "tmvb_kmeans.hip")).read()
    assert '#include "tmvb_nbtile.h"' in src and "nb_tile_scores(" in src
    atomics = re.findall(r"\batomic\w+\(([^,]+),", src)                # integer counters only: the LDS bins, the histogram, the changed-label count
    assert sorted(atomics) == ["&count[u]", "&hist[i]", "changed"] and "atomicAdd(float" not in src and "unsafeAtomic" not in src


def test_julia_shim_binds_the_entry_point():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    for s in (":tmvb_topic_kmeans", "function kmeans(", "mutable struct TmvbKMeansInfo"):
        assert s in src, s
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    names = re.findall(r"\b(\w+)\s*[;,]", re.search(r"typedef struct \{([^}]*)\} tmvb_kmeans_info_t;", hdr).group(1))
    body = src[src.index("mutable struct TmvbKMeansInfo"):]
    body = body[:body.index("TmvbKMeansInfo() =")]
    assert re.findall(r"(\w+)::", body) == names


def test_the_kernels_are_in_the_resource_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr_
    names = ("km_feature_kernel", "km_norm_kernel", "km_assign_kernel", "km_run_sum_kernel", "km_finalize_kernel", "km_seed_dist_kernel", "km_seed_pick_kernel")
    assert all(kr_.BENCHED.get(k) == 0 for k in names)
    lib = os.path.join(ROOT, "topicmodelsvb.jl_amd", "libtmvb_hip.so")
    if not (os.path.exists(lib) and os.path.exists(kr_.READELF)):
        pytest.skip("needs the built library and llvm-readelf")
    rows = [r for r in kr_.kernels(lib) if r["demangled"].startswith(names)]
    assert len(rows) == len(names) and all(r["scratch"] == 0 and r["vgpr_spills"] == 0 for r in rows), rows


def test_the_gpu_tolerances_are_frozen_from_their_measurement():
    """a tolerance is at least 1 x and at most 10 x the worst deviation measured on the MI355X -- and here never above cap(K)."""
    import test_kmeans_gpu as g
    ev = json.load(open(os.path.join(ROOT, "profiles", "kmeans_tolerances_measured.json")))["kmeans.score_abs"]
    assert sorted(int(k) for k in ev["measured"]) == sorted(g.TOL) == sorted(g.FLOAT_KS)
    for K, tol in g.TOL.items():
        worst = ev["measured"][str(K)]
        assert worst <= tol <= max(10 * worst, 0.0) and tol <= kr.cap(K), (K, worst, tol, kr.cap(K))
        assert ev["cap"][str(K)] == kr.cap(K)
