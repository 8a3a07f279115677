"""
The document map without a device (include/tmvb.h, "map documents in two dimensions"):

  * self-checks of tests/docmap_restatement.py: its gradient is the central finite difference of its own KL (M = 7); every row of p_cond sums to 1
    within 1e-15 n -- so every point carries 1 / M of the mass of P and P sums to 1 --; the achieved entropy is log u within 1e-12 on random distances;
    the blocked sum has the stated order; the fp32 update by hand; the Philox start against the library's own generator;
  * the wrapper's argument errors;
  * every TMVB_EINVAL / TMVB_ESHAPE case of both entry points from a NULL context (they are judged before the device), then TMVB_ENODEVICE on a
    machine without a GPU;
  * the tolerance literals of tests/test_docmap_gpu.py: at most 10 x their MI355X measurement (profiles/docmap_tolerances_measured.json) and, for the
    repulsion, below the caps of the error model;
  * the planted groups of the end-to-end GPU test through the restatement alone (M = 300 keeps it to seconds): every point's nearest 2-D neighbour is in
    its own group, purity 1.0 -- five groups, theta_d ~ Dirichlet(200 c_g + 0.05), c_g ~ Dirichlet(0.3), K = 12, as the issue states them: no further
    separation was needed;
  * header, structures, SOURCES, Makefile, Philox stage, Julia shim, mutant flag and kernel resource table.
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import docmap_restatement as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE, ENODEVICE = 1, 2, 7


def small(M=7, n=3, u=2.0, seed=1):
    theta = dr.planted_theta(M=M, K=4, groups=2, seed=seed)[0]
    idx, d2, count = dr.knn(theta, n)
    beta, p = dr.affinity(d2, count, u)
    return idx, d2, count, beta, p, dr.symmetrize(idx, p, count)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_gradient_is_the_finite_difference_of_the_kl():
    csr = small()[5]
    y = np.random.Generator(np.random.PCG64(0)).standard_normal((7, 2)).astype(np.float32)
    g = dr.gradient64(y, *csr)
    fd = np.zeros((7, 2))
    for i in range(7):
        for c in range(2):
            yp, ym = y.astype(np.float64), y.astype(np.float64)
            yp[i, c] += 1e-6
            ym[i, c] -= 1e-6
            fd[i, c] = (dr.kl64(yp, *csr) - dr.kl64(ym, *csr)) / 2e-6
    assert np.abs(fd - g).max() <= 1e-8 * max(1.0, np.abs(g).max())
    rep, z, _, _ = dr.repulsion64(y)
    att, _ = dr.attraction64(y, *csr)
    np.testing.assert_allclose(4.0 * (att - rep / (z.sum() - 7)), g, rtol=1e-13, atol=1e-16)


def test_rows_of_p_and_the_achieved_entropy():
    rng = np.random.Generator(np.random.PCG64(2))
    for n, u in ((5, 2.0), (64, 20.0), (63, 30.5)):
        M = 40
        d2 = rng.random((M, n)).astype(np.float32) * np.float32(rng.choice([1e-3, 1.0, 50.0]))
        count = np.full(M, n, dtype=np.int32)
        beta, p = dr.affinity(d2, count, u)
        assert np.all(np.abs(p.sum(axis=1) - 1.0) <= 1e-15 * n)
        for i in range(M):
            D = d2[i].astype(np.float64)
            assert abs(dr.row_entropy(D - D.min(), beta[i]) - np.log(u)) <= 1e-12
    idx, d2, count, beta, p, (row_ptr, col, val) = small(M=30, n=6, u=2.5)
    assert abs(float(val.astype(np.float64).sum()) - 1.0) <= len(val) * 2.0 ** -24
    i, j = dr.edges(row_ptr, col)
    dense = np.zeros((30, 30), dtype=np.float32)
    dense[i, j] = val
    assert np.array_equal(dense, dense.T) and np.all(np.diag(dense) == 0) and np.all(np.diff(row_ptr) >= 6)
    assert all(np.all(np.diff(col[row_ptr[r]:row_ptr[r + 1]]) > 0) for r in range(30))


def test_short_rows_are_uniform():
    d2 = np.array([[0.5, 0.1, 0.9], [0.3, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    beta, p = dr.affinity(d2, np.array([3, 2, 0]), 2.0)
    assert beta[1] == 0.0 and beta[2] == 0.0 and beta[0] > 0 and np.array_equal(p[1], [0.5, 0.5, 0.0]) and np.all(p[2] == 0)
    assert not dr.reachable(d2, np.array([3, 2, 0]), 2.0)[1:].any()


def test_blocked_sum_has_the_stated_order():
    v = np.zeros(2 * dr.RUN + 1)
    v[0], v[1:dr.RUN], v[dr.RUN] = 2.0 ** 53, 1.0, 2.0 ** 53
    assert dr.blocked(v) == 2.0 ** 54                                # block 0: 2^53 swallows every 1 that follows it
    v[dr.RUN + 1:] = 1.0
    assert dr.blocked(v) == 2.0 ** 54 and dr.blocked(v[::-1]) != float(np.sum(v))


def test_update_by_hand():
    g = np.array([[1.0, -1.0], [0.0, 2.0]], dtype=np.float32)
    y = np.array([[1.0, 1.0], [3.0, 5.0]], dtype=np.float32)
    vel = np.array([[-1.0, -1.0], [4.0, 0.0]], dtype=np.float32)
    gain = np.array([[1.0, 1.0], [0.012, 1.0]], dtype=np.float32)
    y1, v1, g1 = dr.update32(g, y, vel, gain, 0.5, 2.0, 0.01)
    f = np.float32
    assert np.array_equal(g1, np.array([[f(1) + f(0.2), f(0.8)], [f(0.01), f(0.8)]], dtype=np.float32)) and f(0.012) * f(0.8) < f(0.01)
    assert np.array_equal(v1, np.array([[f(-0.5) - f(2) * g1[0, 0], f(-0.5) + f(2) * f(0.8)], [f(2.0), -(f(2) * f(0.8)) * f(2)]], dtype=np.float32))
    raw = y + v1
    assert np.array_equal(y1, raw - raw.astype(np.float64).mean(axis=0).astype(np.float32))


def test_start_against_the_library_philox(tmvb):
    y = dr.init_y(1000, 2 ** 40 + 3)
    assert y.dtype == np.float32 and np.abs(y).max() <= 1e-4 and abs(float(y.mean())) < 1e-5 and len(np.unique(y)) > 1990
    assert np.array_equal(dr.init_y(10, 5), dr.init_y(1000, 5)[:10]) and not np.array_equal(dr.init_y(10, 5), dr.init_y(10, 6))
    # the generator itself: known-answer vectors of Philox4x32-10 (Random123's kat_vectors)
    assert [int(v) for v in dr.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in dr.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_the_planted_groups_separate_in_the_restatement_alone():
    theta, g = dr.planted_theta(M=300)
    idx, d2, count = dr.knn(theta, 64)
    _, p = dr.affinity(d2, count, 20.0)
    csr = dr.symmetrize(idx, p, count)
    y = dr.layout64(dr.pca_init(theta), *csr, 750, eta=50.0)[0]
    assert dr.purity(y, g) == 1.0


# ------------------------------------------------------------------------------------------------------------------ the wrapper
def test_wrapper_argument_errors(tmvb):
    theta = dr.planted_theta(M=12, K=4, groups=2)[0]
    for kw, exc, msg in ((dict(metric="dot"), ValueError, "metric"), (dict(n_neighbors=12), ValueError, "n_neighbors"), (dict(n_neighbors=1), ValueError, "n_neighbors"),
                         (dict(n_neighbors=65), ValueError, "n_neighbors"), (dict(perplexity=11.0), ValueError, "perplexity"), (dict(perplexity=0.5), ValueError, "perplexity"),
                         (dict(perplexity=float("nan")), ValueError, "perplexity"), (dict(iters=-1), ValueError, "iters"), (dict(check=-1), ValueError, "iters and check"),
                         (dict(init="spectral"), ValueError, "init"), (dict(init=np.zeros((3, 2))), tmvb.TopicModelError, "M x 2"), (dict(etaa=1.0), TypeError, "etaa"),
                         (dict(theta=np.ones(5)), tmvb.TopicModelError, "K x M"), (dict(theta=theta[:, :2]), tmvb.TopicModelError, "at least 3")):
        with pytest.raises(exc, match=msg):
            tmvb.map_docs(None, **dict(dict(theta=theta), **kw))
    with pytest.raises(tmvb.TopicModelError):
        tmvb.map_docs(object())
    y = tmvb.docmap.pca_init(theta, "hellinger")
    assert y.dtype == np.float32 and y.shape == (12, 2) and abs(float(y[:, 0].astype(np.float64).std()) - 1e-4) < 1e-9 and np.array_equal(y, dr.pca_init(theta))
    assert tmvb.docmap.default_eta(128804) == 128804 / 48 and tmvb.docmap.default_eta(600) == 50.0


# ------------------------------------------------------------------------------------------------------------------ argument errors of the ABI
def aff_base():
    idx, d2, count = small(M=6, n=3)[:3]
    return dict(idx=idx.copy(), d2=d2.copy(), count=count.copy(), perplexity=2.0, Mc=None, symmetric=True)


def _set(a, pos, v):
    a = a.copy()
    a[pos] = v
    return a


def affinity_error_cases():
    b = aff_base()
    return [
        ("M below 2", dict(b, idx=b["idx"][:1], d2=b["d2"][:1], count=b["count"][:1]), EINVAL, "M = 1"),
        ("n above 64", dict(b, idx=np.zeros((6, 65), dtype=np.int32), d2=np.zeros((6, 65), dtype=np.float32)), EINVAL, "n = 65"),
        ("perplexity below 1", dict(b, perplexity=0.99), EINVAL, "perplexity"),
        ("perplexity nan", dict(b, perplexity=float("nan")), EINVAL, "perplexity"),
        ("perplexity inf", dict(b, perplexity=float("inf")), EINVAL, "perplexity"),
        ("Mc not M", dict(b, Mc=7), EINVAL, "Mc = 7"),
        ("conditional Mc zero", dict(b, Mc=0, symmetric=False), EINVAL, "Mc = 0"),
        ("count above n", dict(b, count=_set(b["count"], 2, 4)), ESHAPE, "count = 4 outside [0, n] (row 2)"),
        ("count negative", dict(b, count=_set(b["count"], 0, -1)), ESHAPE, "count = -1"),
        ("index at M", dict(b, idx=_set(b["idx"], (1, 1), 6)), ESHAPE, "neighbour index 6 outside [0, Mc) (row 1)"),
        ("index negative", dict(b, idx=_set(b["idx"], (4, 0), -1)), ESHAPE, "neighbour index -1"),
        ("conditional index at Mc", dict(b, Mc=5, symmetric=False, idx=_set(b["idx"], (0, 0), 5)), ESHAPE, "neighbour index 5"),
        ("own neighbour", dict(b, idx=_set(b["idx"], (3, 2), 3)), ESHAPE, "among its own neighbours (row 3)"),
        ("index twice", dict(b, idx=_set(b["idx"], (5, 0), b["idx"][5, 1])), ESHAPE, "listed twice (row 5)"),
        ("negative distance", dict(b, d2=_set(b["d2"], (2, 1), -0.5)), ESHAPE, "negative or non-finite distance (row 2)"),
        ("nan distance", dict(b, d2=_set(b["d2"], (0, 0), np.nan)), ESHAPE, "negative or non-finite distance (row 0)"),
        ("inf distance", dict(b, d2=_set(b["d2"], (5, 2), np.inf)), ESHAPE, "negative or non-finite distance (row 5)"),
    ]


def lay_base():
    row_ptr, col, val = small(M=6, n=3)[5]
    return dict(M=6, row_ptr=row_ptr, col=col, val=val, iters=3, y=np.zeros((6, 2), dtype=np.float32))


def layout_error_cases():
    b = lay_base()
    bad_ptr = b["row_ptr"].copy()
    bad_ptr[3] = bad_ptr[2] - 1
    desc = b["col"].copy()
    desc[[0, 1]] = desc[[1, 0]]
    return [
        ("iters negative", dict(b, iters=-1), EINVAL, "iters = -1"),
        ("iters above 100000", dict(b, iters=100001), EINVAL, "iters = 100001"),
        ("iter0 negative", dict(b, iter0=-1), EINVAL, "iter0 = -1"),
        ("exag_iters negative", dict(b, exag_iters=-1), EINVAL, "must not be negative"),
        ("check negative", dict(b, check=-2), EINVAL, "must not be negative"),
        ("j_split negative", dict(b, j_split=-1), EINVAL, "must not be negative"),
        ("exaggeration below 1", dict(b, exaggeration=0.5), EINVAL, "exaggeration"),
        ("exaggeration nan", dict(b, exaggeration=float("nan")), EINVAL, "exaggeration"),
        ("eta zero", dict(b, eta=0.0), EINVAL, "eta"),
        ("eta inf", dict(b, eta=float("inf")), EINVAL, "eta"),
        ("momentum one", dict(b, momentum1=1.0), EINVAL, "momentum"),
        ("momentum negative", dict(b, momentum0=-0.1), EINVAL, "momentum"),
        ("min_gain zero", dict(b, min_gain=0.0), EINVAL, "min_gain"),
        ("min_grad_norm negative", dict(b, min_grad_norm=-1.0), EINVAL, "min_grad_norm"),
        ("seeded start after iteration 0", dict(b, y=None, iter0=5), EINVAL, "needs iter0 == 0"),
        ("row_ptr not from 0", dict(b, row_ptr=b["row_ptr"] + 1, col=np.concatenate([b["col"], [0]]), val=np.concatenate([b["val"], [0]])), ESHAPE, "row_ptr[0] != 0"),
        ("row_ptr descending", dict(b, row_ptr=bad_ptr), ESHAPE, "row_ptr not ascending or beyond 2^31 (row 2)"),
        ("column at M", dict(b, col=_set(b["col"], len(b["col"]) - 1, 6)), ESHAPE, "outside [0, M) or on the diagonal (row 5)"),
        ("diagonal", dict(b, col=_set(b["col"], 0, 0)), ESHAPE, "on the diagonal (row 0)"),
        ("columns descending", dict(b, col=desc), ESHAPE, "not strictly ascending (row 0)"),
        ("negative value", dict(b, val=_set(b["val"], 3, -1e-3)), ESHAPE, "negative or non-finite value"),
        ("nan value", dict(b, val=_set(b["val"], 3, np.nan)), ESHAPE, "negative or non-finite value"),
        ("nan state", dict(b, y=_set(b["y"], (2, 1), np.nan)), ESHAPE, "non-finite state (entry 5)"),
        ("inf gain", dict(b, gain=_set(np.ones((6, 2), dtype=np.float32), (0, 0), np.inf)), ESHAPE, "non-finite state (entry 0)"),
    ]


def call_layout(tmvb, ctx, kw):
    kw = dict(kw)
    return tmvb.map_layout_raw(ctx, kw.pop("M"), kw.pop("row_ptr"), kw.pop("col"), kw.pop("val"), kw.pop("iters"), **kw)


@pytest.mark.parametrize("case", affinity_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_affinity_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = tmvb.map_affinity_raw(None, **kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


@pytest.mark.parametrize("case", layout_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_layout_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call_layout(tmvb, None, kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_errors_that_only_the_abi_can_say(tmvb):
    """M beyond the range, 2 M n beyond 2^31, the NULL arguments and a short kl_cap: the C calls themselves (no entry is read before these are judged)"""
    L = tmvb.lib()
    PD, P32, P64, PF = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    i32, f32, f64, i64 = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.float32), np.zeros(64), np.zeros(64, dtype=np.int64)
    a = [i32.ctypes.data_as(P32), f32.ctypes.data_as(PF), i32.ctypes.data_as(P32), f64.ctypes.data_as(PD), f64.ctypes.data_as(PD), i64.ctypes.data_as(P64),
         i32.ctypes.data_as(P32), f32.ctypes.data_as(PF)]

    def aff(M, n, p=a, Mc=None):
        rc = L.tmvb_map_affinity(None, C.c_int64(M), C.c_int64(M if Mc is None else Mc), C.c_int32(n), p[0], p[1], p[2], C.c_double(2.0), p[3], p[4], p[5], p[6], p[7])
        return rc, L.tmvb_last_error().decode()

    for M, n, msg in ((1, 2, "M = 1"), (0, 2, "M = 0"), (-3, 2, "M = -3"), (2 ** 31, 2, "M = 2147483648"), (4, 0, "n = 0"), (4, -1, "n = -1"), (2 ** 30, 1, "2 M n")):
        rc, err = aff(M, n)
        assert rc == EINVAL and msg in err, (M, n, rc, err)
    for hole in range(8):                                                            # 5 .. 7 alone: only some of row_ptr, col, val
        rc, err = aff(4, 2, [None if q == hole else v for q, v in enumerate(a)])
        assert rc == EINVAL and "NULL argument" in err, (hole, rc, err)
    rc, err = aff(0, 2, a[:5] + [None, None, None], Mc=4)
    assert rc == EINVAL and "M = 0" in err

    P = tmvb.docmap.MapParams(4, 0, 250, 2, 0, 0, 0, 12.0, 0.0, 0.5, 0.8, 50.0, 0.01)
    b = [i64.ctypes.data_as(P64), i32.ctypes.data_as(P32), f32.ctypes.data_as(PF), C.pointer(P), f32.ctypes.data_as(PF), f32.ctypes.data_as(PF),
         f32.ctypes.data_as(PF), f64.ctypes.data_as(PD), i32.ctypes.data_as(P32)]

    def lay(M, p=b, cap=8):
        rc = L.tmvb_map_layout(None, C.c_int64(M), p[0], p[1], p[2], p[3], None, None, None, p[4], p[5], p[6], C.c_int32(cap), p[7], p[8], None, None, None, None, None)
        return rc, L.tmvb_last_error().decode()

    for M, msg in ((1, "M = 1"), (0, "M = 0"), (2 ** 31, "M = 2147483648")):
        rc, err = lay(M)
        assert rc == EINVAL and msg in err, (M, rc, err)
    for hole in range(9):
        rc, err = lay(4, [None if q == hole else v for q, v in enumerate(b)])
        assert rc == EINVAL and "NULL argument" in err, (hole, rc, err)
    rc, err = lay(4, cap=3)                                                           # iters / check + 2 = 4
    assert rc == EINVAL and "kl_cap = 3" in err


def test_valid_arguments_without_a_device_are_enodevice(tmvb):
    """No silent CPU path: the arguments pass, then a NULL context on a machine without a GPU is TMVB_ENODEVICE.  (With a GPU in sight the NULL
    context is served by it: tests/test_docmap_gpu.py covers the live path.)"""
    if tmvb.lib().tmvb_device_count() > 0:
        return
    rc, res = tmvb.map_affinity_raw(None, **aff_base())
    assert rc == ENODEVICE and "no HIP device" in res, (rc, res)
    rc, res = tmvb.map_affinity_raw(None, **dict(aff_base(), Mc=9, symmetric=False))
    assert rc == ENODEVICE and "no HIP device" in res, (rc, res)
    for kw in (lay_base(), dict(lay_base(), y=None, iters=0), dict(lay_base(), iter0=300, check=2, min_grad_norm=1e-7, j_split=3)):
        rc, res = call_layout(tmvb, None, kw)
        assert rc == ENODEVICE and "no HIP device" in res, (rc, res)
    with pytest.raises(tmvb.EngineError):
        tmvb.map_docs(None, theta=dr.planted_theta(M=12, K=4, groups=2)[0])


# ------------------------------------------------------------------------------------------------------------------ the repository's own records
def test_the_gpu_tolerances_are_frozen_from_their_measurement():
    """A tolerance is at least 1 x and at most 10 x the worst deviation measured on the MI355X; the repulsion's stay below the caps of the error model."""
    import test_docmap_gpu as g
    ev = json.load(open(os.path.join(ROOT, "profiles", "docmap_tolerances_measured.json")))
    tol = {"beta_rel": g.BETA_TOL, "rep_units": g.REP_TOL, "z_units": g.Z_TOL, "free_rel": g.FREE_TOL}
    assert sorted(ev["measured"]) == sorted(tol) == sorted(g.WORST)
    for k, t in tol.items():
        assert 0 < ev["measured"][k] <= t <= 10 * ev["measured"][k], (k, ev["measured"][k], t)
    assert g.REP_TOL <= dr.RUN + 24 == ev["cap"]["rep_units"] and g.Z_TOL <= dr.RUN + 8 == ev["cap"]["z_units"]
    assert dr.REP_CAP == (dr.RUN + 24) * 2.0 ** -24 and dr.Z_CAP == (dr.RUN + 8) * 2.0 ** -24
    assert 14 + (dr.RUN - 1) <= dr.RUN + 24 and 6 + (dr.RUN - 1) <= dr.RUN + 8      # the per-term errors and the run's adds fit the caps


def test_header_structures_sources_and_exports(tmvb):
    D = tmvb.docmap
    for f in ("tmvb_map_affinity", "tmvb_map_layout"):
        assert f in tmvb.exported_symbols() and hasattr(C.CDLL(tmvb.LIB_PATH), f)
    assert tmvb.lib().tmvb_abi_version() == 2                        # new functions do not break an existing caller
    for name in ("map_docs", "map_affinity_raw", "map_layout_raw", "DocMap"):
        assert name in tmvb.__all__ and getattr(tmvb, name) is not None
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    define = lambda n: int(re.search(r"#define " + n + r"\s+(\d+)", hdr).group(1))
    assert define("TMVB_MAP_BISECT") == D.BISECT == dr.BISECT and define("TMVB_MAP_RUN") == D.RUN == dr.RUN and define("TMVB_MAP_SEG") == D.SEG == dr.SEG
    assert define("TMVB_MAP_SLOTS") == D.SLOTS == dr.SLOTS and define("TMVB_NB_TOPN_MAX") == 64
    for cname, S, size in (("tmvb_map_params_t", D.MapParams, 64), ("tmvb_map_info_t", D.MapInfo, 48)):
        fields = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", hdr).group(1)
        assert re.findall(r"\b(\w+)\s*[;,]", fields) == [f[0] for f in S._fields_] and C.sizeof(S) == size
    assert "tmvb_docmap.hip" in tmvb._lib.SOURCES and "$(CSRC)/tmvb_docmap.hip" in open(os.path.join(ROOT, "Makefile")).read()
    csrc = os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc")
    assert re.search(r"TMVB_RNG_MAP = %d\b" % dr.RNG_MAP, open(os.path.join(csrc, "tmvb_philox.h")).read()) and D.RNG_MAP == dr.RNG_MAP
    assert "TMVB_MUTANT_MAP_Z_SELF" in open(os.path.join(csrc, "tmvb_internal.h")).read()
    assert "tmvb_docmap.hip -DTMVB_MUTANT_MAP_Z_SELF=1" in open(os.path.join(ROOT, "tools", "build_mutants.sh")).read()
    head = open(os.path.join(csrc, "tmvb_call.h")).read().split("#pragma once")[0]
    assert "tmvb_map_affinity" in head and "tmvb_map_layout" in head
    src = open(os.path.join(csrc, "tmvb_docmap.hip")).read()
    assert not re.findall(r"\batomic\w+\(", src) and "unsafeAtomic" not in src        # fixed-order sums only


def test_julia_shim_binds_the_entry_points():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    for s in (":tmvb_map_affinity", ":tmvb_map_layout", "function map_docs(", "mutable struct TmvbMapParams", "mutable struct TmvbMapInfo"):
        assert s in src, s
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    for cname, jname in (("tmvb_map_params_t", "TmvbMapParams"), ("tmvb_map_info_t", "TmvbMapInfo")):
        names = re.findall(r"\b(\w+)\s*[;,]", re.search(r"typedef struct \{([^}]*)\} " + cname + ";", hdr).group(1))
        body = src[src.index("mutable struct " + jname):]
        body = body[:body.index("\nend")]
        assert re.findall(r"(\w+)::", body) == names, jname


def test_the_kernels_are_in_the_resource_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr_
    names = ("map_repulse_kernel", "map_finish_kernel", "map_attract_kernel<", "map_update_kernel", "map_affinity_kernel")
    assert all(kr_.BENCHED.get(k) == 0 for k in names)
