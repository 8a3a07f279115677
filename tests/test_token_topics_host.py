"""
CPU tests of the word-topic assignments (include/tmvb.h: tmvb_token_topics, tmvb_digamma_f64; topicmodelsvb.jl_amd/token_topics.py):

  * tests/token_topics_restatement.py equals the NumPy oracle's update_phi on a golden fixture;
  * every argument error of tmvb_token_topics is TMVB_EINVAL and comes before the device, a NULL context without a device is TMVB_ENODEVICE;
  * tmvb_digamma_f64 against mpmath;
  * token_factors per family against the formulas of update_phi! on the golden fixtures; the filtered models raise;
  * the tolerance literals of the GPU module against their recorded MI355X measurement (profiles/token_topics_tolerances_measured.json) and the cap;
  * the new translation unit takes its device memory and events from tmvb_call.
"""
import json
import os
import re
import types

import numpy as np
import pytest

import token_topics_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE = 1, 7


def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


# ------------------------------------------------------------------------------------------------------------------ restatement
def test_restatement_equals_the_oracles_update_phi():
    from oracle import oracle_np as onp
    g = load("lda_m40_v60_k7")
    K, V, ptr = int(g["K"]), int(g["V"]), g["doc_ptr"]
    docs = [(g["terms"][ptr[d]:ptr[d + 1]], g["counts"][ptr[d]:ptr[d + 1]]) for d in range(len(ptr) - 1)]
    o = onp.LDA(docs, V, K, g["beta"])
    r = tr.responsibilities(np.exp(g["Elogtheta"]), g["beta"], ptr, g["terms"], None, tr.EPSILON, rounded=False)
    for d in range(len(docs)):
        o.Elogtheta[d] = g["Elogtheta"][:, d].copy()
        o.update_phi(d)
        assert o.phi.shape == (K, ptr[d + 1] - ptr[d])
        assert np.allclose(r[ptr[d]:ptr[d + 1]].T, o.phi, rtol=1e-13, atol=0)
    ref = tr.restate(np.exp(g["Elogtheta"]), g["beta"], ptr, g["terms"], g["counts"], [3, 3, 0], tr.EPSILON, 8)
    assert ref["top_idx"].shape == (2 * (ptr[4] - ptr[3]) + ptr[1], 8) and np.all(ref["top_idx"][:, 7] == -1) and np.all(ref["top_r"][:, 7] == 0)
    assert np.array_equal(ref["hard"][0], ref["hard"][1]) and ref["hard"][2].sum() == g["counts"][:ptr[1]].sum()
    assert tr.cap(50) == 62 * 2.0 ** -24


def test_top_t_breaks_ties_towards_the_lower_topic():
    r = np.array([[0.25, 0.5, 0.25, 0.0], [0.1, 0.1, 0.4, 0.4]], dtype=np.float32)
    idx, val = tr.top_t(r, 3)
    assert idx.tolist() == [[1, 0, 2], [2, 3, 0]] and val.tolist() == [[0.5, 0.25, 0.25], [np.float32(0.4), np.float32(0.4), np.float32(0.1)]]


# ------------------------------------------------------------------------------------------------------------------ argument errors
@pytest.fixture(scope="module")
def small(tmvb):
    K, M, V = 3, 4, 6
    pc = types.SimpleNamespace(doc_ptr=np.array([0, 2, 2, 5, 6]), terms=np.array([0, 5, 1, 2, 3, 4]), counts=np.array([1, 2, 1, 1, 3, 1]))
    return K, V, np.ones((K, M)), np.ones((K, V)), pc


def test_the_symbols_are_new(tmvb):
    L = tmvb.lib()
    assert hasattr(L, "tmvb_token_topics") and hasattr(L, "tmvb_digamma_f64")
    assert {"tmvb_token_topics", "tmvb_digamma_f64"} <= set(tmvb.exported_symbols())
    assert tmvb.token_topics_raw is not None and tmvb.phi is not None and tmvb.TokenTopics is not None


def bad(pc, **kw):
    d = dict(doc_ptr=pc.doc_ptr.copy(), terms=pc.terms.copy(), counts=pc.counts.copy())
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_argument_errors_come_before_the_device(tmvb, small):
    K, V, A, B, pc = small
    raw = lambda *a, **kw: tmvb.token_topics_raw(None, *a, **kw)           # a NULL context: whatever passes the checks ends in ENODEVICE or EINVAL(ctx)
    last = ENODEVICE if tmvb.lib().tmvb_device_count() < 1 else EINVAL
    cases = {
        "K = 0": raw(0, V, np.ones((0, 4)), np.ones((0, V)), pc),
        "K = 1025": raw(1025, V, np.ones((1025, 4)), np.ones((1025, V)), pc),
        "t = 0": raw(K, V, A, B, pc, top=0),
        "t = 9": raw(K, V, A, B, pc, top=9),
        "eps below 2^-100": raw(K, V, A, B, pc, eps=2.0 ** -101),
        "eps = 0": raw(K, V, A, B, pc, eps=0.0),
        "eps above 1": raw(K, V, A, B, pc, eps=1.5),
        "eps NaN": raw(K, V, A, B, pc, eps=float("nan")),
        "doc id = M": raw(K, V, A, B, pc, docs=[0, 4]),
        "doc id < 0": raw(K, V, A, B, pc, docs=[-1]),
        "term = V": raw(K, V, A, B, bad(pc, terms=np.array([0, 5, 1, 2, 3, 6]))),
        "term < 0": raw(K, V, A, B, bad(pc, terms=np.array([0, 5, -1, 2, 3, 4]))),
        "count = 0": raw(K, V, A, B, bad(pc, counts=np.array([1, 2, 0, 1, 3, 1]))),
        "doc_ptr decreases": raw(K, V, A, B, bad(pc, doc_ptr=np.array([0, 2, 1, 5, 6]))),
        "doc_ptr starts at 1": raw(K, V, A, B, bad(pc, doc_ptr=np.array([1, 2, 2, 5, 6]))),
        "negative A": raw(K, V, np.where(np.arange(12).reshape(3, 4) == 7, -1e-300, A), B, pc),
        "NaN A": raw(K, V, np.where(np.arange(12).reshape(3, 4) == 0, np.nan, A), B, pc),
        "negative B": raw(K, V, A, np.where(np.arange(18).reshape(3, 6) == 17, -1.0, B), pc),
        "NaN B": raw(K, V, A, np.where(np.arange(18).reshape(3, 6) == 4, np.nan, B), pc),
        "infinite B": raw(K, V, A, np.where(np.arange(18).reshape(3, 6) == 4, np.inf, B), pc),
        "every output NULL": raw(K, V, A, B, pc, phi=False, hard=False, select=False),
        "max_chunk_entries < 0": raw(K, V, A, B, pc, max_chunk_entries=-1),
        "A of the wrong shape": raw(K, V, np.ones((K, 5)), B, pc),
    }
    for name, (rc, msg) in cases.items():
        assert rc == EINVAL and isinstance(msg, str) and msg, (name, rc, msg)
        assert "ctx is NULL" not in msg, (name, msg)
    # the edges of the legal ranges pass every check and reach the context test
    for kw in (dict(eps=2.0 ** -100), dict(eps=1.0), dict(top=8), dict(docs=[]), dict(docs=[3, 3, 1]), dict(phi=True, hard=False, select=False)):
        rc, msg = raw(K, V, A, B, pc, **kw)
        assert rc == last and ("no HIP device" in msg or "ctx is NULL" in msg), (kw, rc, msg)
    # a negative value in a column of A that docs does not name is not read
    rc, msg = raw(K, V, np.where(np.arange(12).reshape(3, 4) == 7, -1.0, A), B, pc, docs=[0, 1, 2])
    assert rc == last, msg


# ------------------------------------------------------------------------------------------------------------------ digamma
def test_digamma_f64_against_mpmath(tmvb):
    import importlib
    digamma = importlib.import_module(tmvb.__name__ + ".token_topics").digamma      # the package attribute of that name is the function
    x = np.concatenate([np.logspace(-3, 6, 400), [1.0, 2.0, 6.999999, 7.0, 7.000001, 0.5, 1.2116321449683622, 1.2116321449683620, 1.4616, 1.4617, 1.7116321449683622, 1.7116321449683625]])
    y = digamma(x)
    assert y.shape == x.shape and digamma(np.zeros((2, 0))).shape == (2, 0)
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    ref = np.array([float(mpmath.digamma(mpmath.mpf(float(v)))) for v in x])
    rel = np.abs(y - ref) / np.abs(ref)
    print(f"tmvb_digamma_f64 against mpmath on {len(x)} points in [1e-3, 1e6]: worst relative error {float(rel.max()):.3e} at x = {x[rel.argmax()]:.6g}")
    assert np.all(rel <= 1e-14)


# ------------------------------------------------------------------------------------------------------------------ factors by family
def test_token_factors_lda(tmvb):
    g = load("lda_m40_v60_k7")
    m = types.SimpleNamespace(K=7, alpha=g["alpha"], Elogtheta=g["Elogtheta"], beta=g["beta"])
    A, B = tmvb.token_factors(m)
    assert np.array_equal(A, np.exp(g["Elogtheta"])) and np.array_equal(B, g["beta"])


def test_token_factors_ctm(tmvb):
    from oracle import oracle_np as onp
    g = load("ctm_m40_v60_k5")
    m = types.SimpleNamespace(K=5, mu=g["mu"], sigma=g["sigma"], lam=g["lam"], beta=g["beta"])
    A, B = tmvb.token_factors(m)
    assert np.array_equal(A, np.exp(g["lam"] - g["lam"].max(axis=0))) and np.array_equal(B, g["beta"]) and A.max(axis=0).tolist() == [1.0] * 40
    ptr, terms = g["doc_ptr"], g["terms"]
    r = tr.responsibilities(A, B, ptr, terms, None, tr.EPSILON, rounded=False)
    for d in (0, 7, 39):                                   # update_phi!(::CTM): additive_logistic(log beta[:, terms] .+ lambda_d), src/CTM.jl:175-178
        w = terms[ptr[d]:ptr[d + 1]]
        with np.errstate(divide="ignore"):
            ref = onp.additive_logistic_cols(np.log(g["beta"][:, w]) + g["lam"][:, d][:, None])
        assert np.allclose(r[ptr[d]:ptr[d + 1]].T, ref, rtol=1e-12, atol=1e-25)


@pytest.mark.parametrize("name", ["ctpf_m40_v60_u15_k4", "ctpf_m30_v40_u12_k6_r1"])
def test_token_factors_ctpf(tmvb, name):
    from oracle import oracle_np as onp
    from scipy.special import digamma
    g = load(name)
    m = types.SimpleNamespace(K=int(g["K"]), alef=g["alef"], gimel=g["gimel"], dalet=g["dalet"], bet=g["bet"])
    A, B = tmvb.token_factors(m)
    a = digamma(g["gimel"]) - np.log(g["dalet"])[:, None] - np.log(g["bet"])[:, None]
    b = digamma(g["alef"])
    assert np.allclose(A, np.exp(a - a.max(axis=0)), rtol=1e-12, atol=0) and np.allclose(B, np.exp(b - b.max(axis=0)), rtol=1e-12, atol=0)
    assert np.all(A.max(axis=0) == 1.0) and np.all(B.max(axis=0) == 1.0)
    ptr, terms = g["doc_ptr"], g["terms"]
    r = tr.responsibilities(A, B, ptr, terms, None, tr.EPSILON, rounded=False)
    for d in (0, 11, len(ptr) - 2):                        # update_phi!(::CTPF), src/CTPF.jl:327-330
        w = terms[ptr[d]:ptr[d + 1]]
        ref = onp.additive_logistic_cols(a[:, d][:, None] + b[:, w])
        assert np.allclose(r[ptr[d]:ptr[d + 1]].T, ref, rtol=1e-11, atol=1e-25)


@pytest.mark.parametrize("name", ["flda_m40_v60_k5", "fctm_m30_v50_k4"])
def test_filtered_models_raise(tmvb, name):
    g = load(name)
    m = types.SimpleNamespace(**{k: g[k] for k in g.files})
    with pytest.raises(tmvb.TopicModelError, match="tau"):
        tmvb.token_factors(m)
    with pytest.raises(tmvb.TopicModelError):
        tmvb.token_topics(m)
    with pytest.raises(tmvb.TopicModelError):
        tmvb.token_factors(types.SimpleNamespace(K=3))
    with pytest.raises(ValueError):
        tmvb.token_topics(types.SimpleNamespace(K=3), top=9)


# ------------------------------------------------------------------------------------------------------------------ frozen tolerances
def test_the_gpu_tolerances_are_frozen_from_their_measurement():
    """a tolerance is at least 1 x and at most 10 x the worst deviation measured on the MI355X, and never above the derivable cap"""
    import test_token_topics_gpu as g
    ev = json.load(open(os.path.join(ROOT, "profiles", "token_topics_tolerances_measured.json")))["token_topics.r_rel"]
    assert sorted(int(k) for k in ev["measured"]) == sorted(g.TOL) == sorted(g.FLOAT_KS)
    for K, tol in g.TOL.items():
        measured = ev["measured"][str(K)]
        assert measured >= 0.0 and measured <= tol <= 10.0 * measured, (K, tol, measured)
        assert tol <= tr.cap(K) and ev["tolerance"][str(K)] == tol and ev["cap"][str(K)] == tr.cap(K)


# ------------------------------------------------------------------------------------------------------------------ the unit's device scratch
def test_the_unit_owns_no_device_scratch():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_token_topics.hip")).read()
    assert '#include "tmvb_call.h"' in src
    for pat in (r"hipMalloc\(", r"hipFree\(", r"hipEventCreate\(", r"hipEventDestroy\(", r"struct \w*_pool", r"auto cleanup", r"#define [A-Z]+_(HIP|TRY)"):
        assert not re.search(pat, src), f"tmvb_token_topics.hip: {pat} -- device memory and events of a call come from tmvb_call (csrc/tmvb_call.h)"
    assert "getenv" not in src                             # no environment switch
