"""
Held-out evaluation on the device (tmvb_corpus_split, tmvb_heldout_loglik and their Python mirror) against the NumPy restatements of
tests/test_heldout_host.py: the split bit for bit, the log-likelihood within a tolerance frozen from its own MI355X measurement.

With TMVB_HELDOUT_RECORD=<file> the worst relative deviation of ll[d] seen by this module is written to that file at its end; the
committed copy of such a run is profiles/heldout_tolerances_measured.json, and tests/test_heldout_host.py asserts
1 <= LL_REL_TOL / measured <= 10.
"""
import json
import math
import os

import numpy as np
import pytest

from test_heldout_host import (ROOT, _CSR, call_loglik, call_split, gamma_stochastic, host_split, loglik_error_cases, mixed_corpus, np_loglik,
                               split_error_cases)

pytestmark = pytest.mark.gpu

# |ll_device[d] - ll_numpy[d]| / |ll_numpy[d]| over every document with tokens of every case below.  The device rounds theta and beta' to
# fp32 and takes the K-term dot product in fp32 FMAs (logarithm and sums are fp64); measured on the MI355X: 3.2e-8
# (profiles/heldout_tolerances_measured.json).
LL_REL_TOL = 2e-7
WORST = {"heldout.ll_rel": 0.0}


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    out = os.environ.get("TMVB_HELDOUT_RECORD", "")
    if not out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"heldout.ll_rel": {"measured": WORST["heldout.ll_rel"], "tolerance": LL_REL_TOL,
                                      "what": "max over documents with tokens of |ll - ll_numpy_fp64| / |ll_numpy_fp64|, all cases of tests/test_heldout_gpu.py"}}, f, indent=1)


# ------------------------------------------------------------------------------------------------------------------ split
SPLIT_M, SPLIT_V, SPLIT_SEED = 257, 60, 20261017
SIX = ("obs_ptr", "obs_terms", "obs_counts", "held_ptr", "held_terms", "held_counts")


@pytest.fixture(scope="module")
def split_input():
    return mixed_corpus(SPLIT_M, SPLIT_V, seed=31)


def do_split(tmvb, ctx, csr, frac, seed=SPLIT_SEED, doc_offset=0):
    doc_ptr, terms, counts = csr
    rc, res = tmvb.split_corpus_raw(ctx, len(doc_ptr) - 1, SPLIT_V, doc_ptr, terms, counts, frac, seed, doc_offset)
    assert rc == 0, res
    return res


def dense(doc_ptr, terms, counts, M, V):
    out = np.zeros((M, V), dtype=np.int64)
    np.add.at(out, (np.repeat(np.arange(M), np.diff(doc_ptr)), terms), counts)
    return out


def test_the_input_has_the_shapes_it_claims(split_input):
    doc_ptr, terms, counts = split_input
    assert set(np.diff(doc_ptr)) == {0, 1, 3, 64, 65, 700}
    assert {1, 4, 5, 5000} <= set(counts.tolist()) and (counts == 5000).sum() == 1


@pytest.mark.parametrize("frac", [0.0, 0.25, 0.5, 1.0])
def test_split_equals_the_host_restatement_bit_for_bit(tmvb, ctx, split_input, frac):
    doc_ptr, terms, counts = split_input
    res = do_split(tmvb, ctx, split_input, frac)
    want = host_split(doc_ptr, terms, counts, frac, SPLIT_SEED)
    for name, w in zip(SIX, want):
        assert res[name].dtype == w.dtype and np.array_equal(res[name], w), name
    assert res["nnz_obs"] == len(want[1]) and res["nnz_held"] == len(want[4])
    assert res["sum_obs"] == want[2].sum(dtype=np.int64) and res["sum_held"] == want[5].sum(dtype=np.int64)
    # obs + held is the input, both sides are corpora over the same M and V
    M = SPLIT_M
    both = dense(res["obs_ptr"], res["obs_terms"], res["obs_counts"], M, SPLIT_V) + dense(res["held_ptr"], res["held_terms"], res["held_counts"], M, SPLIT_V)
    assert np.array_equal(both, dense(doc_ptr, terms, counts, M, SPLIT_V))
    for side in ("obs", "held"):
        pc = tmvb.PackedCorpus(res[side + "_ptr"], res[side + "_terms"], res[side + "_counts"], SPLIT_V)
        assert pc.M == M
        tmvb.check_corp(pc.to_corpus())
    if frac == 0.0:
        assert res["nnz_held"] == 0 and np.array_equal(res["obs_counts"], counts)
    if frac == 1.0:
        assert res["nnz_obs"] == 0 and np.array_equal(res["held_counts"], counts) and np.array_equal(res["held_ptr"], doc_ptr)


def test_split_seed_and_slice(tmvb, ctx, split_input):
    doc_ptr, terms, counts = split_input
    a = do_split(tmvb, ctx, split_input, 0.5)
    b = do_split(tmvb, ctx, split_input, 0.5)
    for name in SIX:
        assert a[name].tobytes() == b[name].tobytes(), name
    c = do_split(tmvb, ctx, split_input, 0.5, seed=SPLIT_SEED + 1)
    assert not np.array_equal(a["held_counts"], c["held_counts"])
    # documents [100, 180) of the full call are the call M = 80, doc_offset = 100
    lo, hi = doc_ptr[100], doc_ptr[180]
    part = do_split(tmvb, ctx, (doc_ptr[100:181] - lo, terms[lo:hi], counts[lo:hi]), 0.5, doc_offset=100)
    for side in ("obs", "held"):
        full = tmvb.PackedCorpus(a[side + "_ptr"], a[side + "_terms"], a[side + "_counts"], SPLIT_V).shard(100, 180)
        assert np.array_equal(part[side + "_ptr"], full.doc_ptr) and np.array_equal(part[side + "_terms"], full.terms)
        assert np.array_equal(part[side + "_counts"], full.counts)
    # without doc_offset the same documents split differently
    other = do_split(tmvb, ctx, (doc_ptr[100:181] - lo, terms[lo:hi], counts[lo:hi]), 0.5)
    assert not np.array_equal(other["held_counts"], part["held_counts"])


def test_python_split_corpus(tmvb, split_input):
    doc_ptr, terms, counts = split_input
    pc = tmvb.PackedCorpus(doc_ptr, terms, counts, SPLIT_V)
    obs, held = tmvb.split_corpus(pc, frac=0.25, seed=SPLIT_SEED)
    want = host_split(doc_ptr, terms, counts, 0.25, SPLIT_SEED)
    got = (obs.doc_ptr, obs.terms, obs.counts, held.doc_ptr, held.terms, held.counts)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and obs.V == held.V == SPLIT_V
    small = tmvb.PackedCorpus(doc_ptr[:7], terms[:doc_ptr[6]], counts[:doc_ptr[6]], SPLIT_V)
    o2, h2 = tmvb.split_corpus(small.to_corpus(), frac=0.25, seed=SPLIT_SEED)          # a Corpus is accepted too
    assert np.array_equal(o2.counts, obs.shard(0, 6).counts) and np.array_equal(h2.terms, held.shard(0, 6).terms)


@pytest.mark.parametrize("case", split_error_cases() + loglik_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_argument_errors_with_a_live_context(tmvb, ctx, case):
    _, kw, status, msg = case
    rc, res = (call_split if "frac" in kw else call_loglik)(tmvb, ctx, kw)
    assert rc == status and msg in (res["error"] if isinstance(res, dict) else res), (rc, res)


# ------------------------------------------------------------------------------------------------------------------ log-likelihood
# (K, V, entries of one extra long document): every K whose lane count per entry or tail differs (K = 1, 3: one lane, partial chunk;
# 50: 13 chunks on 4 lanes; 64: no partial chunk, a chunk of pads; 70: 8 lanes; 130: 16 lanes; 1024: a wave per entry, five chunks a lane)
LL_CASES = [(1, 60, 0), (3, 60, 0), (50, 60, 0), (64, 60, 0), (70, 60, 0), (130, 60, 0), (1024, 60, 0), (50, 2000, 0), (50, 6000, 5000), (130, 6000, 5000)]
LL_M = 130
_inputs = {}


def ll_input(K, V, long_doc):
    """theta, beta, CSR and the NumPy fp64 answers for both smoothings: computed once, shared, never changed"""
    key = (K, V, long_doc)
    if key not in _inputs:
        doc_ptr, terms, counts = mixed_corpus(LL_M, V, seed=1000 + K + V, long_doc=long_doc)
        M = len(doc_ptr) - 1
        theta = np.asfortranarray(gamma_stochastic(M, K, seed=2000 + K).T)
        beta = np.asfortranarray(gamma_stochastic(K, V, seed=3000 + K + V))
        ref = {s: np_loglik(theta, beta, doc_ptr, terms, counts, s) for s in (0.0, 1e-3)}
        for a in (theta, beta, doc_ptr, terms, counts):
            a.setflags(write=False)
        _inputs[key] = (theta, beta, doc_ptr, terms, counts, ref)
    return _inputs[key]


def compare_ll(res, ll_ref, tok_ref, what):
    assert np.array_equal(res.tokens, tok_ref), what
    has = tok_ref > 0
    assert np.all(res.ll[~has] == 0.0), what
    rel = np.abs(res.ll[has] - ll_ref[has]) / np.abs(ll_ref[has])
    worst = float(rel.max())
    WORST["heldout.ll_rel"] = max(WORST["heldout.ll_rel"], worst)
    print(f"heldout.ll_rel {what}: worst {worst:.3e} (tolerance {LL_REL_TOL:.1e})")
    assert worst <= LL_REL_TOL, (what, worst)


@pytest.mark.parametrize("smooth", [0.0, 1e-3])
@pytest.mark.parametrize("K,V,long_doc", LL_CASES)
def test_loglik_against_numpy_fp64(tmvb, ctx, K, V, long_doc, smooth):
    theta, beta, doc_ptr, terms, counts, ref = ll_input(K, V, long_doc)
    rc, res = tmvb.heldout_loglik_raw(ctx, K, V, theta, beta, _CSR(doc_ptr, terms, counts), smooth)
    assert rc == 0, res
    assert res.zero_prob_tokens == 0 and np.all(np.isfinite(res.ll))
    if long_doc:
        assert doc_ptr[-1] - doc_ptr[-2] == 5000
    compare_ll(res, ref[smooth][0], ref[smooth][1], f"K={K} V={V} long={long_doc} smooth={smooth}")
    assert res.perplexity == pytest.approx(math.exp(-ref[smooth][0].sum() / ref[smooth][1].sum()), rel=1e-5)


def test_zero_probability(tmvb, ctx):
    K, V, z = 3, 20, 7
    beta = gamma_stochastic(K, V, seed=5)
    beta[:, z] = 0.0
    beta /= beta.sum(axis=1, keepdims=True)
    theta = gamma_stochastic(6, K, seed=6).T
    doc_ptr = np.array([0, 3, 5, 5, 9, 11, 14], dtype=np.int64)
    terms = np.array([1, z, 4, 0, 2, 3, 5, 6, 8, 9, z, 10, 11, 12], dtype=np.int32)
    counts = np.array([2, 3, 1, 1, 1, 4, 1, 2, 1, 1, 7, 5, 1, 1], dtype=np.int32)
    csr = _CSR(doc_ptr, terms, counts)
    rc, res = tmvb.heldout_loglik_raw(ctx, K, V, theta, beta, csr, 0.0)
    assert rc == 0, res
    ll_ref, tok_ref = np_loglik(theta, beta, doc_ptr, terms, counts, 0.0)
    bad = np.array([True, False, False, False, True, False])
    assert np.all(np.isneginf(res.ll[bad])) and np.all(np.isneginf(ll_ref[bad])) and res.zero_prob_tokens == 3 + 7
    assert res.perplexity == math.inf and np.array_equal(res.tokens, tok_ref)
    ok = ~bad & (tok_ref > 0)
    assert res.ll[2] == 0.0 and np.all(np.abs(res.ll[ok] - ll_ref[ok]) <= LL_REL_TOL * np.abs(ll_ref[ok]))
    rc, res = tmvb.heldout_loglik_raw(ctx, K, V, theta, beta, csr, 1e-3)
    assert rc == 0, res
    assert res.zero_prob_tokens == 0 and np.all(np.isfinite(res.ll)) and math.isfinite(res.perplexity)
    ll_s, _ = np_loglik(theta, beta, doc_ptr, terms, counts, 1e-3)
    compare_ll(res, ll_s, tok_ref, "zero column, smooth=1e-3")


def test_loglik_is_bitwise_reproducible(tmvb, ctx):
    for key in ((50, 6000, 5000), (1024, 60, 0)):
        theta, beta, doc_ptr, terms, counts, _ = ll_input(*key)
        a = tmvb.heldout_loglik_raw(ctx, key[0], key[1], theta, beta, _CSR(doc_ptr, terms, counts), 0.0)[1]
        b = tmvb.heldout_loglik_raw(ctx, key[0], key[1], theta, beta, _CSR(doc_ptr, terms, counts), 0.0)[1]
        assert a.ll.tobytes() == b.ll.tobytes() and np.array_equal(a.tokens, b.tokens)


# ------------------------------------------------------------------------------------------------------------------ end to end
E2E_K, E2E_V = 5, 300


@pytest.fixture(scope="module")
def corpora(tmvb):
    """a known 5-topic model, a training draw of 600 documents and a second draw of 300.

    Each topic is 3/4 a sparse Gamma(0.08) draw and 1/4 uniform.  Without smoothing a term that the training draw never shows has
    beta = 0 in every trained topic, and a held-out occurrence of it scores -inf by the rule of the zero-probability test (CTM's fold-in
    takes log beta of it); a finite perplexity therefore needs every term in the training draw.  The uniform quarter gives every term
    at least 0.25 / 300 in every topic: 600 documents of mean length 80 show it 40 times on average, and the chance that any of the
    300 terms stays unseen is below 300 exp(-40) ~ 1e-15."""
    gen = tmvb.LDA(tmvb.PackedCorpus([0, 1], [0], [80], E2E_V), E2E_K)
    rng = np.random.Generator(np.random.PCG64(77))
    topics = rng.gamma(0.08, size=(E2E_K, E2E_V))
    topics = 0.75 * topics / topics.sum(axis=1, keepdims=True) + 0.25 / E2E_V
    gen.beta = np.asfortranarray(topics / topics.sum(axis=1, keepdims=True))
    gen.alpha = np.full(E2E_K, 0.3)
    return tmvb.gencorp(gen, 600, seed=101), tmvb.gencorp(gen, 300, seed=202)


def numpy_perplexity(res, beta, held):
    ll, tok = np_loglik(res.theta, beta, held.doc_ptr, held.terms, held.counts, 0.0)
    return ll, math.exp(-ll.sum() / tok.sum())


@pytest.mark.parametrize("family", ["LDA", "CTM"])
def test_perplexity_of_a_trained_model(tmvb, corpora, family):
    train, test = corpora
    kw = dict(iter=30, tol=0.0, checkelbo=math.inf, printelbo=False)
    if family == "LDA":
        model, fresh = tmvb.LDA(train, E2E_K), tmvb.LDA(train, E2E_K)
        tmvb.gpu_train(model, **kw)
    else:
        model, fresh = tmvb.CTM(train, E2E_K), tmvb.CTM(train, E2E_K)
        tmvb.gpu_train_ctm(model, **kw)
    ppl = tmvb.perplexity(model, test, frac=0.5, seed=9)
    assert math.isfinite(ppl)
    obs, held = tmvb.split_corpus(test, 0.5, 9)
    res = tmvb.heldout_loglik(model, obs, held)
    assert res.zero_prob_tokens == 0 and res.tokens.sum() == held.counts.sum(dtype=np.int64) > 0
    ll_ref, ppl_ref = numpy_perplexity(res, model.beta, held)
    compare_ll(res, ll_ref, held.C, f"end to end {family}")
    # all ll share a sign, so log perplexity = -sum ll / sum tokens carries at most the per-document relative deviation
    assert abs(math.log(ppl) - math.log(ppl_ref)) <= LL_REL_TOL * math.log(ppl_ref)
    assert abs(math.log(res.perplexity) - math.log(ppl_ref)) <= LL_REL_TOL * math.log(ppl_ref)
    untrained = tmvb.perplexity(fresh, test, frac=0.5, seed=9)
    print(f"perplexity {family}: trained {ppl:.2f}, untrained {untrained:.2f}, uniform {E2E_V}")
    assert ppl < untrained and ppl < E2E_V


def test_filtered_models_dispatch_ctpf_and_vocabulary_raise(tmvb, corpora):
    train, test = corpora
    small = test.shard(0, 60)
    for model in (tmvb.fLDA(train, E2E_K), tmvb.fCTM(train, E2E_K)):
        ppl = tmvb.perplexity(model, small, frac=0.5, seed=3, iter=3)
        assert math.isfinite(ppl) and ppl > 1.0
    pf = tmvb.PackedCorpus([0, 2], [0, 1], [1, 1], 3, [0, 1], [0], [1], 2)
    with pytest.raises(tmvb.TopicModelError, match="CTPF"):
        tmvb.perplexity(tmvb.CTPF(pf, 2), pf)
    other = tmvb.PackedCorpus(small.doc_ptr, small.terms, small.counts, E2E_V + 1)
    with pytest.raises(tmvb.CorpusError, match="identical vocabularies"):
        tmvb.perplexity(tmvb.LDA(train, E2E_K), other)
