"""
Co-document counts on the device (tmvb_corpus_codocfreq and its Python mirror) against the NumPy checker of tests/test_coherence_host.py:
the counts exactly, the scores at rel 1e-12 (the tolerance reasoning stands in that module's docstring).

The shapes are the smallest at which each mechanism can go wrong: M around one 64-document word of the bit matrix (1, 63, 64, 65, 130), around
one chunk of the pair pass (TMVB_CODF_CHUNK_DOCS - 1, the chunk, + 1) and past two chunks with a partial word at the end; N = 2 (one pair
off the diagonal), 10 (55 pairs: the last round of the four waves is partial) and 64 (the LDS tile full, 2 080 pairs).
"""
import numpy as np
import pytest

import presentations as pr
from test_coherence_host import CHUNK_DOCS as CHUNK, EINVAL, assert_scores, np_codf, np_scores, random_corpus

pytestmark = pytest.mark.gpu

# CHUNK = TMVB_CODF_CHUNK_DOCS, 4 096 documents: the ids of the parametrised cases carry its value (4095, 4096, 4097, 8262)
V = 97
EVERY, NOWHERE = 0, 1               # an id every document of corpus B contains; an id no document contains
MS = [1, 63, 64, 65, 130, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 70]
KN = [(1, 2), (3, 10), (7, 64)]


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()


def draw_top(K, N, seed):
    """rows drawn without replacement; EVERY leads every row (one id shared by all topics), NOWHERE is the second word of topic 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    top = np.stack([np.concatenate([[EVERY], rng.choice(np.arange(2, V), size=N - 1, replace=False)]) for _ in range(K)])
    top[0, 1] = NOWHERE
    assert all(len(set(r)) == N for r in top.tolist())
    return top


_CORPORA = {}


def corpora(M):
    """A: empty documents, EVERY an id like any other, NOWHERE in none.  B: EVERY in every document (no document is empty), NOWHERE in none."""
    if M not in _CORPORA:
        a = random_corpus(M, V, seed=1000 + M, nowhere=(NOWHERE,))
        b = random_corpus(M, V, seed=2000 + M, everywhere=(EVERY,), nowhere=(NOWHERE,))
        if M >= 63:
            assert (np.diff(a[0]) == 0).any() and (np.diff(b[0]) > 0).all()
        _CORPORA[M] = (a, b)
    return _CORPORA[M]


def np_df(M, doc_ptr, terms):
    """df[V]: documents that contain each id, from the distinct (document, id) pairs"""
    doc = np.repeat(np.arange(M, dtype=np.int64), np.diff(doc_ptr))
    return np.bincount(np.unique(doc * V + terms) % V, minlength=V)


def run(tmvb, ctx, M, Vv, csr, top, budget=0):
    rc, res = tmvb.codocfreq_raw(ctx, M, Vv, csr[0], csr[1], csr[2], top, budget)
    assert rc == 0, res
    return res


@pytest.mark.parametrize("M,K,N", [(M, K, N) for M in MS for (K, N) in KN], ids=lambda v: str(v))
def test_counts_against_numpy(tmvb, ctx, M, K, N):
    top = draw_top(K, N, seed=7 * K + N)
    for name, csr in zip("AB", corpora(M)):
        res = run(tmvb, ctx, M, V, csr, top)
        got, want = res["codf"], np_codf(M, V, csr[0], csr[1], top)
        assert got.dtype == np.int64 and got.shape == (K, N, N)
        assert np.array_equal(got, np.transpose(got, (0, 2, 1))), name                                   # symmetric
        assert np.array_equal(np.diagonal(got, axis1=1, axis2=2), np_df(M, csr[0], csr[1])[top]), name   # the diagonal is the document frequency
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        assert res["n_slots"] == len(np.unique(top)) and res["n_batches"] == 1
        assert np.all(got[0, 1, :] == 0)                                                                 # NOWHERE occurs in no document
        if name == "B":
            assert np.all(got[:, 0, 0] == M)                                                             # EVERY occurs in every document
        assert_scores(tmvb.coherence_from_counts(got, M), np_scores(want, M))


def test_presentations_give_the_identical_counts(tmvb, ctx):
    """the same corpus with entries shuffled, ids repeated with counts split, documents permuted, ids relabelled (top relabelled alike)"""
    canon = pr.canonical(seed=pr.SEED, M=130, V=200)
    rng = np.random.Generator(np.random.PCG64(5))
    hot = canon.info["hot"]
    top = np.stack([np.concatenate([hot, rng.choice(np.setdiff1d(np.arange(200), hot), size=8, replace=False)]) for _ in range(3)])
    base = run(tmvb, ctx, canon.M, canon.V, (canon.doc_ptr, canon.terms, canon.counts), top)["codf"]
    assert np.array_equal(base, np_codf(canon.M, canon.V, canon.doc_ptr, canon.terms, top))
    assert base[0, 0, 1] >= canon.M - 3                              # the two hot ids share every document but the one-entry and the empty ones
    forms = [pr.shuffled(canon, np.random.default_rng(101)), pr.uncondensed(canon, np.random.default_rng(1000)),
             pr.docs_permuted(canon, np.random.default_rng(103)), pr.relabelled(canon, np.random.default_rng(104))]
    assert forms[1].info is canon.info and len(forms[1].terms) > len(canon.terms)                        # ids are repeated inside documents
    for p in forms:
        got = run(tmvb, ctx, p.M, p.V, (p.doc_ptr, p.terms, p.counts), p.term_to[top])["codf"]
        assert np.array_equal(got, base), p.name


def test_batches_equal_one_batch_bit_for_bit(tmvb, ctx):
    M, K, N = 130, 7, 10
    csr = corpora(M)[0]
    top = draw_top(K, N, seed=3)
    one = run(tmvb, ctx, M, V, csr, top)
    T, W = len(np.unique(top)), (M + 63) // 64
    assert one["n_batches"] == 1 and one["n_slots"] == T and T // 3 >= N
    budget = (T * W * 8) // 3                                        # a batch holds at most T / 3 slots: at least three batches
    many = run(tmvb, ctx, M, V, csr, top, budget)
    assert many["n_batches"] >= 3 and many["n_slots"] == T
    assert many["codf"].tobytes() == one["codf"].tobytes()
    each = run(tmvb, ctx, M, V, csr, top, N * W * 8)                 # exactly one topic's need: K batches
    assert each["n_batches"] == K and each["codf"].tobytes() == one["codf"].tobytes()
    rc, msg = tmvb.codocfreq_raw(ctx, M, V, csr[0], csr[1], csr[2], top, N * W * 8 - 1)
    assert rc == EINVAL and f"one topic needs {N * W * 8} bytes" in msg, (rc, msg)


@pytest.mark.parametrize("m", [64, 37])
def test_counts_are_additive_over_document_shards(tmvb, ctx, m):
    M, K, N = 130, 3, 10
    ptr, terms, counts = corpora(M)[0]
    top = draw_top(K, N, seed=4)
    whole = run(tmvb, ctx, M, V, (ptr, terms, counts), top)["codf"]
    a = run(tmvb, ctx, m, V, (ptr[:m + 1], terms[:ptr[m]], counts[:ptr[m]]), top)["codf"]
    b = run(tmvb, ctx, M - m, V, (ptr[m:] - ptr[m], terms[ptr[m]:], counts[ptr[m]:]), top)["codf"]
    assert np.array_equal(a + b, whole)


def test_two_calls_give_equal_bytes(tmvb, ctx):
    M = 2 * CHUNK + 70
    csr = corpora(M)[1]
    top = draw_top(7, 64, seed=9)
    a, b = run(tmvb, ctx, M, V, csr, top), run(tmvb, ctx, M, V, csr, top)
    assert a["codf"].tobytes() == b["codf"].tobytes()
    assert a["ms"]["bitset"] > 0 and a["ms"]["pairs"] > 0


def check_end_to_end(tmvb, model, pc, topn):
    r = tmvb.coherence(model, pc, topn=topn)
    top = np.array([np.asarray(t)[:topn] for t in model.topics], dtype=np.int64) - 1                    # the mirror's topics are 1-based
    assert np.array_equal(r.top, top) and top.min() >= 0 and top.max() < pc.V
    want = np_codf(pc.M, pc.V, pc.doc_ptr, pc.terms, top)
    assert np.array_equal(r.codf, want) and np.array_equal(r.df, np.diagonal(want, axis1=1, axis2=2))
    assert_scores((r.umass, r.npmi, r.undefined_pairs), np_scores(want, pc.M))
    assert r.diversity == len(np.unique(top)) / top.size and r.n_batches == 1
    assert r.mean_npmi == pytest.approx(float(np.mean(r.npmi)), rel=1e-15)
    # an explicit 0-based array is the same question
    assert np.array_equal(tmvb.coherence(top, pc).codf, want)


def test_end_to_end_on_trained_models(tmvb):
    pc = tmvb.syn_nsf(M=120, V=300, seed=4)
    m = tmvb.LDA(pc, 3)
    tmvb.gpu_train(m, iter=4, tol=0.0, checkelbo=float("inf"), printelbo=False)
    assert not np.array_equal(m.topics[0], np.arange(1, pc.V + 1))                                      # train! ordered the topics
    check_end_to_end(tmvb, m, pc, 5)
    pf = tmvb.syn_citeu(M=60, V=150, U=20, seed=5)
    f = tmvb.CTPF(pf, 3)
    tmvb.gpu_train_ctpf(f, iter=3, tol=0.0, checkelbo=float("inf"), printelbo=False)
    eb = f.alef / f.bet[:, None]                                                                        # CTPF's topics come from alef ./ bet
    assert all(np.all(np.diff(eb[k, np.asarray(t)[:5] - 1]) <= 0) and eb[k, t[0] - 1] == eb[k].max() for k, t in enumerate(f.topics))
    check_end_to_end(tmvb, f, pf, 5)
