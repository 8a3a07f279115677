"""
tmvb_token_topics on the device (include/tmvb.h, "word-topic assignments") against tests/token_topics_restatement.py.

  1. exact selection with ties   integer factors in [0, 3], eps = 2^-100: y is an exact small integer (or eps), distinct y differ by >= 1/9
                                 relative and cannot round to equal r, so top_idx and hard are checked bit-exact
  2. document lengths            0, 1, G - 1, G, G + 1 entries (G = entries per trip of a wave, from info), one document just past the
                                 short / long cut, one of 3 000 entries
  3. floating factors            every dense r within TOL[K] r64, sum_k r within K 2^-24 of 1
  4. self-consistency            top_idx / top_r = the lexsort of the device's own dense bits; hard = the counts grouped by top_idx[:, 0]
  5. purity                      identical bytes over docs lists, single documents, calls, chunk sizes and output sets
  6. wrappers                    phi(model, d) after gpu_train on the golden corpora, token_topics(model, corp=new)

TOL[K] bounds |r - r64| / r64 (r64 from the fp64 factors as given).  Each literal is within [1, 10] x the worst deviation case 3 measured on
an MI355X (profiles/token_topics_tolerances_measured.json; a run with TMVB_TT_RECORD=<file> writes such a record at the module's end) and
never above cap(K) = (K + 12) 2^-24 (tests/test_token_topics_host.py asserts both).
"""
import json
import os

import numpy as np
import pytest

import token_topics_restatement as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, V = 40, 60
EXACT_KS = [1, 3, 4, 5, 16, 17, 50, 64, 65, 130, 300, 1024]        # 300: lanes_per_entry = 32, which the others leave out
LANES = {1: 1, 3: 1, 4: 1, 5: 1, 16: 1, 17: 2, 50: 4, 64: 4, 65: 8, 130: 16, 300: 32, 1024: 64}
FLOAT_KS = [1, 3, 50, 65, 130, 1024]
TOL = {1: 0.0, 3: 8.0e-7, 50: 1.2e-6, 65: 1.3e-6, 130: 1.1e-6, 1024: 1.2e-6}
WORST = {K: 0.0 for K in FLOAT_KS}
EPS_EXACT = 2.0 ** -100


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    out = os.environ.get("TMVB_TT_RECORD", "")
    if not out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"token_topics.r_rel": {"measured": {str(K): WORST[K] for K in FLOAT_KS}, "tolerance": {str(K): TOL[K] for K in FLOAT_KS},
                                          "cap": {str(K): tr.cap(K) for K in FLOAT_KS},
                                          "what": "per K, max over entries and topics of |r - r64| / r64, the floating case of "
                                                  "tests/test_token_topics_gpu.py"}}, f, indent=1)


def corpus(tmvb, lengths, seed, V=V):
    rng = np.random.Generator(np.random.PCG64(seed))
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(ptr[-1])
    return tmvb.PackedCorpus(ptr, rng.integers(0, V, size=n).astype(np.int32), rng.integers(1, 6, size=n).astype(np.int32), V)


def base_lengths(seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    L = rng.integers(1, 24, size=M)
    L[[5, 17]] = 0
    return L


def integer_factors(K, Md, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 4, size=(K, Md)).astype(np.float64), rng.integers(0, 4, size=(K, V)).astype(np.float64)


def floating_factors(K, Md, seed):
    """Gamma factors with exact zeros; a fifth of the documents and of the terms scaled so that their products fall below eps"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A, B = rng.standard_gamma(0.5, size=(K, Md)), rng.standard_gamma(0.3, size=(K, V))
    A[rng.random(A.shape) < 0.1] = 0.0
    B[rng.random(B.shape) < 0.1] = 0.0
    A[K // 2, 1::7] = 0.0
    B[K // 2, 2::7] = 0.0
    A[:, ::5] *= 1e-20
    B[:, ::5] *= 1e-18
    return A, B


def run(tmvb, ctx, A, B, pc, **kw):
    rc, res = tmvb.token_topics_raw(ctx, A.shape[0], B.shape[1], A, B, pc, **kw)
    assert rc == 0, res
    return res


def assert_exact(res, ref, t, tag):
    assert np.array_equal(res["top_idx"], ref["top_idx"]), (tag, t, np.argwhere(res["top_idx"] != ref["top_idx"])[:5])
    assert np.array_equal(res["hard"], ref["hard"]), (tag, t)
    assert np.all(np.abs(res["top_r"].astype(np.float64) - ref["top_r"]) <= tr.cap(ref["r"].shape[1]) * ref["top_r"]), (tag, t)


# ------------------------------------------------------------------------------------------------------------------ 1. exact selection with ties
@pytest.mark.parametrize("K", EXACT_KS)
def test_exact_selection_with_ties(tmvb, ctx, K):
    pc = corpus(tmvb, base_lengths(), 11)
    A, B = integer_factors(K, M, 100 + K)
    for t in (1, 2, 8):                                    # 8 > K at K in {1, 3, 4, 5}: slots past K hold -1 and 0
        res = run(tmvb, ctx, A, B, pc, top=t, eps=EPS_EXACT)
        ref = tr.restate(A, B, pc.doc_ptr, pc.terms, pc.counts, None, EPS_EXACT, t)
        assert res["info"]["lanes_per_entry"] == LANES[K] and res["info"]["nsel"] == len(pc.terms)
        ties = int(np.sum(np.sort(ref["r"], axis=1)[:, -1] == np.sort(ref["r"], axis=1)[:, -2])) if K > 1 else 0
        print(f"token_topics exact K = {K} t = {t}: {ties} of {len(pc.terms)} entries have a tie for the best topic")
        assert K == 1 or ties > 0
        assert_exact(res, ref, t, K)
        if t > K:
            assert np.all(res["top_idx"][:, K:] == -1) and np.all(res["top_r"][:, K:] == 0)


# ------------------------------------------------------------------------------------------------------------------ 2. document lengths
@pytest.mark.parametrize("K", [3, 50])
def test_document_lengths_where_a_path_changes(tmvb, ctx, K):
    probe = run(tmvb, ctx, *integer_factors(K, 1, 1), corpus(tmvb, [1], 1), eps=EPS_EXACT)
    G = 64 // probe["info"]["lanes_per_entry"]
    lengths = [0, 1, G - 1, G, G + 1, 4 * G, 4 * G + 1, 3000, 0, 2]        # 4 G: the last length of the one-wave kernel
    pc = corpus(tmvb, lengths, 21)
    A, B = integer_factors(K, len(lengths), 200 + K)
    res = run(tmvb, ctx, A, B, pc, top=2, eps=EPS_EXACT, phi=True)
    ref = tr.restate(A, B, pc.doc_ptr, pc.terms, pc.counts, None, EPS_EXACT, 2)
    assert res["info"]["n_long"] == 2 and res["info"]["n_short"] == len(lengths) - 4 and res["info"]["chunks"] == 1      # empty documents: no work item
    assert_exact(res, ref, 2, K)
    assert np.all(np.abs(res["phi"].astype(np.float64) - ref["r"]) <= tr.cap(K) * ref["r"])
    for s in range(len(lengths)):                          # document by document: the same rows
        one = run(tmvb, ctx, A, B, pc, docs=[s], top=2, eps=EPS_EXACT, phi=True)
        a, b = ref["ptr"][s], ref["ptr"][s + 1]
        assert np.array_equal(one["top_idx"], res["top_idx"][a:b]) and np.array_equal(one["phi"].view(np.uint32), res["phi"][a:b].view(np.uint32))
        assert np.array_equal(one["hard"][0], res["hard"][s])


# ------------------------------------------------------------------------------------------------------------------ 3. floating factors
def floating_case(tmvb, ctx, K):
    pc = corpus(tmvb, base_lengths(), 31)
    A, B = floating_factors(K, M, 300 + K)
    return pc, A, B, run(tmvb, ctx, A, B, pc, top=4, phi=True)


@pytest.mark.parametrize("K", FLOAT_KS)
def test_floating_factors(tmvb, ctx, K):
    pc, A, B, res = floating_case(tmvb, ctx, K)
    r64 = tr.responsibilities(A, B, pc.doc_ptr, pc.terms, None, tr.EPSILON, rounded=False)
    y = tr.EPSILON + A[:, np.repeat(np.arange(M), np.diff(pc.doc_ptr))].T * B[:, pc.terms].T
    assert np.any(A == 0) and np.any(B == 0) and (K == 1 or np.any((y < 2 * tr.EPSILON) & (y > tr.EPSILON)))      # zeros and products below eps are there
    r = res["phi"].astype(np.float64)
    worst = float((np.abs(r - r64) / r64).max())
    dsum = float(np.abs(r.sum(axis=1) - 1.0).max())
    print(f"token_topics floating K = {K}: worst |r - r64| / r64 = {worst:.3e} (tolerance {TOL[K]:.3e}, cap {tr.cap(K):.3e}); worst |sum r - 1| = {dsum:.3e} "
          f"(bound {K * tr.U:.3e})")
    WORST[K] = max(WORST[K], worst)
    assert TOL[K] <= tr.cap(K)
    assert np.all(np.abs(r - r64) <= TOL[K] * r64)
    assert dsum <= K * tr.U


# ------------------------------------------------------------------------------------------------------------------ 4. self-consistency
@pytest.mark.parametrize("K", [3, 50, 130])
def test_selection_is_the_lexsort_of_the_devices_own_dense_bits(tmvb, ctx, K):
    pc, A, B, res = floating_case(tmvb, ctx, K)
    idx, val = tr.top_t(res["phi"], 4)
    assert np.array_equal(res["top_idx"], idx)
    assert np.array_equal(res["top_r"].view(np.uint32), val.view(np.uint32))
    ptr = np.asarray(pc.doc_ptr)
    assert np.array_equal(res["hard"], tr.hard_counts(res["top_idx"][:, 0], np.asarray(pc.counts, dtype=np.int64), ptr, K))
    C = np.bincount(np.repeat(np.arange(M), np.diff(ptr)), weights=pc.counts, minlength=M).astype(np.int64)
    assert np.array_equal(res["hard"].sum(axis=1), C)                                      # every row sums to C_d


# ------------------------------------------------------------------------------------------------------------------ 5. purity
def same(a, b, sel=None):
    for k in ("top_idx", "top_r", "phi"):
        if a[k] is None or b[k] is None:
            continue
        x, y = a[k], (b[k] if sel is None else b[k][sel])
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k


@pytest.mark.parametrize("K", [5, 50, 130])
def test_purity(tmvb, ctx, K):
    pc, A, B, full = floating_case(tmvb, ctx, K)
    ptr = np.asarray(pc.doc_ptr)
    rows = lambda docs: np.concatenate([np.arange(ptr[d], ptr[d + 1]) for d in docs]).astype(np.int64)
    again = run(tmvb, ctx, A, B, pc, top=4, phi=True)
    same(again, full); assert np.array_equal(again["hard"], full["hard"])
    docs = np.random.Generator(np.random.PCG64(5)).permutation(M).tolist() + [3, 3, 17, 0]          # permuted, with repeats and an empty document
    perm = run(tmvb, ctx, A, B, pc, docs=docs, top=4, phi=True)
    same(perm, full, rows(docs)); assert np.array_equal(perm["hard"], full["hard"][docs])
    for d in (0, 5, 9, M - 1):
        one = run(tmvb, ctx, A, B, pc, docs=[d], top=4, phi=True)
        same(one, full, rows([d])); assert np.array_equal(one["hard"][0], full["hard"][d])
    for chunk in (1, 7, 0):
        c = run(tmvb, ctx, A, B, pc, top=4, phi=True, max_chunk_entries=chunk)
        same(c, full); assert np.array_equal(c["hard"], full["hard"])
        assert c["info"]["chunks"] == (1 if chunk == 0 else -(-len(pc.terms) // chunk))
        c = run(tmvb, ctx, A, B, pc, docs=docs, top=4, max_chunk_entries=chunk)                       # selection only, cut documents
        same(c, perm); assert np.array_equal(c["hard"], perm["hard"]) and c["phi"] is None
    only = run(tmvb, ctx, A, B, pc, top=4, phi=False)
    same(only, full); assert np.array_equal(only["hard"], full["hard"])
    dense = run(tmvb, ctx, A, B, pc, phi=True, hard=False, select=False)
    same(dense, full); assert dense["top_idx"] is None and dense["hard"] is None
    top1 = run(tmvb, ctx, A, B, pc, top=1, hard=False)
    assert np.array_equal(top1["top_idx"][:, 0], full["top_idx"][:, 0])
    # a document with permuted entries gives permuted rows
    d = int(np.argmax(np.diff(ptr)))
    p = np.random.Generator(np.random.PCG64(6)).permutation(int(ptr[d + 1] - ptr[d]))
    terms, counts = np.array(pc.terms), np.array(pc.counts)
    terms[ptr[d]:ptr[d + 1]] = terms[ptr[d]:ptr[d + 1]][p]; counts[ptr[d]:ptr[d + 1]] = counts[ptr[d]:ptr[d + 1]][p]
    shuf = run(tmvb, ctx, A, B, tmvb.PackedCorpus(ptr, terms, counts, V), docs=[d], top=4, phi=True)
    same(shuf, full, rows([d])[p]); assert np.array_equal(shuf["hard"][0], full["hard"][d])


# ------------------------------------------------------------------------------------------------------------------ 6. wrappers
def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def check_phi(tmvb, model, A, B, K):
    pc = model.corp
    got = tmvb.phi(model, list(range(1, pc.M + 1)))
    r64 = tr.responsibilities(A, B, pc.doc_ptr, pc.terms, None, tr.EPSILON, rounded=False)
    ptr = np.asarray(pc.doc_ptr)
    for d in range(pc.M):
        assert got[d].shape == (K, ptr[d + 1] - ptr[d]) and got[d].dtype == np.float32
        assert np.all(np.abs(got[d].T.astype(np.float64) - r64[ptr[d]:ptr[d + 1]]) <= tr.cap(K) * r64[ptr[d]:ptr[d + 1]]), d
    d = int(np.argmax(np.diff(ptr))) + 1
    assert np.array_equal(tmvb.phi(model, d), got[d - 1])
    tt = tmvb.token_topics(model, top=2)
    assert np.array_equal(tt.topic, tr.top_t(np.concatenate([g.T for g in got]), 2)[0]) and np.array_equal(tt.hard.sum(axis=1), np.asarray(pc.C, dtype=np.int64))
    assert np.array_equal(tt.zero_based_docs, np.arange(pc.M)) and np.array_equal(tt.doc_ptr, ptr) and np.array_equal(tt.terms, pc.terms)


@pytest.mark.parametrize("name", ["lda_m40_v60_k3", "lda_m40_v60_k7", "lda_m30_v50_k70_empty"])
def test_phi_of_a_trained_lda(tmvb, name):
    g = load(name)
    K, Vg = int(g["K"]), int(g["V"])
    m = tmvb.LDA(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], Vg), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_phi(tmvb, m, np.exp(m.Elogtheta), m.beta, K)
    if K == 7:                                             # a new corpus goes through predict first
        new = corpus(tmvb, [4, 0, 9], 41, Vg)
        tt = tmvb.token_topics(m, corp=new, top=3)
        p = tmvb.predict(new, m)
        ref = tr.restate(np.exp(p.Elogtheta), m.beta, new.doc_ptr, new.terms, new.counts, None, tr.EPSILON, 4)
        assert tt.topic.shape == (13, 3) and np.array_equal(tt.hard.sum(axis=1), [int(new.counts[:4].sum()), 0, int(new.counts[4:].sum())])
        close = np.abs(ref["top_r"][:, :-1] - ref["top_r"][:, 1:]).min(axis=1) > 4 * tr.cap(K)         # rows whose fp64 order is beyond rounding
        assert close.any() and np.array_equal(tt.topic[close], ref["top_idx"][close][:, :3])
        with pytest.raises(tmvb.CorpusError):
            tmvb.token_topics(m, corp=corpus(tmvb, [3], 1, Vg + 1))


def test_phi_of_a_trained_ctm(tmvb):
    g = load("ctm_m40_v60_k5")
    K, Vg = int(g["K"]), int(g["V"])
    m = tmvb.CTM(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], Vg), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train_ctm(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_phi(tmvb, m, np.exp(m.lam - m.lam.max(axis=0, keepdims=True)), m.beta, K)


@pytest.mark.parametrize("name", ["ctpf_m40_v60_u15_k4", "ctpf_m30_v40_u12_k6_r1"])
def test_phi_of_a_trained_ctpf(tmvb, name):
    from scipy.special import digamma
    g = load(name)
    K, Vg, U = int(g["K"]), int(g["V"]), int(g["U"])
    m = tmvb.CTPF(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], Vg, g["rdr_ptr"], g["readers"], g["ratings"], U), K)
    m.alef = np.asfortranarray(g["alef0"]); m.alef_old = m.alef.copy(order="F")
    tmvb.gpu_train_ctpf(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    a = digamma(m.gimel) - np.log(m.dalet)[:, None] - np.log(m.bet)[:, None]
    b = digamma(m.alef)
    check_phi(tmvb, m, np.exp(a - a.max(axis=0, keepdims=True)), np.exp(b - b.max(axis=0, keepdims=True)), K)
