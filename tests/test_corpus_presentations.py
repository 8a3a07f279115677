"""
The premise of tests/test_corpus_presentations_gpu.py, on the CPU: in fp64 a model does not care how its corpus is presented.

  * every presentation of tests/presentations.py is the canonical CSR again once condensed, sorted and mapped back;
  * P5 puts two entries of one document on postings 255 and 256 of a hot id (two partial-sum slots of the statistics pass), and moves both long
    documents to another kernel of lda_build_buckets (K = 50);
  * three free-running iterations of each of the five models reproduce the canonical run after mapping, every state field and the ELBO trajectory,
    at rel <= 1e-10 (only the fp64 summation order differs): the NumPy oracle (oracle/oracle_np.py) on P1 - P4, and on P5 / P6 thin subclasses of it
    whose update_*_doc scatters use np.add.at.  WHY subclasses: the shipped oracle keeps quirk Q1 of SURVEY.md -- the reference's `X[:, idx] += ...`
    OVERWRITES a repeated id -- and stays that way; the engine's contract for repeats (include/tmvb.h: they accumulate, the result is that of the
    condensed document) is what the accumulating subclasses state.  The NumPy oracle runs Python loops per document, per entry and topic in CTPF's
    update_elbo!: it gets a corpus of the same make at M = 40, V = 100 (CTPF: M = 24, V = 60, U = 12; the straddle and the buckets are properties of the device's builders, not
    of the model);
  * THE ONE EXCEPTION: CTPF's ELBO under P5 / P6.  _binom_lgamma_sum and _multinomial_entropy are not additive in a count: the Binomial sums cancel
    between them and -lgamma(c + 1) per entry is left, so splitting entries moves the ELBO by presentations.ctpf_elbo_shift, a constant of the
    presentation.  It is asserted that the ELBO DOES differ there, by exactly that constant, and nowhere else;
  * the C oracle (oracle/oracle.py) at full size on P1 - P4 agrees with its own canonical run at the same bound.
"""
import numpy as np
import pytest

import presentations as P
from oracle import oracle_np as onp

RTOL = 1e-10
K_NP = 3


# ------------------------------------------------------------------------------------------------ the presentations themselves
@pytest.fixture(scope="module")
def canons():
    return {"plain": P.canonical(), "cover": P.canonical(cover=True), "readers": P.canonical(U=120)}


@pytest.mark.parametrize("which", ["plain", "cover", "readers"])
def test_every_presentation_is_the_canonical_corpus(canons, which):
    c = canons[which]
    want = (c.doc_ptr, c.terms, c.counts, c.rdr_ptr, c.readers, c.ratings)
    L = np.diff(c.doc_ptr)
    sp = c.info["special"]
    assert L[sp["empty"]] == 0 and (L[sp["one"]], c.counts[c.doc_ptr[sp["one"]]]) == (1, 1) and (L[sp["seven"]], c.counts[c.doc_ptr[sp["seven"]]]) == (1, 7)
    assert (L[sp["long_a"]], L[sp["long_b"]]) == (300, 700) and c.M >= 320
    for h in c.info["hot"]:
        assert len(c.postings(h)[0]) == 318 > P.CHUNK                     # every non-empty document but one: two chunks
    used = np.zeros(c.V, bool); used[c.terms] = True
    assert (~used).sum() == (0 if which == "cover" else 50)
    if which == "readers":
        assert len(c.postings(c.info["hot_reader"], readers=True)[0]) > P.CHUNK and (np.diff(c.rdr_ptr) == 0).sum() >= 30 and c.ratings.max() > 1
    for name in P.NAMES:
        p = P.present(c, name)
        for a, b in zip(want, p.condensed()):
            assert np.array_equal(a, b), name
        assert np.array_equal(np.sort(p.doc_of), np.arange(c.M)) and np.array_equal(np.sort(p.term_to), np.arange(c.V))
        assert np.array_equal(p.term_to[c.terms[p.entry_of]], p.terms) and np.array_equal(np.bincount(p.entry_of, weights=p.counts, minlength=len(c.counts)), c.counts)
        info = p.numpy_info()
        assert info["sum_counts"] == c.counts.sum() and info["sum_ratings"] == c.ratings.sum()
        assert (info["n_docs_with_duplicate_terms"] > 0) == (name in ("P5", "P6"))
    # each presentation does what its name says
    p1, p2, p3, p5 = (P.present(c, n) for n in ("P1", "P2", "P3", "P5"))
    d = sp["long_a"]
    assert not np.array_equal(p1.terms[p1.doc_ptr[d]:p1.doc_ptr[d + 1]], c.terms[c.doc_ptr[d]:c.doc_ptr[d + 1]])
    assert np.all(np.diff(p2.terms[p2.doc_ptr[d]:p2.doc_ptr[d + 1]]) < 0)
    assert list(p3.doc_of[-3:]) == [sp["empty"], sp["long_a"], sp["long_b"]]
    same_len = [(x, y) for x in range(c.M) for y in range(x + 1, min(x + 40, c.M)) if L[x] == L[y] and L[x] > 1]
    assert any(p3.pos_of[x] > p3.pos_of[y] for x, y in same_len)           # equal-length documents swapped: the stable longest-first sort keeps it
    a = p5.doc_ptr[p5.pos_of[sp["seven"]]]
    assert p5.doc_ptr[p5.pos_of[sp["seven"]] + 1] - a == 3 and len(set(p5.terms[a:a + 3])) == 1 and p5.counts[a:a + 3].sum() == 7
    rep = [np.flatnonzero(np.diff(np.sort(p5.terms[p5.doc_ptr[i]:p5.doc_ptr[i + 1]])) == 0).size for i in range(p5.M)]
    adj = [np.flatnonzero(np.diff(p5.terms[p5.doc_ptr[i]:p5.doc_ptr[i + 1]]) == 0).size for i in range(p5.M)]
    assert sum(adj) < 0.2 * sum(rep)                                       # the repeats are not adjacent as a rule


@pytest.mark.parametrize("which", ["plain", "cover", "readers"])
def test_p5_straddles_a_chunk_boundary_of_the_statistics_pass(canons, which):
    """posting order = id-major, then document order, then entry order (the counting sort of tmvb_build_inv_index), restated from the sort itself"""
    p = P.present(canons[which], "P5")
    h, pos = P.straddle(p)
    j = p.term_to[h]
    doc_of_entry = np.repeat(np.arange(p.M), np.diff(p.doc_ptr))
    order = np.lexsort((np.arange(len(p.terms)), doc_of_entry, p.terms))       # by id, then document, then entry
    mine = order[p.terms[order] == j]
    assert np.array_equal(mine, p.postings(j)[1])
    assert doc_of_entry[mine[P.CHUNK - 1]] == doc_of_entry[mine[P.CHUNK]] == pos
    assert P.straddle(canons[which]) is None                                   # a condensed corpus cannot have it


def lda_bucket_k50(n):
    """lda_build_buckets (csrc/tmvb_lda.hip) at K = 50: KP = 52, 13 floats per lane, up to 4 register tiles, 6 token pairs per lane of the grid-tile kernel"""
    if n > 64 * 4 * 4:
        return "lds-tile"                    # longer than long_max = 64 * max_tiles * TMVB_LONG_WAVES = 1024
    if n > 32 * 6 * 4:
        return "long-register"               # 768 < n <= 1024: lda_estep_reg_long_kernel, four waves
    if n > 32 * 6 * 2:
        return "grid-4-wave"                 # 384 < n <= 768
    if n > 32 * 6:
        return "grid-2-wave"                 # 192 < n <= 384
    return "grid"                            # one wave per document


def test_p5_moves_the_long_documents_to_other_kernels(canons):
    c = canons["plain"]
    p = P.present(c, "P5")
    sp = c.info["special"]
    before = [int(np.diff(c.doc_ptr)[sp[k]]) for k in ("long_a", "long_b")]
    after = [int(np.diff(p.doc_ptr)[p.pos_of[sp[k]]]) for k in ("long_a", "long_b")]
    assert before == [300, 700] and after == [454, 1068]                       # entries, not unique ids
    assert [lda_bucket_k50(n) for n in before] == ["grid-2-wave", "grid-4-wave"]
    assert [lda_bucket_k50(n) for n in after] == ["grid-4-wave", "lds-tile"]
    assert np.sort(np.diff(p.doc_ptr))[-3] <= 192                                # every other document stays on one wave


# ------------------------------------------------------------------------------------------------ the NumPy oracle, accumulating
class AccLDA(onp.LDA):
    def update_beta_doc(self, d):
        terms, counts = self.docs[d]
        np.add.at(self.beta_temp, (slice(None), terms), self.phi * counts[None, :])


class AccfLDA(onp.fLDA):
    def update_beta_doc(self, d):
        terms, counts = self.docs[d]
        np.add.at(self.beta_temp, (slice(None), terms), self.phi * (self.tau[d] * counts)[None, :])

    def update_kappa_doc(self, d):
        terms, counts = self.docs[d]
        np.add.at(self.kappa_temp, terms, (1.0 - self.tau[d]) * counts)


class AccCTM(onp.CTM):
    update_beta_doc = AccLDA.update_beta_doc


class AccfCTM(onp.fCTM):
    update_beta_doc = AccfLDA.update_beta_doc
    update_kappa_doc = AccfLDA.update_kappa_doc


class AccCTPF(onp.CTPF):
    def update_he_doc(self, d):
        readers, ratings = self.docs[d][2], self.docs[d][3]
        np.add.at(self.he_temp, (slice(None), readers), (self.xi[:self.K, :] + self.xi[self.K:, :]) * ratings[None, :])

    def update_alef_doc(self, d):
        terms, counts = self.docs[d][0], self.docs[d][1]
        np.add.at(self.alef_temp, (slice(None), terms), self.phi * counts[None, :])


NP_MODELS = {"lda": (onp.LDA, AccLDA), "flda": (onp.fLDA, AccfLDA), "ctm": (onp.CTM, AccCTM), "fctm": (onp.fCTM, AccfCTM), "ctpf": (onp.CTPF, AccCTPF)}


def init_of(model, K, V, seed=5):
    rng = np.random.default_rng(seed)
    b = rng.standard_exponential(size=(K, V)); b /= b.sum(axis=1, keepdims=True)
    if model == "ctpf":
        return dict(alef0=np.exp(b - 0.5))
    g = dict(beta0=b)
    if model in ("flda", "fctm"):
        k = rng.standard_exponential(size=V); g["kappa0"] = k / k.sum()
    return g


def np_state(m, model):
    """the NumPy oracle keeps per-document vectors in lists: K x M matrices and flat per-entry arrays, as oracle/oracle.py and the device hold them"""
    out = {}
    for n in P.FIELDS[model]:
        v = getattr(m, n)
        if isinstance(v, list):
            v = np.concatenate(v) if P.KIND[n] == "entry" else np.stack(v, axis=1)
        out[n] = np.array(v, dtype=np.float64) if not np.isscalar(v) else float(v)
    return out


def np_run(model, p, K, accumulate):
    cls = NP_MODELS[model][1 if accumulate else 0]
    init = {n: p.cols(v) for n, v in init_of(model, K, p.V).items()}
    if model == "ctpf":
        m = cls(p.doc_lists(readers=True), p.V, p.U, K, init["alef0"])
    else:
        m = cls(p.doc_lists(), p.V, K, *[init[n] for n in ("beta0", "kappa0") if n in init])
    traj = np.array(m.train(iter=3, tol=-np.inf, checkelbo=1))
    assert len(traj) == 3
    return traj, np_state(m, model)


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-6 * np.abs(b).max() + 1e-300)).max())


def assert_same_run(model, p, traj, state, traj0, state0, elbo_shift=0.0):
    o = P.view(state0, p)
    for n in P.FIELDS[model]:
        assert close(state[n], getattr(o, n)) <= RTOL, (model, p.name, n, close(state[n], getattr(o, n)))
    assert close(traj, traj0 + elbo_shift) <= RTOL, (model, p.name, traj, traj0 + elbo_shift)


@pytest.mark.parametrize("model", sorted(NP_MODELS))
def test_numpy_oracle_reproduces_the_canonical_run_on_every_presentation(model):
    if model == "ctpf":                                            # update_elbo! evaluates a Binomial pmf per entry and topic in Python: smaller still, K = 2
        c, K = P.canonical(seed=3, M=24, V=60, U=12), 2
    else:
        c, K = P.canonical(seed=3, M=40, V=100, cover=model in ("ctm", "fctm")), K_NP
    traj0, state0 = np_run(model, c, K, False)
    assert np.all(np.isfinite(traj0))
    t_acc, s_acc = np_run(model, c, K, True)                    # a condensed corpus: accumulating and overwriting are the same thing
    assert_same_run(model, c, t_acc, s_acc, traj0, state0)
    for name in P.NAMES[1:]:
        p = P.present(c, name)
        split = name in ("P5", "P6")
        traj, state = np_run(model, p, K, accumulate=split)
        shift = P.ctpf_elbo_shift(p) if model == "ctpf" else 0.0
        assert (shift != 0.0) == (model == "ctpf" and split)
        if shift:                                                  # the named exception: it does differ, and by the constant
            assert np.all(np.abs(traj - traj0) > 1e-6 * np.abs(traj0)) and shift > 0
        assert_same_run(model, p, traj, state, traj0, state0, shift)
    # and the shipped (overwriting, quirk Q1) oracle is NOT that on a corpus with repeats: the subclasses are what makes P5 comparable
    p5 = P.present(c, "P5")
    _, s_q1 = np_run(model, p5, K, False)
    f = "alef" if model == "ctpf" else "beta"
    assert close(s_q1[f], getattr(P.view(state0, p5), f)) > 1e-3


# ------------------------------------------------------------------------------------------------ the C oracle, P1 - P4
def c_oracle(oracle, model, p, K):
    init = {n: p.cols(v) for n, v in init_of(model, K, p.V).items()}
    csr = oracle.CSR(p.doc_ptr, p.terms, p.counts, p.V, *((p.rdr_ptr, p.readers, p.ratings, p.U) if p.U else ()))
    cls = dict(lda=oracle.LDA, flda=oracle.fLDA, ctm=oracle.CTM, fctm=oracle.fCTM, ctpf=oracle.CTPF)[model]
    return cls(csr, K, *[init[n] for n in ("beta0", "alef0", "kappa0") if n in init])


@pytest.mark.parametrize("model,K", [("lda", 7), ("flda", 9), ("ctm", 12), ("fctm", 4), ("ctpf", 8)])
def test_c_oracle_agrees_with_itself_on_p1_to_p4(oracle, canons, model, K):
    c = canons["readers" if model == "ctpf" else "cover" if model in ("ctm", "fctm") else "plain"]
    runs = {}
    for name in P.NAMES[:5]:
        p = P.present(c, name)
        om = c_oracle(oracle, model, p, K)
        traj = np.asarray(om.train(iter=3, tol=-np.inf, checkelbo=1))
        assert len(traj) == 3 and np.all(np.isfinite(traj))
        runs[name] = (p, traj, P.snapshot(om, P.FIELDS[model]))
    _, traj0, state0 = runs["P0"]
    for name in P.NAMES[1:5]:
        p, traj, state = runs[name]
        assert_same_run(model, p, traj, state, traj0, state0)
