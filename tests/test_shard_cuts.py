"""
The CPU side of the sharded oracle tests (tests/test_sharded_oracle_gpu.py):

  * the four partitions of tests/shard_cuts.py cover [0, M) without overlap on each of the three canonical corpora (plain, with the covering document
    of CTM, with readers), and ragged6 has its five properties (an empty rank between two that hold documents, a rank with only the empty document,
    one with only the 700-term document, one with a single one-entry document, two with the rest);
  * the PREMISE of comparing a sharded device run with the whole-corpus oracle, in fp64 for LDA: per-shard oracle E-steps (the oracle-backed engine
    of tests/test_dist_gloo.py), the packed statistics summed over the ranks in float64, one identical M-step -- reproduces the whole-corpus oracle
    step to 1e-10 under even3 and ragged6, the empty rank and the nnz = 0 rank included.  (The other models' oracles are not extended for this.)
"""
import types

import numpy as np
import pytest

import presentations as P
import shard_cuts as SC
from test_dist_gloo import OracleLDAEngine

CANON = {"plain": dict(), "cover": dict(cover=True), "ctpf": dict(U=120)}
_C = {}


def _canon(kind):
    if kind not in _C:
        _C[kind] = P.canonical(**CANON[kind])
    return _C[kind]


@pytest.mark.parametrize("kind", sorted(CANON))
@pytest.mark.parametrize("name", SC.NAMES)
def test_partitions_cover_the_corpus(tmvb, kind, name):
    canon = _canon(kind)
    p, corpus, cuts = SC.partition(tmvb, canon, name)             # asserts cover / no overlap (and ragged6's properties) itself
    W = len(cuts) - 1
    assert W == (6 if name == "ragged6" else int(name[4:]))
    assert corpus.M == canon.M == p.M and corpus.nnz == canon.doc_ptr[-1] and corpus.nR == canon.rdr_ptr[-1]
    # the shards, put side by side again, are the presentation's CSR
    shards = [corpus.shard(cuts[r], cuts[r + 1]) for r in range(W)]
    assert [s.M for s in shards] == list(np.diff(cuts))
    assert np.array_equal(np.concatenate([s.terms for s in shards]), p.terms) and np.array_equal(np.concatenate([s.counts for s in shards]), p.counts)
    assert np.array_equal(np.concatenate([s.readers for s in shards]), p.readers)
    assert np.array_equal(np.concatenate([[0]] + [s.doc_ptr[1:] + p.doc_ptr[cuts[r]] for r, s in enumerate(shards)]), p.doc_ptr)
    if name != "ragged6":
        w = np.array([s.nnz + s.nR for s in shards], dtype=np.float64)
        assert w.max() <= 2.0 * w.mean() + p.info["canon"].V                 # near-even: no rank beyond twice its share plus one long document


def test_ragged6_properties_are_checked_not_assumed(tmvb):
    """check_ragged refuses cuts that lack a property (so a change of the canonical corpus cannot hollow ragged6 out unseen)"""
    canon = _canon("plain")
    p, _, cuts = SC.partition(tmvb, canon, "ragged6")
    SC.check_ragged(p, cuts)
    a = cuts[1]
    for bad in ([0, a, a + 1, a + 1, a + 2, a + 3, p.M],           # the empty rank gone, the empty document's rank first
                [0, a - 1, a - 1, a + 1, a + 2, a + 3, p.M],       # the empty document shares its rank
                [0, a, a, a + 1, a + 3, a + 3, p.M]):              # the long document shares its rank, the one-entry rank is empty
        SC.check_cuts(p, bad, 6)
        with pytest.raises(AssertionError):
            SC.check_ragged(p, bad)
    with pytest.raises(AssertionError):
        SC.check_cuts(p, [0, a, a, a + 1, a + 2, a + 3, p.M - 1], 6)
    # and the canonical order could not have carried it: the three documents are not neighbours there
    sp = canon.info["special"]
    assert max(sp["empty"], sp["long_b"], sp["one"]) - min(sp["empty"], sp["long_b"], sp["one"]) > 2


def test_the_sharded_runs_stayed_inside_the_existing_keys():
    """profiles/sharded_tolerances_measured.json is `TMVB_TOL_RECORD=1 pytest -m gpu` of the two sharded oracle files on one MI355X: every quantity they
    compare uses an existing key of tests/tol.py unchanged, and the worst value measured lies inside it (no `sharded.*` key was needed; a quantity that
    leaves its key gets one, at most 10 x its measurement, with the rounding that causes it named in DESIGN.md section 6)."""
    import json
    import os
    import tol
    ev = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sharded_tolerances_measured.json")))
    assert len(ev) >= 30 and not [k for k in tol.TOL if k.startswith("sharded.")]
    for k, m in ev.items():
        assert k in tol.TOL and 0.0 <= m <= tol.TOL[k], (k, m, tol.TOL.get(k))
    for fam in ("lda", "ctm", "ctpf", "flda", "fctm"):
        assert f"{fam}.elbo_rel_free" in ev                                # every model's sharded train! was measured
    for k in ("lda.gamma_rel", "lda.alpha_rel", "ctm.lambda_err", "ctm.sigma_rel", "ctpf.shape_rel", "ctpf.rates_rel"):
        assert k in ev                                                     # and the stepwise file's per-document and global keys


@pytest.mark.parametrize("name", ["even3", "ragged6"])
def test_sharded_oracle_step_reproduces_the_whole_corpus_step(tmvb, oracle, name):
    K, VITER = 7, 3
    canon = _canon("plain")
    beta0 = tmvb.dirichlet_rows(K, canon.V, seed=5)
    whole = oracle.LDA(oracle.CSR(canon.doc_ptr, canon.terms, canon.counts, canon.V), K, beta0)
    p, corpus, cuts = SC.partition(tmvb, canon, name)
    W = len(cuts) - 1
    ranks = [OracleLDAEngine(oracle, corpus.shard(cuts[r], cuts[r + 1]), K, beta0, corpus.M) for r in range(W)]
    for it in range(2):
        whole.estep(viter=VITER, vtol=0.0); whole.update_beta(); whole.update_alpha()
        e_o = whole.update_elbo()
        for e in ranks:
            e.estep(VITER, 0.0); e.reduce_docs()
        total = sum(e.stats.numpy().astype(np.float64) for e in ranks)               # rank order, float64
        for e in ranks:
            e.stats[:] = e.stats.new_tensor(total)
            e.update_beta(); e.update_alpha(1000, 1.0 / K ** 2)
        e_s = sum(e.local_elbo() for e in ranks)
        want = P.view(dict(gamma=whole.gamma, Elogtheta=whole.Elogtheta, beta=whole.beta, alpha=whole.alpha), p)
        got = types.SimpleNamespace(gamma=np.concatenate([e.m.gamma for e in ranks], axis=1), Elogtheta=np.concatenate([e.m.Elogtheta for e in ranks], axis=1))
        assert got.gamma.shape == want.gamma.shape
        np.testing.assert_allclose(got.gamma, want.gamma, rtol=1e-10)
        np.testing.assert_allclose(got.Elogtheta, want.Elogtheta, rtol=1e-10)
        for e in ranks:
            np.testing.assert_allclose(e.m.beta, want.beta, rtol=1e-10, atol=1e-300)
            np.testing.assert_allclose(e.m.alpha, want.alpha, rtol=1e-10)
            assert np.array_equal(e.m.beta, ranks[0].m.beta) and np.array_equal(e.m.alpha, ranks[0].m.alpha)
        assert abs(e_s - e_o) <= 1e-10 * abs(e_o), (it, e_s, e_o)
        empty = [r for r in range(W) if cuts[r] == cuts[r + 1]]
        assert (len(empty) == 1) == (name == "ragged6")
        for r in empty:
            assert ranks[r].local_elbo() == 0.0
