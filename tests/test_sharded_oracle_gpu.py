"""
Document-sharded iterations against the fp64 oracle, stepwise, at even and at ragged shard cuts -- one process, one device open.

The other sharded tests (tests/test_dist_gpu.py, test_comm_gpu.py, test_sliced_allreduce_gpu.py) compare a world-2 run with the device's own
single-context run, at near-even cuts and loose literal tolerances: an error the two runs share, or one that only a rank without documents makes, is
invisible to them.  Here every rank of a partition (tests/shard_cuts.py: even2, even3, even8, ragged6 -- the last with a rank that holds NO document,
one that holds only the empty document, one with only the 700-term document, one with a single one-entry document) is a sharded handle on a context of
its own, and the all-reduce is SCRIPTED through free-standing host communicators: pass 1 copies every rank's packed statistics out, the test sums the
W copies in float64 in rank order and rounds once to float32, pass 2 hands that total to every rank.  Then the M-step and update_elbo! of every rank.

Two teacher-forced iterations with pinned sweeps (viter = 3, vtol = 0) on the canonical corpus of tests/presentations.py; before each, every rank is
forced with the oracle's state (per-document fields sliced to its documents, globals whole) -- two, because what a rank leaves in its statistics
buffer after the first must not leak into the second (an empty CTM rank that kept the all-reduced scatter matrix in its tail would hand it back:
mutant mut_ctm_empty_tail, tests/test_mutants_gpu.py).  The C oracle runs once per (model, K) on the whole corpus, cached by
tests/test_corpus_presentations_gpu.py, whose step / force / compare functions and frozen teacher-forced keys (tests/tol.py) are the ones used here,
over EVERY entry:

  * per-document fields of all ranks side by side in document order, the globals of rank 0 and the summed ELBO (LDA / CTM: sum of the ranks'
    update_elbo!, each scaling its corpus term by M / M_total; CTPF: sum of the document parts + the global part once) through the model's compare;
  * the globals of every rank array_equal to rank 0's (every rank received the same total), CTPF's global ELBO part too;
  * doc_sweeps() = 3 for every non-empty document; an empty rank's update_elbo! finite, its CTPF document part exactly 0.0.

What a sharded step adds to the single-context arithmetic is one more rounding of each statistic (W fp32 partial sums, summed in fp64, rounded once)
and, for LDA, alpha from the fp32 Elogtheta sum of the statistics tail instead of the fp64 device sum.  Measured on MI355X
(profiles/sharded_tolerances_measured.json), every quantity stays inside its single-context key.
"""
import types

import numpy as np
import pytest

import presentations as P
import shard_cuts as SC
from test_corpus_presentations_gpu import MODELS, VITER, canon, oracle_states

pytestmark = pytest.mark.gpu

CASES = [("lda", 7, 0), ("lda", 50, 0), ("lda", 130, 0), ("lda", 50, 3), ("ctm", 12, 0), ("ctm", 50, 0), ("ctm", 100, 0), ("ctpf", 8, 0), ("ctpf", 50, 0)]


def _mstep(model, gm):
    """the model's step of tests/test_corpus_presentations_gpu.py behind its E-step and reduce_docs"""
    if model == "lda":
        gm.update_beta(); gm.update_alpha()
    elif model == "ctm":
        gm.update_beta(); gm.update_sigma(); gm.update_mu()
    else:
        gm.mstep()


def _estep(model, gm):
    gm.estep(viter=VITER, vtol=0.0)
    gm.reduce_docs()


def _slice(o, names, d0, d1):
    """an oracle state (a presentations.view) cut to the documents [d0, d1): per-document fields sliced, globals whole"""
    s = types.SimpleNamespace()
    for n in names:
        v = getattr(o, n)
        if P.KIND.get(n, "plain") == "doc":
            v = np.asarray(v)[..., d0:d1]
            v = np.asfortranarray(v) if v.ndim == 2 else v.copy()
        setattr(s, n, v)
    return s


class Rank:
    """one sharded handle on a context of its own + its free-standing host communicator with a scripted callback"""

    def __init__(self, tmvb, model, K, shard, M_total, W, r):
        self.ctx = tmvb.DeviceContext(0)
        self.gm = {"lda": tmvb.gpuLDA, "ctm": tmvb.gpuCTM, "ctpf": tmvb.gpuCTPF}[model](shard, K, ctx=self.ctx)
        if model == "ctpf":
            self.gm.set_distributed(True)
        else:
            self.gm.set_distributed(M_total, True)
        self.copy, self.total = None, None
        self.comm = tmvb.Communicator.host(self.ctx, W, r, self._fn)

    def _fn(self, a):
        if self.total is None:
            self.copy = np.array(a, copy=True)                         # pass 1: look, leave unchanged
        else:
            assert a.shape == self.total.shape and a.dtype == self.total.dtype
            a[:] = self.total                                          # pass 2: the total every rank receives

    def allreduce(self):
        ptr, n = self.gm.stats()
        self.comm.allreduce(ptr, n)
        return n

    def close(self):
        self.gm.close(); self.comm.close(); self.gm.dcorp.close(); self.ctx.close()


def scripted_allreduce(ranks):
    for k in ranks:
        k.copy, k.total = None, None
        n = k.allreduce()
        assert k.copy is not None and k.copy.shape == (n,) and k.copy.dtype == np.float32
    assert len({k.copy.shape for k in ranks}) == 1
    tot = np.zeros(ranks[0].copy.shape, dtype=np.float64)
    for k in ranks:                                                    # rank order, float64
        tot += k.copy.astype(np.float64)
    tot = tot.astype(np.float32)                                       # rounded once
    for k in ranks:
        k.total = tot
        k.allreduce()
        k.total = None


@pytest.mark.parametrize("part", SC.NAMES)
@pytest.mark.parametrize("model,K,pieces", CASES, ids=[f"{m}_k{k}" + (f"_pieces{q}" if q else "") for m, k, q in CASES])
def test_sharded_teacher_forced_fixed_sweeps(tmvb, oracle, model, K, pieces, part, monkeypatch):
    if pieces:
        monkeypatch.setenv("TMVB_LDA_PIECES", str(pieces))             # read at create
    mod, _, compare, names, _ = MODELS[model]
    c = canon(model)
    p, corpus, cuts = SC.partition(tmvb, c, part)
    W = len(cuts) - 1
    states = oracle_states(tmvb, oracle, model, K, True)
    ranks = [Rank(tmvb, model, K, corpus.shard(cuts[r], cuts[r + 1]), corpus.M, W, r) for r in range(W)]
    empty = [r for r in range(W) if cuts[r] == cuts[r + 1]]
    assert (len(empty) == 1) == (part == "ragged6")
    doc_fields = [n for n in names if P.KIND.get(n, "plain") == "doc"]
    glob_fields = [n for n in names if n not in doc_fields]
    nonempty = np.diff(p.doc_ptr) > 0
    try:
        for it in range(2):
            before = P.view({n: states[it][n] for n in names}, p)
            for r, k in enumerate(ranks):
                mod.force(k.gm, _slice(before, names, cuts[r], cuts[r + 1]))
            for k in ranks:
                _estep(model, k.gm)
            scripted_allreduce(ranks)
            for k in ranks:
                _mstep(model, k.gm)
            if model == "ctpf":
                parts = [k.gm.update_elbo_parts() for k in ranks]
                e_g = sum(a for a, _ in parts) + parts[0][1]
                for r in range(W):
                    assert parts[r][1] == parts[0][1], (r, parts)           # the global part: the same on every rank
                    assert np.isfinite(parts[r][0]) and np.isfinite(parts[r][1])
                for r in empty:
                    assert parts[r][0] == 0.0, parts[r]
            else:
                es = [k.gm.update_elbo() for k in ranks]
                assert np.all(np.isfinite(es)), es
                e_g = sum(es)
            for k in ranks:
                k.gm.update_host()
            whole = types.SimpleNamespace(**{n: getattr(ranks[0].gm, n) for n in glob_fields})
            for n in doc_fields:
                setattr(whole, n, np.concatenate([np.asarray(getattr(k.gm, n)) for k in ranks], axis=-1))
            want = P.view(states[it + 1], p)
            assert all(getattr(whole, n).shape == np.shape(getattr(want, n)) for n in doc_fields)
            compare(whole, want, e_g, (model, K, part, it))
            for r, k in enumerate(ranks):
                for n in glob_fields:
                    assert np.array_equal(getattr(k.gm, n), getattr(ranks[0].gm, n)), (part, it, r, n)
            sw = np.concatenate([k.gm.doc_sweeps() for k in ranks])
            assert np.all(sw[nonempty] == VITER) and np.array_equal(sw, want.sw), (part, it, np.flatnonzero(sw != want.sw))
    finally:
        for k in ranks:
            k.close()
