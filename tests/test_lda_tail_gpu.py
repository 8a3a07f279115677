"""
The pipelined LDA iteration with the side stream at high priority, on a small corpus with the plan forced by TMVB_LDA_PIECES.

TMVB_LDA_SIDE_PRIORITY only moves the long documents' kernels and the side chain (Elogtheta column sums, update_alpha!) to another hardware queue, so
these tests are a regression net for STREAM ORDERING and nothing else: on or off the state must be the same bits, which can fail only if a dependency
between the streams is missing; and the paths around the tail (the second statistics buffer merged by update_beta! or handed out before it, train!'s
checked iterations, a sharded handle) are run once with the stream as it now is, against the fp64 oracle or against the stepwise calls.

The corpus has documents in every grid class of KP = 52 and for both long kernels (the ones aux[1] carries).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tol import within          # tests/tol.py holds the frozen tolerances

V = 600


def tail_corpus():
    """~3 000 documents over 600 terms: 2 400 of 8-64 unique terms, 300 of 65-96, 150 of 97-128, 100 of 129-192, four of 193-384, two of 385-768;
    term 0 is in every document (more than one chunk of postings in every piece)."""
    rng = np.random.Generator(np.random.PCG64(20261020))
    lens = np.concatenate([rng.integers(8, 65, 2400), rng.integers(65, 97, 300), rng.integers(97, 129, 150), rng.integers(129, 193, 100),
                           [200, 250, 300, 384], [400, 590]])
    rng.shuffle(lens)
    w = 1.0 / np.arange(1, V, dtype=np.float64) ** 0.9
    w /= w.sum()
    ptr, terms, counts = [0], [], []
    for n in lens:
        t = np.concatenate([[0], 1 + rng.choice(V - 1, size=int(n) - 1, replace=False, p=w)]).astype(np.int32)
        t.sort()
        terms.append(t); counts.append(rng.integers(1, 6, len(t)).astype(np.int32)); ptr.append(ptr[-1] + len(t))
    return np.asarray(ptr, dtype=np.int64), np.concatenate(terms), np.concatenate(counts)


@pytest.fixture(scope="module")
def corp():
    return tail_corpus()


@pytest.fixture(scope="module")
def beta0(tmvb):
    return {K: tmvb.dirichlet_rows(K, V, seed=3) for K in (50, 100)}


def model(tmvb, monkeypatch, corp, beta0, K, pieces=None, side_priority=True, ctx=None):
    """a gpuLDA on the corpus with the switches as given (both are read when the model is created)"""
    if pieces is None:
        monkeypatch.delenv("TMVB_LDA_PIECES", raising=False)
    else:
        monkeypatch.setenv("TMVB_LDA_PIECES", str(pieces))
    monkeypatch.setenv("TMVB_LDA_SIDE_PRIORITY", "1" if side_priority else "0")
    pc = tmvb.PackedCorpus(corp[0], corp[1], corp[2], V)
    gm = tmvb.gpuLDA(pc, K, ctx=ctx) if ctx is not None else tmvb.gpuLDA(pc, K)
    gm.beta = np.asfortranarray(beta0[K]); gm.beta_old = gm.beta.copy(order="F"); gm.update_buffer()
    return gm


def iterate(gm, K, n=5, viter=10, vtol=None):
    vtol = 1.0 / K ** 2 if vtol is None else vtol
    for _ in range(n):
        gm.estep(viter, vtol); gm.reduce_docs(); gm.update_beta(); gm.update_alpha(1000, 1.0 / K ** 2)
    gm.update_host()
    return gm


def same_bits(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("beta", "alpha", "gamma", "Elogtheta"))


def test_corpus_and_forced_plan(tmvb, monkeypatch, corp, beta0):
    doc_ptr, terms, _ = corp
    lens = np.diff(doc_ptr)
    assert 2900 <= len(lens) <= 3100 and terms.max() == V - 1
    for lo, hi, least in ((1, 64, 100), (65, 96, 50), (97, 128, 50), (129, 192, 50), (193, 384, 3), (385, 768, 1)):     # grid classes of KP = 52, the two long kernels
        assert ((lens >= lo) & (lens <= hi)).sum() >= least, (lo, hi)
    # TMVB_LDA_PIECES is honoured below the size at which the default takes the pipelined plan
    gm = model(tmvb, monkeypatch, corp, beta0, 50, pieces=3)
    assert gm.estep_pieces() == 3
    gm.close()


def test_side_priority_keeps_every_bit_k50(tmvb, monkeypatch, corp, beta0):
    """Five iterations as bench.py calls them: the side stream at high priority against a normal one, and the new path twice."""
    ref = iterate(model(tmvb, monkeypatch, corp, beta0, 50, pieces=3, side_priority=False), 50)
    new = iterate(model(tmvb, monkeypatch, corp, beta0, 50, pieces=3), 50)
    assert same_bits(new, ref)
    again = iterate(model(tmvb, monkeypatch, corp, beta0, 50, pieces=3), 50)
    assert same_bits(again, new)
    np.testing.assert_allclose(new.beta.sum(axis=1), 1.0, rtol=1e-5)


def test_statistics_handed_out_before_update_beta(tmvb, monkeypatch, corp, beta0):
    """stats() between the E-step and update_beta!, and an E-step behind an E-step: the second buffer is merged on the context's stream while the side
    chain runs on the other queue -- same bits with either stream."""
    a = model(tmvb, monkeypatch, corp, beta0, 50, pieces=3)
    b = model(tmvb, monkeypatch, corp, beta0, 50, pieces=3, side_priority=False)
    for gm in (a, b):
        for _ in range(2):
            gm.estep(10, 1.0 / 2500); gm.reduce_docs(); gm.stats(); gm.update_beta(); gm.update_alpha(1000, 1.0 / 2500)
        gm.estep(10, 1.0 / 2500); gm.estep(10, 1.0 / 2500); gm.reduce_docs(); gm.update_beta(); gm.update_alpha(1000, 1.0 / 2500)     # an E-step behind an E-step
        gm.update_host()
    assert same_bits(a, b)


@pytest.mark.parametrize("K,pieces,want", [(50, 3, 3), (100, 2, 2), (100, None, 1), (50, 1, 1)])
def test_against_the_oracle(tmvb, oracle, monkeypatch, corp, beta0, K, pieces, want):
    """Five iterations against the fp64 oracle at the frozen LDA tolerances (oracle/parity.py): the K = 50 plan (high-priority side stream), two pieces
    (what K = 100 takes on a large corpus) and the one-pass plan (both keep a normal stream)."""
    from oracle import parity
    gm = model(tmvb, monkeypatch, corp, beta0, K, pieces=pieces)
    assert gm.estep_pieces() == want
    om = oracle.LDA(oracle.CSR(corp[0], corp[1], corp[2], V), K, beta0[K])
    block, _ = parity.lda_parity(gm, om, iters=5)
    assert block["pass"], block["worst"]
    np.testing.assert_allclose(gm.beta.sum(axis=1), 1.0, rtol=1e-5)


def test_train_elbo_trajectory_equals_stepwise(tmvb, monkeypatch, corp, beta0):
    """train! with a check in every iteration (lda_elbo_doc_kernel on a third stream waits for the side stream's events) against the same operators
    called one by one with the host synchronising in between, which collect the parts in every E-step (TMVB_LDA_ELBO_PARTS=2): same trajectory, same state."""
    K = 50
    a = model(tmvb, monkeypatch, corp, beta0, K, pieces=3)
    traj = np.asarray(a.train(iter=5, tol=0.0, checkelbo=1, printelbo=False), dtype=np.float64)
    monkeypatch.setenv("TMVB_LDA_ELBO_PARTS", "2")
    b = model(tmvb, monkeypatch, corp, beta0, K, pieces=3)
    step = []
    for _ in range(5):
        b.estep(10, 1.0 / K ** 2); b.synchronize()
        b.reduce_docs(); b.synchronize()
        b.update_beta(); b.synchronize()
        b.update_alpha(1000, 1.0 / K ** 2); b.synchronize()
        step.append(b.update_elbo())
    b.update_host()
    assert a.elbo_form() == 1 and b.elbo_form() == 1
    assert len(traj) == 5 and np.array_equal(traj, np.asarray(step, dtype=np.float64)), (traj, step)
    assert same_bits(a, b)


def test_sharded_handle_on_one_gpu(tmvb, monkeypatch, corp, beta0):
    """A sharded handle (host transport, one rank holding every document) accumulates all passes in the one buffer it all-reduces: no second buffer
    there.  Pinned sweeps; against the single-context run at the teacher-forced keys."""
    K = 50
    ref = iterate(model(tmvb, monkeypatch, corp, beta0, K, pieces=3), K, viter=5, vtol=0.0)
    ctx = tmvb.DeviceContext(0)
    comm = tmvb.Communicator.host(ctx, 1, 0, lambda a: None)
    gm = model(tmvb, monkeypatch, corp, beta0, K, pieces=3, ctx=ctx)
    gm.set_comm(comm, gm.M)
    ptr, n = gm.stats()
    for _ in range(5):
        gm.estep(5, 0.0); gm.reduce_docs(); comm.allreduce(ptr, n); gm.update_beta(); gm.update_alpha(1000, 1.0 / K ** 2)
    gm.update_host()

    def rel(x, y):
        return np.abs(x - y) / np.maximum(np.abs(y), 1e-300)
    within("lda.gamma_rel", rel(gm.gamma, ref.gamma), "gamma")
    within("lda.Elogtheta_rel", rel(gm.Elogtheta, ref.Elogtheta), "Elogtheta")
    big = ref.beta > 1e-6
    within("lda.beta_rel", rel(gm.beta[big], ref.beta[big]), "beta")
    within("lda.beta_abs", np.abs(gm.beta - ref.beta), "beta")
    within("lda.alpha_rel", rel(gm.alpha, ref.alpha), "alpha")
    gm.close(); comm.close()
