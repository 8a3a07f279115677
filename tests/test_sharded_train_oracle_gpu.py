"""
The in-library sharded train (set_comm + train: the all-reduce of the packed statistics, the ELBO all-reduce and the stop decision inside
libtmvb_hip.so, csrc/tmvb_train.h) against the fp64 oracle's train! on the whole corpus, for all five models -- the only route by which fLDA and fCTM
shard (tmvb_fctm_* has no stats entry, and the grouped all-reduce refuses host communicators), hence concurrent ranks: three processes on one GPU,
the host transport with gloo carrying the sums, as tests/test_comm_gpu.py.

World 3 at ragged cuts: rank 0 holds the documents [0, M // 3) of the canonical corpus of tests/presentations.py, rank 1 holds NONE, rank 2 the rest
(the empty document M // 3 first).  Same corpus, K and initial state as test_train_free_running of tests/test_corpus_presentations_gpu.py, and the same
frozen keys (tests/tol.py): the trajectory of EVERY rank at the model's *.elbo_rel_free, the globals of FREE[model] at their *_free keys, tau of the
filtered models side by side over the ranks with the oracle's length; trajectory and globals array_equal across the three ranks.

The stop rule (LDA and CTPF, one per model family of the train loop): tol half way between two of the oracle's ELBO increments, chosen by stop_plan of
tests/test_train_loop_gpu.py -- every increment at least 100 x the model's *.elbo_rel_free x |ELBO| away from it, asserted on the oracle before any rank
is spawned -- so all three ranks must stop at exactly the oracle's iteration.
"""
import os
import sys
import tempfile
from datetime import timedelta

import numpy as np
import pytest

import presentations as P
import shard_cuts as SC
from test_corpus_presentations_gpu import FREE, MODELS, _init, canon, new_oracle
from test_train_loop_gpu import ITER, stop_plan
from tol import within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
WORLD = 3


def cuts_of(M):
    return [0, M // 3, M // 3, M]


def _gloo_sum(dist):
    import torch

    def fn(a):
        t = torch.from_numpy(a)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return fn


def _worker(rank, world, initfile, out_dir, model, iters, tol):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import tmvb_amd
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    tm = tmvb_amd.pkg
    c = canon(model)
    K = FREE[model][0]
    corpus = SC.packed(tm, c)
    cuts = cuts_of(corpus.M)
    shard = corpus.shard(cuts[rank], cuts[rank + 1])
    ctx = tm.DeviceContext(0)
    comm = tm.Communicator.host(ctx, world, rank, _gloo_sum(dist))
    gm = {"lda": tm.gpuLDA, "ctm": tm.gpuCTM, "ctpf": tm.gpuCTPF, "flda": tm.gpufLDA, "fctm": tm.gpufCTM}[model](shard, K, ctx=ctx)
    init = _init(tm, model, K, c.V)
    if model == "ctpf":
        gm.alef = np.asfortranarray(init["alef0"]); gm.alef_old = gm.alef.copy(order="F")
    else:
        gm.beta = np.asfortranarray(init["beta0"]); gm.beta_old = gm.beta.copy(order="F")
        if model in ("flda", "fctm"):
            gm.kappa = np.array(init["kappa0"], dtype=np.float64); gm.kappa_old = gm.kappa.copy()
    gm.update_buffer()
    if model == "ctpf":
        gm.set_comm(comm)
    elif model == "flda":
        gm.set_comm(comm, corpus.M, int(np.sum(corpus.C)))
    else:
        gm.set_comm(comm, corpus.M)
    kw = dict(recs=False) if model == "ctpf" else {}
    traj = gm.train(iter=iters, tol=tol, checkelbo=1, printelbo=False, **kw)
    out = {f: np.asarray(getattr(gm, f), dtype=np.float64) for f, _, _ in FREE[model][2]}
    if model in ("flda", "fctm"):
        out["tau"] = np.asarray(gm.tau, dtype=np.float64)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), traj=np.asarray(traj, dtype=np.float64), M=shard.M, **out)
    gm.close(); comm.close()
    dist.barrier()
    dist.destroy_process_group()


def _run(model, iters, tol):
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(WORLD, os.path.join(td, "init"), td, model, iters, tol), nprocs=WORLD, join=True)
        return [dict(np.load(os.path.join(td, f"rank{r}.npz"))) for r in range(WORLD)]


@pytest.mark.parametrize("model", sorted(FREE))
def test_sharded_train_world3_with_an_empty_rank(tmvb, oracle, model):
    K, ekey, fields = FREE[model]
    om = new_oracle(tmvb, oracle, model, K)
    t_o = np.asarray(om.train(iter=5, tol=0.0, checkelbo=1))
    assert len(t_o) == 5
    final = P.snapshot(om, MODELS[model][3])
    res = _run(model, 5, 0.0)
    M = canon(model).M
    assert [int(r["M"]) for r in res] == [M // 3, 0, M - M // 3]
    for q, r in enumerate(res):
        assert len(r["traj"]) == 5
        within(ekey, np.abs(r["traj"] - t_o) / np.abs(t_o), (model, "rank", q, r["traj"], t_o))
        assert np.array_equal(r["traj"], res[0]["traj"]), (model, q)                    # the same stop decision on every rank
        for f, key, how in fields:
            if f == "tau":
                continue
            a, b = r[f], np.asarray(final[f], dtype=np.float64)
            within(key, np.abs(a - b) / (np.abs(b) if how == "rel" else 1.0), (model, "rank", q, f))
            assert np.array_equal(a, res[0][f]), (model, q, f)
    if model in ("flda", "fctm"):
        tau = np.concatenate([r["tau"] for r in res])
        assert tau.shape == np.shape(final["tau"]) and len(res[1]["tau"]) == 0
        for f, key, how in fields:
            if f == "tau":
                within(key, np.abs(tau - final["tau"]), (model, "tau"))


@pytest.mark.parametrize("model", ["lda", "ctpf"])
def test_sharded_train_world3_stops_where_the_oracle_stops(tmvb, oracle, model):
    K = FREE[model][0]
    om = new_oracle(tmvb, oracle, model, K)
    base = om.update_elbo(store=False)
    traj = np.asarray(om.train(iter=ITER, tol=0.0, checkelbo=1), dtype=np.float64)
    assert len(traj) == ITER and np.all(np.isfinite(traj))
    o = dict(base=base, traj=traj, emax=float(np.max(np.abs(np.concatenate([[base], traj])))))
    s, tol, margin, bound = stop_plan(o, model, 1)
    assert tol > 0 and 1 < s < ITER and margin >= bound, (model, s, tol, margin, bound)   # such a gap exists in the oracle's trajectory
    res = _run(model, ITER, tol)
    print(f"{model}: stop index {s}, tol {tol:.6g}, margin {margin:.4g} >= {bound:.4g}, ranks stopped at {[len(r['traj']) for r in res]}")
    for q, r in enumerate(res):
        assert len(r["traj"]) == s, (model, "rank", q, "stopped at", len(r["traj"]), "expected", s, r["traj"], traj)
        assert np.all(np.isfinite(r["traj"])) and np.array_equal(r["traj"], res[0]["traj"])
