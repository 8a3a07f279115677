#!/usr/bin/env python
"""Stochastic (minibatch) CTM training against train! on SYN-NSF: held-out perplexity against device time, and where a step's time goes.

    python tools/ctm_svi_bench.py [--K 50 100] [--batch 1024 4096 16384] [--epochs 2] [--train-iter 150] [--out profiles/ctm_svi_bench.json]

Per K: the corpus is split by tokens (split_corpus, frac 0.5), every model trains on the observed side and is scored on the held-out side
(heldout_loglik: document-completion perplexity; a second score with laplace_smooth = 1e-6, because train! leaves beta = 0 for terms the observed
side never shows and a single such held-out token makes the plain score inf: zero_prob_tokens counts them).
  initial      the untrained model
  train!       gpu_train_ctm's device part, gpuCTM.train(iter = --train-iter, checkelbo = Inf): HIP events around the call (its uploads and downloads
               included), perplexity of the result
  stochastic   gpuCTMStochastic at every --batch, tau0 = 1, kappa = 0.7, --epochs epochs in corpus order, after two warm-up steps from which the
               initial state is restored: device time of run() and of final_pass(), perplexity, and (TMVB_ESTEP_TIMING=1) the per-step milliseconds
               split E-step / fused update (blend + normalise + tail) / sigma and mu
  composed     the same step from the existing stepwise operators on ONE shard handle of `batch` documents, in this process and this call (estep +
               reduce_docs, update_beta, update_sigma, update_mu; the handle is `distributed` like the driver's, so update_sigma inverts on the
               critical path): the yardstick -- update_beta + update_sigma + update_mu is what the fused update and its sigma / mu launch stand in for
  fused update achieved fraction of 8 TB/s on its algorithmic bytes: blend reads Sbar, S_b and writes both (4 K V floats), normalise reads Sbar and
               writes the padded beta (K V + KP V floats), the tail reads two and writes two of T = 2 K + K^2 floats
No threshold is set.  One JSON document, also printed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TMVB_ESTEP_TIMING", "1")
import tmvb_amd as tm  # noqa: E402

HBM_BYTES_PER_S = 8e12
SMOOTH = 1e-6


def kpad(K):
    q = (K + 3) // 4
    return 4 * (q + 1 - (q & 1))


def timed(ctx, fn):
    a, b = ctx.timing_event(), ctx.timing_event()
    a.record(); fn(); b.record()
    ms = a.elapsed_ms(b)
    a.close(); b.close()
    return ms


def score(model, obs, held):
    r = tm.heldout_loglik(model, obs, held)
    return dict(perplexity=r.perplexity if np.isfinite(r.perplexity) else None,      # null: inf (zero_prob_tokens > 0)
                zero_prob_tokens=r.zero_prob_tokens, perplexity_smoothed=tm.heldout_loglik(model, obs, held, laplace_smooth=SMOOTH).perplexity)


def host_model(obs, K, src=None):
    m = tm.CTM(obs, K, seed=7)
    if src is not None:
        m.mu, m.sigma, m.invsigma = np.array(src.mu), np.asfortranarray(src.sigma), np.asfortranarray(src.invsigma)
        m.beta = np.asfortranarray(src.beta / src.beta.sum(axis=1, keepdims=True))
    return m


def bench_train(obs, held, K, iters):
    g = tm.gpuCTM(obs, K, seed=7)
    ms = timed(g.ctx, lambda: g.train(iter=iters, tol=0.0, checkelbo=float("inf"), printelbo=False))
    out = dict(iter=iters, call_ms=ms, **score(host_model(obs, K, g), obs, held))
    g.close(); g.dcorp.close(); g.ctx.close()
    return out


def bench_stochastic(obs, held, K, batch, epochs):
    t0 = time.time()
    g = tm.gpuCTMStochastic(obs, K, batch=batch, seed=7)
    create_s = time.time() - t0
    g.set_schedule(1.0, 0.7)
    order = tm.svi_order(g.B, epochs)
    g.update_host()                          # the initial state, statistic included
    g.run(order[:2]); g.synchronize()        # warm-up: code objects, function attributes
    g.t = 0
    g.update_buffer()                        # ... and back to the initial state
    run_ms = timed(g.ctx, lambda: g.run(order))
    parts = g.last_run_ms()
    final_ms = timed(g.ctx, lambda: g.final_pass())
    g.update_host()
    n = max(parts["steps"], 1)
    upd_ms = parts["update_ms"] / n
    KV, KPV, T = K * obs.V, kpad(K) * obs.V, 2 * K + K * K
    algo_bytes = 4.0 * (4 * KV + KV + KPV + 4 * T)
    out = dict(batch=batch, B=g.B, epochs=epochs, steps=parts["steps"], create_s=create_s, run_device_ms=run_ms, final_pass_device_ms=final_ms,
               per_step_ms=dict(estep=parts["estep_ms"] / n, update=upd_ms, sigma_mu=parts["sigma_mu_ms"] / n, total=run_ms / n),
               fused_update=dict(algorithmic_bytes=algo_bytes, ms=upd_ms, frac_of_8TBs=algo_bytes / (upd_ms * 1e-3) / HBM_BYTES_PER_S if upd_ms > 0 else None),
               **score(host_model(obs, K, g), obs, held))
    g.close()
    return out


def bench_composed(obs, K, batch, reps=50):
    """the step from the stepwise operators on one shard handle: per-operator device ms (mean of `reps` steps after 5 warm-up steps)"""
    shard = obs.shard(0, min(batch, obs.M))
    g = tm.gpuCTM(shard, K, seed=7)
    g.set_distributed(shard.M, True)        # as the driver's handles: no sigma staged under the E-step, update_sigma! inverts when it is called
    ops = dict(estep=lambda: (g.estep(), g.reduce_docs()), update_beta=g.update_beta, update_sigma=g.update_sigma, update_mu=g.update_mu)
    for _ in range(5):
        for f in ops.values():
            f()
    ms = {k: 0.0 for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            ms[k] += timed(g.ctx, f) / reps
    ms["mstep"] = ms["update_beta"] + ms["update_sigma"] + ms["update_mu"]
    ms["total"] = ms["estep"] + ms["mstep"]
    g.close(); g.dcorp.close(); g.ctx.close()
    return dict(batch=batch, reps=reps, per_step_ms=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[50, 100])
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--train-iter", type=int, default=150)
    ap.add_argument("--M", type=int, default=128804)
    ap.add_argument("--V", type=int, default=25319)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctm_svi_bench.json"))
    a = ap.parse_args()
    corp = tm.syn_nsf(M=a.M, V=a.V)
    obs, held = tm.split_corpus(corp, 0.5, seed=1)
    res = dict(corpus=dict(name="SYN-NSF", M=corp.M, V=corp.V, observed_tokens=int(obs.counts.sum()), heldout_tokens=int(held.counts.sum())),
               schedule=dict(tau0=1.0, kappa=0.7), configs=[])
    for K in a.K:
        cfg = dict(K=K, initial=score(host_model(obs, K), obs, held), train=bench_train(obs, held, K, a.train_iter), stochastic=[], composed=[])
        print(json.dumps(dict(K=K, train=cfg["train"])), flush=True)
        for batch in a.batch:
            cfg["stochastic"].append(bench_stochastic(obs, held, K, batch, a.epochs))
            cfg["composed"].append(bench_composed(obs, K, batch))
            print(json.dumps(dict(K=K, **cfg["stochastic"][-1], composed=cfg["composed"][-1]["per_step_ms"])), flush=True)
        res["configs"].append(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
