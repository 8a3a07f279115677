#!/usr/bin/env python3
"""gencorp on the device at SYN-NSF shape -> profiles/gencorp_bench.json.

Generates M = 128 804 documents over V = 25 319 terms from the K = 50 SYN-NSF generating topics (the Zipf-tilted Gamma rows of
`synthetic_lda_corpus`, alpha = its theta concentration 0.1, mean_C = the SYN-NSF mean document length) through tmvb_lda_gencorp, and
records the per-stage device times, the whole-call wall time (host checks, uploads, downloads included), tokens/s and -- for context only,
it is a different sampler on a different processor -- the wall time of the NumPy generator behind SYN-NSF on the same host.

    python tools/gencorp_bench.py [--repeats 5] [--out profiles/gencorp_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def syn_nsf_topics(V, seed, Kstar=50, topic_conc=0.05, zipf_s=1.05):
    """The generating topics of synthetic_lda_corpus(M, V, seed): the same first draws of the same generator."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = 1.0 / np.arange(1, V + 1, dtype=np.float64) ** zipf_s
    rng.shuffle(base)
    topics = rng.gamma(topic_conc, size=(Kstar, V)) * base[None, :] + 1e-300
    return topics / topics.sum(axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--M", type=int, default=128804)
    ap.add_argument("--V", type=int, default=25319)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gencorp_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("gencorp_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    K = 50
    t0 = time.perf_counter()
    ref = tm.syn_nsf(M=args.M, V=args.V, seed=args.seed)
    numpy_s = time.perf_counter() - t0
    mean_C = float(ref.C.mean())
    beta = np.asfortranarray(syn_nsf_topics(args.V, args.seed))
    alpha = np.full(K, 0.1)
    ctx = tm.DeviceContext(0)
    runs = []
    for r in range(args.repeats + 1):                   # the first call is the warm-up (code object load, first allocations)
        t0 = time.perf_counter()
        rc, res = tm.gencorp_raw(ctx, K, args.V, beta, args.M, mean_C, alpha=alpha, seed=args.seed)
        wall = time.perf_counter() - t0
        assert rc == 0, res
        runs.append({"wall_s": wall, "ms": res["ms"], "tokens": res["sum_counts"], "nnz": res["nnz"]})
    timed = runs[1:]
    med = lambda xs: float(np.median(xs))
    stage = {s: med([r["ms"][s] for r in timed]) for s in ("tables", "docs", "tokens", "condense")}
    device_ms = sum(stage.values())
    tokens = timed[0]["tokens"]
    out = {
        "what": "tmvb_lda_gencorp at SYN-NSF shape, one MI355X; medians over the timed repeats (first call = warm-up, listed apart)",
        "M": args.M, "V": args.V, "K": K, "mean_C": mean_C, "seed": args.seed, "repeats": args.repeats,
        "tokens": tokens, "nnz": timed[0]["nnz"],
        "device_ms_per_stage": stage, "device_ms_total": device_ms,
        "wall_s_whole_call": med([r["wall_s"] for r in timed]), "wall_s_first_call": runs[0]["wall_s"],
        "tokens_per_s_device": tokens / (device_ms * 1e-3), "tokens_per_s_wall": tokens / med([r["wall_s"] for r in timed]),
        "context_only_numpy_synthetic_lda_corpus_wall_s": numpy_s,
        "context_note": "synthetic_lda_corpus is the host NumPy generator behind SYN-NSF (multinomial topic counts per document, then one sorted "
                        "search per topic); another sampler on another processor, not a like-for-like baseline",
        "runs": runs,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("tokens", "device_ms_per_stage", "device_ms_total", "wall_s_whole_call", "tokens_per_s_device",
                                          "context_only_numpy_synthetic_lda_corpus_wall_s")}))


if __name__ == "__main__":
    main()
