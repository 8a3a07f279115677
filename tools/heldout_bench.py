#!/usr/bin/env python3
"""Held-out evaluation on the device at SYN-NSF shape -> profiles/heldout_bench.json.

Splits SYN-NSF (M = 128 804, V = 25 319) at frac = 0.5 through tmvb_corpus_split and scores the held-out side through
tmvb_heldout_loglik at K = 50 and K = 100 (theta: Dirichlet(0.1) columns, beta: dirichlet_rows -- the values do not change the work),
and times a NumPy fp64 restatement of both on the same inputs on this host.  Recorded side by side: device time per stage (HIP events
around kernels and scans), whole-call wall time (host checks, fp32 staging, uploads, downloads included), the NumPy wall time, and the
scoring kernel's achieved fraction of 8 TB/s on its algorithmic bytes nnz (8 + 4 KP) + 4 M K + 8 M.  No threshold is asserted: the parent
commit has no device path to compare with, and the NumPy figure is another algorithm's cost on another processor.

    python tools/heldout_bench.py [--repeats 5] [--out profiles/heldout_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12


def numpy_loglik(theta, beta, doc_ptr, terms, counts, chunk_docs=4096):
    """fp64, chunked over documents so that the K x nnz gathers stay in cache-sized pieces"""
    M = len(doc_ptr) - 1
    ll = np.zeros(M)
    for d0 in range(0, M, chunk_docs):
        d1 = min(M, d0 + chunk_docs)
        a, b = doc_ptr[d0], doc_ptr[d1]
        doc = np.repeat(np.arange(d0, d1), np.diff(doc_ptr[d0:d1 + 1]))
        p = np.einsum("kn,kn->n", theta[:, doc], beta[:, terms[a:b]])
        np.add.at(ll, doc, counts[a:b] * np.log(p))
    return ll


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--M", type=int, default=128804)
    ap.add_argument("--V", type=int, default=25319)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heldout_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    from test_heldout_host import host_split
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("heldout_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    pc = tm.syn_nsf(M=args.M, V=args.V, seed=args.seed)
    ctx = tm.DeviceContext(0)
    med = lambda xs: float(np.median(xs))

    # ---- split
    runs = []
    for r in range(args.repeats + 1):                   # the first call is the warm-up (code object load, first allocations)
        t0 = time.perf_counter()
        rc, res = tm.split_corpus_raw(ctx, pc.M, pc.V, pc.doc_ptr, pc.terms, pc.counts, 0.5, args.seed)
        wall = time.perf_counter() - t0
        assert rc == 0, res
        runs.append({"wall_s": wall, "ms": res["ms"]})
    t0 = time.perf_counter()
    want = host_split(pc.doc_ptr, pc.terms, pc.counts, 0.5, args.seed)
    numpy_split_s = time.perf_counter() - t0
    same = all(np.array_equal(res[k], w) for k, w in zip(("obs_ptr", "obs_terms", "obs_counts", "held_ptr", "held_terms", "held_counts"), want))
    held = tm.PackedCorpus(res["held_ptr"], res["held_terms"], res["held_counts"], pc.V)
    split = {"nnz": pc.nnz, "tokens": int(pc.counts.sum(dtype=np.int64)), "nnz_obs": res["nnz_obs"], "nnz_held": res["nnz_held"],
             "sum_held": res["sum_held"], "device_ms": {s: med([x["ms"][s] for x in runs[1:]]) for s in ("draw", "compact")},
             "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"],
             "numpy_restatement_wall_s": numpy_split_s, "equals_numpy_restatement": bool(same), "runs": runs}

    # ---- log-likelihood of the held-out side
    scores = {}
    for K in (50, 100):
        rng = np.random.Generator(np.random.PCG64(args.seed + K))
        theta = rng.gamma(0.1, size=(K, pc.M)) + 1e-12
        theta = np.asfortranarray(theta / theta.sum(axis=0, keepdims=True))
        beta = np.asfortranarray(tm.dirichlet_rows(K, pc.V, seed=7))
        runs = []
        for r in range(args.repeats + 1):
            t0 = time.perf_counter()
            rc, out = tm.heldout_loglik_raw(ctx, K, pc.V, theta, beta, held, 0.0)
            wall = time.perf_counter() - t0
            assert rc == 0, out
            runs.append({"wall_s": wall, "ms_kernel": out.ms_kernel})
        t0 = time.perf_counter()
        ll_np = numpy_loglik(theta, beta, held.doc_ptr, held.terms, held.counts)
        numpy_s = time.perf_counter() - t0
        has = out.tokens > 0
        q = (K + 3) // 4
        KP = 4 * (q if q & 1 else q + 1)
        nbytes = held.nnz * (8 + 4 * KP) + 4 * pc.M * K + 8 * pc.M
        ms = med([x["ms_kernel"] for x in runs[1:]])
        scores[f"K{K}"] = {"K": K, "KP": KP, "nnz": held.nnz, "M": pc.M, "algorithmic_bytes": nbytes, "device_ms_kernel": ms,
                           "achieved_fraction_of_8TBps": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S,
                           "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"],
                           "numpy_fp64_wall_s": numpy_s, "perplexity": out.perplexity,
                           "max_rel_dev_from_numpy": float((np.abs(out.ll[has] - ll_np[has]) / np.abs(ll_np[has])).max()), "runs": runs}
    result = {"what": "tmvb_corpus_split and tmvb_heldout_loglik at SYN-NSF shape, one MI355X; medians over the timed repeats (first call = warm-up, "
                      "listed apart); the NumPy figures are the fp64 restatements on the host of the same machine, for context",
              "M": args.M, "V": args.V, "seed": args.seed, "repeats": args.repeats, "split": split, "loglik": scores}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"split_ms": split["device_ms"], "split_numpy_s": numpy_split_s, "split_equal": same,
                      "loglik": {k: {n: v[n] for n in ("device_ms_kernel", "achieved_fraction_of_8TBps", "wall_s_whole_call", "numpy_fp64_wall_s",
                                                       "max_rel_dev_from_numpy")} for k, v in scores.items()}}))
    ctx.close()


if __name__ == "__main__":
    main()
