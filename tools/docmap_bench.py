#!/usr/bin/env python3
"""The document map at SYN-NSF shape -> profiles/docmap_bench.json.

Documents: M = 128 804 Dirichlet(0.1) columns of K = 50 and 100 topics (as tools/cluster_bench.py), metric HELLINGER, 64 neighbours, perplexity 20,
PCA start, 750 iterations, KL every 50.  Recorded per K: device time PER ITERATION of the repulsion (all M^2 pairs, with the segment sums and Z), the
attraction and the update (the library's sums over the call divided by the iterations); pair interactions per second beside the fp32 vector peak -- per
pair the kernel issues 2 subtractions, 2 fmas for d, 1 reciprocal, 1 add, 1 multiply and 2 fmas = 9 instructions or 13 flops with an fma as two; the
peak is 157.3 TFLOP/s with packed fmas, i.e. 39.3e12 plain instructions per second over all lanes --; the whole map_docs call (neighbours, entropy
search, host symmetrisation, PCA, upload, the 15 KL evaluations, download); and one iteration of the same arithmetic in fp64 NumPy on the first
--host-docs documents on the host of the same machine.  No threshold is asserted.

    python tools/docmap_bench.py [--iters 750] [--out profiles/docmap_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_VECTOR_FLOPS = 157.3e12
PEAK_LANE_INSTRUCTIONS = PEAK_F32_VECTOR_FLOPS / 4.0        # a packed fma is 4 flops per lane and clock
INSTR_PER_PAIR, FLOPS_PER_PAIR = 9, 13


def host_iteration(y, row_ptr, col, val, chunk=1024):
    """the forces of one iteration in fp64 NumPy, rows in chunks: seconds"""
    t0 = time.perf_counter()
    y = y.astype(np.float64)
    M = len(y)
    rep, z = np.zeros((M, 2)), 0.0
    for b in range(0, M, chunk):
        dx, dy = y[b:b + chunk, 0][:, None] - y[None, :, 0], y[b:b + chunk, 1][:, None] - y[None, :, 1]
        q = 1.0 / (1.0 + dx * dx + dy * dy)
        z += q.sum()
        q *= q
        rep[b:b + chunk, 0], rep[b:b + chunk, 1] = (q * dx).sum(axis=1), (q * dy).sum(axis=1)
    i = np.repeat(np.arange(M), np.diff(row_ptr))
    d = y[i] - y[col]
    t = (val.astype(np.float64) / (1.0 + (d * d).sum(axis=1)))[:, None] * d
    att = np.stack([np.bincount(i, t[:, c], minlength=M) for c in range(2)], axis=1)
    g = 4.0 * (att - rep / (z - M))
    return time.perf_counter() - t0, float(np.abs(g).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=128804)
    ap.add_argument("--iters", type=int, default=750)
    ap.add_argument("--host-docs", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "docmap_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("docmap_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    M = args.M
    cases = {}
    for K in (50, 100):
        rng = np.random.Generator(np.random.PCG64(args.seed + K))
        g = rng.standard_gamma(0.1, size=(K, M)) + 1e-300
        x = np.asfortranarray(g / g.sum(axis=0))
        tm.map_docs(None, theta=x[:, :4096], iters=5)                  # warm-up: code object load, first allocations
        t0 = time.perf_counter()
        m = tm.map_docs(None, theta=x, iters=args.iters)
        wall = time.perf_counter() - t0
        it = max(m.iters, 1)
        per = {k: m.ms[k] / it for k in ("repulsion", "attraction", "update")}
        pairs = float(M) * float(M)
        rate = pairs / (per["repulsion"] * 1e-3)
        sub = tm.map_docs(None, theta=x[:, :args.host_docs], iters=20)
        hs, hg = host_iteration(sub.xy, *sub._csr)
        cases[f"K{K}"] = {
            "K": K, "M": M, "iters": m.iters, "n_neighbors": m.n_neighbors, "perplexity": m.perplexity, "nnz_of_P": int(m._csr[0][-1]),
            "device_ms_per_iteration": dict(per, total=sum(per.values())), "device_ms_neighbors": m.ms["neighbors"],
            "pairs_per_iteration": pairs, "pairs_per_second": rate, "instructions_per_pair": INSTR_PER_PAIR, "flops_per_pair": FLOPS_PER_PAIR,
            "tflops": rate * FLOPS_PER_PAIR / 1e12, "fraction_of_157.3_TF": rate * FLOPS_PER_PAIR / PEAK_F32_VECTOR_FLOPS,
            "fraction_of_the_plain_instruction_rate": rate * INSTR_PER_PAIR / PEAK_LANE_INSTRUCTIONS,
            "wall_s_whole_map_docs": wall, "kl_first_last": [float(m.kl[0]), float(m.kl[-1])], "kl_iters": [int(v) for v in m.kl_iters],
            "host_subset": {"documents": args.host_docs, "host_numpy_fp64_s_per_iteration": hs, "max_abs_gradient": hg,
                            "device_ms_per_iteration_on_the_subset": sum(sub.ms[k] for k in ("repulsion", "attraction", "update")) / max(sub.iters, 1)}}
        print(K, json.dumps(cases[f"K{K}"]["device_ms_per_iteration"]), f"wall {wall:.2f} s, host {hs:.2f} s / iteration on {args.host_docs}", flush=True)
    result = {"what": "map_docs at SYN-NSF shape (HELLINGER, Dirichlet(0.1) columns, 64 neighbours, perplexity 20, PCA start), one MI355X, one timed call per K "
                      "after a small warm-up call; per-iteration times = the call's sums of HIP event intervals divided by the iterations; the repulsion is exact "
                      "(all M^2 pairs); the host figure is one iteration of the same forces in chunked fp64 NumPy on a document subset on the host of the same "
                      "machine; no threshold",
              "M": M, "seed": args.seed, "peak_f32_vector_tflops": PEAK_F32_VECTOR_FLOPS / 1e12, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
