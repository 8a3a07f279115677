#!/usr/bin/env python3
"""Nearest documents in topic space at SYN-NSF shape -> profiles/neighbors_bench.json.

Database: Md = 128 804 Dirichlet(0.1) columns of K = 50 and 100 topics (the shape of a trained model's topic proportions over SYN-NSF),
metric HELLINGER, n = 10; queries: all pairs (every document against every other, 8.3e11 multiply-adds at K = 50) and the "documents like
this one" case, Mq = 1 and Mq = 64.  Recorded per case: device time of the feature, scan and merge kernels (HIP events around the kernels
only), the database splits the library chose, whole-call wall time (host checks, the fp64 upload and the download included), and the achieved
rate 2 Mq Md K / ms_scan beside the 157.3 TFLOP/s f32 matrix peak -- on the useful flops: padding K to kp and Mq to whole 128-query tiles
is the kernel's cost, not its work.  For the host: a blocked NumPy fp32 GEMM + argpartition + sort on 2 048 queries, timed, and SCALED to Mq
(labelled so: it is no measurement at Mq); its neighbours are compared with the device's on those queries (the sets, where the n-th and
n + 1-th host scores differ by more than the two roundings).  No threshold is asserted.

    python tools/neighbors_bench.py [--repeats 3] [--out profiles/neighbors_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MATRIX_FLOPS = 157.3e12
HOST_QUERIES = 2048


def host_topn(F, q_rows, n, block=256):
    """fp32 features F[Md, K]; queries = rows q_rows of F, self excluded -> (idx[len, n], seconds)"""
    t0 = time.perf_counter()
    out = np.empty((len(q_rows), n), dtype=np.int64)
    for b in range(0, len(q_rows), block):
        rows = q_rows[b:b + block]
        S = F[rows] @ F.T
        S[np.arange(len(rows)), rows] = -np.inf
        part = np.argpartition(-S, n, axis=1)[:, :n]
        sc = np.take_along_axis(S, part, axis=1)
        order = np.lexsort((part, -sc), axis=1)
        out[b:b + block] = np.take_along_axis(part, order, axis=1)
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--M", type=int, default=128804)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("neighbors_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    ctx = tm.DeviceContext(0)
    med = lambda xs: float(np.median(xs))
    Md, n = args.M, 10
    cases = {}
    for K in (50, 100):
        rng = np.random.Generator(np.random.PCG64(args.seed + K))
        g = rng.standard_gamma(0.1, size=(K, Md)) + 1e-300
        xd = np.asfortranarray(g / g.sum(axis=0))
        F = np.sqrt(xd.T).astype(np.float32)
        q_rows = np.arange(HOST_QUERIES)
        host_idx, host_s = host_topn(F, q_rows, n)
        for name, Mq in (("all_pairs", Md), ("Mq1", 1), ("Mq64", 64)):
            runs = []
            for r in range(args.repeats + 1):               # the first call is the warm-up (code object load, first allocations)
                t0 = time.perf_counter()
                rc, res = tm.neighbors_raw(ctx, K, 1, xd, None, 0, n, 0, Mq=Mq)
                wall = time.perf_counter() - t0
                assert rc == 0, res
                runs.append({"wall_s": wall, "ms": res["ms"]})
            ms = {k: med([x["ms"][k] for x in runs[1:]]) for k in ("prep", "scan", "merge")}
            flops = 2.0 * Mq * Md * K
            m = min(Mq, HOST_QUERIES)
            same = [set(a.tolist()) == set(b.tolist()) for a, b in zip(res["idx"][:m], host_idx[:m])]
            cases[f"K{K}_{name}"] = {
                "K": K, "kp": res["kp"], "Mq": Mq, "Md": Md, "n": n, "splits": res["splits"], "device_ms": ms, "useful_flops": flops,
                "scan_tflops": flops / (ms["scan"] * 1e-3) / 1e12, "fraction_of_157.3_TF": flops / (ms["scan"] * 1e-3) / PEAK_F32_MATRIX_FLOPS,
                "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"],
                "host_numpy_fp32_wall_s_on_2048_queries": host_s, "host_numpy_fp32_wall_s_SCALED_to_Mq_not_measured": host_s * Mq / HOST_QUERIES,
                "queries_compared_with_host": m, "queries_with_the_same_neighbour_set_as_host": int(np.sum(same)), "runs": runs}
    result = {"what": "tmvb_topic_neighbors at SYN-NSF shape (HELLINGER, Dirichlet(0.1) columns, n = 10), one MI355X; medians over the timed repeats "
                      "(first call = warm-up, listed apart); rates on the useful flops 2 Mq Md K; the host figure is a blocked NumPy fp32 GEMM + "
                      "argpartition on 2 048 queries on the host of the same machine, scaled to Mq where labelled so; no threshold",
              "Md": Md, "seed": args.seed, "repeats": args.repeats, "peak_f32_matrix_tflops": PEAK_F32_MATRIX_FLOPS / 1e12, "cases": cases}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {q: v[q] for q in ("splits", "device_ms", "scan_tflops", "wall_s_whole_call", "host_numpy_fp32_wall_s_SCALED_to_Mq_not_measured",
                                            "queries_with_the_same_neighbour_set_as_host")} for k, v in cases.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
