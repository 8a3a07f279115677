#!/usr/bin/env python3
"""Held-out recommendation metrics at SYN-CITEU shape -> profiles/recs_eval_bench.json.

SYN-CITEU (M = 16 980 documents, V = 8 000, U = 5 551 users), 20 % of the (document, reader) entries held out (split_readers, mode "entry"),
gpuCTPF trained on the rest for --iters iterations at K = 50 and K = 100.  Recorded per K:
  * rec_eval(by="user"): device time of the four stages (HIP events around the kernels only), the database splits the library chose, the
    whole-call wall time (the fp64 factors from the host state, host checks, uploads and the metrics included), medians over the timed repeats,
    the first call listed apart;
  * the route without tmvb_score_ranks, timed in the same process on the same trained handle: recommend(scores=False) -- two M x U key
    matrices, two segmented sorts, 2 x M x U int32 to the host -- plus the host lookup of each held-out document's position in urecs[u];
    how many of those positions equal the ranks (nothing pins the score bits of tmvb_ctpf_recs.hip to this kernel's, so this is a count, not
    an assertion);
  * the model's mean recall@N and percentile rank next to two baselines through the same entry point: popularity (K = 1, xd = observed reader
    counts, xq = 1) and random (the expectation, pct_rank 0.5).
No threshold is asserted.

    python tools/recs_eval_bench.py [--repeats 3] [--iters 30] [--out profiles/recs_eval_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOPN = (10, 20, 50, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--M", type=int, default=16980)
    ap.add_argument("--V", type=int, default=8000)
    ap.add_argument("--U", type=int, default=5551)
    ap.add_argument("--frac", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recs_eval_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    recs = sys.modules[tm.__name__ + ".recs_eval"]
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("recs_eval_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    med = lambda xs: float(np.median(xs))
    pf = tm.syn_citeu(M=args.M, V=args.V, U=args.U)
    obs, held = tm.split_readers(pf, args.frac, args.seed)
    excl = recs._unique_rows(*recs.transpose_csr(obs.rdr_ptr, obs.readers, obs.U))
    tgt = recs._unique_rows(held.user_ptr, held.docs)
    means = lambda m: {"recall": {str(int(n)): float(v) for n, v in zip(TOPN, m["mean_recall"])}, "ndcg": {str(int(n)): float(v) for n, v in zip(TOPN, m["mean_ndcg"])},
                       "mrr": m["mean_mrr"], "pct_rank": m["mean_pct_rank"]}
    cases = {}
    for K in (50, 100):
        g = tm.gpuCTPF(obs, K)
        t0 = time.perf_counter()
        g.train(iter=args.iters, tol=0.0, checkelbo=float("inf"), printelbo=False, recs=False)
        train_s = time.perf_counter() - t0
        runs = []
        for _ in range(args.repeats + 1):                   # the first call is the warm-up (code object load, first allocations)
            t0 = time.perf_counter()
            r = tm.rec_eval(g, held, topn=TOPN, by="user")
            runs.append({"wall_s": time.perf_counter() - t0, "ms": r.ms})
        ms = {k: med([x["ms"][k] for x in runs[1:]]) for k in ("prep", "pairs", "scan", "fix")}
        # the route of the parent commit: every ranking, then a lookup
        base = []
        for _ in range(2):
            t0 = time.perf_counter()
            ms_scores, ms_rank = g.recommend(scores=False)
            t1 = time.perf_counter()
            pos = np.empty(len(tgt[1]), dtype=np.int64)
            for u in range(obs.U):
                a, b = tgt[0][u], tgt[0][u + 1]
                if b > a:
                    where = np.empty(obs.M + 1, dtype=np.int64)
                    where[g.urecs[u]] = np.arange(len(g.urecs[u]))
                    pos[a:b] = where[tgt[1][a:b] + 1]                                    # urecs holds 1-based ids
            t2 = time.perf_counter()
            base.append({"recommend_wall_s": t1 - t0, "lookup_wall_s": t2 - t1, "device_ms": {"scores": ms_scores, "rank": ms_rank}})
        agree = int(np.count_nonzero(pos == r.rank))
        with recs.call_context(0, g.ctx) as ctx:
            rc, pop = tm.rec_ranks_raw(ctx, 1, np.diff(obs.rdr_ptr).astype(np.float64)[None, :], np.ones((1, obs.U)), excl, tgt)
        assert rc == 0, pop
        pop_m = tm.rank_metrics(tgt[0], pop["rank"], pop["n_cand"], TOPN)
        flops = 2.0 * obs.U * obs.M * K
        cases[f"K{K}"] = {
            "K": K, "Mq_users": obs.U, "Md_documents": obs.M, "held_out_pairs": int(r.n_targets), "users_with_held_out": int(r.n_queries), "excluded_pairs": int(excl[0][-1]),
            "train_iters": args.iters, "train_wall_s": train_s, "splits": r.splits, "device_ms": ms, "device_ms_sum": sum(ms.values()),
            "useful_flops_scan": flops, "scan_tflops": flops / (ms["scan"] * 1e-3) / 1e12,
            "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"], "runs": runs,
            "parent_route": {"what": "recommend(scores=False) + host lookup of the held-out positions in urecs, same handle, same process; second of two runs",
                             "runs": base, "wall_s": base[-1]["recommend_wall_s"] + base[-1]["lookup_wall_s"],
                             "positions_equal_to_ranks": agree, "positions_compared": int(len(pos))},
            "quality": {"model": means({k: getattr(r, k) for k in ("mean_recall", "mean_ndcg", "mean_mrr", "mean_pct_rank")}), "popularity": means(pop_m),
                        "random_expectation": {"pct_rank": 0.5}}}
        g.close()
    result = {"what": "rec_eval(by='user') on SYN-CITEU, one MI355X; medians over the timed repeats (first call = warm-up, listed apart); device times are HIP "
                      "events around the kernels only; the scan rate is on the useful flops 2 U M K; no threshold",
              "M": args.M, "V": args.V, "U": args.U, "frac": args.frac, "seed": args.seed, "repeats": args.repeats, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {q: v[q] for q in ("splits", "device_ms", "wall_s_whole_call", "quality")} | {"parent_route_wall_s": v["parent_route"]["wall_s"],
                          "positions_equal": v["parent_route"]["positions_equal_to_ranks"], "of": v["parent_route"]["positions_compared"]} for k, v in cases.items()}))


if __name__ == "__main__":
    main()
