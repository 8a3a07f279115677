#!/usr/bin/env python3
"""Top-n recommendations at SYN-CITEU shape -> profiles/rectopn_bench.json.

SYN-CITEU (M = 16 980 documents, V = 8 000, U = 5 551 users), gpuCTPF trained for --iters iterations at K = 50 and K = 100.  Recorded per K,
for n = 15 and 64, by user (5 551 queries against 16 980 documents) and by doc (the roles swapped):
  * recommend_topn on the trained handle: device time of the three stages of tmvb_score_topn (HIP events around the kernels only), the
    database splits the library chose, the whole-call wall time (the state download, the fp64 factors, the exclusion lists, host checks and
    uploads included), medians over the timed repeats, the first call listed apart; the bytes the call downloads (idx, score);
  * the route that exists without tmvb_score_topn, timed in the same process on the same handle: recommend(scores=False) -- two M x U key
    matrices, two segmented sorts, 2 x M x U int32 to the host -- followed by taking the first n entries of every row; its downloaded bytes;
  * how many queries have identical id lists on the two routes and, where they differ, the largest gap between the fp64 scores of the two
    ids in one slot, relative to that score and in units of (K + 3) 2^-24, the derived bound of one fp32 score (nothing pins the score bits
    of tmvb_ctpf_recs.hip, which reads the handle's fp32 state, to this kernel's, which reads fp64 host factors: a count, not an assertion).
No threshold is asserted.

    python tools/rectopn_bench.py [--repeats 3] [--iters 30] [--out profiles/rectopn_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--M", type=int, default=16980)
    ap.add_argument("--V", type=int, default=8000)
    ap.add_argument("--U", type=int, default=5551)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectopn_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    recs = sys.modules[tm.__name__ + ".recs_eval"]
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("rectopn_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    med = lambda xs: float(np.median(xs))
    pf = tm.syn_citeu(M=args.M, V=args.V, U=args.U)
    cases = {}
    for K in (50, 100):
        g = tm.gpuCTPF(pf, K)
        t0 = time.perf_counter()
        g.train(iter=args.iters, tol=0.0, checkelbo=float("inf"), printelbo=False, recs=False)
        train_s = time.perf_counter() - t0
        # the route of the parent commit: every ranking, then the head of each
        base = []
        for _ in range(2):
            t0 = time.perf_counter()
            ms_scores, ms_rank = g.recommend(scores=False)
            t1 = time.perf_counter()
            heads = {(by, n): [np.asarray(r[:n]) - 1 for r in rows] for by, rows in (("user", g.urecs), ("doc", g.drecs)) for n in (15, 64)}
            t2 = time.perf_counter()
            base.append({"recommend_wall_s": t1 - t0, "heads_wall_s": t2 - t1, "device_ms": {"scores": ms_scores, "rank": ms_rank}})
        X, Y = recs.ctpf_factors(g)
        eps = (K + 3) * 2.0 ** -24
        for by, xd, xq in (("user", X, Y), ("doc", Y, X)):
            Md, Mq = xd.shape[1], xq.shape[1]
            for n in (15, 64):
                runs = []
                for _ in range(args.repeats + 1):           # the first call is the warm-up (code object load, first allocations)
                    t0 = time.perf_counter()
                    r = g.recommend_topn(topn=n, by=by)
                    runs.append({"wall_s": time.perf_counter() - t0, "ms": r.ms})
                ms = {k: med([x["ms"][k] for x in runs[1:]]) for k in ("prep", "scan", "merge")}
                same, gap = 0, 0.0
                for q, head in enumerate(heads[(by, n)]):
                    mine = r.idx[q, :r.count[q]]
                    if len(mine) == len(head) and np.array_equal(mine, head):
                        same += 1
                        continue
                    m = min(len(mine), len(head))
                    d = np.flatnonzero(mine[:m] != head[:m])
                    if len(mine) != len(head):
                        gap = float("inf")
                    elif len(d):
                        sa, sb = xq[:, q] @ xd[:, mine[d]], xq[:, q] @ xd[:, head[d]]
                        gap = max(gap, float((np.abs(sa - sb) / np.maximum(sa, sb)).max()))
                flops = 2.0 * Mq * Md * K
                cases[f"K{K}_{by}_n{n}"] = {
                    "K": K, "by": by, "n": n, "Mq": Mq, "Md": Md, "excluded_pairs": int(pf.nR), "train_iters": args.iters, "train_wall_s": train_s, "splits": r.splits,
                    "device_ms": ms, "device_ms_sum": sum(ms.values()), "useful_flops_scan": flops, "scan_tflops": flops / (ms["scan"] * 1e-3) / 1e12,
                    "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"], "runs": runs,
                    "downloaded_bytes": int(Mq * n * 8),                                       # idx int32 + score fp32; count is read off idx
                    "parent_route": {"what": "recommend(scores=False), then the first n entries of every row of urecs and drecs (both sides, both n, in one pass: "
                                             "the rankings of the two sides come from one call); same handle, same process; second of two runs",
                                     "runs": base, "wall_s": base[-1]["recommend_wall_s"] + base[-1]["heads_wall_s"],
                                     "downloaded_bytes": int(2 * args.M * args.U * 4 + (args.M + args.U) * 4)},
                    "queries_with_identical_ids": same, "queries": Mq,
                    "largest_fp64_score_gap_where_ids_differ": {"relative": gap, "in_units_of_(K+3)*2^-24": gap / eps}}
        g.close()
    result = {"what": "recommend_topn on SYN-CITEU, one MI355X; medians over the timed repeats (first call = warm-up, listed apart); device times are HIP events "
                      "around the kernels only; the scan rate is on the useful flops 2 Mq Md K; no threshold",
              "M": args.M, "V": args.V, "U": args.U, "repeats": args.repeats, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {q: v[q] for q in ("splits", "device_ms", "wall_s_whole_call", "downloaded_bytes", "queries_with_identical_ids", "queries")} |
                      {"parent_route_wall_s": v["parent_route"]["wall_s"], "parent_bytes": v["parent_route"]["downloaded_bytes"],
                       "gap_eps": v["largest_fp64_score_gap_where_ids_differ"]["in_units_of_(K+3)*2^-24"]} for k, v in cases.items()}))


if __name__ == "__main__":
    main()
