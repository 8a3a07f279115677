#!/usr/bin/env python3
"""Clustering in topic space at SYN-NSF shape -> profiles/cluster_bench.json.

Documents: M = 128 804 Dirichlet(0.1) columns of K = 50 and 100 topics (the shape of a trained model's topic proportions over SYN-NSF; no planted
groups, so Lloyd's loop has real work), metric HELLINGER, C = 16, 256 and 1 024 clusters, k-means++ seeding, tol = 0, at most --max-iter updates.
Recorded per case: device time of the features, of the seeding, and of the assignment (with the two inertia kernels) and the update PER ITERATION
(the library's sums over the call divided by the number of each), the whole call's wall time (host checks, the fp64 upload and the downloads
included), the iterations to stop = 1 (or that --max-iter came first), and the rate of the assignment on its useful flops 2 M C K beside the
157.3 TFLOP/s f32 matrix peak -- padding K to kp and C to whole tiles of 128 is the kernel's cost, not its work.  For the host: the fp64 NumPy
Lloyd loop on the first --host-docs documents from the device's own seeds of a call on that subset, both stopped after --host-iter updates;
labels compared, seconds per host iteration.  No threshold is asserted.

    python tools/cluster_bench.py [--repeats 2] [--out profiles/cluster_bench.json]
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


def host_lloyd(F, c, iters):
    """fp64 Lloyd on features F[M, K] from centroids c[C, K]: (labels, updates done, seconds per iteration)"""
    t0 = time.perf_counter()
    prev, t = None, 0
    while True:
        s = F @ c.T - 0.5 * (c * c).sum(axis=1)[None, :]
        label = np.argmax(s, axis=1)
        if (prev is not None and np.array_equal(prev, label)) or t == iters:
            break
        for k in np.unique(label):
            c[k] = F[label == k].mean(axis=0)
        prev, t = label, t + 1
    return label, t, (time.perf_counter() - t0) / (t + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--M", type=int, default=128804)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--host-docs", type=int, default=16384)
    ap.add_argument("--host-iter", type=int, default=10)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("cluster_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    ctx = tm.DeviceContext(0)
    med = lambda xs: float(np.median(xs))
    M = args.M
    cases = {}
    for K in (50, 100):
        rng = np.random.Generator(np.random.PCG64(args.seed + K))
        g = rng.standard_gamma(0.1, size=(K, M)) + 1e-300
        x = np.asfortranarray(g / g.sum(axis=0))
        F64 = np.sqrt(x[:, :args.host_docs].T)
        for C in (16, 256, 1024):
            runs = []
            for r in range(args.repeats + 1):               # the first call is the warm-up (code object load, first allocations)
                t0 = time.perf_counter()
                rc, res = tm.kmeans_raw(ctx, K, 1, x, C, None, args.seed, args.max_iter, 0.0)
                wall = time.perf_counter() - t0
                assert rc == 0, res
                runs.append({"wall_s": wall, "ms": res["ms"], "iters": res["iters"], "stop": res["stop"]})
                print(f"K = {K} C = {C} run {r}: {wall:.3f} s, iters {res['iters']}, stop {res['stop']}, ms {res['ms']}", flush=True)
            it = res["iters"]
            ms = {k: med([q["ms"][k] for q in runs[1:]]) for k in ("prep", "seed", "assign", "update")}
            assign_ms, update_ms = ms["assign"] / (it + 1), ms["update"] / max(it, 1)
            flops = 2.0 * M * C * K
            # the host on a subset, from the device's own seeds there
            rc, sub = tm.kmeans_raw(ctx, K, 1, x[:, :args.host_docs], C, None, args.seed, args.host_iter, 0.0)
            assert rc == 0, sub
            hl, ht, hs = host_lloyd(F64, F64[sub["seeds"]].astype(np.float32).astype(np.float64), args.host_iter)
            cases[f"K{K}_C{C}"] = {
                "K": K, "kp": res["kp"], "M": M, "C": C, "iters": it, "stop": res["stop"], "reached_stop_1": bool(res["stop"] == 1), "n_empty": res["n_empty"],
                "inertia_first_last": [float(res["inertia"][0]), float(res["inertia"][it])],
                "device_ms": {"features": ms["prep"], "seeding": ms["seed"], "assign_per_iteration": assign_ms, "update_per_iteration": update_ms,
                              "assign_all": ms["assign"], "update_all": ms["update"]},
                "useful_flops_per_assignment": flops, "assign_tflops": flops / (assign_ms * 1e-3) / 1e12,
                "fraction_of_157.3_TF": flops / (assign_ms * 1e-3) / PEAK_F32_MATRIX_FLOPS,
                "wall_s_whole_call": med([q["wall_s"] for q in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"],
                "host_subset": {"documents": args.host_docs, "updates_allowed": args.host_iter, "device_updates": sub["iters"], "host_updates": ht,
                                "labels_equal": int(np.sum(hl == sub["label"])), "host_numpy_fp64_s_per_iteration": hs,
                                "device_ms_per_iteration_on_the_subset": (sub["ms"]["assign"] + sub["ms"]["update"]) / (sub["iters"] + 1)},
                "runs": runs}
    result = {"what": "tmvb_topic_kmeans at SYN-NSF shape (HELLINGER, Dirichlet(0.1) columns, k-means++, tol = 0), one MI355X; medians over the timed repeats "
                      "(first call = warm-up, listed apart); per-iteration times = the call's sums over its assignments (iters + 1, the two inertia kernels "
                      "included) and updates (iters); rates on the useful flops 2 M C K; the host figure is the fp64 NumPy Lloyd loop on a document subset "
                      "on the host of the same machine from the device's seeds; no threshold",
              "M": M, "seed": args.seed, "repeats": args.repeats, "max_iter": args.max_iter, "peak_f32_matrix_tflops": PEAK_F32_MATRIX_FLOPS / 1e12, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {q: v[q] for q in ("iters", "stop", "device_ms", "assign_tflops", "wall_s_whole_call")} for k, v in cases.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
