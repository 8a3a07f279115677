#!/usr/bin/env python3
"""Topic comparison at SYN-NSF shape (V = 25 319) -> profiles/topic_compare_bench.json.

Topic-word matrices: K = 50 and K = 100 Dirichlet(0.05) rows over V terms (the sparsity of a trained model's beta).  Recorded:
  * self-comparison (b = NULL) at both K under all four metrics, and ten stacked runs of K = 100 = 1 000 x 1 000 pairs (what topic_stability sends down in
    ONE call): device time of the prep, pair and merge kernels from the call's own HIP events (median, min and max over --repeats calls after one
    warm-up call), the whole call's wall time (host checks of the rows, the fp64 upload and the download included), the groups of runs the library
    chose, and element operations per second = KA KB V / pair-kernel time -- the pairs of the full matrix, although for JS, HELLINGER and TV the tiles
    below the diagonal are mirrored and not computed (the figure is what a caller gets; `computed_fraction` says how much of it was computed);
  * tmvb_term_relevance at both K, n = 30, lambda = 0.6: device time of the score pass, the sort with the selection and the per-term pass, wall time;
  * NumPy fp64 on the same host for the divergences: the first --host-rows rows against all KB rows, one vectorised expression per metric, the
    seconds SCALED by KA / host_rows to the full matrix and labelled as scaled.
Nobody had measured the fp64 log and divide rates of this part before; no threshold is asserted.

    python tools/topic_compare_bench.py [--repeats 5] [--out profiles/topic_compare_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = (("js", 0, 0.0), ("hellinger", 1, 0.0), ("tv", 2, 0.0), ("kl", 3, 1e-3))


def host_divergence(metric, a, b):
    """plain vectorised NumPy fp64 (numpy.sum: not the library's order), a: rows x V, b: KB x V"""
    p, q = a[:, None, :], b[None, :, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == "js":
            s = p + q
            return 0.5 * (np.where(p > 0, p * np.log(2 * p / s), 0.0) + np.where(q > 0, q * np.log(2 * q / s), 0.0)).sum(axis=-1)
        if metric == "hellinger":
            return np.sqrt(0.5 * ((np.sqrt(p) - np.sqrt(q)) ** 2).sum(axis=-1))
        if metric == "tv":
            return 0.5 * np.abs(p - q).sum(axis=-1)
        V = a.shape[1]
        p, q = (p + 1e-3) / (1 + 1e-3 * V), (q + 1e-3) / (1 + 1e-3 * V)
        return (p * np.log(p / q)).sum(axis=-1)


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--V", type=int, default=25319)
    ap.add_argument("--host-rows", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topic_compare_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("topic_compare_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    ctx = tm.DeviceContext(0)
    rng = np.random.default_rng(args.seed)
    V = args.V
    mats = {K: np.asfortranarray(rng.dirichlet(np.full(V, 0.05), size=K)) for K in (50, 100)}
    mats[1000] = np.asfortranarray(np.vstack([rng.dirichlet(np.full(V, 0.05), size=100) for _ in range(10)]))
    out = {"V": V, "repeats": args.repeats, "divergence": [], "relevance": [],
           "note": "device ms from the calls' own HIP events around the kernels; wall seconds include host checks, upload and download"}
    for K, a in mats.items():
        tiles = (K + 31) // 32
        for name, code, smooth in METRICS:
            if K == 1000 and name in ("tv", "kl"):
                continue
            tm.topic_divergence_raw(ctx, code, a, None, smooth)                      # warm-up
            ms, wall, res = {"prep": [], "pairs": [], "merge": []}, [], None
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                rc, res = tm.topic_divergence_raw(ctx, code, a, None, smooth)
                wall.append(time.perf_counter() - t0)
                assert rc == 0, res
                for k in ms:
                    ms[k].append(res["ms"][k])
            rows = min(args.host_rows, K)
            t0 = time.perf_counter()
            h = host_divergence(name, np.ascontiguousarray(a[:rows]), np.ascontiguousarray(a))
            host_s = time.perf_counter() - t0
            ops = float(K) * K * V
            rec = {"K": K, "metric": name, "smooth": smooth, "splits": res["splits"], "runs": res["runs"],
                   "computed_fraction": 1.0 if name == "kl" else tiles * (tiles + 1) / 2 / (tiles * tiles),
                   "device_ms": {k: stats(v) for k, v in ms.items()}, "wall_s": stats(wall), "element_ops": ops,
                   "element_ops_per_s": ops / (np.median(ms["pairs"]) * 1e-3),
                   "host_numpy_fp64_s_scaled": host_s * K / rows, "host_rows": rows, "host_scaled_by": K / rows,
                   "max_abs_diff_to_host_rows": float(np.nanmax(np.abs(np.where(np.isfinite(h), res["D"][:rows] - h, 0.0))))}
            out["divergence"].append(rec)
            print(json.dumps(rec))
    for K in (50, 100):
        beta = mats[K]
        pi = rng.dirichlet(np.full(K, 2.0))
        pw = pi @ beta
        pw /= pw.sum()
        tm.term_relevance_raw(ctx, beta, pw, pi, 0.6, 30)
        ms, wall = {"score": [], "select": [], "terms": []}, []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            rc, res = tm.term_relevance_raw(ctx, beta, pw, pi, 0.6, 30)
            wall.append(time.perf_counter() - t0)
            assert rc == 0, res
            for k in ms:
                ms[k].append(res["ms"][k])
        rec = {"K": K, "n": 30, "lambda": 0.6, "device_ms": {k: stats(v) for k, v in ms.items()}, "wall_s": stats(wall)}
        out["relevance"].append(rec)
        print(json.dumps(rec))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
