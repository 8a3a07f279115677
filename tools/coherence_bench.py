#!/usr/bin/env python3
"""Co-document counts on the device at SYN-NSF shape -> profiles/coherence_bench.json.

Counts the co-documents of the N top words of K topics over SYN-NSF (M = 128 804, V = 25 319, 10.9 M entries) through
tmvb_corpus_codocfreq for K = 50 and 100, N = 10 and 20 (top: the N most probable ids of every row of dirichlet_rows(K, V) scaled by the
corpus's term frequencies, so that the rows hold frequent, partly shared terms as trained topics do), and times the NumPy restatement of
the tests on the same inputs on this host (scipy.sparse if importable, else the dense NumPy form).  Recorded side by side: device time of
the two kernels (HIP events around the kernels only), whole-call wall time (host checks, slot map, uploads, download included), the
restatement's wall time, and the achieved fraction of 8 TB/s on the bytes model of DESIGN 2.11: the build reads nnz 8 B (term id and the
map entry it gathers) and the pair pass reads K N W 8 B, each topic's rows once.  No threshold is asserted: the parent commit has no device
path to compare with, and the host figure is another algorithm's cost on another processor.

    python tools/coherence_bench.py [--repeats 5] [--out profiles/coherence_bench.json]
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


def host_codf(M, V, doc_ptr, terms, top):
    """(codf, what): the restatement of tests/test_coherence_host.py, through scipy.sparse when it is there"""
    try:
        import scipy.sparse as sp
    except ImportError:
        from test_coherence_host import np_codf
        return np_codf(M, V, doc_ptr, terms, top), "numpy dense"
    ids, inv = np.unique(top, return_inverse=True)
    slot = np.full(V, -1, dtype=np.int64); slot[ids] = np.arange(len(ids))
    doc = np.repeat(np.arange(M), np.diff(doc_ptr))
    s = slot[terms]
    keep = s >= 0
    B = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int64), (doc[keep], s[keep])), shape=(M, len(ids)))
    B.data[:] = 1                                           # duplicates were summed: presence only
    G = np.asarray((B.T @ B).todense())
    sl = inv.reshape(top.shape)
    return np.stack([G[np.ix_(r, r)] for r in sl]), "scipy.sparse"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--M", type=int, default=128804)
    ap.add_argument("--V", type=int, default=25319)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coherence_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("coherence_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    pc = tm.syn_nsf(M=args.M, V=args.V, seed=args.seed)
    tf = np.bincount(pc.terms, minlength=pc.V).astype(np.float64) + 1.0
    ctx = tm.DeviceContext(0)
    med = lambda xs: float(np.median(xs))
    W = (pc.M + 63) // 64
    cases = {}
    for K in (50, 100):
        weight = tm.dirichlet_rows(K, pc.V, seed=7) * tf[None, :]
        order = np.argsort(-weight, axis=1, kind="stable")
        for N in (10, 20):
            top = np.ascontiguousarray(order[:, :N])
            runs = []
            for r in range(args.repeats + 1):               # the first call is the warm-up (code object load, first allocations)
                t0 = time.perf_counter()
                rc, res = tm.codocfreq_raw(ctx, pc.M, pc.V, pc.doc_ptr, pc.terms, pc.counts, top)
                wall = time.perf_counter() - t0
                assert rc == 0, res
                runs.append({"wall_s": wall, "ms": res["ms"]})
            t0 = time.perf_counter()
            want, how = host_codf(pc.M, pc.V, pc.doc_ptr, pc.terms, top)
            host_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            umass, npmi, undef = tm.coherence_from_counts(res["codf"], pc.M)
            score_s = time.perf_counter() - t0
            ms_b, ms_p = med([x["ms"]["bitset"] for x in runs[1:]]), med([x["ms"]["pairs"] for x in runs[1:]])
            bytes_b, bytes_p = pc.nnz * 8, K * N * W * 8
            cases[f"K{K}_N{N}"] = {
                "K": K, "N": N, "n_slots": res["n_slots"], "n_batches": res["n_batches"], "words_per_row": W,
                "device_ms": {"bitset": ms_b, "pairs": ms_p}, "model_bytes": {"bitset": bytes_b, "pairs": bytes_p},
                "achieved_fraction_of_8TBps": {"bitset": bytes_b / (ms_b * 1e-3) / HBM_BYTES_PER_S, "pairs": bytes_p / (ms_p * 1e-3) / HBM_BYTES_PER_S},
                "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"],
                "host_restatement": how, "host_restatement_wall_s": host_s, "equals_host_restatement": bool(np.array_equal(res["codf"], want)),
                "scoring_wall_s": score_s, "mean_umass": float(np.nanmean(umass)), "mean_npmi": float(np.nanmean(npmi)),
                "undefined_pairs": int(undef.sum()), "runs": runs}
    result = {"what": "tmvb_corpus_codocfreq at SYN-NSF shape, one MI355X; medians over the timed repeats (first call = warm-up, listed apart); the host "
                      "figure is the restatement of the tests on the host of the same machine, for context",
              "M": pc.M, "V": pc.V, "nnz": pc.nnz, "seed": args.seed, "repeats": args.repeats, "cases": cases}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {n: v[n] for n in ("device_ms", "achieved_fraction_of_8TBps", "wall_s_whole_call", "host_restatement_wall_s",
                                            "equals_host_restatement")} for k, v in cases.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
