#!/usr/bin/env python3
"""Topics by group at SYN-NSF size -> profiles/group_topics_bench.json.

Corpus: SYN-NSF (M = 128 804, V = 25 319, about 10.9 M entries).  Factors: A = K Dirichlet(0.1) columns per document, B = K Dirichlet(0.05)
rows over the terms (tools/token_topics_bench.py's), K = 50 and 100, eps = EPSILON, n = 10.  Groups: G = 1, 20 and 200 contiguous blocks of
documents of equal size.  Recorded per (K, G), medians of --repeats calls after one warm-up: the host time of the index build (info.ms_index),
the device time of the accumulation (segments, combine, row sums), of the selection (normalisation, segmented sort, heads) and of the pooled row
with both divergences (HIP events around the kernels only), the whole call's wall time (host checks, fp32 staging, index, uploads, downloads), and
the index's shape (runs, segments, chunks of groups).
Yardstick 1: the kernel time of tmvb_token_topics (top = 1, no dense output, no hard counts) on the same entries and matrices: the same row
gathers and the same responsibilities, written per entry instead of added per (group, term).
Yardstick 2: the NumPy fp64 restatement (responsibilities, np.add.at into S_g, row sums) on the first --host-docs documents with the same
contiguous groups, on the host of the same machine; `host_numpy_wall_s_scaled` is that time SCALED to the whole corpus by the ratio of entries --
a figure, not a measurement of the whole corpus.  No threshold is asserted.

    python tools/group_topics_bench.py [--repeats 2] [--host-docs 4096] [--out profiles/group_topics_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPSILON = 1.5777218104420236e-30


def header_define(name):
    """an integer #define of include/tmvb.h (a variant library built with another value names it in TMVB_LIB_VARIANT)"""
    import re
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(os.path.join(ROOT, "include", "tmvb.h")).read()).group(1))


def host_restatement(A, B, ptr, terms, counts, group, G, n_docs, block=1 << 16):
    """blocked NumPy fp64 on documents [0, n_docs): S[G'][K][V] for the groups those documents touch and its row sums; seconds"""
    t0 = time.perf_counter()
    n, K, V = int(ptr[n_docs]), A.shape[0], B.shape[1]
    doc_of = np.repeat(np.arange(n_docs), np.diff(ptr[:n_docs + 1]))
    gs = np.unique(group[:n_docs])
    slot = np.full(G, -1); slot[gs] = np.arange(len(gs))
    S = np.zeros((len(gs), V, K))
    At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    for a in range(0, n, block):
        b = min(a + block, n)
        y = EPSILON + At[doc_of[a:b]] * Bt[terms[a:b]]
        r = y / y.sum(axis=1, keepdims=True) * counts[a:b, None]
        np.add.at(S, (slot[group[doc_of[a:b]]], terms[a:b]), r)
    mass = S.sum(axis=1)
    return mass, n, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--host-docs", type=int, default=4096, help="documents of the NumPy yardstick; 0 leaves it out")
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_topics_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("group_topics_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    ctx = tm.DeviceContext(0)
    med = lambda xs: float(np.median(xs))
    pc = tm.syn_nsf()
    M, V, ptr = pc.M, pc.V, np.asarray(pc.doc_ptr)
    terms, counts = np.asarray(pc.terms), np.asarray(pc.counts)
    cases = {}
    for K in (50, 100):
        rng = np.random.Generator(np.random.PCG64(args.seed + K))
        g = rng.standard_gamma(0.1, size=(K, M)) + 1e-300
        A = np.asfortranarray(g / g.sum(axis=0))
        g = rng.standard_gamma(0.05, size=(K, V)) + 1e-300
        B = np.asfortranarray(g / g.sum(axis=1, keepdims=True))
        tt = []
        for r in range(args.repeats + 1):
            rc, res = tm.token_topics_raw(ctx, K, V, A, B, pc, top=1, phi=False, hard=False)
            assert rc == 0, res
            tt.append(res["info"]["ms_kernel"])
        tt_ms = med(tt[1:])
        for G in (1, 20, 200):
            group = np.minimum(np.arange(M) * G // M, G - 1).astype(np.int32)
            runs = []
            for r in range(args.repeats + 1):               # the first call is the warm-up (code object load, first allocations)
                t0 = time.perf_counter()
                rc, res = tm.group_topics_raw(ctx, K, V, A, B, pc, group, G, topn=10)
                wall = time.perf_counter() - t0
                assert rc == 0, res
                runs.append(dict(res["info"], wall_s=wall))
            info = res["info"]
            nd = min(args.host_docs, M)
            h_mass, h_n, h_s = host_restatement(A, B, ptr, terms, counts.astype(np.float64), group, G, nd) if nd > 0 else (None, 0, 0.0)
            out = {"K": K, "G": G, "n": 10, "nsel": info["nsel"], "runs": info["runs"], "segments": info["segments"], "group_chunks": info["group_chunks"],
                   "lanes_per_entry": info["lanes_per_entry"],
                   "index_ms_host": med([x["ms_index"] for x in runs[1:]]), "accum_ms": med([x["ms_accum"] for x in runs[1:]]),
                   "select_ms": med([x["ms_select"] for x in runs[1:]]), "shift_drift_ms": med([x["ms_shift"] for x in runs[1:]]),
                   "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"],
                   "token_topics_kernel_ms_same_entries": tt_ms, "accum_ms_over_token_topics_kernel_ms": med([x["ms_accum"] for x in runs[1:]]) / tt_ms,
                   "host_numpy_docs": nd, "host_numpy_entries": h_n, "host_numpy_wall_s": h_s, "host_numpy_wall_s_scaled": h_s * info["nsel"] / max(h_n, 1),
                   "host_numpy_scaled_by": "entries of the whole corpus / entries of the subset",
                   "sum_mass_over_tokens_worst": float(np.abs(res["mass"].sum(axis=1) / np.maximum(res["tokens"], 1) - 1.0).max()), "all_runs": runs}
            cases[f"K{K}_G{G}"] = out
            print(f"K = {K} G = {G}: index {out['index_ms_host']:.1f} ms, accum {out['accum_ms']:.3f} ms, select {out['select_ms']:.3f} ms, shift {out['shift_drift_ms']:.3f} ms, "
                  f"whole call {out['wall_s_whole_call']:.2f} s; token_topics kernel {tt_ms:.3f} ms; host (scaled) {out['host_numpy_wall_s_scaled']:.1f} s", file=sys.stderr, flush=True)
    result = {"what": "tmvb_group_topics at SYN-NSF size (Dirichlet(0.1) document columns, Dirichlet(0.05) topic rows, eps = EPSILON, n = 10, G contiguous blocks of "
                      "documents), one MI355X; medians over the timed repeats (first call = warm-up, listed apart); *_ms = HIP events around the kernels only, "
                      "index_ms_host = the host's counting sorts; yardsticks: tmvb_token_topics' kernel on the same entries, and a blocked NumPy fp64 restatement on "
                      "a subset of the documents whose time is SCALED to the corpus by entries; no threshold",
              "M": M, "V": V, "entries": int(ptr[-1]), "seed": args.seed, "repeats": args.repeats, "TMVB_GT_SEG": header_define("TMVB_GT_SEG"), "library_variant": os.environ.get("TMVB_LIB_VARIANT", ""), "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    keys = ("runs", "segments", "group_chunks", "index_ms_host", "accum_ms", "select_ms", "shift_drift_ms", "wall_s_whole_call", "accum_ms_over_token_topics_kernel_ms",
            "host_numpy_wall_s_scaled")
    print(json.dumps({k: {q: v[q] for q in keys} for k, v in cases.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
