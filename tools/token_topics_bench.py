#!/usr/bin/env python3
"""Word-topic assignments at SYN-NSF size -> profiles/token_topics_bench.json.

Corpus: SYN-NSF (M = 128 804, V = 25 319, about 10.9 M entries).  Factors: A = K Dirichlet(0.1) columns per document, B = K Dirichlet(0.05)
rows over the terms (the shapes of a trained LDA's exp(Elogtheta) and beta), K = 50 and 100, eps = EPSILON.  Cases per K:
    scan_t1, scan_t4      selection only (no dense output) over the whole corpus, hard counts on -- what token_topics() runs
    scan_t1_nohard        the same without the hard counts
    dense_1doc            dense phi of the longest document
    dense_1024docs        dense phi of the first 1 024 documents
Recorded per case: the kernels' device time (HIP events around the kernels only, info.ms_kernel) and the whole call's wall time (host checks,
fp32 staging, uploads and downloads included), medians of --repeats runs after one warm-up; the algorithmic bytes
    read   nsel (8 + 4 KP) + 4 Ms K        written   8 t nsel (selection) or 4 K nsel (dense), + 8 Ms K with hard
and their rate as a fraction of 8 TB/s; the wall time of the blocked NumPy fp64 restatement of the same case on the same host and whether
its best topics equal the device's (entries whose fp64 best and second differ by less than 2 cap(K) relative are not compared).
In the same run: tmvb_heldout_loglik's kernel time on the same entries with the same two matrices (it gathers the same rows and reduces them
to a sum).  No threshold is asserted.

    python tools/token_topics_bench.py [--repeats 5] [--out profiles/token_topics_bench.json]
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
HBM = 8.0e12


def kpad(K):
    q = (K + 3) // 4
    return 4 * (q if q % 2 else q + 1)


def host_restatement(A, B, doc_ptr, terms, counts, docs, t, dense, block=1 << 18):
    """blocked NumPy fp64: (top_idx[nsel, t], margin[nsel], phi or None, seconds)"""
    t0 = time.perf_counter()
    ptr = np.asarray(doc_ptr)
    take = np.concatenate([np.arange(ptr[d], ptr[d + 1]) for d in docs]) if len(docs) < len(ptr) - 1 else np.arange(ptr[-1])
    doc_of = np.repeat(np.asarray(docs), ptr[np.asarray(docs) + 1] - ptr[np.asarray(docs)])
    n, K = len(take), A.shape[0]
    idx = np.empty((n, t), dtype=np.int32)
    margin = np.empty(n)
    phi = np.empty((n, K)) if dense else None
    At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    for a in range(0, n, block):
        b = min(a + block, n)
        y = EPSILON + At[doc_of[a:b]] * Bt[terms[take[a:b]]]
        r = y / y.sum(axis=1, keepdims=True)
        if dense:
            phi[a:b] = r
        part = np.argpartition(-r, min(t, K - 1), axis=1)[:, :t + 1]
        val = np.take_along_axis(r, part, axis=1)
        order = np.lexsort((part, -val), axis=1)
        part, val = np.take_along_axis(part, order, axis=1), np.take_along_axis(val, order, axis=1)
        idx[a:b] = part[:, :t]
        margin[a:b] = (val[:, 0] - val[:, 1]) / val[:, 0]
    return idx, margin, phi, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_topics_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("token_topics_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    ctx = tm.DeviceContext(0)
    med = lambda xs: float(np.median(xs))
    pc = tm.syn_nsf()
    M, V, ptr = pc.M, pc.V, np.asarray(pc.doc_ptr)
    terms, counts = np.asarray(pc.terms), np.asarray(pc.counts)
    longest = int(np.argmax(np.diff(ptr)))
    cases = {}
    for K in (50, 100):
        rng = np.random.Generator(np.random.PCG64(args.seed + K))
        g = rng.standard_gamma(0.1, size=(K, M)) + 1e-300
        A = np.asfortranarray(g / g.sum(axis=0))
        g = rng.standard_gamma(0.05, size=(K, V)) + 1e-300
        B = np.asfortranarray(g / g.sum(axis=1, keepdims=True))
        KP, cap = kpad(K), (K + 12) * 2.0 ** -24
        ho = []
        for r in range(args.repeats + 1):
            rc, res = tm.heldout_loglik_raw(ctx, K, V, A, B, pc)
            assert rc == 0, res
            ho.append(res.ms_kernel)
        heldout_ms = med(ho[1:])
        host_scan = None
        for name, docs, t, kw in (("scan_t1", None, 1, dict(phi=False, hard=True)), ("scan_t4", None, 4, dict(phi=False, hard=True)),
                                  ("scan_t1_nohard", None, 1, dict(phi=False, hard=False)),
                                  ("dense_1doc", [longest], 1, dict(phi=True, hard=False, select=False)),
                                  ("dense_1024docs", list(range(1024)), 1, dict(phi=True, hard=False, select=False))):
            runs = []
            for r in range(args.repeats + 1):               # the first call is the warm-up (code object load, first allocations)
                t0 = time.perf_counter()
                rc, res = tm.token_topics_raw(ctx, K, V, A, B, pc, docs=docs, top=t, **kw)
                wall = time.perf_counter() - t0
                assert rc == 0, res
                runs.append({"wall_s": wall, "ms_kernel": res["info"]["ms_kernel"]})
            info = res["info"]
            nsel, Ms = info["nsel"], (M if docs is None else len(docs))
            dense = kw["phi"]
            rd = nsel * (8 + 4 * KP) + 4 * Ms * K
            wr = (4 * K * nsel if dense else 8 * t * nsel) + (8 * Ms * K if kw["hard"] else 0)
            ms = med([x["ms_kernel"] for x in runs[1:]])
            if docs is None:                                # the whole corpus once per K, with the four best topics: the three scans share it
                if host_scan is None:
                    host_scan = host_restatement(A, B, ptr, terms, counts, list(range(M)), 4, False)
                h_idx, margin, h_phi, host_s = host_scan
            else:
                h_idx, margin, h_phi, host_s = host_restatement(A, B, ptr, terms, counts, docs, t, dense)
            out = {"K": K, "KP": KP, "t": t, "docs": Ms, "nsel": nsel, "outputs": {k: bool(v) for k, v in kw.items()}, "info": info,
                   "kernel_ms": ms, "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"],
                   "algorithmic_bytes": {"read": rd, "written": wr}, "fraction_of_8TBs": (rd + wr) / (ms * 1e-3) / HBM if ms > 0 else None,
                   "host_numpy_fp64_wall_s": host_s, "host_numpy_top": 4 if docs is None else t, "runs": runs}
            if not dense:
                clear = margin > 2 * cap
                out["entries_compared_with_host"] = int(clear.sum())
                out["entries_with_the_same_best_topic_as_host"] = int(np.sum(res["top_idx"][clear, 0] == h_idx[clear, 0]))
                out["kernel_ms_over_heldout_kernel_ms"] = ms / heldout_ms
            else:
                out["worst_rel_deviation_from_host_fp64"] = float((np.abs(res["phi"].astype(np.float64) - h_phi) / h_phi).max())
            cases[f"K{K}_{name}"] = out
            print(f"K = {K} {name}: kernel {ms:.3f} ms, whole call {out['wall_s_whole_call'] * 1e3:.1f} ms, host {host_s:.2f} s", file=sys.stderr, flush=True)
        cases[f"K{K}_heldout_loglik_same_entries"] = {"K": K, "kernel_ms": heldout_ms, "runs_ms": ho,
                                                      "algorithmic_bytes_read": int(ptr[-1]) * (8 + 4 * KP) + 4 * M * K,
                                                      "fraction_of_8TBs": (int(ptr[-1]) * (8 + 4 * KP) + 4 * M * K) / (heldout_ms * 1e-3) / HBM}
    result = {"what": "tmvb_token_topics at SYN-NSF size (Dirichlet(0.1) document columns, Dirichlet(0.05) topic rows, eps = EPSILON), one MI355X; medians "
                      "over the timed repeats (first call = warm-up, listed apart); kernel_ms = HIP events around the kernels only; the host figure is a "
                      "blocked NumPy fp64 restatement on the host of the same machine; tmvb_heldout_loglik's kernel on the same entries and matrices "
                      "beside it; no threshold",
              "M": M, "V": V, "entries": int(ptr[-1]), "seed": args.seed, "repeats": args.repeats, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    keys = ("nsel", "kernel_ms", "wall_s_whole_call", "fraction_of_8TBs", "host_numpy_fp64_wall_s", "kernel_ms_over_heldout_kernel_ms",
            "entries_compared_with_host", "entries_with_the_same_best_topic_as_host", "worst_rel_deviation_from_host_fp64")
    print(json.dumps({k: {q: v[q] for q in keys if q in v} for k, v in cases.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
