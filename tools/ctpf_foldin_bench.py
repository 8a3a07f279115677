#!/usr/bin/env python3
"""CTPF fold-in of users at SYN-CITEU shape -> profiles/ctpf_foldin_bench.json.

SYN-CITEU (M = 16 980 documents, V = 8 000, U = 5 551 users), gpuCTPF trained for --iters iterations at K = 50 and K = 100.  Recorded per K, for
all 5 551 training libraries and for a 64-user slice (users 0 .. 63), folded in on the trained handle (tmvb_ctpf_foldin_users_on, defaults
viter = 10, vtol = 1 / K^2, he0 = 1):
  * ms_prep (the table kernel) and ms_sweeps (the user kernels), HIP events around the kernels only; the whole-call wall time (host checks, sorting,
    uploads and the download included); medians over the timed repeats, the first call listed apart; users on the register and on the workgroup path;
  * the fraction of 8 TB/s that ms_sweeps is on this bytes model: W rows of kp floats, gathered once per user on the register path and once per
    executed sweep on the workgroup path, plus he in and out (K doubles each) per user; ms_prep against 2 K M floats read (the handle's fp32 state)
    and kp M floats written;
  * the fp64 NumPy restatement (tests/ctpf_foldin_restatement.py) on the same host for the 64-user slice, wall time and the largest relative
    deviation of the device from it over the users whose sweep counts agree;
  * what exists without the fold-in for the same need: one train(iter = --iters, recs = False) of the corpus, wall time;
  * the top-15 overlap between recommend_new_users on the training libraries and recommend_topn of the trained model: mean |A & B| / 15 over the
    users and the number of users with identical lists.  Reported, not thresholded.
No threshold is asserted.

    python tools/ctpf_foldin_bench.py [--repeats 3] [--iters 30] [--out profiles/ctpf_foldin_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--M", type=int, default=16980)
    ap.add_argument("--V", type=int, default=8000)
    ap.add_argument("--U", type=int, default=5551)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctpf_foldin_bench.json"))
    args = ap.parse_args()
    import tmvb_amd
    tm = tmvb_amd.pkg
    import ctpf_foldin_restatement as R
    from oracle import oracle as oc
    oc.build(); oc.lib()
    if tm.lib().tmvb_device_count() < 1:
        raise SystemExit("ctpf_foldin_bench needs a gfx950 device; the HIP engine has no CPU fallback")
    med = lambda xs: float(np.median(xs))
    pf = tm.syn_citeu(M=args.M, V=args.V, U=args.U)
    libs = R.transposed_libraries(pf.rdr_ptr, pf.readers, pf.ratings, pf.U)
    lens = np.diff(libs[0])
    cases = {}
    for K in (50, 100):
        g = tm.gpuCTPF(pf, K)
        t0 = time.perf_counter()
        g.train(iter=args.iters, tol=0.0, checkelbo=float("inf"), printelbo=False, recs=False)
        g.synchronize()
        train_s = time.perf_counter() - t0
        kp = (K + 3) // 4 * 4
        for name, n_users in (("all", pf.U), ("slice64", min(64, pf.U))):
            ptr = libs[0][:n_users + 1]
            csr = (ptr, libs[1][:ptr[-1]] + 1, libs[2][:ptr[-1]])                 # 1-based ids for foldin_users
            runs = []
            for _ in range(args.repeats + 1):                                       # the first call is the warm-up
                t0 = time.perf_counter()
                f = tm.foldin_users(g, (csr[0], csr[1]), csr[2])
                runs.append({"wall_s": time.perf_counter() - t0, "ms_prep": f.info["ms_prep"], "ms_sweeps": f.info["ms_sweeps"]})
            ms_prep, ms_sweeps = med([x["ms_prep"] for x in runs[1:]]), med([x["ms_sweeps"] for x in runs[1:]])
            ln = lens[:n_users]
            on_reg = ln <= f.info["capacity"]
            gathers = int(ln[on_reg].sum() + (ln[~on_reg] * f.sweeps[~on_reg]).sum())
            sweep_bytes = gathers * kp * 4 + n_users * K * 16
            prep_bytes = (2 * K + kp) * pf.M * 4
            case = {"K": K, "users": n_users, "library_entries": int(ptr[-1]), "longest_library": int(ln.max()), "train_iters": args.iters,
                    "users_reg": f.info["n_reg"], "users_long": f.info["n_long"], "capacity": f.info["capacity"], "kp": kp,
                    "sweeps_hist": np.bincount(f.sweeps, minlength=11).tolist(),
                    "ms_prep": ms_prep, "ms_sweeps": ms_sweeps, "wall_s_whole_call": med([x["wall_s"] for x in runs[1:]]), "wall_s_first_call": runs[0]["wall_s"],
                    "runs": runs, "bytes_model": {"sweeps": int(sweep_bytes), "prep": int(prep_bytes), "row_gathers": gathers},
                    "fraction_of_8TBps": {"sweeps": sweep_bytes / (ms_sweeps * 1e-3) / 8e12, "prep": prep_bytes / (ms_prep * 1e-3) / 8e12},
                    "parent_route": {"what": "train(iter, recs=False) of the corpus: the only way to he of a user who was not in training", "wall_s": train_s}}
            if name == "slice64":
                g.update_host()
                st = R.State(g.gimel, g.zayin, g.dalet, g.het, g.vav, g.e)
                t0 = time.perf_counter()
                ref, sw = R.foldin_direct(oc.digamma, st, ptr, libs[1][:ptr[-1]], libs[2][:ptr[-1]])
                case["numpy_fp64"] = {"wall_s": time.perf_counter() - t0, "users_with_equal_sweeps": int((sw == f.sweeps).sum())}
                same = sw == f.sweeps
                if same.any():
                    case["numpy_fp64"]["max_rel_deviation"] = float((np.abs(f.he[:, same] - ref[:, same]) / np.abs(ref[:, same])).max())
            cases[f"K{K}_{name}"] = case
        # recommendations for the training users as if they were new, against the trained model's own
        rn = tm.recommend_new_users(g, (libs[0], libs[1] + 1), libs[2], topn=15)
        rt = g.recommend_topn(topn=15, by="user")
        inter = np.array([len(set(rn.idx[u, :rn.count[u]]) & set(rt.idx[u, :rt.count[u]])) for u in range(pf.U)])
        cases[f"K{K}_all"]["top15_overlap_with_recommend_topn"] = {
            "mean_fraction": float((inter / 15.0).mean()), "users_with_identical_lists": int(sum(np.array_equal(rn.idx[u], rt.idx[u]) for u in range(pf.U))),
            "users": pf.U, "note": "he of the fold-in is a fixed point under frozen document factors from he0 = 1 (<= 10 sweeps); the trained he moved with them"}
        g.close()
    result = {"what": "foldin_users on SYN-CITEU, one MI355X; medians over the timed repeats (first call = warm-up, listed apart); device times are HIP events "
                      "around the kernels only; no threshold set",
              "M": args.M, "V": args.V, "U": args.U, "repeats": args.repeats, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {q: v[q] for q in ("users_reg", "users_long", "ms_prep", "ms_sweeps", "wall_s_whole_call", "fraction_of_8TBps")} |
                      {"parent_wall_s": v["parent_route"]["wall_s"]} for k, v in cases.items()}))


if __name__ == "__main__":
    main()
