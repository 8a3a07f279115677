#!/usr/bin/env python
"""Register / scratch / LDS figures of every kernel in libtmvb_hip.so, from the code objects' own metadata.

    python tools/kernel_resources.py [lib.so]             table of every kernel (sorted by scratch, then registers)
    python tools/kernel_resources.py --check [lib.so]     the build-time check: every kernel named in BENCHED must exist and keep its
                                                          private segment (scratch) within its ceiling; build() fails otherwise

Round-4 review: the benched CTM kernel owned 512 registers and still spilled to 428 B / lane of scratch, and nothing in the repository said
so.  The .so carries one clang offload bundle per translation unit (section .hip_fatbin, magic __CLANG_OFFLOAD_BUNDLE__); each gfx950 entry
is an ELF code object whose NT_AMDGPU_METADATA note (llvm-readelf --notes) lists, per kernel, .vgpr_count / .agpr_count / .sgpr_count /
.private_segment_fixed_size / .vgpr_spill_count / .sgpr_spill_count / .group_segment_fixed_size.  No GPU needed.
"""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

# The kernels behind the numbers of bench.py's line (demangled-name prefixes) and the scratch bytes per lane each may use.  Everything that is
# timed runs without scratch -- except the lane-per-document CTM kernel, whose 388 B (428 in round 4) round 5 could not remove
# without losing time (profiles/r5_ctm_token_experiments.txt); its ceiling is that figure, so that it cannot silently grow.
BENCHED = {
    # config 2 / 3: LDA K = 50 (13 chunks per row) and K = 100 (25)
    "lda_estep_grid_kernel<13,": 0, "lda_estep_grid_kernel<25,": 0, "lda_estep_grid_long_kernel<13,": 0, "lda_estep_grid_long_kernel<25,": 0,
    "termstats_recompute_kernel<13,": 0, "termstats_recompute_kernel<25,": 0, "termstats_multi_kernel": 0, "beta_norm_kernel": 0, "lda_alpha_kernel<": 0,
    # config 4: CTM K = 50
    "ctm_estep_batch_kernel<52, false, false>": 388, "ctm_estep_quad_kernel<52, false>": 96, "ctm_scatter_mfma_kernel": 0, "ctm_sigma_mu_kernel": 0,
    # config 5: CTPF K = 50
    "ctpf_estep_grid_narrow_kernel<13>": 0, "ctpf_estep_grid_wide_kernel<13>": 0, "ctpf_estep_grid_long2_kernel<13>": 0, "termstats_recompute2_kernel<13": 0,
    "ctpf_mstep_kernel": 0,
    # held-out evaluation (tools/heldout_bench.py): the scoring kernel's two workgroup sizes and the split's draw kernel
    "heldout_loglik_kernel<64>": 0, "heldout_loglik_kernel<256>": 0, "split_draw_kernel": 0,
    # topic coherence (tools/coherence_bench.py): the bit-matrix build and the pair pass of the co-document counts
    "codf_bitset_kernel": 0, "codf_pairs_kernel": 0,
    # nearest documents in topic space (tools/neighbors_bench.py): features, the fused MFMA scan / top-n, the merge of the splits' lists
    "nb_feature_kernel": 0, "nb_scan_kernel": 0, "nb_merge_kernel": 0,
    # held-out recommendation ranks (tools/recs_eval_bench.py): features, pair scores, target sort, the fused MFMA scan / count, the exclusion fix
    "rk_feature_kernel": 0, "rk_pairs_kernel": 0, "rk_sort_kernel": 0, "rk_scan_kernel": 0, "rk_fix_kernel": 0,
    # top-n recommendations (tools/rectopn_bench.py): features, the fused MFMA scan / exclusion search / top-n, the merge of the splits' lists
    "rt_feature_kernel": 0, "rt_scan_kernel": 0, "rt_merge_kernel": 0,
    # search by words (tools/search_bench.py): features, the fused MFMA scan / fp64 log over the query segments / top-n, the merge of the splits' lists
    "sr_feature_kernel": 0, "sr_scan_kernel": 0, "sr_merge_kernel": 0,
    # word-topic assignments (tools/token_topics_bench.py): both workgroup sizes, selection only and selection + dense stores
    "token_topics_kernel<64, false>": 0, "token_topics_kernel<256, false>": 0, "token_topics_kernel<64, true>": 0, "token_topics_kernel<256, true>": 0,
    # clustering in topic space (tools/cluster_bench.py): features and norms, the fused MFMA assignment, the fixed-order update, the k-means++ rounds
    "km_feature_kernel": 0, "km_norm_kernel": 0, "km_assign_kernel": 0, "km_run_sum_kernel": 0, "km_finalize_kernel": 0, "km_seed_dist_kernel": 0,
    "km_seed_pick_kernel": 0,
    # document map (tools/docmap_bench.py): the entropy search, the all-pairs repulsion and its segment sums, the edge sums (forces and KL), the update
    "map_affinity_kernel": 0, "map_repulse_kernel": 0, "map_finish_kernel": 0, "map_attract_kernel<": 0, "map_update_kernel": 0,
    # topic comparison (tools/topic_compare_bench.py): the transpose, the fp64 pair kernel under its four metrics, the merge of the run sums; relevance
    "td_prep_kernel": 0, "td_pairs_kernel<": 0, "td_merge_kernel<": 0, "tr_score_kernel": 0, "tr_select_kernel": 0, "tr_terms_kernel": 0,
    # topics by group (tools/group_topics_bench.py): the accumulation over the (group, term) index, the combine of the long runs, the fixed-order row kernels
    "group_topics_kernel": 0, "gt_combine_kernel": 0, "gt_rowsum_kernel": 0, "gt_norm_kernel": 0, "gt_pool_kernel": 0, "gt_select_kernel": 0, "gt_js_kernel": 0,
    # stochastic LDA training (tools/svi_bench.py): the fused global update -- blend + partial row sums, then normalise
    "svi_blend_kernel<": 0, "svi_norm_kernel": 0,
    # stochastic CTM training (tools/ctm_svi_bench.py): the tail of the fused global update -- recentre in fp64, blend (the K x V part is the two above)
    "ctm_svi_tail_kernel": 0,
}


def code_objects(path):
    """the gfx950 ELF images inside the clang offload bundles of `path`"""
    blob = open(path, "rb").read()
    out, pos = [], 0
    while True:
        pos = blob.find(MAGIC, pos)
        if pos < 0:
            break
        n = struct.unpack_from("<Q", blob, pos + 24)[0]
        p = pos + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos += 24
    return out


def demangle(names):
    try:
        exe = next(e for e in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "/usr/bin/c++filt", "c++filt") if e == "c++filt" or os.path.exists(e))
        r = subprocess.run([exe], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
        out = r.stdout.splitlines()
        return out if len(out) == len(names) else names
    except Exception:
        return names


def kernels(path):
    rows = []
    for img in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img); f.flush()
            txt = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.(?=agpr_count|args)", txt):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m or ".vgpr_count" not in blk:
                continue
            g = lambda k, d=0: int((re.search(r"\." + k + r":\s+(\d+)", blk) or [0, d])[1])
            rows.append({"name": m.group(1), "vgpr": g("vgpr_count"), "agpr": g("agpr_count"), "sgpr": g("sgpr_count"),
                         "scratch": g("private_segment_fixed_size"), "vgpr_spills": g("vgpr_spill_count"), "sgpr_spills": g("sgpr_spill_count"),
                         "lds": g("group_segment_fixed_size"), "wg": g("max_flat_workgroup_size")})
    dm = demangle([r["name"] for r in rows])
    for r, d in zip(rows, dm):
        r["demangled"] = re.sub(r"^void ", "", d)
    return rows


def check(rows):
    bad = []
    for pref, ceiling in BENCHED.items():
        hit = [r for r in rows if r["demangled"].startswith(pref)]
        if not hit:
            bad.append(f"benched kernel {pref!r} not found in the library")
        for r in hit:
            if r["scratch"] > ceiling:
                bad.append(f"{r['demangled'][:90]}: {r['scratch']} B of scratch per lane (ceiling {ceiling}); {r['vgpr_spills']} VGPR + {r['sgpr_spills']} SGPR spills")
    return bad


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    lib = argv[0] if argv else os.path.join(ROOT, "topicmodelsvb.jl_amd", "libtmvb_hip.so")
    rows = kernels(lib)
    if "--check" in sys.argv:
        bad = check(rows)
        for b in bad:
            print("KERNEL RESOURCE CHECK:", b)
        print(f"kernel resource check: {len(rows)} kernels, {len(BENCHED)} benched prefixes, {'FAILED' if bad else 'ok'}")
        sys.exit(1 if bad else 0)
    if "--json" in sys.argv:
        print(json.dumps(rows)); return
    if "--benched" in sys.argv:
        rows = [r for r in rows if any(r["demangled"].startswith(p) for p in BENCHED)]
    rows.sort(key=lambda r: (-r["scratch"], -(r["vgpr"] + r["agpr"]), r["demangled"]))
    print(f"# {os.path.basename(lib)}: {len(rows)} gfx950 kernels (llvm-readelf --notes of the embedded code objects; tools/kernel_resources.py)")
    print(f"{'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch_B':>9} {'v_spill':>7} {'s_spill':>7} {'lds_B':>7}  benched  kernel")
    for r in rows:
        b = "*" if any(r["demangled"].startswith(p) for p in BENCHED) else " "
        print(f"{r['vgpr']:5d} {r['agpr']:5d} {r['sgpr']:5d} {r['scratch']:9d} {r['vgpr_spills']:7d} {r['sgpr_spills']:7d} {r['lds']:7d}     {b}     {r['demangled'][:130]}")


if __name__ == "__main__":
    main()
