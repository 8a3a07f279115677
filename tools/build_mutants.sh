#!/bin/bash
# The deliberately WRONG libraries of tests/test_mutants_gpu.py, tests/test_heldout_mutant_gpu.py, tests/test_coherence_mutant_gpu.py, tests/test_neighbors_mutant_gpu.py, tests/test_recranks_mutant_gpu.py, tests/test_rectopn_mutant_gpu.py, tests/test_search_mutant_gpu.py, tests/test_token_topics_mutant_gpu.py, tests/test_kmeans_mutant_gpu.py, tests/test_docmap_mutant_gpu.py, tests/test_topic_compare_mutant_gpu.py and tests/test_group_topics_mutant_gpu.py (negative controls of the parity suite), each = the shipped objects with one
# translation unit recompiled under a -DTMVB_MUTANT_* flag (csrc/tmvb_internal.h lists them):
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_lda_eps.so     epsilon dropped from LDA's phi / gamma            (src/LDA.jl:152, :145)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_ctpf_bet.so    log bet for log vav in CTPF's xi                   (src/CTPF.jl:336 vs src/gpuCTPF.jl:624)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_ctm_mu.so      update_sigma! centred on the new mu                (src/CTM.jl:207-208, quirk Q2)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_flda_eps.so    the filtered models' log(beta + eps) without epsilon (src/fLDA.jl:184, :191)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_fctm_order.so  fCTM's sweep in CTM's order, vsq before lambda     (src/fCTM.jl:239-240)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_lda_stats_eps.so  LDA's statistics pass without eps * sum w      (src/LDA.jl:152)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_flda_entropy.so   fLDA's ELBO without the 0 < tau < 1 guard of H(tau) (src/fLDA.jl:94-97)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_lda_stale_parts.so  tmvb_lda_estep keeps the previous iteration's ELBO parts marked valid (tests/test_train_loop_gpu.py, scenario E)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_index_repeat.so   tmvb_build_inv_index drops the repeated postings of an id inside a document (quirk Q1's overwrite; tests/test_corpus_presentations_gpu.py, P5)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_heldout_tail.so   held-out scoring kernel without the last partial 16-byte chunk of a beta row (tests/test_heldout_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_coherence_tail.so  pair kernel of the co-document counts without the last partial 64-document word (tests/test_coherence_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_neighbors_tail.so  scan kernel of the nearest-document search without the last partial database tile (tests/test_neighbors_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_recranks_tail.so  scan kernel of the held-out ranks without the last partial database tile (tests/test_recranks_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_rectopn_last_excl.so  scan kernel of the top-n recommendations whose search never finds the last id of an exclusion list (tests/test_rectopn_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_ctm_empty_tail.so  a CTM shard without documents keeps the previous iteration's scatter matrix in its statistics tail (tests/test_sharded_oracle_gpu.py, ragged6)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_svi_keep_stats.so  fused global update of stochastic LDA training without the clearing of the batch's statistics (tests/test_svi_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_ctm_svi_no_recentre.so  tail kernel of stochastic CTM training that blends the running scatter matrix without recentring it on the current mu (tests/test_ctm_svi_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_foldin_drop_zayin.so  table kernel of the CTPF fold-in without the zayin term of W (tests/test_ctpf_foldin_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_search_drop_last_entry.so  scan kernel of the word search whose walk over a query's column segment stops one entry early (tests/test_search_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_tt_tie_last.so  top-t selection of the word-topic assignments whose merge across lanes lets the higher topic id win an exact tie (tests/test_token_topics_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_kmeans_no_bias.so  assignment kernel of the k-means clustering whose epilogue compares the dot products without b_c = -n_c / 2 (tests/test_kmeans_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_docmap_z_with_self.so  normaliser of the document map that keeps the M self terms: Z = the blocked sum of zrow without - M (tests/test_docmap_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_topicdiv_drop_tail.so  pair kernel of the topic divergences without the last partial run of 256 terms (tests/test_topic_compare_mutant_gpu.py)
#   topicmodelsvb.jl_amd/libtmvb_hip_mut_gt_seg_cut.so  combine kernel of the grouped word-topic statistics without the last segment of a run longer than one segment (tests/test_group_topics_mutant_gpu.py)
# Needs the shipped build first (python -c "import __graft_entry__ as g; g.build()").  In parallel, but two builds of one translation unit never in the same batch (they share a temporary): tmvb_ctm.hip and
# tmvb_lda.hip have three variants each (tmvb_core.hip one: mut_index_repeat), hence three batches.  About 4 minutes for the first two batches plus one more build of tmvb_lda.hip and tmvb_ctm.hip.
cd "$(dirname "$0")/.." || exit 1
tools/build_variant.sh mut_lda_eps tmvb_lda.hip -DTMVB_MUTANT_LDA_NO_EPS=1 &
tools/build_variant.sh mut_ctpf_bet tmvb_ctpf.hip -DTMVB_MUTANT_CTPF_LOG_BET=1 &
tools/build_variant.sh mut_index_repeat tmvb_core.hip -DTMVB_MUTANT_INDEX_SKIP_REPEAT=1 &
tools/build_variant.sh mut_ctm_mu tmvb_ctm.hip -DTMVB_MUTANT_CTM_SIGMA_NEW_MU=1 &
tools/build_variant.sh mut_flda_eps tmvb_flda.hip -DTMVB_MUTANT_FLDA_NO_EPS=1 &
wait
tools/build_variant.sh mut_fctm_order tmvb_ctm.hip -DTMVB_MUTANT_FCTM_VSQ_FIRST=1 &
tools/build_variant.sh mut_lda_stats_eps tmvb_lda.hip -DTMVB_MUTANT_LDA_STATS_NO_EPS=1 &
tools/build_variant.sh mut_flda_entropy tmvb_flda.hip -DTMVB_MUTANT_FLDA_H_NO_GUARD=1 &
tools/build_variant.sh mut_heldout_tail tmvb_heldout.hip -DTMVB_MUTANT_HELDOUT_DROP_TAIL=1 &
wait
tools/build_variant.sh mut_lda_stale_parts tmvb_lda.hip -DTMVB_MUTANT_LDA_STALE_PARTS=1 &
tools/build_variant.sh mut_coherence_tail tmvb_coherence.hip -DTMVB_MUTANT_CODF_DROP_TAIL=1 &
tools/build_variant.sh mut_neighbors_tail tmvb_neighbors.hip -DTMVB_MUTANT_NB_DROP_TAIL=1 &
tools/build_variant.sh mut_recranks_tail tmvb_recranks.hip -DTMVB_MUTANT_RK_DROP_TAIL=1 &
tools/build_variant.sh mut_rectopn_last_excl tmvb_rectopn.hip -DTMVB_MUTANT_TOPN_MISS_LAST_EXCL=1 &
tools/build_variant.sh mut_ctm_empty_tail tmvb_ctm.hip -DTMVB_MUTANT_CTM_EMPTY_SHARD_TAIL=1 &
tools/build_variant.sh mut_svi_keep_stats tmvb_lda_svi.hip -DTMVB_MUTANT_SVI_KEEP_BATCH_STATS=1 &
tools/build_variant.sh mut_ctm_svi_no_recentre tmvb_ctm_svi.hip -DTMVB_MUTANT_CTM_SVI_NO_RECENTRE=1 &
tools/build_variant.sh mut_foldin_drop_zayin tmvb_ctpf_foldin.hip -DTMVB_MUTANT_FOLDIN_DROP_ZAYIN=1 &
tools/build_variant.sh mut_search_drop_last_entry tmvb_search.hip -DTMVB_MUTANT_SEARCH_DROP_LAST_ENTRY=1 &
tools/build_variant.sh mut_tt_tie_last tmvb_token_topics.hip -DTMVB_MUTANT_TT_TIE_LAST=1 &
tools/build_variant.sh mut_kmeans_no_bias tmvb_kmeans.hip -DTMVB_MUTANT_KM_NO_BIAS=1 &
tools/build_variant.sh mut_docmap_z_with_self tmvb_docmap.hip -DTMVB_MUTANT_MAP_Z_SELF=1 &
tools/build_variant.sh mut_topicdiv_drop_tail tmvb_topic_compare.hip -DTMVB_MUTANT_TD_DROP_TAIL=1 &
tools/build_variant.sh mut_gt_seg_cut tmvb_group_topics.hip -DTMVB_MUTANT_GT_SEG_CUT=1 &
wait
ls -la topicmodelsvb.jl_amd/libtmvb_hip_mut_*.so
