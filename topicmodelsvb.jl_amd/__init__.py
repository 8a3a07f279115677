"""
topicmodelsvb.jl_amd -- MI355X (gfx950) variational-inference engine behind TopicModelsVB.jl's
`TopicModel / train! / @gpu` surface.  Product code: HIP kernels + C ABI in csrc/ (built into
libtmvb_hip.so), and this thin host mirror of the reference's operator interface.

Import through the `tmvb_amd` shim at the repo root (the directory name is not a legal module name).
"""
from ._lib import (CorpusError, DocumentError, EngineError, TopicModelError, build, exported_symbols, lib, LIB_PATH)
from .corpus import (Corpus, Document, PackedCorpus, check_corp, check_doc, dirichlet_rows, readcorp, readcorp_packed, syn_citeu,
                     syn_nsf, synthetic_lda_corpus, writecorp)
from .lda import LDA, DeviceContext, DeviceCorpus, check_model, gpuLDA, gpu_train, predict, topicdist
from .ctm import CTM, check_model_ctm, gpuCTM, gpu_train_ctm, predict_ctm, topicdist_ctm
from .ctpf import CTPF, check_model_ctpf, gpuCTPF, gpu_train_ctpf, topicdist_ctpf
from .comm import Communicator, rccl_version
from .flda import fLDA, check_model_flda, gpufLDA, gpu_train_flda, predict_flda
from .fctm import fCTM, check_model_fctm, gpufCTM, gpu_train_fctm, predict_fctm
from .gencorp import gencorp, gencorp_raw, gendoc
from .heldout import HeldoutResult, heldout_loglik, heldout_loglik_raw, perplexity, split_corpus, split_corpus_raw
from .coherence import CoherenceResult, coherence, coherence_from_counts, coherence_from_counts_raw, codocfreq_raw
from .neighbors import NeighborsResult, docsim, neighbors_raw, topic_proportions
from .cluster import ClusterResult, cluster_docs, kmeans_raw
from .docmap import DocMap, map_affinity_raw, map_docs, map_layout_raw
from .topic_compare import (RelevantTerms, TopicComparison, TopicMap, TopicStability, assignment_raw, compare_topics, pcoa, relevant_terms,
                            term_frequencies, term_relevance_raw, topic_distances, topic_divergence_raw, topic_map, topic_share, topic_stability,
                            topic_word_matrix)
from .search import SearchInfo, SearchResult, pack_queries, search, search_raw
from .token_topics import TokenTopics, phi, token_factors, token_topics, token_topics_raw
from .group_topics import GroupTopics, group_index_raw, group_topics, group_topics_raw, time_bins
from .recs_eval import (HeldReaders, RecEvalResult, rank_metrics, rank_metrics_raw, rec_eval, rec_quality, rec_ranks_raw, split_readers,
                        split_readers_raw)
from .recs_topn import RecTopN, rec_topn_raw, recommend_topn
from .ctpf_foldin import (FOLDIN_REG_CAPACITY, FOLDIN_REG_CAPACITY_BIGK, FoldinUsers, foldin_libraries, foldin_reg_capacity, foldin_users,
                          foldin_users_raw, predict_ctpf, recommend_new_docs, recommend_new_users)
from .lda_svi import gpuLDAStochastic, gpu_train_stochastic, svi_cuts, svi_order, svi_rho
from .ctm_svi import gpuCTMStochastic, gpu_train_ctm_stochastic

__all__ = ["CorpusError", "DocumentError", "EngineError", "TopicModelError", "build", "exported_symbols", "lib", "LIB_PATH",
           "Corpus", "Document", "PackedCorpus", "check_corp", "check_doc", "dirichlet_rows", "readcorp", "readcorp_packed", "writecorp",
           "syn_citeu", "syn_nsf", "synthetic_lda_corpus", "LDA", "DeviceContext", "DeviceCorpus", "check_model", "gpuLDA",
           "gpu_train", "predict", "topicdist", "predict_ctm", "topicdist_ctm", "CTM", "check_model_ctm", "gpuCTM", "gpu_train_ctm", "CTPF", "check_model_ctpf", "gpuCTPF", "gpu_train_ctpf", "Communicator", "rccl_version", "fLDA", "check_model_flda", "gpufLDA", "gpu_train_flda", "fCTM", "check_model_fctm", "gpufCTM", "gpu_train_fctm", "predict_flda", "predict_fctm", "topicdist_ctpf",
           "gencorp", "gencorp_raw", "gendoc",
           "HeldoutResult", "heldout_loglik", "heldout_loglik_raw", "perplexity", "split_corpus", "split_corpus_raw",
           "CoherenceResult", "coherence", "coherence_from_counts", "coherence_from_counts_raw", "codocfreq_raw",
           "NeighborsResult", "docsim", "neighbors_raw", "topic_proportions",
           "ClusterResult", "cluster_docs", "kmeans_raw",
           "DocMap", "map_affinity_raw", "map_docs", "map_layout_raw",
           "RelevantTerms", "TopicComparison", "TopicMap", "TopicStability", "assignment_raw", "compare_topics", "pcoa", "relevant_terms",
           "term_frequencies", "term_relevance_raw", "topic_distances", "topic_divergence_raw", "topic_map", "topic_share", "topic_stability",
           "topic_word_matrix",
           "SearchInfo", "SearchResult", "pack_queries", "search", "search_raw",
           "TokenTopics", "phi", "token_factors", "token_topics", "token_topics_raw",
           "GroupTopics", "group_index_raw", "group_topics", "group_topics_raw", "time_bins",
           "HeldReaders", "RecEvalResult", "rank_metrics", "rank_metrics_raw", "rec_eval", "rec_quality", "rec_ranks_raw", "split_readers", "split_readers_raw",
           "RecTopN", "rec_topn_raw", "recommend_topn",
           "FOLDIN_REG_CAPACITY", "FOLDIN_REG_CAPACITY_BIGK", "FoldinUsers", "foldin_libraries", "foldin_reg_capacity", "foldin_users", "foldin_users_raw",
           "predict_ctpf", "recommend_new_docs", "recommend_new_users",
           "gpuLDAStochastic", "gpu_train_stochastic", "svi_cuts", "svi_order", "svi_rho",
           "gpuCTMStochastic", "gpu_train_ctm_stochastic"]
