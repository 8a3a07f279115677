"""
The C ABI of libtmvb_hip.so as ctypes sees it: one line per function of include/tmvb.h, in the header's order, and the mirrors of
the header's structs.  `_lib.lib()` applies the table once, right after loading the library; nothing else in the package assigns
argtypes or restype.  A new ABI function gets one line here (and a mirror Structure if it has an info struct);
tests/test_abi_table_host.py holds every line and every mirror to the header.

Spelling: `<return> <name>(<argument types>)`, `type*n` for n arguments of one type in a row, a Structure's name for a pointer to it.
"""
from __future__ import annotations

import ctypes as C
import re

P_i64 = C.POINTER(C.c_int64)
P_i32 = C.POINTER(C.c_int32)
P_dbl = C.POINTER(C.c_double)
P_f32 = C.POINTER(C.c_float)
VP = C.c_void_p
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)      # tmvb_host_allreduce_fn

TYPES = {
    "void": None, "int": C.c_int, "i32": C.c_int32, "i64": C.c_int64, "f32": C.c_float, "f64": C.c_double, "char": C.c_char, "str": C.c_char_p,
    "pi32": P_i32, "pi64": P_i64, "pf32": P_f32, "pf64": P_dbl, "pu8": C.POINTER(C.c_uint8), "pu32": C.POINTER(C.c_uint32),
    "vp": VP, "pvp": C.POINTER(VP),           # void*, void**
    "h": VP, "ph": C.POINTER(VP),             # an opaque handle (tmvb_ctx*, tmvb_lda*, ...), and handle** / handle* const*
    "fn": HOST_ALLREDUCE_FN,
}

STRUCTS = {}                                  # header typedef name -> its mirror


def _struct(name, typedefs, spec):
    """A ctypes.Structure from "type: field field; type: field ..." in the header's field order."""
    fields = [(f, TYPES[t.strip()]) for part in spec.split(";") for t, fs in [part.split(":")] for f in fs.split()]
    cls = type(name, (C.Structure,), {"_fields_": fields, "__doc__": typedefs, "__module__": __name__})
    for t in typedefs.split(", "):
        STRUCTS[t] = cls
    TYPES[name] = C.POINTER(cls)
    return cls


CorpusInfo = _struct("CorpusInfo", "tmvb_corpus_info_t", "i64: M V U nnz nR sum_counts sum_ratings max_doc_len max_readers n_empty_docs "
                     "n_docs_with_duplicate_terms n_docs_with_duplicate_readers")
DocFile = _struct("DocFile", "tmvb_docfile_t", "i64: M nnz nR V_seen U_seen; pi64: doc_ptr; pi32: terms counts; pi64: rdr_ptr; pi32: readers ratings")
GenCorpResult = _struct("GenCorpResult", "tmvb_gencorp_t", "i64: M nnz sum_counts; pi64: doc_ptr; pi32: terms counts; pf32: log_theta; pi32: doc_topic; "
                        "pi64: topic_term; f32: ms_tables ms_docs ms_tokens ms_condense")
SplitResult = _struct("SplitResult", "tmvb_split_t", "i64: M nnz_obs nnz_held sum_obs sum_held; pi64: obs_ptr; pi32: obs_terms obs_counts; "
                      "pi64: held_ptr; pi32: held_terms held_counts; f32: ms_draw ms_compact")
CodfInfo = _struct("CodfInfo", "tmvb_codf_info_t", "i64: n_slots; i32: n_batches; f32: ms_bitset ms_pairs")
NeighborsInfo = _struct("NeighborsInfo", "tmvb_neighbors_info_t", "i32: splits kp; f32: ms_prep ms_scan ms_merge")
KMeansInfo = _struct("KMeansInfo", "tmvb_kmeans_info_t", "i32: iters stop n_empty kp; i64: moved_last; f32: ms_prep ms_seed ms_assign ms_update")
MapParams = _struct("MapParams", "tmvb_map_params_t", "i32: iters iter0 exag_iters check j_split reserved; i64: seed; f64: exaggeration min_grad_norm; "
                    "f32: momentum0 momentum1 eta min_gain")
MapInfo = _struct("MapInfo", "tmvb_map_info_t", "i32: iters stop n_kl j_split; f64: Z grad_norm; f32: ms_rep ms_att ms_upd reserved")
SearchInfo = _struct("SearchInfo", "tmvb_search_info_t", "i32: splits kp col_tiles; f32: ms_prep ms_scan ms_merge")
TokenTopicsInfo = _struct("TokenTopicsInfo", "tmvb_token_topics_info_t", "i64: nsel n_short n_long; i32: chunks lanes_per_entry; f32: ms_kernel")
ReaderSplit = _struct("ReaderSplit", "tmvb_rsplit_t", "i64: M n_obs n_held; pi64: obs_ptr; pi32: obs_readers obs_ratings; pi64: held_ptr; "
                      "pi32: held_readers held_ratings")
RecRanksInfo = _struct("RecRanksInfo", "tmvb_recranks_info_t", "i32: splits kp; f32: ms_prep ms_pairs ms_scan ms_fix")
RecTopNInfo = _struct("RecTopNInfo", "tmvb_rectopn_info_t", "i32: splits kp; f32: ms_prep ms_scan ms_merge")
FoldinInfo = _struct("FoldinInfo", "tmvb_foldin_info_t", "i32: kp capacity; i64: n_reg n_long; f32: ms_prep ms_sweeps")
SviInfo = _struct("SviInfo", "tmvb_lda_svi_info_t, tmvb_ctm_svi_info_t", "i32: B K; i64: M V t; f64: tau0 kappa rho; f32: c0 c1")
TopicDivInfo = _struct("TopicDivInfo", "tmvb_topicdiv_info_t", "i32: splits runs; f32: ms_prep ms_pairs ms_merge")
RelevanceInfo = _struct("RelevanceInfo", "tmvb_relevance_info_t", "f32: ms_score ms_select ms_terms")
GroupTopicsInfo = _struct("GroupTopicsInfo", "tmvb_group_topics_info_t", "i64: nsel runs segments; i32: group_chunks lanes_per_entry; "
                          "f32: ms_index ms_accum ms_select ms_shift")

_TABLE = """
int  tmvb_abi_version()
str  tmvb_last_error()
int  tmvb_device_count()
int  tmvb_ctx_create(i32 vp ph)
int  tmvb_ctx_destroy(h)
int  tmvb_ctx_synchronize(h)
int  tmvb_event_create(h ph)
int  tmvb_event_record(h)
int  tmvb_event_elapsed_ms(h h pf32)
int  tmvb_event_destroy(h)
int  tmvb_special_f32(h i32 pf32 pf32 i64)
int  tmvb_topic_order(h pf64 i32 i64 pi32)
int  tmvb_comm_unique_id(vp)
int  tmvb_comm_create_rccl(h vp i32 i32 ph)
int  tmvb_comm_create_rccl_all(ph i32 ph)
int  tmvb_comm_create_host(h i32 i32 fn vp ph)
int  tmvb_comm_destroy(h)
int  tmvb_comm_info(h pi32*3)
int  tmvb_comm_allreduce(h vp i64 i32)
int  tmvb_rccl_version()
int  tmvb_corpus_create(h i64*3 pi64 pi32 pi32 pi64 pi32 pi32 ph)
int  tmvb_corpus_destroy(h)
int  tmvb_corpus_info(h CorpusInfo)
int  tmvb_docfile_read(str char i32*4 DocFile)
void tmvb_docfile_free(DocFile)
int  tmvb_lda_create(h h i32 ph)
int  tmvb_lda_destroy(h)
int  tmvb_lda_set_state(h pf64*7)
int  tmvb_lda_get_state(h pf64*7)
int  tmvb_lda_estep(h i32 f64)
int  tmvb_lda_stats(h pvp pi64)
int  tmvb_lda_bind_stats(h vp i64)
int  tmvb_lda_reduce_docs(h)
int  tmvb_lda_set_distributed(h i64 i32)
int  tmvb_lda_update_beta(h)
int  tmvb_lda_update_alpha(h i32 f64)
int  tmvb_lda_update_elbo(h pf64)
int  tmvb_lda_train(h i32 f64 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_lda_set_comm(h h i64)
int  tmvb_lda_estep_allreduce(h i32 f64)
int  tmvb_allreduce_plan(pf64 i64 i32 pi64 pi32 pi32)
int  tmvb_lda_train_group(ph i32 i32 f64 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_lda_sweep_hist(h pi64 i32)
int  tmvb_lda_doc_sweeps(h pu8)
int  tmvb_lda_elbo_form(h pi32)
int  tmvb_lda_estep_launches(h pi32)
int  tmvb_lda_estep_pieces(h pi32)
int  tmvb_lda_last_estep_ms(h pf32)
int  tmvb_flda_create(h h i32 ph)
int  tmvb_flda_destroy(h)
int  tmvb_flda_set_state(h pf64*12)
int  tmvb_flda_get_state(h pf64*12)
int  tmvb_flda_estep(h i32 f64)
int  tmvb_flda_reduce_docs(h)
int  tmvb_flda_stats(h pvp pi64)
int  tmvb_flda_update_beta(h)
int  tmvb_flda_update_alpha(h i32 f64)
int  tmvb_flda_update_eta(h)
int  tmvb_flda_update_elbo(h pf64)
int  tmvb_flda_train(h i32 f64 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_flda_set_comm(h h i64 i64)
int  tmvb_flda_train_group(ph i32 i32 f64 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_flda_doc_sweeps(h pu8)
int  tmvb_flda_elbo_form(h pi32)
int  tmvb_flda_last_estep_ms(h pf32)
int  tmvb_ctm_create(h h i32 ph)
int  tmvb_ctm_destroy(h)
int  tmvb_ctm_set_state(h pf64*10)
int  tmvb_ctm_get_state(h pf64*10)
int  tmvb_ctm_estep(h i32 f64 i32 f64)
int  tmvb_ctm_reduce_docs(h)
int  tmvb_ctm_stats(h pvp pi64)
int  tmvb_ctm_bind_stats(h vp i64)
int  tmvb_ctm_set_distributed(h i64 i32)
int  tmvb_ctm_update_beta(h)
int  tmvb_ctm_update_sigma(h)
int  tmvb_ctm_update_mu(h)
int  tmvb_ctm_update_elbo(h pf64)
int  tmvb_ctm_elbo_form(h pi32)
int  tmvb_ctm_train(h i32 f64 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_ctm_set_comm(h h i64)
int  tmvb_ctm_train_group(ph i32 i32 f64 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_ctm_sweep_hist(h pi64 i32 pi64)
int  tmvb_ctm_doc_sweeps(h pu8)
int  tmvb_ctm_last_estep_ms(h pf32)
int  tmvb_ctm_solver_stats(h pi64)
int  tmvb_fctm_create(h h i32 ph)
int  tmvb_fctm_destroy(h)
int  tmvb_fctm_set_state(h pf64*15)
int  tmvb_fctm_get_state(h pf64*15)
int  tmvb_fctm_estep(h i32 f64 i32 f64)
int  tmvb_fctm_reduce_docs(h)
int  tmvb_fctm_update_beta(h)
int  tmvb_fctm_update_sigma(h)
int  tmvb_fctm_update_mu(h)
int  tmvb_fctm_update_elbo(h pf64)
int  tmvb_fctm_train(h i32 f64 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_fctm_set_comm(h h i64)
int  tmvb_fctm_train_group(ph i32 i32 f64 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_fctm_sweep_hist(h pi64 i32 pi64)
int  tmvb_fctm_doc_sweeps(h pu8)
int  tmvb_fctm_solver_stats(h pi64)
int  tmvb_fctm_elbo_form(h pi32)
int  tmvb_ctpf_create(h h i32 ph)
int  tmvb_ctpf_destroy(h)
int  tmvb_ctpf_set_state(h pf64*10)
int  tmvb_ctpf_set_state_old(h pf64*8)
int  tmvb_ctpf_get_state(h pf64*10)
int  tmvb_ctpf_estep(h i32 f64)
int  tmvb_ctpf_reduce_docs(h)
int  tmvb_ctpf_stats(h pvp pi64)
int  tmvb_ctpf_bind_stats(h vp i64)
int  tmvb_ctpf_set_distributed(h i32)
int  tmvb_ctpf_mstep(h)
int  tmvb_ctpf_update_elbo(h pf64)
int  tmvb_ctpf_elbo_form(h pi32)
int  tmvb_ctpf_update_elbo_parts(h pf64 pf64)
int  tmvb_ctpf_train(h i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_ctpf_set_comm(h h)
int  tmvb_ctpf_train_group(ph i32 i32 f64 i32 f64 i32 pf64 pi32 pf64)
int  tmvb_ctpf_sweep_hist(h pi64 i32)
int  tmvb_ctpf_doc_sweeps(h pu8)
int  tmvb_ctpf_last_estep_ms(h pf32)
int  tmvb_ctpf_recommend(h pf64 pi32*4 pf32 pf32)
int  tmvb_lda_gencorp(h i32 i64 pf64 pf64 i64 i64 f64 f64 i64 i32 GenCorpResult)
int  tmvb_ctm_gencorp(h i32 i64 pf64*3 i64 i64 f64 f64 i64 i32 GenCorpResult)
void tmvb_gencorp_free(GenCorpResult)
int  tmvb_philox4x32_10(pu32*3)
int  tmvb_corpus_split(h i64 i64 pi64 pi32 pi32 f64 i64 i64 SplitResult)
void tmvb_split_free(SplitResult)
int  tmvb_heldout_loglik(h i32 i64 i64 pf64 pf64 pi64 pi32 pi32 f64 pf64 pi64 pi64 pf32)
int  tmvb_corpus_codocfreq(h i64 i64 pi64 pi32 pi32 i32 i32 pi32 i64 pi64 CodfInfo)
int  tmvb_coherence_from_counts(i32 i32 i64 pi64 pf64 pf64 pi32)
int  tmvb_topic_neighbors(h i32 i32 i64 pf64 i64 pf64 i64 i32 i32 pi32 pf32 pi32 NeighborsInfo)
int  tmvb_topic_kmeans(h i32 i32 i64 pf64 i32 pf64 i64 i32 f64 pi32 pf64 pi64 pf32 pf64 pi32 KMeansInfo)
int  tmvb_map_affinity(h i64 i64 i32 pi32 pf32 pi32 f64 pf64 pf64 pi64 pi32 pf32)
int  tmvb_map_layout(h i64 pi64 pi32 pf32 MapParams pf32*6 i32 pf64 pi32 pf64*3 pf32 MapInfo)
int  tmvb_topic_search(h i32 i64 i64 pf64 pf64 f64 i64 pi64 pi32 pi32 i32 i32 pi32 pf32 pi32 SearchInfo)
int  tmvb_token_topics(h i32 i64 i64 pf64 pf64 pi64 pi32*3 i64 f64 i32 i64 pi32 pf32 pf32 pi64 TokenTopicsInfo)
int  tmvb_digamma_f64(pf64 pf64 i64)
int  tmvb_readers_split(i64 i64 pi64 pi32 pi32 f64 i64 i64 i32 ReaderSplit)
void tmvb_rsplit_free(ReaderSplit)
int  tmvb_score_ranks(h i32 i64 pf64 i64 pf64 pi64 pi32 pi64 pi32 i32 pi32 pi32 pf32 RecRanksInfo)
int  tmvb_rank_metrics(i64 pi64 pi32 pi32 i32 pi32 pf64*6 pi64)
int  tmvb_score_topn(h i32 i64 pf64 i64 pf64 pi64 pi32 i32 i32 pi32 pf32 pi32 RecTopNInfo)
int  tmvb_ctpf_foldin_users(h i32 i64 pf64*5 f64 i64 pi64 pi32 pi32 pf64 i32 f64 pf64 pi32 FoldinInfo)
int  tmvb_ctpf_foldin_users_on(h i64 pi64 pi32 pi32 pf64 i32 f64 pf64 pi32 FoldinInfo)
int  tmvb_lda_svi_create(h i64 i64 pi64 pi32 pi32 i32 pi64 i32 ph)
int  tmvb_lda_svi_destroy(h)
int  tmvb_lda_svi_set_state(h pf64*7 pi64)
int  tmvb_lda_svi_get_state(h pf64*7 pi64)
int  tmvb_lda_svi_set_schedule(h f64 f64)
int  tmvb_lda_svi_run(h pi32 i64 i32 f64 i32 f64)
int  tmvb_lda_svi_final_pass(h i32 f64)
int  tmvb_lda_svi_info(h SviInfo)
int  tmvb_lda_svi_doc_sweeps(h pu8)
int  tmvb_lda_svi_last_run_ms(h pf32*3 pi64)
int  tmvb_ctm_svi_create(h i64 i64 pi64 pi32 pi32 i32 pi64 i32 ph)
int  tmvb_ctm_svi_destroy(h)
int  tmvb_ctm_svi_set_state(h pf64*13 pi64)
int  tmvb_ctm_svi_get_state(h pf64*13 pi64)
int  tmvb_ctm_svi_set_schedule(h f64 f64)
int  tmvb_ctm_svi_run(h pi32 i64 i32 f64 i32 f64)
int  tmvb_ctm_svi_final_pass(h i32 f64 i32 f64)
int  tmvb_ctm_svi_info(h SviInfo)
int  tmvb_ctm_svi_doc_sweeps(h pu8)
int  tmvb_ctm_svi_last_run_ms(h pf32*3 pi64)
int  tmvb_topic_divergence(h i32 i64 i32 pf64 i32 pf64 f64 i32 pf64 TopicDivInfo)
int  tmvb_term_relevance(h i32 i64 pf64*3 f64 i32 pi32 pf64 pi32 pf64*3 RelevanceInfo)
int  tmvb_assignment(i32 i32 pf64 pi32 pf64)
int  tmvb_group_topics(h i32 i64 i64 pf64 pf64 pi64 pi32*3 i32 f64 i32 i32 pi64 pi64 pf64 pi32 pf64*4 GroupTopicsInfo)
int  tmvb_group_index(i64 i64 pi64 pi32 pi32 i32 pi64 pi64 pi32 pi32 pi64)
"""


def _parse(table):
    out = {}
    for ret, name, args in re.findall(r"^(\w+)\s+(\w+)\((.*)\)$", table, flags=re.M):
        argtypes = []
        for tok in args.split():
            t, _, n = tok.partition("*")
            argtypes += [TYPES[t]] * int(n or 1)
        out[name] = (TYPES[ret], argtypes)
    return out


PROTOTYPES = _parse(_TABLE)                   # name -> (restype, argtypes), in the header's order


def apply(L):
    """Declare every function of the table on the loaded library."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
