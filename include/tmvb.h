/*
 * tmvb.h -- C ABI of libtmvb_hip.so, the MI355X (gfx950) variational-inference engine that
 * replaces TopicModelsVB.jl's OpenCL backend (gpuLDA / gpuCTM / gpuCTPF) behind the package's
 * `TopicModel / train! / @gpu` surface.
 *
 * Every entry point cites the reference interface it replaces (file:line relative to the
 * reference repository root).  The reference drives its device through one Julia function per
 * kernel pair (update_phi!, update_gamma!, ...); this engine fuses the per-document sweep into one
 * kernel, so the per-document operator triple maps onto a single `*_estep` call that follows the
 * CPU path's per-document semantics (src/LDA.jl:170-180), which is the parity target -- not the
 * OpenCL path's global-median rule (src/gpuLDA.jl:361).
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (streams and device pointers travel
 *     as void*).
 *   - all host matrices are column-major K x (.) Float64, exactly the memory of the reference's
 *     Matrix{Float64} (beta) or of hcat(model.gamma...) (per-document vectors).
 *   - term / reader ids are 0-based (the reference subtracts 1 on upload, src/modelutils.jl:371).
 *   - every call returns a status code; tmvb_last_error() gives the message of the last failure on
 *     the calling thread.  Calls are synchronous on return unless stated otherwise.
 *   - the library copies host data in/out during the call and never retains host pointers.
 *   - quirk Q1: the reference overwrites (does not accumulate) duplicate term ids inside one
 *     document (src/LDA.jl:131); this engine accumulates.  Corpora must be condensed
 *     (src/Corpus.jl:523) for parity; tmvb_corpus_create reports duplicates via
 *     tmvb_corpus_info.
 */
#ifndef TMVB_H
#define TMVB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMVB_ABI_VERSION 2

/* status codes (reference: ArgumentError src/gpuLDA.jl:349-351, TopicModelError
 * src/modelutils.jl:1-5, CorpusError src/Corpus.jl:85-89) */
#define TMVB_OK          0
#define TMVB_EINVAL      1   /* bad argument            -> ArgumentError   */
#define TMVB_ESHAPE      2   /* inconsistent sizes      -> TopicModelError */
#define TMVB_ECORPUS     3   /* corpus failed check_corp -> CorpusError    */
#define TMVB_ENOMEM      4
#define TMVB_EHIP        5   /* HIP runtime failure */
#define TMVB_ENONFINITE  6   /* non-finite statistic / state */
#define TMVB_ENODEVICE   7   /* no usable gfx950 device */
#define TMVB_ERCCL       8   /* RCCL / host-collective failure (document-sharded runs) */

typedef struct tmvb_ctx    tmvb_ctx;
typedef struct tmvb_corpus tmvb_corpus;
typedef struct tmvb_lda    tmvb_lda;
typedef struct tmvb_ctm    tmvb_ctm;
typedef struct tmvb_ctpf   tmvb_ctpf;
typedef struct tmvb_comm   tmvb_comm;
typedef struct tmvb_flda   tmvb_flda;
typedef struct tmvb_fctm   tmvb_fctm;

int         tmvb_abi_version(void);
const char* tmvb_last_error(void);

/* Number of visible HIP devices (0 when there is no GPU); never fails. */
int tmvb_device_count(void);

/* ---- context: replaces cl.create_compute_context() (src/gpuLDA.jl:64) ----
 * One context = one GPU + one in-order stream.  `hip_stream` may be NULL (the library creates its
 * own stream) or an existing hipStream_t owned by the caller (e.g. the host framework's current
 * stream, so that its collectives are ordered with the engine's kernels). */
int tmvb_ctx_create(int32_t device_id, void* hip_stream, tmvb_ctx** out);
int tmvb_ctx_destroy(tmvb_ctx* ctx);
int tmvb_ctx_synchronize(tmvb_ctx* ctx);

/* Timing events on the context's stream for a host that measures the library's asynchronous calls (bench.py's HIP-event bracket around
 * the E-step): HIP events WITH time stamps and WITHOUT the system-scope fence a default event performs when it completes
 * (hipEventDisableSystemFence -- the flag HIP documents for timing; two default events per 0.77 ms LDA iteration cost it 1.4 %).
 * tmvb_event_elapsed_ms waits for `stop`.  Events belong to the device of the context that created them. */
typedef struct tmvb_event tmvb_event;
int tmvb_event_create(tmvb_ctx* ctx, tmvb_event** out);
int tmvb_event_record(tmvb_event* ev);                                  /* on the creating context's stream */
int tmvb_event_elapsed_ms(tmvb_event* start, tmvb_event* stop, float* ms);
int tmvb_event_destroy(tmvb_event* ev);
/* Diagnostics: evaluate the engine's fp32 device special functions on host data (the accuracy pins of the tests).
 * which: 0 = digamma (x > 0; src/utils.jl:21-53's algorithm), 1 = exp as used for exp(Elogtheta) (x <= 0 in exact
 * arithmetic), 2 = the rcp-based reciprocal 1/x. */
int tmvb_special_f32(tmvb_ctx* ctx, int32_t which, const float* x, float* y, int64_t n);
/* model.topics behind every train! of the reference: topics[i] = reverse(sortperm(vec(beta[i,:]))) (src/gpuLDA.jl:374, src/gpuCTM.jl and
 * src/gpuCTPF.jl alike; CTPF passes alef ./ bet).  beta: the model's K x V field, column-major, fp64, on the HOST; topics: K rows of V column
 * ids, row-major, 1-based like the reference's, on the host.  One stable segmented sort on the device, read backwards: ties come out in the
 * order sortperm + reverse gives them.  K * V < 2^31. */
int tmvb_topic_order(tmvb_ctx* ctx, const double* beta, int32_t K, int64_t V, int32_t* topics);


/* ---- communicator: document-sharded multi-GPU behind the C ABI (new: the reference is single-device, src/gpuLDA.jl:64;
 * the closest precedent is the v0.6 batch accumulation `newbeta +=`, v0.6/src/gpuLDA.jl:200-225) ----
 * Documents are conditionally independent given the globals, so every GPU runs the fused E-step on its own contiguous
 * document shard and the ONLY exchange per outer iteration is one all-reduce (sum, f32) of the packed sufficient
 * statistics (tmvb_*_stats); every rank then runs the identical deterministic M-step.  A communicator carries that
 * all-reduce.  Three ways to make one:
 *   tmvb_comm_create_rccl      one process per GPU: rank 0 calls tmvb_comm_unique_id and hands the 128 bytes to the other
 *                              ranks by any host channel (MPI.jl / Distributed.jl / a file / torch.distributed); every
 *                              rank then calls this (ncclCommInitRank) -- RCCL over xGMI.
 *   tmvb_comm_create_rccl_all  one process, one host thread, n GPUs (ncclCommInitAll); the n communicators are used
 *                              together through the *_train_group entry points.
 *   tmvb_comm_create_host      a host-supplied all-reduce on HOST memory (MPI_Allreduce, gloo, ...): the library stages
 *                              the buffer through pinned memory.  For hosts without RCCL connectivity and for tests.
 * All collectives are enqueued on the context's stream. */
#define TMVB_UNIQUE_ID_BYTES 128
#define TMVB_F32 0
#define TMVB_F64 1
int tmvb_comm_unique_id(void* id_out /* TMVB_UNIQUE_ID_BYTES */);
int tmvb_comm_create_rccl(tmvb_ctx* ctx, const void* unique_id, int32_t nranks, int32_t rank, tmvb_comm** out);
int tmvb_comm_create_rccl_all(tmvb_ctx* const* ctxs, int32_t n, tmvb_comm** out /* [n] */);
/* sum-all-reduce `count` elements of `dtype` (TMVB_F32 / TMVB_F64) in place in host_buf across the ranks; 0 = success */
typedef int (*tmvb_host_allreduce_fn)(void* user, void* host_buf, int64_t count, int32_t dtype);
int tmvb_comm_create_host(tmvb_ctx* ctx, int32_t nranks, int32_t rank, tmvb_host_allreduce_fn fn, void* user, tmvb_comm** out);
int tmvb_comm_destroy(tmvb_comm* comm);
/* backend: 0 = RCCL, 1 = host callback */
int tmvb_comm_info(const tmvb_comm* comm, int32_t* nranks, int32_t* rank, int32_t* backend);
/* In-place sum-all-reduce of device memory on the communicator's context stream (asynchronous for RCCL). */
int tmvb_comm_allreduce(tmvb_comm* comm, void* dev_ptr, int64_t count, int32_t dtype);
/* RCCL version code linked into the library (ncclGetVersion), 0 when it cannot be queried. */
int tmvb_rccl_version(void);

/* ---- corpus upload: the corpus half of update_buffer! (src/modelutils.jl:370-388, :438-472) ----
 * doc_ptr[M+1], terms[nnz], counts[nnz]; rdr_ptr/readers/ratings may be NULL when U == 0.
 * Validates the check_doc / check_corp rules (src/Corpus.jl:41-50, :111-122): ids in range,
 * counts and ratings positive, offsets monotone.
 * PRESENTATION: inside a document the term (and reader) ids need be neither sorted nor unique, and documents and ids may come in
 * any order.  A repeated id ACCUMULATES: every model computes what it computes on the condensed document (unique ids, counts
 * summed; condense_corp!, src/Corpus.jl:523), up to the fp32 summation order -- the reference's CPU path differs there, it
 * overwrites (quirk Q1).  Per-entry outputs (tau) hold one value per ENTRY, equal for the repeats of an id; a
 * document's length (tmvb_corpus_info.max_doc_len, the kernel it runs on) is its number of entries.  One quantity is not additive
 * in a count: CTPF's ELBO holds -lgamma(count + 1) per entry, so splitting an entry shifts it by a constant of the corpus.
 * tests/test_corpus_presentations_gpu.py holds every model to this. */
int tmvb_corpus_create(tmvb_ctx* ctx, int64_t M, int64_t V, int64_t U,
                       const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts,
                       const int64_t* rdr_ptr, const int32_t* readers, const int32_t* ratings,
                       tmvb_corpus** out);
int tmvb_corpus_destroy(tmvb_corpus* corp);

typedef struct {
    int64_t M, V, U, nnz, nR;
    int64_t sum_counts, sum_ratings;
    int64_t max_doc_len, max_readers;
    int64_t n_empty_docs;
    int64_t n_docs_with_duplicate_terms;   /* quirk Q1 */
    int64_t n_docs_with_duplicate_readers;
} tmvb_corpus_info_t;
int tmvb_corpus_info(const tmvb_corpus* corp, tmvb_corpus_info_t* out);

/* ---- docfile ingest: the document part of readcorp (src/Corpus.jl:277-299) straight into the packed CSR ----
 * The reference's text format: one document = a block of 1 + counts + readers + ratings lines of `delim`-separated
 * positive integers (terms; then counts, readers, ratings as switched on).  Missing counts / ratings default to 1
 * (src/Corpus.jl:18-21).  Ids are converted to 0-based.  With condense != 0 equal term ids of a document are merged and
 * their counts added, terms sorted ascending (condense_corp!, src/Corpus.jl:523-531) -- the form the engine needs
 * (quirk Q1).  A block that does not parse fails with TMVB_ECORPUS and the reference's message
 * "document d beginning on line l failed to load." (:295).  The arrays are allocated by the library; release each
 * with tmvb_host_free.  V_seen / U_seen = 1 + the largest 0-based term / reader id read (0 if none). */
typedef struct {
    int64_t M, nnz, nR, V_seen, U_seen;
    int64_t* doc_ptr;  int32_t* terms;   int32_t* counts;     /* [M+1], [nnz], [nnz] */
    int64_t* rdr_ptr;  int32_t* readers; int32_t* ratings;    /* [M+1], [nR], [nR] */
} tmvb_docfile_t;
int tmvb_docfile_read(const char* path, char delim, int32_t counts, int32_t readers, int32_t ratings, int32_t condense,
                      tmvb_docfile_t* out);
void tmvb_docfile_free(tmvb_docfile_t* f);

/* ============================== LDA (src/gpuLDA.jl, oracle src/LDA.jl) ============================== */

/* gpuLDA(corp, K) (src/gpuLDA.jl:45-84).  State is initialised as the constructor does
 * (alpha=1, gamma=1, Elogtheta=psi(1)-psi(K)) except beta, which the reference draws from
 * Dirichlet(V,1) with Julia's RNG (:57): beta is uniform 1/V until tmvb_lda_set_state. */
int tmvb_lda_create(tmvb_ctx* ctx, tmvb_corpus* corp, int32_t K, tmvb_lda** out);
int tmvb_lda_destroy(tmvb_lda* h);

/* State half of update_buffer! (src/modelutils.jl:390-396) / the field copies of @gpu
 * (src/macros.jl:115-134).  NULL pointers leave the field unchanged; beta_old / Elogtheta_old
 * default to copies of beta / Elogtheta (they only feed the pre-training ELBO, src/macros.jl:126-132).
 * alpha[K], beta[K*V], gamma[K*M], Elogtheta[K*M]. */
int tmvb_lda_set_state(tmvb_lda* h, const double* alpha, const double* beta, const double* beta_old,
                       const double* gamma, const double* Elogtheta, const double* Elogtheta_old,
                       const double* elbo);
/* update_host! (src/modelutils.jl:501-516) without phi (never materialised).  NULL = skip. */
int tmvb_lda_get_state(tmvb_lda* h, double* alpha, double* beta, double* beta_old,
                       double* gamma, double* Elogtheta, double* Elogtheta_old, double* elbo);

/* update_phi! / update_gamma! / update_Elogtheta! sweeps + update_beta!(model, d) for every
 * document, with the CPU path's per-document early exit (src/LDA.jl:170-180; replaces the launches
 * at src/gpuLDA.jl:338-339, :294, :263-264, :202).  Accumulates the beta sufficient statistics
 * (the reference's beta_temp) on the device.  Asynchronous on the context's stream. */
int tmvb_lda_estep(tmvb_lda* h, int32_t viter, double vtol);

/* Packed sufficient statistics for the host's collective (new: the reference is single-device).
 * Layout: float32 [ S (K*V, column-major) | Elogtheta_sum (K) ]; *n_f32 = K*V + K.
 * tmvb_lda_reduce_docs must have run after the E-step for the tail to be valid.
 * A multi-process host all-reduces (sum) this buffer between tmvb_lda_reduce_docs and
 * tmvb_lda_update_beta; every rank then runs the identical M-step. */
int tmvb_lda_stats(tmvb_lda* h, void** dev_ptr, int64_t* n_f32);
/* Use caller-owned device memory (>= K*V+K floats) for the packed statistics. */
int tmvb_lda_bind_stats(tmvb_lda* h, void* dev_ptr, int64_t n_f32);
/* Elogtheta_sum = sum_d Elogtheta[:,d] (src/LDA.jl:98; replaces the kernel at src/gpuLDA.jl:264). */
int tmvb_lda_reduce_docs(tmvb_lda* h);
/* Document-sharded runs: M_total = corpus-wide document count used by update_alpha!;
 * distributed != 0 makes update_alpha! read Elogtheta_sum from the (all-reduced) statistics tail. */
int tmvb_lda_set_distributed(tmvb_lda* h, int64_t M_total, int32_t distributed);

/* update_beta!(model) (src/LDA.jl:121-125; replaces src/gpuLDA.jl:201-204): beta_old <- beta,
 * beta <- row-normalised statistics, statistics <- 0. */
int tmvb_lda_update_beta(tmvb_lda* h);
/* update_alpha! (src/LDA.jl:97-118; replaces the host fp32 loop at src/gpuLDA.jl:132-154):
 * fp64 Newton on the device. */
int tmvb_lda_update_alpha(tmvb_lda* h, int32_t niter, double ntol);
/* update_elbo! (src/LDA.jl:83-93) evaluated on the device from the current state; returns the sum
 * over this context's documents (a multi-process host adds the ranks' values) and stores it.  Right after
 * estep -> update_beta the corpus-level term E_q[log p(w)] = sum S .* log(beta + eps) comes from update_beta's statistics;
 * a document-sharded context (global S after the all-reduce) contributes the share M / M_total of it, so the ranks'
 * values still add up to the ELBO. */
int tmvb_lda_update_elbo(tmvb_lda* h, double* elbo);

/* train! (src/gpuLDA.jl:347-376 signature, src/LDA.jl:161-187 semantics incl. check_elbo!
 * src/modelutils.jl:574-585).  checkelbo <= 0 means Inf.  elbo_traj[iter] (may be NULL) receives the
 * ELBO per outer iteration (NaN where not evaluated); *elbo_baseline (may be NULL) the ELBO evaluated before the first
 * iteration (src/LDA.jl:167; the value the first printed delta refers to), or the stored model.elbo when it is not
 * evaluated.  With a communicator attached (tmvb_lda_set_comm) this is the document-sharded train!: every rank calls it
 * with the same arguments; one all-reduce of the packed statistics per iteration, and of the ELBO when it is checked,
 * so all ranks stop at the same iteration. */
int tmvb_lda_train(tmvb_lda* h, int32_t iter, double tol, int32_t niter, double ntol,
                   int32_t viter, double vtol, int32_t checkelbo,
                   double* elbo_traj, int32_t* iters_done, double* elbo_baseline);
/* Attach (comm != NULL) or detach a communicator: the handle's corpus is this rank's document shard of a corpus of
 * M_total documents.  Implies tmvb_lda_set_distributed.  The communicator is not owned by the handle. */
int tmvb_lda_set_comm(tmvb_lda* h, tmvb_comm* comm, int64_t M_total);

/* One rank's E-step, per-document sums and the sum-all-reduce of the packed statistics over the handle's communicator, in one
 * asynchronous call (the sharded train! uses it when the process drives one handle; a host that composes the iteration itself calls
 * it INSTEAD of tmvb_lda_estep + tmvb_lda_reduce_docs + tmvb_comm_allreduce, then tmvb_lda_update_beta / _alpha as before).
 * The collective of the multi-device precedent (v0.6/src/gpuLDA.jl:200-225: the host gathers every device's buffer after the
 * E-step) is issued in pieces, in the same order on every rank: (1) the Elogtheta_sum tail (K floats) on a side stream as soon as
 * the document kernels' column sums exist, i.e. under the statistics pass -- tmvb_lda_update_alpha then starts from that event
 * instead of after the whole buffer; (2) with TMVB_AR_SLICES = S > 1 (default 1) the last statistics pass runs in S vocabulary
 * slices and the slab of S a slice completes is all-reduced on the side stream while the next slice's pass runs; (3) the last
 * (or only) slab on the context's stream.  The first call on a communicator is collective beyond that: the ranks sum their
 * postings per term (V doubles) to agree on the cuts and the order.  Every rank must call it the same number of times.  Results are
 * identical on every rank, and equal to the three-call form's up to the fp32 summation order of the collective: bit for bit with one or two
 * ranks (tests/test_sliced_allreduce_gpu.py), while with three or more the ring / tree chunking of RCCL depends on a buffer's offset and length, so
 * the K-float tail and the slabs reduced as separate collectives may differ from ONE collective of K*V + K floats in the last bit.
 * OPT-IN since round 5: the library's sharded train! and bench.py issue the three-call form (one collective per iteration) unless
 * TMVB_FUSED_ALLREDUCE=1 -- two streams of collectives on one communicator have not run on multi-GPU hardware yet.  TMVB_EINVAL without a communicator. */
int tmvb_lda_estep_allreduce(tmvb_lda* h, int32_t viter, double vtol);

/* The slab plan tmvb_lda_estep_allreduce derives from the GLOBAL postings per term (host arithmetic only, no device: every rank
 * computes the same plan from the same all-reduced counts).  counts[V] >= 0; want >= 1 slabs asked for.  Out: *slices = S (<= want,
 * <= V, 1 if every count is zero), cuts[0..S] (slab s = term ids [cuts[s], cuts[s + 1]), cuts[0] = 0, cuts[S] = V; equal shares of
 * postings(v) / nnz + 1 / V), order[0..S) (the slabs in issue order: Johnson's rule for pass-then-wire).  The caller provides
 * want + 1 and want entries. */
int tmvb_allreduce_plan(const double* counts, int64_t V, int32_t want, int64_t* cuts, int32_t* order, int32_t* slices);
/* One host thread, n GPUs: hs[i] carries the i-th communicator of tmvb_comm_create_rccl_all (n = 1: same as
 * tmvb_lda_train).  The n all-reduces of an iteration are issued as one RCCL group. */
int tmvb_lda_train_group(tmvb_lda* const* hs, int32_t n, int32_t iter, double tol, int32_t niter, double ntol,
                         int32_t viter, double vtol, int32_t checkelbo,
                         double* elbo_traj, int32_t* iters_done, double* elbo_baseline);

/* Diagnostics: histogram of sweeps per document of the last E-step (hist[0..viter]), and the per-document counts
 * themselves (out[M], corpus document order, saturating at 255). */
int tmvb_lda_sweep_hist(tmvb_lda* h, int64_t* hist, int32_t nbins);
int tmvb_lda_doc_sweeps(tmvb_lda* h, uint8_t* out);
/* Which form the last tmvb_lda_update_elbo / check of tmvb_lda_train took (update_elbo!, src/LDA.jl:83-93): *form = 1 the decomposed form -- the
 * iteration's own statistics passes left sum_n c_n log s_n per postings chunk, update_beta! left sum S (log beta_new - log beta_old), and one
 * per-document kernel adds Elogptheta, sum_k (gamma_k - alpha_k)(Elogtheta_k - Elogtheta_old_k) and the Dirichlet entropy: no second walk over the
 * corpus; taken by every iteration tmvb_lda_train checks (K <= 124: the statistics pass recomputes the token weights up to KP = 124; viter > 0) and, with TMVB_LDA_ELBO_PARTS=2 at tmvb_lda_create, by the stepwise operators too;
 * *form = 0 the token walk (phi rebuilt from beta_old / Elogtheta_old per token: any state, e.g. right after tmvb_lda_set_state);
 * TMVB_LDA_ELBO_PARTS=0 forces it.  Both evaluate the same sum; they differ by fp32 rounding only (tests/test_lda_elbo_parts_gpu.py). */
int tmvb_lda_elbo_form(tmvb_lda* h, int32_t* form);
/* Number of kernel launches one tmvb_lda_estep issues (one per document-length bucket). */
int tmvb_lda_estep_launches(tmvb_lda* h, int32_t* n);
/* Number of document pieces tmvb_lda_estep runs its statistics passes in, as fixed at tmvb_lda_create (1: one pass over the corpus' own index;
 * TMVB_LDA_PIECES overrides the size rule). */
int tmvb_lda_estep_pieces(tmvb_lda* h, int32_t* pieces);
/* Timing of the last tmvb_lda_estep on the context's stream, from HIP events (ms). */
int tmvb_lda_last_estep_ms(tmvb_lda* h, float* ms);

/* ============================== fLDA (new device path; oracle src/fLDA.jl) ==============================
 * Filtered LDA: LDA plus a per-token Bernoulli switch tau_n (prior eta) and a background distribution kappa.  The reference
 * has NO accelerator path for it (`@gpu train!` on an fLDA does nothing, src/macros.jl:274-278); SURVEY.md section 8 f4 names
 * it as the next row.  The entry points mirror the LDA ones; the per-document operator chain update_phi! / update_tau! /
 * update_gamma! / update_Elogtheta! (src/fLDA.jl:188, :180, :173, :166) is one fused kernel.  K <= 1024 (1, 2, 4, 8 or 16 topic slots per lane, as LDA).
 * tau / tau_old are flat double[nnz] arrays in the CSR token order of tmvb_corpus_create (= vcat(model.tau...)). */
int tmvb_flda_create(tmvb_ctx* ctx, tmvb_corpus* corp, int32_t K, tmvb_flda** out);           /* fLDA(corp, K), src/fLDA.jl:28-60 */
int tmvb_flda_destroy(tmvb_flda* h);
/* NULL = unchanged; kappa_old / beta_old / Elogtheta_old / tau_old default to the current values.  eta[1], alpha[K], kappa[V],
 * beta[K*V], gamma[K*M], Elogtheta[K*M], tau[nnz]. */
int tmvb_flda_set_state(tmvb_flda* h, const double* eta, const double* alpha, const double* kappa, const double* kappa_old,
                        const double* beta, const double* beta_old, const double* gamma, const double* Elogtheta,
                        const double* Elogtheta_old, const double* tau, const double* tau_old, const double* elbo);
int tmvb_flda_get_state(tmvb_flda* h, double* eta, double* alpha, double* kappa, double* kappa_old, double* beta, double* beta_old,
                        double* gamma, double* Elogtheta, double* Elogtheta_old, double* tau, double* tau_old, double* elbo);
/* sweeps of src/fLDA.jl:224-233 + update_beta!(model, d) (:159) + update_kappa!(model, d) (:145) for every document */
int tmvb_flda_estep(tmvb_flda* h, int32_t viter, double vtol);
int tmvb_flda_reduce_docs(tmvb_flda* h);                                /* Elogtheta_sum, src/fLDA.jl:129 */
/* Packed statistics: float32 [ S (K*V) | kappa_stats (V) | Elogtheta_sum (K) ]. */
int tmvb_flda_stats(tmvb_flda* h, void** dev_ptr, int64_t* n_f32);
int tmvb_flda_update_beta(tmvb_flda* h);                                /* update_beta! (:152) and update_kappa! (:138) */
int tmvb_flda_update_alpha(tmvb_flda* h, int32_t niter, double ntol);   /* update_alpha! (:128-150) */
int tmvb_flda_update_eta(tmvb_flda* h);                                 /* update_eta! (:122-124); after update_beta */
int tmvb_flda_update_elbo(tmvb_flda* h, double* elbo);                  /* update_elbo! (:108-118) */
/* train! (src/fLDA.jl:213-247); arguments as tmvb_lda_train. */
int tmvb_flda_train(tmvb_flda* h, int32_t iter, double tol, int32_t niter, double ntol, int32_t viter, double vtol,
                    int32_t checkelbo, double* elbo_traj, int32_t* iters_done, double* elbo_baseline);
/* Document-sharded run: the shard belongs to a corpus of M_total documents and C_total tokens (sum of all counts). */
int tmvb_flda_set_comm(tmvb_flda* h, tmvb_comm* comm, int64_t M_total, int64_t C_total);
int tmvb_flda_train_group(tmvb_flda* const* hs, int32_t n, int32_t iter, double tol, int32_t niter, double ntol, int32_t viter,
                          double vtol, int32_t checkelbo, double* elbo_traj, int32_t* iters_done, double* elbo_baseline);
int tmvb_flda_doc_sweeps(tmvb_flda* h, uint8_t* out);
/* As tmvb_lda_elbo_form (update_elbo!, src/fLDA.jl:108-118): *form = 1 if the last tmvb_flda_update_elbo / check of tmvb_flda_train took the decomposed
 * form -- the checked iteration's document kernel left per token the log-sum-exp of its last phi column and the exponent update_tau! forms
 * (sum_i phi_in log(beta_old + eps), :184), update_beta! left sum S (log(beta_new + eps) - log(beta_old + eps)), and one elementwise pass per document adds
 * c_n [lse_n + (tau_n - tau_old_n) A_n + (1 - tau_n) log(kappa + eps) + H(tau_n)], sum_i (gamma_i - alpha_i)(Elogtheta_i - Elogtheta_old_i), the Dirichlet
 * terms and Elogpc: no phi is rebuilt; *form = 0 the token walk (any state, e.g. after tmvb_flda_set_state).  TMVB_FLDA_ELBO_PARTS at tmvb_flda_create:
 * 0 never, 1 (default) the iterations tmvb_flda_train checks, 2 every E-step collects (the stepwise operators take the form too).  viter > 0. */
int tmvb_flda_elbo_form(tmvb_flda* h, int32_t* form);
int tmvb_flda_last_estep_ms(tmvb_flda* h, float* ms);

/* ============================== CTM (src/gpuCTM.jl, oracle src/CTM.jl) ============================== */

/* gpuCTM(corp, K) (src/gpuCTM.jl:45-98).  Constructor state as src/CTM.jl:37-48 (mu=0, sigma=invsigma=I,
 * lambda=0, vsq=1, logzeta=0.5); beta is uniform until tmvb_ctm_set_state (the reference draws it with
 * Julia's RNG).  K <= 256 (CTM_MAX_K; beyond it the Julia shim trains on the reference's CPU model behind a warning).  E-step kernels behind
 * tmvb_ctm_estep: K <= 52 -- one LANE per
 * document, invsigma streamed through scalar registers, the lambda Newton systems solved by Jacobi-preconditioned CG to
 * max(1e-4 |g|, 5 % of ntol); its documents of more than 2048 unique terms (and everything under TMVB_CTM_BATCH=0) -- one wave
 * per document, Gauss-Jordan in registers (lane = matrix row); 52 < K <= 128 -- one wave per document, lane = matrix row (two
 * topic slots per lane beyond 64), the same CG against one copy of invsigma in LDS per workgroup (TMVB_CTM_GENERIC_CG=0: round 1's
 * Gauss-Jordan through LDS, 30 times slower at K = 100); 128 < K <= 256 -- four topic slots per lane, invsigma read from global memory by
 * columns (L2-resident), the whole LDS for the tile windows, update_sigma!'s fp64 inversion in a global workspace, dense E rows and the
 * scalar statistics kernel beyond KP / 4 = 64 chunks (K > 252).  fCTM: the same limits. */
int tmvb_ctm_create(tmvb_ctx* ctx, tmvb_corpus* corp, int32_t K, tmvb_ctm** out);
int tmvb_ctm_destroy(tmvb_ctm* h);

/* update_buffer! state half (src/modelutils.jl:420-431) / @gpu field copies (src/macros.jl:152-175).
 * mu[K], sigma[K*K], invsigma[K*K], beta[K*V], lambda[K*M], vsq[K*M], logzeta[M]; NULL = unchanged;
 * beta_old / lambda_old default to beta / lambda. */
int tmvb_ctm_set_state(tmvb_ctm* h, const double* mu, const double* sigma, const double* invsigma,
                       const double* beta, const double* beta_old, const double* lambda,
                       const double* lambda_old, const double* vsq, const double* logzeta, const double* elbo);
/* update_host! (src/modelutils.jl:519-537) without phi. */
int tmvb_ctm_get_state(tmvb_ctm* h, double* mu, double* sigma, double* invsigma, double* beta, double* beta_old,
                       double* lambda, double* lambda_old, double* vsq, double* logzeta, double* elbo);

/* update_phi! / update_logzeta! / update_vsq! / update_lambda! sweeps + update_beta!(model, d) for every
 * document with the CPU path's semantics (src/CTM.jl:194-205; replaces the launches at
 * src/gpuCTM.jl:478-479, :425, :390, :342, :254).  Asynchronous on the context's stream. */
int tmvb_ctm_estep(tmvb_ctm* h, int32_t niter, double ntol, int32_t viter, double vtol);
/* sum_d lambda_d, sum_d vsq_d and the scatter matrix sum_d (lambda_d - mu)(lambda_d - mu)^T (f32 MFMA) with
 * the current (= previous-iteration) mu, into the statistics tail.  tmvb_ctm_estep already computes them on a side
 * stream under its statistics pass; the call then only acknowledges that result (it recomputes on the context's stream
 * when lambda / vsq / mu were changed through the API since, or when no E-step came before). */
int tmvb_ctm_reduce_docs(tmvb_ctm* h);
/* Packed statistics for the host's all-reduce: float32 [ S (K*V) | sum_lambda (K) | sum_vsq (K) | scatter (K*K) ]. */
int tmvb_ctm_stats(tmvb_ctm* h, void** dev_ptr, int64_t* n_f32);
int tmvb_ctm_bind_stats(tmvb_ctm* h, void* dev_ptr, int64_t n_f32);
int tmvb_ctm_set_distributed(tmvb_ctm* h, int64_t M_total, int32_t distributed);
/* update_beta! (src/CTM.jl:114-118; replaces src/gpuCTM.jl:253-256). */
int tmvb_ctm_update_beta(tmvb_ctm* h);
/* update_sigma! (src/CTM.jl:108-111; replaces src/gpuCTM.jl:200-206 incl. the host `inv`): uses the
 * PREVIOUS mu (call before tmvb_ctm_update_mu, as train! does, src/CTM.jl:207-208). */
int tmvb_ctm_update_sigma(tmvb_ctm* h);
/* update_mu! (src/CTM.jl:102-104; replaces src/gpuCTM.jl:166-168). */
int tmvb_ctm_update_mu(tmvb_ctm* h);
/* update_elbo! (src/CTM.jl:89-98) on the device; sum over this context's documents. */
int tmvb_ctm_update_elbo(tmvb_ctm* h, double* elbo);
/* As tmvb_lda_elbo_form: *form = 1 if the last tmvb_ctm_update_elbo took the decomposed form (the checked iteration's E-step kernels left
 * sum_i (phi counts)_i (lambda_i - lambda_old_i) per document, its statistics pass sum_n c_n log s_n per postings chunk, update_beta!
 * sum S (log(beta_new + eps) - log beta_old): no token loop), 0 for the token walk (any state).  Every iteration tmvb_ctm_train checks takes
 * it (K <= 124, viter > 0); TMVB_CTM_ELBO_PARTS=2 at tmvb_ctm_create: the stepwise operators too, =0: never. */
int tmvb_ctm_elbo_form(tmvb_ctm* h, int32_t* form);
/* train! (src/gpuCTM.jl:487-519 signature, src/CTM.jl:185-213 semantics); elbo_baseline / communicator as for LDA. */
int tmvb_ctm_train(tmvb_ctm* h, int32_t iter, double tol, int32_t niter, double ntol,
                   int32_t viter, double vtol, int32_t checkelbo, double* elbo_traj, int32_t* iters_done,
                   double* elbo_baseline);
int tmvb_ctm_set_comm(tmvb_ctm* h, tmvb_comm* comm, int64_t M_total);
int tmvb_ctm_train_group(tmvb_ctm* const* hs, int32_t n, int32_t iter, double tol, int32_t niter, double ntol,
                         int32_t viter, double vtol, int32_t checkelbo, double* elbo_traj, int32_t* iters_done,
                         double* elbo_baseline);
/* Diagnostics of the last E-step: sweeps-per-document histogram and total lambda-Newton steps. */
int tmvb_ctm_sweep_hist(tmvb_ctm* h, int64_t* hist, int32_t nbins, int64_t* newton_steps);
int tmvb_ctm_doc_sweeps(tmvb_ctm* h, uint8_t* out);
int tmvb_ctm_last_estep_ms(tmvb_ctm* h, float* ms);
/* Diagnostics of the last E-step when the lane-per-document kernel ran (K <= 52, csrc/tmvb_ctm_batch.h), 12 values: out[0]
 * conjugate-gradient trips, [1] Newton trips, [2] waves (summed over waves); with TMVB_CTM_PROF=1 in the environment also
 * [3..10] shader cycles per phase (token, logzeta, vsq, gradient assembly, CG, gradient mat-vec, lambda update, spare) and
 * [11] whole-kernel cycles.  Zeros otherwise. */
int tmvb_ctm_solver_stats(tmvb_ctm* h, int64_t* out12);

/* ============================== fCTM (new device path; oracle src/fCTM.jl) ==============================
 * Filtered CTM: CTM plus the per-token switch tau_n (prior eta) and the background distribution kappa of fLDA.  No accelerator
 * path in the reference (src/macros.jl:274-278).  Same Newton machinery and K limits as CTM; the per-document chain is
 * update_phi! / update_tau! / update_logzeta! / update_lambda! / update_vsq! (src/fCTM.jl:236-241 -- lambda BEFORE vsq, unlike CTM).
 * eta is a fixed parameter (update_eta! is commented out of train!, src/fCTM.jl:253). */
int tmvb_fctm_create(tmvb_ctx* ctx, tmvb_corpus* corp, int32_t K, tmvb_fctm** out);           /* fCTM(corp, K), src/fCTM.jl:32-65 */
int tmvb_fctm_destroy(tmvb_fctm* h);
/* eta[1], mu[K], sigma/invsigma[K*K], kappa[V], beta[K*V], lambda/vsq[K*M], logzeta[M], tau[nnz] (CSR token order); NULL = unchanged;
 * the *_old arguments default to the current values. */
int tmvb_fctm_set_state(tmvb_fctm* h, const double* eta, const double* mu, const double* sigma, const double* invsigma,
                        const double* kappa, const double* kappa_old, const double* beta, const double* beta_old,
                        const double* lambda, const double* lambda_old, const double* vsq, const double* logzeta,
                        const double* tau, const double* tau_old, const double* elbo);
int tmvb_fctm_get_state(tmvb_fctm* h, double* eta, double* mu, double* sigma, double* invsigma, double* kappa, double* kappa_old,
                        double* beta, double* beta_old, double* lambda, double* lambda_old, double* vsq, double* logzeta,
                        double* tau, double* tau_old, double* elbo);
/* sweeps of src/fCTM.jl:233-248 + update_beta!(model, d) (:155) + update_kappa!(model, d) (:141) for every document.
 * Packed statistics: float32 [ S (K*V) | sum_lambda (K) | sum_vsq (K) | scatter (K*K) | kappa_stats (V) ]. */
int tmvb_fctm_estep(tmvb_fctm* h, int32_t niter, double ntol, int32_t viter, double vtol);
int tmvb_fctm_reduce_docs(tmvb_fctm* h);
int tmvb_fctm_update_beta(tmvb_fctm* h);                                /* update_beta! (:148) and update_kappa! (:134) */
int tmvb_fctm_update_sigma(tmvb_fctm* h);                               /* update_sigma! (:128-131), previous mu */
int tmvb_fctm_update_mu(tmvb_fctm* h);                                  /* update_mu! (:122-124) */
int tmvb_fctm_update_elbo(tmvb_fctm* h, double* elbo);                  /* update_elbo! (:105-115) */
/* train! (src/fCTM.jl:226-262); arguments as tmvb_ctm_train. */
int tmvb_fctm_train(tmvb_fctm* h, int32_t iter, double tol, int32_t niter, double ntol, int32_t viter, double vtol,
                    int32_t checkelbo, double* elbo_traj, int32_t* iters_done, double* elbo_baseline);
int tmvb_fctm_set_comm(tmvb_fctm* h, tmvb_comm* comm, int64_t M_total);
int tmvb_fctm_train_group(tmvb_fctm* const* hs, int32_t n, int32_t iter, double tol, int32_t niter, double ntol, int32_t viter,
                          double vtol, int32_t checkelbo, double* elbo_traj, int32_t* iters_done, double* elbo_baseline);
int tmvb_fctm_sweep_hist(tmvb_fctm* h, int64_t* hist, int32_t nbins, int64_t* newton_steps);
int tmvb_fctm_doc_sweeps(tmvb_fctm* h, uint8_t* out);
/* As tmvb_ctm_solver_stats, for the filtered model's E-step (zeros when the wave-per-document kernels ran). */
int tmvb_fctm_solver_stats(tmvb_fctm* h, int64_t* out12);
/* As tmvb_flda_elbo_form for update_elbo! of src/fCTM.jl:105-115 (lambda for Elogtheta: the E-step kernels' exit test leaves
 * sum_i (phi counts)_i (lambda_i - lambda_old_i) per document); TMVB_FCTM_ELBO_PARTS at tmvb_fctm_create. */
int tmvb_fctm_elbo_form(tmvb_fctm* h, int32_t* form);

/* ============================== CTPF (src/gpuCTPF.jl, oracle src/CTPF.jl) ============================== */

/* gpuCTPF(corp, K) (src/gpuCTPF.jl:68-152).  Constructor state as src/CTPF.jl:81-100 (he=1, rates=1, gimel=zayin=1,
 * hyper-parameters a..h = 0.1); alef is 1 until tmvb_ctpf_set_state (the reference draws it with Julia's RNG, :83).
 * K <= 512: the grid-tile fast path (one topic slot per lane of a 16 x 4 lane grid) covers K <= 60; beyond it one wave per document with
 * 2 / 4 / 8 topic slots per lane (lane l owns topics l, l + 64, ...: K <= 128 / 256 / 512), rows of more than 64 chunks through dense E rows
 * and the scalar statistics kernel. */
int tmvb_ctpf_create(tmvb_ctx* ctx, tmvb_corpus* corp, int32_t K, tmvb_ctpf** out);
int tmvb_ctpf_destroy(tmvb_ctpf* h);
/* update_buffer! state half (src/modelutils.jl:474-493).  hyper[8] = a..h; alef[K*V], he[K*U], bet/vav/dalet/het[K],
 * gimel/zayin[K*M]; NULL = unchanged.  The *_old copies are set equal to the new values. */
int tmvb_ctpf_set_state(tmvb_ctpf* h, const double* hyper, const double* alef, const double* he, const double* bet,
                        const double* vav, const double* dalet, const double* het, const double* gimel,
                        const double* zayin, const double* elbo);
/* The *_old fields of update_buffer! (src/modelutils.jl:474-493): update_elbo! rebuilds phi / xi from them
 * (src/CTPF.jl:239-240) and @gpu copies them (src/macros.jl:229-260), so a trained model that is uploaded again must
 * bring them along or its baseline ELBO differs.  Call after tmvb_ctpf_set_state; NULL = leave unchanged. */
int tmvb_ctpf_set_state_old(tmvb_ctpf* h, const double* alef_old, const double* he_old, const double* bet_old,
                            const double* vav_old, const double* dalet_old, const double* het_old,
                            const double* gimel_old, const double* zayin_old);
/* update_host! (src/modelutils.jl:539-570) without phi / xi.  rates[8*K] = bet, vav, dalet, het, then their *_old. */
int tmvb_ctpf_get_state(tmvb_ctpf* h, double* alef, double* alef_old, double* he, double* he_old, double* rates,
                        double* gimel, double* gimel_old, double* zayin, double* zayin_old, double* elbo);
/* update_xi! / update_phi! / update_zayin! / update_gimel! sweeps + update_he!(d) / update_alef!(d) for every
 * document, CPU-path semantics (src/CTPF.jl:353-365; replaces src/gpuCTPF.jl:667-668, :599-600, :511, :382, :448, :315). */
int tmvb_ctpf_estep(tmvb_ctpf* h, int32_t viter, double vtol);
/* sum_d gimel_d, sum_d zayin_d into the statistics tail. */
int tmvb_ctpf_reduce_docs(tmvb_ctpf* h);
/* Packed statistics: float32 [ alef_stats (K*V) | he_stats (K*U) | sum_gimel (K) | sum_zayin (K) ] (priors NOT included). */
int tmvb_ctpf_stats(tmvb_ctpf* h, void** dev_ptr, int64_t* n_f32);
int tmvb_ctpf_bind_stats(tmvb_ctpf* h, void* dev_ptr, int64_t n_f32);
int tmvb_ctpf_set_distributed(tmvb_ctpf* h, int32_t distributed);
/* update_he!, update_alef!, update_dalet!, update_het!, update_bet!, update_vav! in that order
 * (src/CTPF.jl:366-371; replaces src/gpuCTPF.jl:448, :315, :418, :539, :344, :482). */
int tmvb_ctpf_mstep(tmvb_ctpf* h);
/* update_elbo! (src/CTPF.jl:234-247) on the device.  The Binomial sums of Elogpya/Elogpyb/Elogpz and of the Multinomial
 * entropies cancel identically in :243 and are not evaluated.  _parts returns the per-document part (sum over this
 * context's documents) and the global (beta, eta) part separately for document-sharded hosts. */
int tmvb_ctpf_update_elbo(tmvb_ctpf* h, double* elbo);
/* As tmvb_lda_elbo_form: *form = 1 if the last update_elbo! took the decomposed form -- no entry (token / reader) is walked: the checked iteration's document
 * kernels left their softmax shifts, its statistics passes sum_n c_n log s_n per postings chunk, and the entries' remaining terms are sums the M-step already
 * has (sum (alef - a)(psi(alef) - psi(alef_old)), the row sums of alef, sum_d gimel_d); *form = 0 the table form (any state).  Every iteration tmvb_ctpf_train
 * checks on an unsharded handle takes it (K <= 124, viter > 0); TMVB_CTPF_ELBO_PARTS=2 at tmvb_ctpf_create: the stepwise operators too, =0: never. */
int tmvb_ctpf_elbo_form(tmvb_ctpf* h, int32_t* form);
int tmvb_ctpf_update_elbo_parts(tmvb_ctpf* h, double* doc_part, double* global_part);
/* train! (src/gpuCTPF.jl:677-705 signature, src/CTPF.jl:344-376 semantics).  checkelbo <= 0 means Inf.
 * elbo_baseline / communicator as for LDA (the per-document ELBO part is all-reduced, the global part added once). */
int tmvb_ctpf_train(tmvb_ctpf* h, int32_t iter, double tol, int32_t viter, double vtol, int32_t checkelbo,
                    double* elbo_traj, int32_t* iters_done, double* elbo_baseline);
int tmvb_ctpf_set_comm(tmvb_ctpf* h, tmvb_comm* comm);
int tmvb_ctpf_train_group(tmvb_ctpf* const* hs, int32_t n, int32_t iter, double tol, int32_t viter, double vtol,
                          int32_t checkelbo, double* elbo_traj, int32_t* iters_done, double* elbo_baseline);
int tmvb_ctpf_sweep_hist(tmvb_ctpf* h, int64_t* hist, int32_t nbins);
int tmvb_ctpf_doc_sweeps(tmvb_ctpf* h, uint8_t* out);
int tmvb_ctpf_last_estep_ms(tmvb_ctpf* h, float* ms);
/* Recommendation post-processing at the end of train!(model::CTPF) (src/CTPF.jl:379-399; src/gpuCTPF.jl:711-731 runs the
 * same code on the host).  From the resident state:
 *   scores (or NULL)  double[M*U], column-major M x U as model.scores: sum_k he[k,u]/vav[k] (gimel[k,d]/dalet[k] + zayin[k,d]/het[k])
 *   drecs  (or NULL)  int32[M*U]: row d holds the 0-based users that are not readers of document d, by descending
 *                     score, equal scores in descending index order (= reverse(sortperm(...))); drec_count[d] entries valid
 *   urecs             int32[U*M]: row u holds the 0-based documents outside user u's library, same order; urec_count[u] valid
 * drecs/urecs/drec_count/urec_count are given together or all NULL.  ms_scores / ms_rank (or NULL): device time of the
 * score pass and of the two segmented sorts. */
int tmvb_ctpf_recommend(tmvb_ctpf* h, double* scores, int32_t* drecs, int32_t* drec_count, int32_t* urecs,
                        int32_t* urec_count, float* ms_scores, float* ms_rank);

/* ============================== gendoc / gencorp (src/modelutils.jl:594-649) ==============================
 * A model run as a generative process, on the device: for document d of M, C_d ~ Poisson(mean_C) (the caller passes mean(model.C), :597),
 * theta_d ~ Dirichlet(alpha) (LDA / gpuLDA / fLDA, :598) or additive_logistic(N(mu, sigma)) (CTM / gpuCTM / fCTM, :619; src/utils.jl:125-130),
 * then C_d tokens z ~ Cat(theta_d), w ~ Cat((beta[z,:] + laplace_smooth) / (1 + laplace_smooth V)) (:601-607).  The reference's CTM method
 * draws from `topicdist` at :626, a typo for `topic_dist` that throws as written: the intent is implemented.  The reference returns a Dict's
 * keys / values (unique terms, arbitrary order, :610); here each document is its unique 0-based term ids SORTED ASCENDING with summed counts,
 * the condensed CSR of tmvb_corpus_create.  A document with C_d = 0 is empty (doc_ptr[d + 1] == doc_ptr[d]).  With laplace_smooth = 0 a
 * term whose beta entry is exactly zero is never drawn.  The filtered models' kappa / tau take no part (the reference's gendoc ignores them).
 * Every random number is Philox4x32-10 of (seed, doc_offset + d, stage, draw index): the same seed gives the same bytes, documents
 * [d0, d0 + m) of a large call equal the call (M = m, doc_offset = d0) -- gendoc is M = 1, and shards of a corpus can be generated apart.
 * alpha[K] / mu[K], sigma[K*K] (column-major, symmetric; factored on the host in fp64), beta[K*V] column-major, all on the HOST.
 * flags & 1: also return the diagnostics.  Errors: M <= 0 ("corp_size parameter must be a positive integer.", :643), laplace_smooth < 0
 * ("laplace_smooth parameter must be nonnegative.", :595 / :644), mean_C <= 0 or not finite, K outside [1, 1024] (LDA) / [1, 256] (CTM), or
 * more than 2^26 - 1 documents or
 * 2^31 or more tokens in one call (generate in shards through doc_offset) -> TMVB_EINVAL; beta not right stochastic, alpha not positive, mu not finite, sigma not positive-definite
 * -> TMVB_ESHAPE with check_model's wording (src/modelutils.jl:47, :56, :114, :116); arguments are judged before the device, then ctx == NULL
 * without a visible device -> TMVB_ENODEVICE (there is no CPU path).  The arrays of *out are allocated by the library: tmvb_gencorp_free. */
typedef struct {
    int64_t M, nnz, sum_counts;
    int64_t* doc_ptr; int32_t* terms; int32_t* counts;   /* [M+1], [nnz], [nnz] */
    /* diagnostics, filled only when requested (flags & 1), else NULL */
    float*   log_theta;    /* [M][K]  log theta_d as drawn */
    int32_t* doc_topic;    /* [M][K]  tokens of document d assigned to topic k */
    int64_t* topic_term;   /* [K][V]  tokens drawn as (topic k, term v), before condensing */
    float    ms_tables, ms_docs, ms_tokens, ms_condense;  /* device time per stage: HIP events around the stage's kernels and library sort / scan calls only */
} tmvb_gencorp_t;
int  tmvb_lda_gencorp(tmvb_ctx* ctx, int32_t K, int64_t V, const double* alpha, const double* beta, int64_t M, int64_t doc_offset,
                      double mean_C, double laplace_smooth, int64_t seed, int32_t flags, tmvb_gencorp_t* out);
int  tmvb_ctm_gencorp(tmvb_ctx* ctx, int32_t K, int64_t V, const double* mu, const double* sigma, const double* beta, int64_t M,
                      int64_t doc_offset, double mean_C, double laplace_smooth, int64_t seed, int32_t flags, tmvb_gencorp_t* out);
void tmvb_gencorp_free(tmvb_gencorp_t* g);
/* Diagnostics: one block of the generator behind gencorp (Philox4x32-10; Salmon et al., SC'11), on the host: counter[4], key[2] -> out[4]. */
int  tmvb_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out);

/* ============================== held-out evaluation: token split, predictive log-likelihood ==============================
 * Document completion (the reference has no such function): split the tokens of unseen documents into an
 * observed and a held-out part, fold the observed part in with predict, score the held-out part under the predicted topic proportions.
 *
 * tmvb_corpus_split: the host CSR of tmvb_corpus_create (doc_ptr[M+1], terms[nnz], counts[nnz]) -> two host CSRs over the same M and V.
 * Draw rule: the token occurrences of document d are numbered t = 0 .. C_d - 1 in CSR order (entry j's counts[j] occurrences are
 * consecutive); the 32-bit word of occurrence t is x[t & 3] of Philox4x32-10 with key = seed and counter = (doc_offset + d, stage
 * TMVB_RNG_SPLIT = 5, draw t >> 2) (csrc/tmvb_philox.h: tmvb_rng); occurrence t is HELD OUT iff word < floor(frac * 2^32) (as 64-bit
 * integers: frac = 0 holds out nothing, frac = 1 everything).  Entries whose count became 0 are dropped, the order of terms inside a
 * document is kept, a document may be empty on either side, obs + held reproduces the input exactly, and documents [d0, d0 + m) of a
 * large call equal the call (M = m, doc_offset = d0).  Errors, judged before the device is touched: frac outside [0, 1] or not finite,
 * M <= 0, V <= 0, doc_offset < 0, NULL argument, 2^31 - 1 or more entries, a document of 2^31 or more tokens -> TMVB_EINVAL; doc_ptr
 * not non-decreasing from 0, a term outside [0, V), a count < 1 -> TMVB_ESHAPE; then ctx == NULL without a visible device ->
 * TMVB_ENODEVICE.  The arrays of *out are allocated by the library: tmvb_split_free.  ms_draw / ms_compact: device time of the draw
 * (scan of the counts + draw kernel) and of the compaction (flags, two scans, scatter), HIP events around kernels and scans only. */
typedef struct {
    int64_t M, nnz_obs, nnz_held, sum_obs, sum_held;
    int64_t* obs_ptr;  int32_t* obs_terms;  int32_t* obs_counts;     /* [M+1], [nnz_obs], [nnz_obs] */
    int64_t* held_ptr; int32_t* held_terms; int32_t* held_counts;    /* [M+1], [nnz_held], [nnz_held] */
    float    ms_draw, ms_compact;
} tmvb_split_t;
int  tmvb_corpus_split(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts,
                       double frac, int64_t seed, int64_t doc_offset, tmvb_split_t* out);
void tmvb_split_free(tmvb_split_t* s);

/* tmvb_heldout_loglik: ll[d] = sum_n c_n log( sum_k theta[k,d] beta'[k,w_n] ) over the entries (w_n, c_n) of document d of the host CSR,
 * beta' = (beta + laplace_smooth) / (1 + laplace_smooth V) (gendoc's smoothing, src/modelutils.jl:601-607); tokens[d] = sum_n c_n; an
 * empty document has ll = 0.  An entry whose mixture probability is exactly 0 makes ll[d] = -inf and adds its count to
 * *zero_prob_tokens; no epsilon is added.  theta[K*M] and beta[K*V] are column-major fp64 on the HOST; the device holds both in fp32
 * (beta' in the gather layout [V][KP], KP = 4 * odd >= K), the dot products are fp32 FMAs, the logarithm and the per-document sum fp64.
 * No atomics: two calls give the same bits.  Errors: K outside [1, 1024], laplace_smooth < 0 or not finite, M <= 0, V <= 0, NULL
 * argument, 2^31 - 1 or more entries -> TMVB_EINVAL; bad CSR (as above), beta not right stochastic ("beta must be a right stochastic
 * matrix.", check_model's wording), a theta column with a negative or non-finite entry or a sum further than 1e-6 from 1 -> TMVB_ESHAPE;
 * arguments are judged before the device, then ctx == NULL without a visible device -> TMVB_ENODEVICE.  ms_kernel (or NULL): device
 * time of the scoring kernels. */
int tmvb_heldout_loglik(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t M, const double* theta, const double* beta, const int64_t* doc_ptr,
                        const int32_t* terms, const int32_t* counts, double laplace_smooth, double* ll, int64_t* tokens,
                        int64_t* zero_prob_tokens, float* ms_kernel);

/* ============================== topic coherence: co-document counts, UMass, NPMI ==============================
 * Whether the top words of a topic occur together in documents (the reference has no such function).  Inputs: a reference corpus as the
 * host CSR of tmvb_corpus_create (doc_ptr[M+1], terms[nnz], counts[nnz]) and top[K][N], row-major: for each topic its N top term ids,
 * 0-based, in descending order of probability.  Only presence matters: document d CONTAINS term w iff any of its entries has term w; ids
 * inside a document need be neither sorted nor unique, a repeated id counts the document once, counts are validated (>= 1) and otherwise
 * ignored.
 *
 * tmvb_corpus_codocfreq: codf[K][N][N] (int64, row-major), codf[k][i][j] = number of documents that contain both top[k][i] and
 * top[k][j]; symmetric; the diagonal is the document frequency df[k][i].  These integers are the whole device result, exact and the
 * same bits on every call.  They are ADDITIVE over document shards: the codf of documents [0, m) plus the codf of [m, M) is the codf of
 * the corpus, so a multi-rank host calls this on its shard, sums the integers by any means and scores once.
 * Device path: the distinct ids of top (T <= K N) get slots; a bit matrix bits[T][W], W = ceil(M / 64) 64-bit words (bit d of row s set
 * iff document d contains the term of slot s), is built with one atomic OR per selected CSR entry; the pair pass takes
 * popcount(row_i & row_j) over chunks of TMVB_CODF_CHUNK_DOCS documents.  If T W 8 bytes exceed max_bitset_bytes (0 = the library's
 * default, TMVB_CODF_DEFAULT_BITSET_BYTES = 1 GiB) the topics are processed in batches of consecutive topics whose distinct ids fit, each
 * with its own build pass over the CSR; a single topic that does not fit (N W 8 bytes) is TMVB_EINVAL with the needed bytes in the
 * message.  (The budget counts T W 8; the allocation rounds W up to an even number of words so that rows are 16-byte aligned.)
 * info (or NULL): n_slots = T, n_batches, ms_bitset / ms_pairs = device time of the two kernels summed over the batches (HIP events
 * around the kernels only).
 * Errors, judged before the device is touched: K outside [1, 1024], N outside [2, 64] or N > V, M <= 0, V <= 0, NULL argument,
 * 2^31 - 1 or more entries, max_bitset_bytes < 0 -> TMVB_EINVAL; doc_ptr not non-decreasing from 0, a term outside [0, V), a count < 1,
 * an id of top outside [0, V), an id repeated inside one row of top -> TMVB_ESHAPE; then ctx == NULL without a visible device ->
 * TMVB_ENODEVICE (there is no CPU path).
 *
 * tmvb_coherence_from_counts: host only, touches no device; fp64 arithmetic on the integers.  Per topic, over the pairs i > j (j is the
 * higher-ranked word), D_ij = codf[k][i][j], D_i = codf[k][i][i], M = number of documents behind the counts:
 *   umass[k]  (Mimno et al. 2011, as a mean) mean over the DEFINED pairs of log((D_ij + 1) / D_j); a pair with D_j = 0 is undefined,
 *             skipped and counted in undefined_pairs[k]; NaN if no pair is defined;
 *   npmi[k]   (document as the window; Lau et al. 2014) mean over all pairs of: -1 if D_ij = 0; 0 if D_ij = M; otherwise
 *             log(D_ij M / (D_i D_j)) / -log(D_ij / M).
 * No epsilon is added anywhere; the sums are compensated (Neumaier).  Errors: K outside [1, 1024], N outside [2, 64], M <= 0, NULL
 * argument -> TMVB_EINVAL; codf not symmetric, a negative entry, an off-diagonal entry above either of its diagonal entries, a diagonal
 * entry above M -> TMVB_ESHAPE. */
#define TMVB_CODF_CHUNK_DOCS 4096                           /* documents per workgroup of the pair pass: 64 words of a bit-matrix row */
#define TMVB_CODF_DEFAULT_BITSET_BYTES 1073741824           /* 1 GiB */
typedef struct { int64_t n_slots; int32_t n_batches; float ms_bitset, ms_pairs; } tmvb_codf_info_t;
int tmvb_corpus_codocfreq(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts,
                          int32_t K, int32_t N, const int32_t* top, int64_t max_bitset_bytes, int64_t* codf, tmvb_codf_info_t* info);
int tmvb_coherence_from_counts(int32_t K, int32_t N, int64_t M, const int64_t* codf, double* umass, double* npmi,
                               int32_t* undefined_pairs);

/* ============================== nearest documents in topic space: fused scores and top-n ==============================
 * Which rows of a database of topic proportions are closest to each query row (the reference stops at topicdist(model, d), one document's
 * proportions).  xd is the database, column-major K x Md fp64 on the HOST (row e is xd[K e .. K e + K), as theta in tmvb_heldout_loglik);
 * xq the queries, K x Mq, or NULL: the queries are then database rows [q0, q0 + Mq) and each excludes itself.
 *
 * Features: every row is transformed in fp64 and each value rounded ONCE to fp32.  TMVB_NB_DOT: the row as given.  TMVB_NB_HELLINGER: the
 * rows are distributions, feature = sqrt(x); the score is the Bhattacharyya coefficient = 1 - H^2 (H the Hellinger distance).
 * TMVB_NB_COSINE: rows nonnegative and not all zero, feature = x / ||x||_2 with the fp64 norm.  Rows are padded with zeros to kp (K rounded
 * up to a multiple of 4: rows are 16-byte aligned and the MFMA's k-step of 2 divides them).
 * Score: s(q, e) is the fp32 fmaf chain over k = 0 .. K - 1 in ascending order starting from 0 -- what v_mfma_f32_32x32x2_f32 computes when
 * the K loop feeds its accumulator; padding contributes exactly nothing, so the score of a pair does not depend on tiling.
 * Order: for each query the n best database rows under the TOTAL order (score descending, index ascending on equal scores), listed in that
 * order in idx[Mq][n] (0-based) and score[Mq][n]; count[q] = min(n, number of candidates); slots beyond count[q] hold idx = -1 and
 * score = -inf.  With xq == NULL row q0 + q is no candidate of query q; with xq given q0 must be 0 and nothing is excluded.
 * Purity: the result is a pure function of the inputs -- independent of `splits` (0 = the library's choice: as many database splits as
 * fill the device when there are few query tiles, 1 when there are many; > 0 forces that many, for tests), of tile sizes and of the order
 * in which workgroups finish; two calls give the same bits; queries [q0, q0 + m) of a large call equal the call (Mq = m, q0), which is how
 * a multi-rank host shards the queries.  No atomics on global memory.
 * Device path: a feature kernel (fp64 in, fp32 [M][kp] out); a scan kernel -- a workgroup owns 128 queries and one database split (a run
 * of whole tiles of TMVB_NB_TILE_DB rows), stages both operands through LDS, accumulates on the f32 MFMA and, instead of storing, tests every
 * accumulator entry against its query's n-th best so far (kept in LDS) and inserts the survivors --; a merge kernel takes the splits x n
 * partial lists of a query to the final n under the same order (skipped with one split).
 * info (or NULL): splits = database splits used (at most the number of database tiles), kp, ms_prep / ms_scan / ms_merge = device time of
 * the feature, scan and merge kernels (HIP events around the kernels only).
 * Errors, judged before the device is touched: K outside [1, 1024], n outside [1, TMVB_NB_TOPN_MAX], Md <= 0, Mq <= 0, Md >= 2^31,
 * splits < 0 or > Md, q0 < 0, q0 + Mq > Md with xq == NULL, q0 != 0 with xq given, an unknown metric, a NULL argument -> TMVB_EINVAL; a
 * non-finite entry, HELLINGER: a negative entry or a column sum further than 1e-6 from 1 (the rule of tmvb_heldout_loglik's theta), COSINE:
 * a negative entry or an all-zero row -> TMVB_ESHAPE; then ctx == NULL without a visible device -> TMVB_ENODEVICE (there is no CPU path). */
#define TMVB_NB_DOT 0
#define TMVB_NB_HELLINGER 1
#define TMVB_NB_COSINE 2
#define TMVB_NB_TOPN_MAX 64
#define TMVB_NB_TILE_DB 128                                 /* database rows per tile of the scan kernel */
typedef struct { int32_t splits, kp; float ms_prep, ms_scan, ms_merge; } tmvb_neighbors_info_t;
int tmvb_topic_neighbors(tmvb_ctx* ctx, int32_t K, int32_t metric, int64_t Md, const double* xd, int64_t Mq, const double* xq, int64_t q0,
                         int32_t n, int32_t splits, int32_t* idx, float* score, int32_t* count, tmvb_neighbors_info_t* info);

/* ============================== cluster documents in topic space: k-means with fused assignment ==============================
 * Lloyd's algorithm on the rows of x (column-major K x M fp64 on the HOST, as xd of tmvb_topic_neighbors; the reference has no such function).
 * init: K x C centroids in feature space (column c = centroid c), or NULL: k-means++ on the device.  Outputs: label[M] (0-based), centroid[K C]
 * (the fp32 centroid values widened to fp64, feature space, column c = centroid c), count[C], dist2[M] (each document's squared distance to its
 * centroid), inertia[max_iter + 1] (J^t for t <= iters, NaN beyond), seeds[C] (the chosen document ids; -1 everywhere when init is given).
 *
 * Features: F[M][kp] fp32 as in tmvb_topic_neighbors -- TMVB_KM_EUCLID the row as given, TMVB_KM_HELLINGER sqrt(x), TMVB_KM_COSINE x / ||x||_2 --
 * each value rounded ONCE, kp = K rounded up to a multiple of 4, pads zero.  n_d = the fp32 fmaf chain of f_dk^2 over k = 0 .. K - 1 ascending
 * from 0.  Centroids Cf[C][kp] have the same layout, n_c is the same chain over the centroid, b_c = -0.5f n_c.
 * Assignment: a(d, c) = the f32-MFMA chain of tmvb_topic_neighbors (fp32, k ascending from 0; padding contributes nothing, tiling cannot change
 * a bit); s(d, c) = a(d, c) + b_c, one fp32 add; label[d] = the c of largest s, the LOWEST c on equal s; dist2[d] = max(0, fmaf(-2,
 * s(d, label[d]), n_d)).  J = the fp64 sum of the dist2 values in a fixed order: documents in blocks of TMVB_KM_RUN ascending, each block
 * summed sequentially ascending, the block sums added sequentially ascending.
 * Update: count[c] is an exact integer.  The members of c in ascending document id are cut into runs of TMVB_KM_RUN; each run of F rows is
 * summed sequentially ascending in fp64, the run sums are added sequentially ascending.  EUCLID, HELLINGER: centroid = (float)(sum /
 * (double)count).  COSINE: centroid = (float)(sum / ||sum||_2), the norm in fp64 (spherical k-means).  A cluster without members keeps its
 * centroid; n_empty counts such clusters in the last assignment.  No floating-point atomics anywhere (integer ones for the histogram and
 * the changed-label counter).
 * Loop: c^0 = init rounded once to fp32, or the seeding.  For t = 0, 1, ...: (1) label^t = assign(c^t), which gives J^t; (2) t >= 1 and no label
 * differs from label^(t-1): stop = 1 (c^t is then the mean of these labels); (3) t == max_iter: stop = 0; (4) tol > 0, t >= 1 and J^(t-1) - J^t
 * <= tol J^(t-1): stop = 2; (5) else c^(t+1) = update(label^t, c^t).  Returned: label^t, c^t, count^t, dist2^t, iters = t -- every returned
 * label is the best centroid among the RETURNED centroids.  max_iter = 0 is "assign only".
 * Seeding (init == NULL), k-means++: u_j = tmvb_u53(x[0], x[1]) of tmvb_rng(seed, j, TMVB_RNG_KMEANS, 0, 0).  Seed 0 = document floor(u_0 M).
 * Round j >= 1: m[d] = min over the seeds s so far of D2(d, s), in fp64 from the fp32 features: dot = sum_k (double)f_dk (double)f_sk
 * sequentially ascending (every product is exact), N_d and N_s the same sums of a row with itself, D2 = max(0, (N_d + N_s) - 2 dot).  cum = the
 * prefix sum of m in the blocked order of J: cum(d) = (block sums before d's block, added sequentially from 0) + (m of d's block up to and
 * including d, added sequentially); total = all block sums.  The pick is the first d with cum(d) > u_j total; with total == 0, or no such d,
 * the lowest document id not yet chosen.  c^0 = the picked rows of F.
 * Purity: the same inputs give the same bytes, independent of launch geometry and of the order in which workgroups finish; an assign-only call
 * on documents [a, b) equals that slice of the full assign-only call.
 * info (or NULL): iters, stop, n_empty, kp, moved_last = labels that differ from the previous assignment at the last one (M at t = 0),
 * ms_prep / ms_seed = device time of the feature and seeding kernels, ms_assign / ms_update = device time of ALL assignment (with J) and ALL
 * update steps of the call (HIP events around the kernels).
 * Errors, judged before the device is touched: K outside [1, 1024], C outside [1, min(M, TMVB_KM_CMAX)], M <= 0 or >= 2^31, max_iter outside
 * [0, 10000], tol negative or not finite, an unknown metric, a NULL required argument (everything but init and info) -> TMVB_EINVAL; a
 * non-finite entry of x or init, HELLINGER: a negative entry or a column sum off 1 by more than 1e-6 (x only: init is in feature space),
 * COSINE: a negative entry or an all-zero row -> TMVB_ESHAPE; then ctx == NULL without a visible device -> TMVB_ENODEVICE (no CPU path). */
#define TMVB_KM_EUCLID    0
#define TMVB_KM_HELLINGER 1
#define TMVB_KM_COSINE    2
#define TMVB_KM_CMAX   1024
#define TMVB_KM_RUN     256                                 /* members / documents per fixed-order partial sum */
typedef struct { int32_t iters, stop, n_empty, kp; int64_t moved_last; float ms_prep, ms_seed, ms_assign, ms_update; } tmvb_kmeans_info_t;
int tmvb_topic_kmeans(tmvb_ctx* ctx, int32_t K, int32_t metric, int64_t M, const double* x, int32_t C, const double* init, int64_t seed,
                      int32_t max_iter, double tol, int32_t* label, double* centroid, int64_t* count, float* dist2, double* inertia,
                      int32_t* seeds, tmvb_kmeans_info_t* info);

/* ============================== map documents in two dimensions: exact t-SNE over the topic kNN graph ==============================
 * Two calls (the reference has no such function): tmvb_map_affinity turns the neighbour lists of tmvb_topic_neighbors into the symmetric input
 * similarities P of t-SNE (van der Maaten & Hinton 2008), tmvb_map_layout runs the gradient descent with the EXACT repulsive term: all M^2 pairs,
 * no Barnes-Hut tree, no FFT grid.  Every sum has one order fixed by the constants below, so equal inputs give equal bytes.
 *
 * ---- tmvb_map_affinity.  Inputs on the HOST: idx[M][n] (0-based), d2[M][n] (fp32 squared distances), count[M] -- what tmvb_topic_neighbors
 * returns, with d2 = max(0, 2 - 2 score) for HELLINGER and COSINE features; only the first count[i] slots of row i are read.  perplexity u.
 * Per point i with n_i = count[i], everything in fp64: delta_j = (double)d2_ij - min_j (double)d2_ij; for a trial beta, e_j = exp(-beta delta_j),
 * S = sum_j e_j, T = sum_j delta_j e_j, H(beta) = log S + beta T / S.  S and T are xor-butterfly sums over the 64 lanes of a wave (offsets 32, 16,
 * ... 1), slot j in lane j, empty lanes 0.  Search, a FIXED schedule of TMVB_MAP_BISECT steps without early exit: beta = 1, lo = 0, hi = inf; each
 * step evaluates H(beta); H > log u: lo = beta, beta = (hi == inf ? 2 beta : (beta + hi) / 2); else: hi = beta, beta = (lo + beta) / 2.  beta_i =
 * beta after the last step, p_{j|i} = e_j / S at beta_i.  Rows with n_i <= u (no beta reaches log u): beta_i = 0 and p = 1 / n_i; n_i = 0: an
 * empty row.  Outputs: beta[M], p_cond[M][n] (0 past count), and the symmetrised matrix as CSR (formed on the host side of the library, a counting
 * sort by column and a merge): row i holds every j that lists i or is listed by i, ascending, once; val = (float)((a + b) / (2.0 M)) with a =
 * p_{j|i} (0 if i does not list j), b = p_{i|j} (0 likewise): fp64, rounded once.  The caller allocates row_ptr[M + 1], col[2 M n], val[2 M n];
 * row_ptr[M] entries are used; Mc == M.  The conditional form, for placing new points on a finished map: row_ptr == col == val == NULL, the M >= 1
 * rows are new points, their indices lie in [0, Mc) (the mapped points) and nothing is a self match; only beta and p_cond are returned.
 * Errors, judged before the device is touched: M < 2 or >= 2^31, Mc != M (conditional form: M < 1, Mc outside [1, 2^31)), n outside [1,
 * TMVB_NB_TOPN_MAX], 2 M n >= 2^31, u < 1 or not finite, a NULL argument (only some of row_ptr, col, val given included) -> TMVB_EINVAL;
 * count[i] outside [0, n], an index outside [0, Mc), i among its own neighbours (symmetric form), an index twice in one row, a negative
 * or non-finite distance -> TMVB_ESHAPE; then ctx == NULL without a visible device -> TMVB_ENODEVICE (there is no CPU path).
 *
 * ---- tmvb_map_layout.  P as the CSR above (row_ptr[0] = 0, columns strictly ascending in a row, no diagonal, values finite and >= 0; it need not
 * come from tmvb_map_affinity).  State y, vel, gain: [M][2] fp32.  y0 / vel0 / gain0 are the state on entry (vel0 == NULL: 0; gain0 == NULL: 1;
 * y0 == NULL, allowed only with iter0 == 0: y_ic = (float)(1e-4 (2 u - 1)) in fp64 with u = tmvb_u53(x[0], x[1]) of tmvb_rng(seed, i,
 * TMVB_RNG_MAP, c, 0)); y / vel / gain are the state on return.  Iteration t = 0 .. iters - 1 has the global index T = iter0 + t; e =
 * exaggeration and mu = momentum0 while T < exag_iters, else e = 1 and mu = momentum1.
 * Repulsion, the O(M^2) kernel.  For point i the j's are cut into runs of TMVB_MAP_RUN consecutive indices.  Inside a run, fp32, sequentially
 * ascending from z = rx = ry = 0:  dx = y_ix - y_jx; dy = y_iy - y_jy; d = fmaf(dy, dy, fmaf(dx, dx, 1.0f)); q = an fp32 reciprocal of d with
 * error <= 1 ulp (v_rcp_f32: q is NOT pinned bit for bit); z += q; w = q q; rx = fmaf(w, dx, rx); ry = fmaf(w, dy, ry).  j = i is included
 * (it adds exactly 1 to z and 0 to r).  The run sums are widened to fp64 and added ascending from 0 inside a segment of TMVB_MAP_SEG runs; the
 * segment sums are added ascending from 0: zrow[i], rep[i][2].  Runs and segments depend on M alone, never on launch geometry (j_split = how many
 * workgroups share the segments of one tile of points; 0 = the library's choice), and there are no floating-point atomics.
 * Blocked sum of a column v[M]: blocks of TMVB_MAP_RUN rows, each added sequentially ascending from 0 in fp64, the block sums added sequentially
 * ascending from 0.  Z = blocked(zrow) - (double)M.
 * Attraction, fp64 from the fp32 y: edge number m of row i (m = 0 for its first CSR entry) goes to slot m mod 64; a slot adds its terms
 * (p dx) / (1 + (dx dx + dy dy)), dx = (double)y_ix - (double)y_jx, sequentially ascending from 0; the 64 slots are added ascending from 0: att[i][2].
 * Gradient: g_ic = (float)(4.0 * (e * att_ic - rep_ic / Z)), every operation rounded on its own (no fusing).
 * Update, fp32, every operation rounded on its own: differ = (vel > 0 and g < 0) or (vel < 0 and g > 0); gain = differ ? gain + 0.2f : gain * 0.8f;
 * gain = max(gain, min_gain); vel = mu * vel - (eta * gain) * g; y' = y + vel.  Recentre: m_c = (float)(blocked(y'_c) / (double)M); y = y' - m_c.
 * |g|^2 = blocked((double)g_x (double)g_x + (double)g_y (double)g_y); the gradient norm is its square root.
 * KL of a state y: Z(y) as above; row i: slots as in the attraction with terms p log((p Z) (1 + (dx dx + dy dy))), p > 0 only; KL = blocked(rows).
 * It is evaluated on the state AFTER iteration t whenever check > 0 and (T + 1) mod check == 0, and on the returned state: kl[k], kl_iter[k] = the
 * number of iterations behind that state (T + 1), info->n_kl entries, kl_cap >= iters / check + 2 (check == 0: 2).  The values stay on the device
 * until the call returns.  min_grad_norm > 0: at those checked iterations the host reads the gradient norm of iteration t and stops (stop = 1) when
 * it is below min_grad_norm; that is the only host read inside the loop.
 * Splittable: (iter0 = 0, iters = a) followed by (iter0 = a, iters = b) on the returned state gives the bytes of (iter0 = 0, iters = a + b).
 * Optional outputs (or NULL), the pieces of the LAST gradient evaluation (zeros with iters = 0): rep[M][2], zrow[M], att[M][2] (fp64), grad[M][2]
 * (fp32).  info (or NULL): iters done, stop (0 iters, 1 min_grad_norm), n_kl, j_split used, Z and grad_norm of the last gradient evaluation,
 * ms_rep / ms_att / ms_upd = device time of all repulsion (with Z), attraction and update (with recentring) kernels of the iterations.
 * Error model of the repulsion, per row and first order, in units of 2^-24 relative: dx <= 1, d <= 4, q <= 6, w <= 13, w dx <= 14, and a run of
 * TMVB_MAP_RUN sequential fp32 adds <= (TMVB_MAP_RUN - 1) of sum |terms|:  |rep - rep64| <= (TMVB_MAP_RUN + 24) 2^-24 sum_j |w dx|,  |zrow - z64| <=
 * (TMVB_MAP_RUN + 8) 2^-24 sum_j q.
 * Errors, judged before the device is touched: M < 2 or >= 2^31, iters outside [0, 100000], iter0 < 0, exag_iters < 0, check < 0, j_split < 0,
 * exaggeration < 1, eta <= 0, momentum outside [0, 1), min_gain <= 0, min_grad_norm < 0, any of them not finite, kl_cap too small, y0 == NULL with
 * iter0 != 0, a NULL required argument -> TMVB_EINVAL; a CSR that breaks the rules above or a non-finite state -> TMVB_ESHAPE; then ctx == NULL
 * without a visible device -> TMVB_ENODEVICE (there is no CPU path).  A returned state that is not finite -> TMVB_ENONFINITE. */
#define TMVB_MAP_BISECT 64
#define TMVB_MAP_RUN   256                                  /* consecutive j per fp32 partial sum; rows per block of a blocked sum */
#define TMVB_MAP_SEG    64                                  /* runs per fp64 segment sum */
#define TMVB_MAP_SLOTS  64                                  /* slots of a row's edge sums */
typedef struct { int32_t iters, iter0, exag_iters, check, j_split, reserved; int64_t seed; double exaggeration, min_grad_norm;
                 float momentum0, momentum1, eta, min_gain; } tmvb_map_params_t;
typedef struct { int32_t iters, stop, n_kl, j_split; double Z, grad_norm; float ms_rep, ms_att, ms_upd, reserved; } tmvb_map_info_t;
int tmvb_map_affinity(tmvb_ctx* ctx, int64_t M, int64_t Mc, int32_t n, const int32_t* idx, const float* d2, const int32_t* count, double perplexity,
                      double* beta, double* p_cond, int64_t* row_ptr, int32_t* col, float* val);
int tmvb_map_layout(tmvb_ctx* ctx, int64_t M, const int64_t* row_ptr, const int32_t* col, const float* val, const tmvb_map_params_t* params,
                    const float* y0, const float* vel0, const float* gain0, float* y, float* vel, float* gain, int32_t kl_cap, double* kl,
                    int32_t* kl_iter, double* rep, double* zrow, double* att, float* grad, tmvb_map_info_t* info);

/* ============================== search documents by words: query likelihood with fused top-n ==============================
 * Which documents are about these words (the reference has no such function): the query likelihood of LDA-based retrieval (Wei & Croft
 * 2006) = the held-out log-likelihood of tmvb_heldout_loglik with the roles turned round -- one short "held-out document", every training
 * document's theta.  theta is K x Md and beta K x V, column-major fp64 on the HOST, exactly as in tmvb_heldout_loglik (theta columns are
 * distributions under the 1e-6 rule, beta is right stochastic).  The queries are a CSR: q_ptr[Q+1], q_terms 0-based in [0, V), q_counts
 * >= 1; the entries of a query need be neither sorted nor distinct, their order is the summation order; a query has between 1 and
 * TMVB_SEARCH_TILE_COLS entries.
 *
 * Score.  Theta features: the rows rounded ONCE to fp32 and padded to kp, the TMVB_NB_DOT feature of tmvb_topic_neighbors.  beta' =
 * (beta + laplace_smooth) / (1 + laplace_smooth V) in fp64, rounded once to fp32; only the W = q_ptr[Q] columns the queries name go to
 * the device.  p(d, j) = the fp32 fmaf chain over k ascending from 0 -- what v_mfma_f32_32x32x2_f32 leaves, and the same bits
 * tmvb_topic_neighbors (TMVB_NB_DOT) returns for that pair.  score(q, d) = (float) sum_j c_j log((double) p(d, j)): logarithm and sum in
 * fp64, j over the query's entries in ascending order, ONE accumulator (acc = fma(c_j, log p, acc)), then one rounding to fp32.  p = 0
 * gives -inf; no epsilon is added.
 * Order: the total order of tmvb_topic_neighbors (score descending, index ascending).  A -inf document is a candidate like any other (it
 * comes before an empty slot), so count[q] = min(n, Md).  idx[Q][n] is 0-based, score[Q][n] holds the scores; slots past count[q] hold
 * idx = -1 and score = -inf.
 * Purity: the bits of score(q, d) depend on theta_d, on the query's own entries and on beta', and on nothing else -- not on the other
 * queries, the query's position in a column tile, Md, the row's position, `splits` (as in tmvb_topic_neighbors) or the order in which
 * workgroups finish; two calls give the same bytes; queries [a, b) of a call equal the call on that slice; a call on database rows
 * [a, b) returns for those rows the same score bits as the full call.  No atomics on global memory.
 * Device path: the host packs whole queries, in order, into column tiles of TMVB_SEARCH_TILE_COLS entries (no query straddles a tile);
 * a feature kernel for theta; a scan kernel -- a workgroup owns one column tile and one database split, takes the 128 x 128 tile of p
 * through the tile loop of tmvb_topic_neighbors, puts it into LDS, walks every (row, query) pair's column segment with the fp64 log and
 * inserts the survivors of the threshold test into the query's sorted n-list --; a merge kernel for splits > 1.  Neither the Md x W
 * probability matrix nor the Md x Q score matrix ever exists.
 * info (or NULL): splits, kp, col_tiles = column tiles the queries were packed into, ms_prep / ms_scan / ms_merge = device time of the
 * feature, scan and merge kernels (HIP events around the kernels only).
 * Errors, judged before the device is touched: K outside [1, 1024], n outside [1, TMVB_NB_TOPN_MAX], Md <= 0, V <= 0, Q <= 0, Md or V
 * >= 2^31, splits < 0 or > Md, laplace_smooth < 0 or not finite, a NULL argument, 2^31 - 1 or more entries -> TMVB_EINVAL; q_ptr not
 * non-decreasing from 0, an empty query, a query of more than TMVB_SEARCH_TILE_COLS entries, a term outside [0, V), a count < 1, beta
 * not right stochastic, a bad theta column (the wording of tmvb_heldout_loglik) -> TMVB_ESHAPE; then ctx == NULL without a visible
 * device -> TMVB_ENODEVICE (there is no CPU path). */
#define TMVB_SEARCH_TILE_COLS 128                           /* query entries per column tile; also the most entries one query may have */
typedef struct { int32_t splits, kp, col_tiles; float ms_prep, ms_scan, ms_merge; } tmvb_search_info_t;
int tmvb_topic_search(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t Md, const double* theta, const double* beta, double laplace_smooth,
                      int64_t Q, const int64_t* q_ptr, const int32_t* q_terms, const int32_t* q_counts,
                      int32_t n, int32_t splits, int32_t* idx, float* score, int32_t* count, tmvb_search_info_t* info);

/* ============================== word-topic assignments: per-token responsibilities with fused top-t ==============================
 * Which topic a word belongs to in a document: phi of update_phi! (src/LDA.jl:150-154, src/CTM.jl:175-178, src/CTPF.jl:327-330), the one model
 * output the reference's update_host! fills (src/modelutils.jl:514-515, :534-535, :559-560) and this engine never keeps.  Stateless and
 * family-agnostic: for entry n (term w, count c) of document d
 *     y_k = eps + A[k, d] B[k, w],    r_k = y_k / sum_j y_j,    k = 0 .. K - 1,
 * with A (K x M) and B (K x V) column-major fp64 on the HOST, both nonnegative: LDA A = exp(Elogtheta), B = beta; CTM A = exp(lambda_d -
 * max_k lambda_d), B = beta; CTPF A = exp(psi(gimel_d) - log dalet - log bet - column max), B = exp(psi(alef_w) - column max).  eps is the
 * reference's @positive (EPSILON, src/macros.jl:34-39, src/LDA.jl:152); for CTM and CTPF the eps-form is the softmax wherever sum A B >> eps.
 * Rounding: A, B and eps are rounded ONCE to fp32; y_k = fma(A, B, eps), the sum in a fixed order (per 16-byte chunk ((y0 + y1) + (y2 + y3)),
 * a lane's chunks ascending, the lanes of an entry in an xor butterfly) and the IEEE division are fp32.  With eps in [2^-100, 1] every y_k is a
 * normal positive number.  Products beyond fp32 are the caller's to avoid (shift the columns as above).
 * Selection.  The CSR is tmvb_corpus_create's (a document without entries is legal).  docs[Ms]: 0-based document ids, repeats and any order
 * allowed; NULL = all M documents in order (Ms is then M or 0).  The selected documents' entries are numbered 0 .. nsel - 1 in docs order.
 * Outputs, each may be NULL (top_idx and top_r together), at least one is not:
 *   top_idx[nsel][t], top_r[nsel][t]   the t best topics of every entry under (r bits descending, topic id ascending); slots past K hold -1 and 0;
 *   phi[nsel][K]                       the dense fp32 responsibilities, K contiguous per entry (the reference's hcat layout);
 *   hard[Ms][K]                        int64, sum of c_n over the document's entries whose best topic is k.
 * max_chunk_entries bounds the entries per launch group and with it the padded device buffer of the dense output ([chunk][KP] fp32); 0 = the
 * library's choice: with phi as many entries as keep that buffer at 256 MiB, without phi one chunk.  A document is cut where a chunk ends.
 * Purity: an entry's results depend on its document's A column, its term's B column and eps alone -- not on docs, the chunks, the other outputs
 * or the order in which workgroups finish; two calls give the same bytes.  No atomics.
 * info (or NULL): nsel, n_short / n_long = work items (runs of entries of one document inside one chunk) on the 64- and the 256-lane kernel,
 * chunks, lanes_per_entry (64 / lanes_per_entry entries per trip of a wave), ms_kernel = device time of the kernels (HIP events around them).
 * Errors, judged before the device is touched, all TMVB_EINVAL: K outside [1, 1024], t outside [1, TMVB_TT_TOP_MAX], eps outside [2^-100, 1]
 * or NaN, M <= 0, V <= 0, a NULL input, every output NULL, top_idx without top_r, max_chunk_entries < 0, doc_ptr not non-decreasing from 0,
 * 2^31 - 2 or more entries (of the CSR or selected), a term outside [0, V), a count < 1, an id of docs outside [0, M), a selected document of 2^31 or more tokens, a
 * value of B or of a selected column of A that is negative, NaN or beyond fp32; then ctx == NULL without a visible device -> TMVB_ENODEVICE (there is no CPU path).
 *
 * tmvb_digamma_f64: HOST ONLY, touches no device.  y[i] = psi(x[i]) in fp64 by the engine's host digamma (the recurrence below 7 and the
 * asymptotic series of the reference's own helper, src/utils.jl:21-53, in fp64; within 1/4 of the positive root 1.46163... a Taylor series
 * about the root, which keeps the RELATIVE error at 1e-14 where psi passes through 0), so that the CTPF factors above need no SciPy.  x > 0. */
#define TMVB_TT_TOP_MAX 8
typedef struct { int64_t nsel, n_short, n_long; int32_t chunks, lanes_per_entry; float ms_kernel; } tmvb_token_topics_info_t;
int tmvb_token_topics(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t M, const double* A, const double* B, const int64_t* doc_ptr,
                      const int32_t* terms, const int32_t* counts, const int32_t* docs, int64_t Ms, double eps, int32_t t,
                      int64_t max_chunk_entries, int32_t* top_idx, float* top_r, float* phi, int64_t* hard, tmvb_token_topics_info_t* info);
int tmvb_digamma_f64(const double* x, double* y, int64_t n);

/* ============================== held-out recommendation metrics for CTPF: reader split, fused ranks, metrics ==============================
 * Hold out part of the (document, reader) entries, train on the rest, ask where each held-out document lands in its user's ranking (the
 * reference stops at showdrecs / showurecs).
 *
 * tmvb_readers_split: HOST ONLY, touches no device.  The reader CSR of tmvb_corpus_create (rdr_ptr[M+1], readers[nR] in [0, U), ratings[nR])
 * -> two reader CSRs over the same M, observed and held out.  The order inside a document is kept and obs + held reproduces the input exactly.
 * Draw rule, Philox4x32-10 with key = seed (csrc/tmvb_philox.h: tmvb_rng).  mode TMVB_RSPLIT_ENTRY (in-matrix): entry j of document d takes
 * word x[j & 3] of counter (doc_offset + d, stage TMVB_RNG_RSPLIT_ENTRY = 6, draw j >> 2) and is HELD OUT iff word < floor(frac * 2^32) (as
 * 64-bit integers: frac = 0 holds out nothing, frac = 1 everything).  mode TMVB_RSPLIT_DOCUMENT (out-of-matrix / cold start): document d takes
 * word x[0] of counter (doc_offset + d, stage TMVB_RNG_RSPLIT_DOCUMENT = 7, draw 0); if held, all of its readers go to the held-out side.
 * Documents [d0, d0 + m) of a large call equal the call (M = m, doc_offset = d0).
 * Errors: out == NULL, frac outside [0, 1] or not finite, doc_offset < 0, an unknown mode, M <= 0, U <= 0, a NULL argument -> TMVB_EINVAL;
 * rdr_ptr not non-decreasing from 0, a reader outside [0, U), a rating < 1 -> TMVB_ESHAPE.  The arrays of *out are allocated by the
 * library: tmvb_rsplit_free.
 *
 * tmvb_score_ranks: K in [1, 1024]; database xd, column-major K x Md fp64, queries xq, K x Mq fp64, both on the HOST; per query two lists of
 * 0-based database ids in CSR form, exclusions (excl_ptr[Mq+1], excl_idx) and targets (tgt_ptr[Mq+1], tgt_idx), each strictly ascending
 * within a query and the two disjoint.  Outputs: rank[nT] (nT = tgt_ptr[Mq], in the order of tgt_idx), n_cand[Mq] = Md - |excl(q)|,
 * score[nT] (fp32, or NULL).
 * Features: the rows as given, each value rounded ONCE to fp32, padded to kp exactly as in tmvb_topic_neighbors (TMVB_NB_DOT).
 * Score: s(q, e) is the fp32 fmaf chain over k = 0 .. K - 1 in ascending order starting from 0 -- what v_mfma_f32_32x32x2_f32 computes when
 * the K loop feeds its accumulator.
 * Order: the reference's reverse(sortperm(.)): e comes BEFORE t iff s_e > s_t, or s_e == s_t and e > t -- descending index on ties, NOT the
 * order of tmvb_topic_neighbors.
 * Rank: for target t of query q, rank = #{ e in [0, Md) : e not in excl(q), e != t, e before t }.  The other targets of q are candidates like
 * any other row.  With X = gimel / dalet + zayin / het and Y = he / vav of a CTPF state, users as queries and their observed libraries as
 * exclusions, rank is the 0-based position of t in urecs[u] of tmvb_ctpf_recommend (up to that unit's own rounding of the scores).
 * Purity: the result is a pure function of the inputs -- independent of `splits` (0 = the library's choice, > 0 forces that many database
 * splits, as in tmvb_topic_neighbors), of tile sizes, of the number of target slots in LDS and of the order in which workgroups finish; two
 * calls give the same bits; queries [a, b) of a call equal the call on that slice.
 * Device path: a feature kernel (the layout of tmvb_topic_neighbors); a pair kernel -- the score of every listed (query, id) pair, targets
 * and exclusions alike: one wave takes 32 pairs, feeds the same MFMA the same operand values in the same k order and keeps the diagonal of its
 * 32 x 32 tile, so a pair's score has the same bits here as in the scan --, followed by a sort of each query's targets; a scan kernel -- the
 * tile loop of tmvb_topic_neighbors (a workgroup owns 128 queries and one database split) whose epilogue, instead of storing, counts for every
 * target of a query the rows that come before it (ballot and popcount per 32 rows, integer adds in LDS, then one global integer add per
 * target and split; a tile with more targets than LDS slots runs in passes) --; a fix kernel: rank = count - #{o in excl(q) : o before t},
 * a loop over the query's excluded scores, which keeps every membership test out of the scan.
 * info (or NULL): splits, kp, ms_prep / ms_pairs / ms_scan / ms_fix = device time of the stages (HIP events around the kernels only).
 * Errors, judged before the device is touched: K outside [1, 1024], Md <= 0, Mq <= 0, Md >= 2^31, splits < 0 or > Md, a NULL argument,
 * 2^31 - 1 or more listed ids -> TMVB_EINVAL; a list pointer not non-decreasing from 0, a non-finite entry, ids out of range, not strictly
 * ascending or shared between the two lists of a query -> TMVB_ESHAPE; then ctx == NULL without a visible device -> TMVB_ENODEVICE (there
 * is no CPU path).
 *
 * tmvb_rank_metrics: HOST ONLY, fp64 arithmetic on the integers.  Per query with T >= 1 targets and for each cut-off N of Ns[nN]:
 *   hits@N = #{rank < N};  recall[q][a] = hits / T;  precision[q][a] = hits / N;
 *   ndcg[q][a] = sum_{rank < N} 1 / log2(rank + 2)  /  sum_{i < min(T, N)} 1 / log2(i + 2);
 *   mrr[q] = 1 / (min rank + 1);  pct_rank[q] = mean rank / max(n_cand[q] - 1, 1).
 * A query without targets gets NaN everywhere and is left out of the means.  mean[3 nN + 2]: the means over the queries with targets of
 * recall@Ns, precision@Ns, ndcg@Ns, mrr, pct_rank, in that order (NaN if there is no such query); counts[2]: the number of such queries
 * and the number of targets.  Errors: Mq <= 0, nN < 1, an N < 1, a NULL argument -> TMVB_EINVAL; tgt_ptr not non-decreasing from 0, a rank
 * outside [0, n_cand[q]) -> TMVB_ESHAPE. */
#define TMVB_RSPLIT_ENTRY 0
#define TMVB_RSPLIT_DOCUMENT 1
typedef struct {
    int64_t M, n_obs, n_held;
    int64_t* obs_ptr;  int32_t* obs_readers;  int32_t* obs_ratings;      /* [M+1], [n_obs], [n_obs] */
    int64_t* held_ptr; int32_t* held_readers; int32_t* held_ratings;     /* [M+1], [n_held], [n_held] */
} tmvb_rsplit_t;
int  tmvb_readers_split(int64_t M, int64_t U, const int64_t* rdr_ptr, const int32_t* readers, const int32_t* ratings, double frac, int64_t seed,
                        int64_t doc_offset, int32_t mode, tmvb_rsplit_t* out);
void tmvb_rsplit_free(tmvb_rsplit_t* s);
typedef struct { int32_t splits, kp; float ms_prep, ms_pairs, ms_scan, ms_fix; } tmvb_recranks_info_t;
int tmvb_score_ranks(tmvb_ctx* ctx, int32_t K, int64_t Md, const double* xd, int64_t Mq, const double* xq, const int64_t* excl_ptr,
                     const int32_t* excl_idx, const int64_t* tgt_ptr, const int32_t* tgt_idx, int32_t splits, int32_t* rank, int32_t* n_cand,
                     float* score, tmvb_recranks_info_t* info);
int tmvb_rank_metrics(int64_t Mq, const int64_t* tgt_ptr, const int32_t* rank, const int32_t* n_cand, int32_t nN, const int32_t* Ns, double* recall,
                      double* precision, double* ndcg, double* mrr, double* pct_rank, double* mean, int64_t* counts);

/* ============================== top-n recommendations for CTPF: exclusions fused into the score scan ==============================
 * For every query the n best database rows outside the query's exclusion list: for a user the n best documents outside the library, with
 * the roles swapped the n best users outside a document's readers (the reference's consumers, showurecs(model, users, M = 15) and
 * showdrecs(model, docs, U = 15), read the first 15 entries of a full ranking).  No Md x Mq array and no sort.
 *
 * tmvb_score_topn: K in [1, 1024]; database xd, column-major K x Md fp64, queries xq, K x Mq fp64, both on the HOST; per query a list of
 * 0-based database ids in CSR form (excl_ptr[Mq+1], excl_idx), strictly ascending within a query; an empty list is allowed.  n in
 * [1, TMVB_NB_TOPN_MAX].  Outputs: idx[Mq][n], score[Mq][n] (fp32), count[Mq].
 * Features: the rows as given, each value rounded ONCE to fp32, padded to kp exactly as in tmvb_topic_neighbors (TMVB_NB_DOT).
 * Score: s(q, e) is the fp32 fmaf chain over k = 0 .. K - 1 in ascending order starting from 0 -- what v_mfma_f32_32x32x2_f32 computes when
 * the K loop feeds its accumulator.  The score of a pair has the same bits as the pair's score in tmvb_score_ranks and tmvb_topic_neighbors.
 * Order: the reference's reverse(sortperm(.)), as in tmvb_score_ranks: e comes BEFORE t iff s_e > s_t, or s_e == s_t and e > t -- descending
 * index on ties, NOT the order of tmvb_topic_neighbors.
 * Result: for query q the first count[q] = min(n, Md - |excl(q)|) rows of [0, Md) \ excl(q) under that order, listed in that order in
 * idx[q][.] and score[q][.]; slots beyond count[q] hold idx = -1 and score = -inf.  With X = gimel / dalet + zayin / het of a CTPF state as
 * the database, Y = he / vav as the queries and the users' libraries as exclusions, row u is the first n entries of urecs[u] of
 * tmvb_ctpf_recommend (up to that unit's own rounding of the scores).
 * Purity: the result is a pure function of the inputs -- independent of `splits` (0 = the library's choice, > 0 forces that many database
 * splits, as in tmvb_topic_neighbors), of tile sizes and of the order in which workgroups finish; two calls give the same bits; queries
 * [a, b) of a call equal the call on that slice (its excl_ptr rebased to 0).  No atomics on global memory.
 * Device path: a feature kernel (the layout of tmvb_topic_neighbors); a scan kernel -- the tile loop of tmvb_topic_neighbors (a workgroup
 * owns 128 queries and one database split) with a sorted n-list and its threshold per query in LDS, empty slots (-inf, -1) being the worst
 * key under this order: an accumulator entry is tested against its query's threshold first (one LDS read), only a survivor is looked up in
 * its query's exclusion list (binary search on the device), and only a survivor that is not listed is inserted.  Every (query, row) pair is
 * met once, so an excluded row costs at most one search --; a merge kernel takes the splits x n partial lists of a query to the final n
 * under the same order (skipped with one split).
 * info (or NULL): splits, kp, ms_prep / ms_scan / ms_merge = device time of the stages (HIP events around the kernels only).
 * Errors, judged before the device is touched: K outside [1, 1024], n outside [1, TMVB_NB_TOPN_MAX], Md <= 0, Mq <= 0, Md >= 2^31,
 * splits < 0 or > Md, a NULL argument, 2^31 - 1 or more listed ids -> TMVB_EINVAL; excl_ptr not non-decreasing from 0, a non-finite entry,
 * an id out of range or not strictly ascending -> TMVB_ESHAPE; then ctx == NULL without a visible device -> TMVB_ENODEVICE (there is no
 * CPU path). */
typedef struct { int32_t splits, kp; float ms_prep, ms_scan, ms_merge; } tmvb_rectopn_info_t;
int tmvb_score_topn(tmvb_ctx* ctx, int32_t K, int64_t Md, const double* xd, int64_t Mq, const double* xq, const int64_t* excl_ptr,
                    const int32_t* excl_idx, int32_t n, int32_t splits, int32_t* idx, float* score, int32_t* count, tmvb_rectopn_info_t* info);

/* ============================== CTPF fold-in: user factors of new libraries with every document factor frozen ==============================
 * New: the reference moves he once per walk over the corpus (update_he!, src/CTPF.jl:266-277) and has no predict for CTPF
 * (src/modelutils.jl:831-943).  Here he[:, u] of a user who was not in training is iterated to its fixed point under a trained state.
 * Inputs: K in [1, 512]; gimel, zayin column-major K x M, dalet, het, vav [K], the hyperparameter e > 0; Un libraries in CSR form
 * (lib_ptr[Un + 1], lib_docs: 0-based document ids in [0, M), strictly ascending within a user, lib_ratings >= 1); viter >= 0, vtol >= 0;
 * he0 column-major K x Un, or NULL for all ones (the reference's initial he, src/CTPF.jl:86).
 * Definition.  With psi = digamma and, once per call,
 *     W[i, d] = (exp(psi(gimel[i, d])) / dalet[i] + exp(psi(zayin[i, d])) / het[i]) / vav[i],
 * user u with library lib(u) and ratings r_du runs, from h = he0[:, u],
 *     sweep:  t = psi(h);  p[:, d] = exp(t) .* W[:, d] / sum_j exp(t_j) W[j, d]  for d in lib(u);  h_new = e + sum_{d in lib(u)} r_du p[:, d]
 * for at most viter sweeps; after each sweep h <- h_new, and the loop leaves when ||h_new - h||_2 < vtol held for that sweep -- the exit
 * rule and the sweep count of the document loop (src/CTPF.jl:354-361) with he in the place of gimel.  p[:, d] is xi[1:K, .] + xi[K+1:2K, .]
 * of update_xi! (:334-337) for the pair (d, u): psi(he[i, u]) enters both halves of the 2K-way softmax at index i, so the halves add up in
 * front of all sweeps.  One sweep from h = he is the column he_temp[:, u] that one walk of the reference leaves (update_he!(model, d), :274-277).
 * Outputs: he_out column-major K x Un (fp64 copies of the fp32 results), sweeps_out[Un] = sweeps executed.  viter = 0 returns he0 (rounded to
 * fp32); an empty library gives h = e exactly (rounded once), after two sweeps under the defaults viter = 10, vtol = 1 / K^2.
 * Rounding: every input value is rounded ONCE to fp32; W, the sweeps and the exit test are fp32.  exp(t) is taken after subtracting max_j t_j (p
 * does not change); W needs no shift: exp(psi(x)) <= x, and gimel, zayin are bounded by the corpus's total counts and ratings, so the products
 * stay far inside fp32.  A shape value below 0.012 has exp(psi(x)) below the fp32 normal range and its term of W flushes to 0.
 * Purity: a user's result depends on that user's library, he0 column and the state alone -- not on the other users of the call, their order
 * or number; two calls give the same bits.  No atomics, a fixed summation order.  Users are sorted into launch classes by library length; the
 * results come back in the caller's order.
 * Device path: a table kernel (W as [M][kp] fp32, kp = K rounded up to a multiple of 4); one wave per user for libraries of at most
 * TMVB_FOLDIN_REG_CAP entries (TMVB_FOLDIN_REG_CAP_BIGK for K > 256): the library's W rows are gathered once and stay in registers over all
 * sweeps; a workgroup of four waves per longer library, which gathers the rows again in every sweep and combines the waves' partial sums in
 * LDS in a fixed order.
 * info (or NULL): kp, capacity = the register path's capacity at this K, n_reg / n_long = users on each path, ms_prep (the table kernel) and
 * ms_sweeps (the user kernels), HIP events around the kernels only.
 * Errors, judged before the device is touched: a NULL argument, K outside [1, 512], M <= 0, Un < 0, viter < 0, vtol < 0 or not finite,
 * e <= 0 or not finite, 2^31 - 1 or more library entries -> TMVB_EINVAL; lib_ptr not non-decreasing from 0, a document id outside [0, M),
 * ids not strictly ascending, a rating < 1, a state value (gimel, zayin, dalet, het, vav, he0) that is not positive and finite ->
 * TMVB_ESHAPE; then ctx == NULL without a visible device -> TMVB_ENODEVICE (there is no CPU path).
 * tmvb_ctpf_foldin_users_on: the same operator on the device-resident state of a handle (gimel, zayin, the rates and e as tmvb_ctpf_set_state or
 * training left them, already fp32 / fp64 on the device): no K x M upload, the same bits as the stateless form on the same state. */
#define TMVB_FOLDIN_REG_CAP 32
#define TMVB_FOLDIN_REG_CAP_BIGK 16
typedef struct { int32_t kp, capacity; int64_t n_reg, n_long; float ms_prep, ms_sweeps; } tmvb_foldin_info_t;
int tmvb_ctpf_foldin_users(tmvb_ctx* ctx, int32_t K, int64_t M, const double* gimel, const double* zayin, const double* dalet, const double* het,
                           const double* vav, double e, int64_t Un, const int64_t* lib_ptr, const int32_t* lib_docs, const int32_t* lib_ratings,
                           const double* he0, int32_t viter, double vtol, double* he_out, int32_t* sweeps_out, tmvb_foldin_info_t* info);
int tmvb_ctpf_foldin_users_on(tmvb_ctpf* h, int64_t Un, const int64_t* lib_ptr, const int32_t* lib_docs, const int32_t* lib_ratings,
                              const double* he0, int32_t viter, double vtol, double* he_out, int32_t* sweeps_out, tmvb_foldin_info_t* info);

/* ============================== stochastic (minibatch) training for LDA: stepwise EM ==============================
 * New: the reference's train! moves alpha and beta once per walk over the whole corpus (src/LDA.jl:161-187); the closest precedent for statistics
 * gathered batch by batch is v0.6/src/gpuLDA.jl:200-225.  Here the globals move once per BATCH (Cappe & Moulines / Liang & Klein's stepwise EM, the
 * form of online VB that fits a point-estimate beta).
 * Inputs: a corpus of M documents (CSR as tmvb_corpus_create takes it), K, batch cuts 0 = c_0 < c_1 < ... < c_B = M (batch b = documents
 * [c_b, c_{b+1}), M_b >= 1 of them), a schedule (tau0 >= 0, 0.5 < kappa <= 1; default 1, 0.7).
 * State: alpha[K], beta[K*V] (and beta_old), gamma / Elogtheta [K*M] kept across visits as a warm start, the running statistic Sbar[K*V] and its
 * tail Ebar[K] -- fp32 on the device, scaled to the WHOLE corpus --, and the step counter t (steps taken so far; it continues across calls).
 * Initial statistic, formed when a set_state (or the first run) finds none given: Sbar_0 = (sum of all counts / K) beta_0, so that normalising it
 * gives beta_0 back, and Ebar_0 = sum_d Elogtheta_0[:, d].
 * Step t = 1, 2, ... on batch b:
 *   1. the E-step of the batch's documents under the current alpha, beta: tmvb_lda_estep's kernels with (viter, vtol) and the per-document exit
 *      rule of src/LDA.jl:170-180.  It leaves S_b (update_beta!(model, d), :152) and e_b = sum_{d in b} Elogtheta_d (:98).
 *   2. rho_t = (tau0 + t)^(-kappa) in fp64 on the host; c0 = fp32(1 - rho_t), c1 = fp32(rho_t M / M_b), each rounded once.
 *   3. Sbar <- c0 Sbar + c1 S_b and Ebar <- c0 Ebar + c1 e_b in fp32; the batch's statistics buffer is zero afterwards.
 *   4. beta_old <- beta, beta <- Sbar row-normalised (update_beta!, src/LDA.jl:121-125); alpha by update_alpha!(niter, ntol) (:97-118, fp64 Newton
 *      from the current alpha) with Elogtheta_sum = Ebar and M = the whole corpus's.
 * With tau0 = 0 the first step has rho = 1, c0 = 0: with B = 1 it is exactly one iteration of train!.
 * Steps 3 and 4's beta are one fused update of two launches; the row sums are fixed-order partials without floating-point atomics: the same
 * inputs give the same bits, run([a, b, c, d]) equals run([a, b]) then run([c, d]).  There is no random number in the library: the host decides
 * the order of the visits. */
typedef struct tmvb_lda_svi tmvb_lda_svi;
/* gpuLDA(corp, K) (src/gpuLDA.jl:45-84) over batches.  Corpus checks and error codes are tmvb_corpus_create's (src/Corpus.jl:41-50, :111-122); cuts[B + 1]
 * not strictly increasing from 0 to M -> TMVB_EINVAL.  Constructor state as tmvb_lda_create. */
int tmvb_lda_svi_create(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts, int32_t K,
                        const int64_t* cuts, int32_t B, tmvb_lda_svi** out);
int tmvb_lda_svi_destroy(tmvb_lda_svi* h);
/* update_buffer! / update_host! (src/modelutils.jl:390-396, :501-516) plus the running statistic and the step counter: alpha[K], beta / beta_old /
 * sbar[K*V] column-major, gamma / Elogtheta[K*M] in corpus document order, ebar[K], t[1].  NULL = leave / skip; beta without beta_old sets both. */
int tmvb_lda_svi_set_state(tmvb_lda_svi* h, const double* alpha, const double* beta, const double* beta_old, const double* gamma,
                           const double* Elogtheta, const double* sbar, const double* ebar, const int64_t* t);
int tmvb_lda_svi_get_state(tmvb_lda_svi* h, double* alpha, double* beta, double* beta_old, double* gamma, double* Elogtheta, double* sbar,
                           double* ebar, int64_t* t);
/* tau0 < 0 or not finite, kappa outside (0.5, 1] -> TMVB_EINVAL */
int tmvb_lda_svi_set_schedule(tmvb_lda_svi* h, double tau0, double kappa);
/* n steps of train!'s loop body (src/LDA.jl:170-182) on the batches batches[0 .. n), repeats allowed.  Asynchronous on the context's stream.  A batch id
 * outside [0, B) -> TMVB_EINVAL before anything is enqueued. */
int tmvb_lda_svi_run(tmvb_lda_svi* h, const int32_t* batches, int64_t n, int32_t niter, double ntol, int32_t viter, double vtol);
/* The E-step of every batch under the final alpha, beta (src/LDA.jl:170-180); the globals and the running statistic are not touched.  Afterwards gamma and
 * Elogtheta of all documents belong to the returned model.  Asynchronous. */
int tmvb_lda_svi_final_pass(tmvb_lda_svi* h, int32_t viter, double vtol);
/* rho, c0, c1: of the last step (NaN before the first) */
typedef struct { int32_t B, K; int64_t M, V, t; double tau0, kappa, rho; float c0, c1; } tmvb_lda_svi_info_t;
int tmvb_lda_svi_info(tmvb_lda_svi* h, tmvb_lda_svi_info_t* out);
/* as tmvb_lda_doc_sweeps: out[M], each document's sweeps in the last E-step of ITS batch */
int tmvb_lda_svi_doc_sweeps(tmvb_lda_svi* h, uint8_t* out);
/* Timing of the last tmvb_lda_svi_run from HIP events on the context's stream, like tmvb_lda_last_estep_ms (TMVB_ESTEP_TIMING=1 at create): the sums over its
 * *steps steps of the E-step, the fused update (blend + normalise) and update_alpha!, in ms. */
int tmvb_lda_svi_last_run_ms(tmvb_lda_svi* h, float* ms_estep, float* ms_update, float* ms_alpha, int64_t* steps);

/* ============================== stochastic (minibatch) training for CTM: stepwise EM ==============================
 * New: the reference's train! moves mu, sigma and beta once per walk over the whole corpus (src/CTM.jl:185-217).  Here they move once per BATCH, as
 * alpha and beta do in the LDA section above.
 * Inputs: a corpus of M documents (CSR as tmvb_corpus_create takes it), K <= 256, batch cuts 0 = c_0 < c_1 < ... < c_B = M (batch b = documents
 * [c_b, c_{b+1}), M_b >= 1 of them), a schedule (tau0 >= 0, 0.5 < kappa <= 1; default 1, 0.7).
 * State: the globals mu[K], sigma / invsigma[K*K], beta[K*V] (and beta_old); per document, kept across visits as a warm start, lambda / vsq [K*M] and
 * logzeta[M]; the running statistic -- fp32 on the device, scaled to the WHOLE corpus -- Sbar[K*V], lbar[K] (sum lambda), vbar[K] (sum vsq) and
 * Cbar[K*K], the scatter matrix sum (lambda - m_ref)(lambda - m_ref)^T taken about the vector m_ref[K] (fp64), with m_ref itself; and the step
 * counter t (steps taken so far; it continues across calls).
 * Initial statistic, formed when a set_state (or the first run) finds none given: Sbar_0 = (sum of all counts / K) beta_0, so that normalising it
 * gives beta_0 back; lbar_0 = sum_d lambda_d, vbar_0 = sum_d vsq_d, Cbar_0 = sum_d (lambda_d - mu_0)(lambda_d - mu_0)^T, m_ref = mu_0.  The
 * constructor state (lambda = 0, vsq = 1, mu = 0) gives lbar = 0, vbar = M, Cbar = 0, hence sigma = I.
 * Step t = 1, 2, ... on batch b, mu being the current mean:
 *   1. the E-step of the batch's documents under the current mu, invsigma, beta: tmvb_ctm_estep's kernels with (niter, ntol, viter, vtol) and the
 *      per-document exit rule of src/CTM.jl:194-205.  It leaves S_b (update_beta!(model, d), :122-125), l_b = sum_{d in b} lambda_d, v_b = sum vsq_d
 *      and C_b = sum (lambda_d - mu)(lambda_d - mu)^T (the sums of :102-111, the scatter about the CURRENT mu).
 *   2. rho_t = (tau0 + t)^(-kappa) in fp64 on the host; c0 = fp32(1 - rho_t), c1 = fp32(rho_t M / M_b), each rounded once.
 *   3. Recentre, then blend.  With a = lbar - M m_ref and d = m_ref - mu (before lbar moves): C' = Cbar + a d^T + d a^T + M d d^T, the exact scatter
 *      of the same weighted population about mu, in fp64; Cbar <- c0 C' + c1 C_b (fp64, rounded once), Sbar <- c0 Sbar + c1 S_b,
 *      lbar <- c0 lbar + c1 l_b, vbar <- c0 vbar + c1 v_b (fp32), m_ref <- mu; the batch's statistics buffer is cleared.
 *   4. beta_old <- beta, beta <- Sbar row-normalised (update_beta!, src/CTM.jl:114-119); sigma <- (diag(vbar) + Cbar) / M and invsigma by the fp64
 *      inversion of update_sigma! (:108-111) -- about the PRE-step mu, the reference's order update_sigma! then update_mu! (:207-208) --; then
 *      mu <- lbar / M (update_mu!, :102-104).
 * With tau0 = 0 the first step has rho = 1, c0 = 0, c1 = M / M_b: with B = 1 it is exactly one iteration of train!.
 * Steps 3 and 4 are four launches on the context's stream (blend, normalise, tail, sigma / mu) without floating-point atomics and with a fixed
 * summation order: the same inputs give the same bits, run([a, b, c, d]) equals run([a, b]) then run([c, d]).  There is no random number in the
 * library: the host decides the order of the visits. */
typedef struct tmvb_ctm_svi tmvb_ctm_svi;
/* gpuCTM(corp, K) (src/gpuCTM.jl:6-99) over batches.  Corpus checks and error codes are tmvb_corpus_create's (src/Corpus.jl:41-50, :111-122); K limits are
 * tmvb_ctm_create's; cuts[B + 1] not strictly increasing from 0 to M -> TMVB_EINVAL.  Constructor state as tmvb_ctm_create (src/CTM.jl:37-48). */
int tmvb_ctm_svi_create(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts, int32_t K,
                        const int64_t* cuts, int32_t B, tmvb_ctm_svi** out);
int tmvb_ctm_svi_destroy(tmvb_ctm_svi* h);
/* update_buffer! / update_host! (src/modelutils.jl:400-435, :519-537) plus the running statistic and the step counter: mu[K], sigma / invsigma[K*K],
 * beta / beta_old / sbar[K*V] column-major, lambda / vsq[K*M] and logzeta[M] in corpus document order (lambda_old follows lambda), lbar / vbar / mref[K],
 * cbar[K*K], t[1].  NULL = leave / skip; beta without beta_old sets both; lbar, vbar, cbar and mref are set together or not at all (TMVB_EINVAL). */
int tmvb_ctm_svi_set_state(tmvb_ctm_svi* h, const double* mu, const double* sigma, const double* invsigma, const double* beta, const double* beta_old,
                           const double* lambda, const double* vsq, const double* logzeta, const double* sbar, const double* lbar, const double* vbar,
                           const double* cbar, const double* mref, const int64_t* t);
int tmvb_ctm_svi_get_state(tmvb_ctm_svi* h, double* mu, double* sigma, double* invsigma, double* beta, double* beta_old, double* lambda, double* vsq,
                           double* logzeta, double* sbar, double* lbar, double* vbar, double* cbar, double* mref, int64_t* t);
/* tau0 < 0 or not finite, kappa outside (0.5, 1] -> TMVB_EINVAL (no reference operator: the schedule of the section's head) */
int tmvb_ctm_svi_set_schedule(tmvb_ctm_svi* h, double tau0, double kappa);
/* n steps of train!'s loop body (src/CTM.jl:194-208) on the batches batches[0 .. n), repeats allowed.  Asynchronous on the context's stream.  A batch id
 * outside [0, B) -> TMVB_EINVAL before anything is enqueued. */
int tmvb_ctm_svi_run(tmvb_ctm_svi* h, const int32_t* batches, int64_t n, int32_t niter, double ntol, int32_t viter, double vtol);
/* The E-step of every batch under the final mu, sigma, beta (src/CTM.jl:194-205); the globals and the running statistic are not touched.  Afterwards lambda,
 * vsq and logzeta of all documents belong to the returned model.  Asynchronous. */
int tmvb_ctm_svi_final_pass(tmvb_ctm_svi* h, int32_t niter, double ntol, int32_t viter, double vtol);
/* rho, c0, c1: of the last step (NaN before the first); the bookkeeping of train!'s loop counter (src/CTM.jl:193) */
typedef struct { int32_t B, K; int64_t M, V, t; double tau0, kappa, rho; float c0, c1; } tmvb_ctm_svi_info_t;
int tmvb_ctm_svi_info(tmvb_ctm_svi* h, tmvb_ctm_svi_info_t* out);
/* as tmvb_ctm_doc_sweeps (the sweep loop of src/CTM.jl:196-204): out[M], each document's sweeps in the last E-step of ITS batch */
int tmvb_ctm_svi_doc_sweeps(tmvb_ctm_svi* h, uint8_t* out);
/* Timing of the last tmvb_ctm_svi_run from HIP events on the context's stream, like tmvb_ctm_last_estep_ms (TMVB_ESTEP_TIMING=1 at create): the sums over its
 * *steps steps of the E-step (src/CTM.jl:194-205), the fused update (blend + normalise + tail) and update_sigma! + update_mu! (:207-208), in ms. */
int tmvb_ctm_svi_last_run_ms(tmvb_ctm_svi* h, float* ms_estep, float* ms_update, float* ms_sigma_mu, int64_t* steps);

/* ============================== compare topics: divergences, assignment, relevant terms ==============================
 * The topic side of a trained model (the reference has no such functions): how far apart are the rows of one or two K x V topic-word matrices
 * (near-duplicate topics, matching the topics of two runs: gensim's LdaModel.diff), and which terms say what a topic is about (the relevance
 * ranking of LDAvis, Sievert & Shirley 2014; distinctiveness and saliency of Chuang et al. 2012).
 *
 * ---- tmvb_topic_divergence.  a is column-major KA x V fp64 on the HOST, the layout of beta in tmvb_topic_order: row i is a[i + KA w].  b is
 * KB x V likewise, or NULL: then b = a and KB is ignored.  D[i KB + j] (row-major, fp64) is the divergence of row i of a from row j of b.
 * Arithmetic, all fp64, every operation rounded on its own (no fused multiply-add).  With p = a_iw, q = b_jw, s = p + q the term of w is
 *   TMVB_TD_JS         0.5 * (x + y),  x = p > 0 ? p * log((2 * p) / s) : 0,  y = q > 0 ? q * log((2 * q) / s) : 0;     D = max(0, sum)
 *   TMVB_TD_HELLINGER  0.5 * (d * d),  d = sqrt(p) - sqrt(q), the roots correctly rounded;                              D = sqrt(sum)
 *   TMVB_TD_TV         0.5 * |p - q|;                                                                                   D = sum
 *   TMVB_TD_KL         p' > 0 ? p' * log(p' / q') : 0,  p' = (p + smooth) / (1 + (double)V * smooth), q' likewise; the term is +inf where
 *                      q' = 0 < p';                                                                                      D = max(0, sum)
 * log is the device's fp64 logarithm (within 1 ulp, log(1) = 0 exactly); smooth must be 0 for the other three metrics.
 * Order of every sum: the terms are cut into runs of TMVB_TD_RUN consecutive w, ascending; each run is summed sequentially ascending from 0;
 * the run sums are added sequentially ascending from 0.
 * Purity: the result is a pure function of the inputs.  It does not depend on `splits` (0 = the library's choice: the runs are cut into groups
 * of whole runs only when there are too few pair tiles to fill the device; > 0 forces that many groups, for tests), on tile sizes or on the order
 * in which workgroups finish; two calls give the same bytes; rows [i0, i1) of a call equal the call on that slice of a.  No floating-point
 * atomics.  Bit for bit: D(i, j) = 0 when the two rows are equal ((2 p) / (p + p) is exactly 1); for JS, HELLINGER and TV D[i][j] of (a, b)
 * equals D[j][i] of (b, a), and with b == NULL their matrix is symmetric (tiles below the diagonal are mirrored, not computed).
 * Device path: a prep kernel transposes each operand to row-major rows padded with zeros to whole runs (HELLINGER: sqrt, KL: the smoothing,
 * once per element); the pair kernel is register-tiled like a GEMM -- a workgroup owns 32 x 32 pairs and a group of whole runs, stages the two
 * row panels through LDS (fp64, padded rows, one 16-byte load per lane), each thread keeps 2 x 2 pair sums in registers and walks the run in
 * ascending w --; with more than one group it stores one sum per run and a merge kernel adds them in order.
 * info (or NULL): splits = groups used, runs, ms_prep / ms_pairs / ms_merge = device time of the kernels (HIP events around the kernels only).
 * Errors, judged before the device is touched: KA or KB outside [1, TMVB_TD_KMAX], V <= 0, KA V or KB V >= 2^31, an unknown metric, splits < 0
 * or greater than the number of runs, smooth negative or not finite or nonzero for a metric other than KL, a or D NULL -> TMVB_EINVAL; a
 * non-finite or negative entry, a row sum off 1 by more than 1e-6 -> TMVB_ESHAPE; then ctx == NULL without a visible device ->
 * TMVB_ENODEVICE (there is no CPU path).
 *
 * ---- tmvb_term_relevance.  beta K x V as above, pw[V] the marginal term probabilities, pi[K] the topic shares, lambda in [0, 1], 1 <= n <= V.
 * r(k, w) = lambda * log(phi) + (1 - lambda) * log(phi / p_w) with phi = beta_kw, fp64, every operation rounded on its own; -inf where phi = 0
 * or p_w = 0.  Per topic the n best terms under the total order (score descending, term id ascending on equal scores): idx[K][n] (0-based),
 * score[K][n], count[k] = min(n, number of terms with a finite score); slots past count[k] hold -1 and -inf.  dense (or NULL) receives all
 * K x V scores, row-major.  The selection is the stable descending segmented radix sort that tmvb_topic_order sorts with.
 * Per term, when distinct and saliency are given (both or neither): den = sum_j pi_j beta_jw over j ascending from 0; P(k|w) = (pi_k beta_kw) /
 * den; distinct[w] = sum_k (P > 0 ? P * log(P / pi_k) : 0) over k ascending from 0; saliency[w] = p_w * distinct[w]; both 0 where den = 0.
 * info (or NULL): ms_score / ms_select / ms_terms = device time of the score kernel, the sort with the selection, and the per-term kernel.
 * Errors, judged before the device is touched: K outside [1, TMVB_TD_KMAX], V <= 0, K V >= 2^31, lambda outside [0, 1] or not finite, n outside
 * [1, V], a NULL required argument (everything but dense, distinct, saliency and info), only one of distinct and saliency -> TMVB_EINVAL; a
 * non-finite or negative entry of beta, pw or pi, a row sum of beta, or the sum of pw or of pi, off 1 by more than 1e-6 -> TMVB_ESHAPE; then
 * ctx == NULL without a visible device -> TMVB_ENODEVICE.
 *
 * ---- tmvb_assignment.  Host only.  cost is row-major n x m, n <= m <= TMVB_TD_KMAX, entries finite or +inf.  A minimum-cost assignment of
 * every row to a column of its own by shortest augmenting paths, O(n^2 m): row_to_col[n] (0-based), *total (or NULL) = the sum of the chosen
 * costs over the rows ascending.  n < 1, n > m, m > TMVB_TD_KMAX, a NULL cost or row_to_col -> TMVB_EINVAL; a NaN or -inf cost, or no
 * assignment of finite cost -> TMVB_ESHAPE. */
#define TMVB_TD_JS 0                                        /* Jensen-Shannon divergence, nats, in [0, ln 2] */
#define TMVB_TD_HELLINGER 1                                 /* Hellinger distance, in [0, 1] */
#define TMVB_TD_TV 2                                        /* total variation, in [0, 1] */
#define TMVB_TD_KL 3                                        /* KL(a_i || b_j), directed, may be +inf */
#define TMVB_TD_RUN 256                                     /* terms per fixed-order partial sum */
#define TMVB_TD_KMAX 4096
typedef struct { int32_t splits, runs; float ms_prep, ms_pairs, ms_merge; } tmvb_topicdiv_info_t;
int tmvb_topic_divergence(tmvb_ctx* ctx, int32_t metric, int64_t V, int32_t KA, const double* a, int32_t KB, const double* b,
                          double smooth, int32_t splits, double* D, tmvb_topicdiv_info_t* info);
typedef struct { float ms_score, ms_select, ms_terms; } tmvb_relevance_info_t;
int tmvb_term_relevance(tmvb_ctx* ctx, int32_t K, int64_t V, const double* beta, const double* pw, const double* pi, double lambda,
                        int32_t n, int32_t* idx, double* score, int32_t* count, double* dense, double* distinct, double* saliency,
                        tmvb_relevance_info_t* info);
int tmvb_assignment(int32_t n, int32_t m, const double* cost, int32_t* row_to_col, double* total);

/* ============================== topics by group and over time: grouped word-topic statistics ==============================
 * How the topics differ between parts of the corpus (years, journals, author classes, cluster labels): for every group g of documents the
 * sufficient statistics of the topic-word matrix restricted to g (the reference has no such function; topics_over_time / topics_per_class
 * elsewhere).  Stateless and family-agnostic like tmvb_token_topics, whose conventions apply: everything is on the HOST, A is K x M and B is
 * K x V, column-major fp64, nonnegative; the CSR is doc_ptr[M + 1], terms, counts (ids in any order, repeats inside a document legal).
 *
 * ---- tmvb_group_topics.  group[d] in [0, G) names the group of document d, -1 leaves the document out.
 * Responsibilities: r_k of an entry (w, c) of document d are EXACTLY those of tmvb_token_topics: A, B and eps rounded once to fp32,
 * y_k = fma(A[k, d], B[k, w], eps), the sum in that function's fixed order, r_k = y_k / S the IEEE fp32 division (one device function serves both).
 * Index: the entries of the documents with group[d] >= 0, ordered by (group, term, document, position in the document); a RUN is the entries of
 * one (group, term).  tmvb_group_index returns exactly this order (np.lexsort on the four keys).
 * S_g[k, w] = the fp64 sum over the run's entries of (double)c * (double)r_k (the product is exact for c < 2^29).  Order: a run is cut into
 * segments of TMVB_GT_SEG consecutive entries; inside a segment entry i goes to slot i mod E, E = 64 / lanes_per_entry; a slot adds its
 * entries sequentially ascending from 0; the E slot sums meet in an xor butterfly over the slot number (distances 1, 2, 4, ...: a fixed tree);
 * the segment sums of a run are added sequentially in ascending order, starting from the first.  The order is a function of the inputs alone:
 * not of which workgroup finishes first, of max_chunk_groups or of the outputs asked for.  No floating-point atomics.
 * mass[g][k] = sum_w S_g[k, w]: lane t of 256 adds w = t, t + 256, ... ascending from 0, the 256 sums meet in a halving tree (t += t + 128,
 * then 64, ...).  tokens[g] = sum of c, docs[g] = documents with group[d] == g (empty ones included): exact integers.  sum_k mass[g][k] equals
 * tokens[g] up to rounding; the prevalence of topic k in g is mass[g][k] / sum_j mass[g][j], the caller's to compute.
 * top_idx[g][k][n], top_p[g][k][n]: with beta_g[k, w] = S_g[k, w] / mass[g][k] the n best terms of the row under the total order (p descending,
 * term id ascending on equal p) and their p; the stable descending segmented radix sort of tmvb_term_relevance, chunk_groups K segments of V.
 * A row with mass 0 -- every row of a group without entries -- gets -1 and 0 in every slot.
 * shift[g][k] = the Jensen-Shannon divergence (nats; the addend and the clamp of TMVB_TD_JS) of beta_g[k, .] from the pooled row
 * pooled[k, .] = (sum_g S_g[k, .] added in ascending g from 0) / its row sum (the order of mass).  drift[g][k] = the same divergence from
 * beta_g'[k, .], g' the nearest lower group id that has entries; 0 for the first group with entries.  Both are 0 for a group without entries.
 * The sum over w runs in the order of mass.  shift and drift may be NULL, together or singly.  dense (or NULL) receives every S_g, [G][K][V].
 * max_chunk_groups bounds the groups whose K x V fp64 blocks are on the device at once; 0 = the library's choice: as many as keep that buffer
 * at 256 MiB and chunk_groups K V < 2^31 (the sort).  EVERY output is bit-identical for every value of it, over calls, and with or without
 * dense, shift or drift.  (With more than one chunk and shift asked for, the statistics are accumulated twice: the pooled row needs every group.)
 * S, mass, tokens and docs are additive over document shards (up to the rounding of the fp64 sums); the selection and the divergences are not.
 * info (or NULL): nsel = selected entries, runs, segments = work items of the accumulation kernel, group_chunks, lanes_per_entry, ms_index =
 * host time of the index build, ms_accum / ms_select / ms_shift = device time of the accumulation with its combine and row sums, of the
 * normalisation, sort and selection, and of the pooled row with both divergences (HIP events around the kernels only).
 * Errors, judged before the device is touched -> TMVB_EINVAL: K outside [1, 1024], G outside [1, 65536], eps outside [2^-100, 1] or NaN, M <= 0
 * or V <= 0 (or 2^31 - 1 and more), n outside [1, min(V, 64)], K V >= 2^31, a NULL required argument (everything but shift, drift, dense and
 * info), max_chunk_groups < 0; then the data: a doc_ptr that does not start at 0 or decreases, 2^31 - 2 or more entries, a term outside
 * [0, V), a count < 1 or >= 2^29, a group id outside [-1, G), a negative, NaN or beyond-fp32 value of B or of a selected column of A.  Then
 * ctx == NULL without a visible device -> TMVB_ENODEVICE (there is no CPU path).
 *
 * ---- tmvb_group_index.  HOST ONLY, touches no device (like tmvb_digamma_f64): the index the kernel walks, by two stable counting sorts (by
 * term, then by group) on at most 16 host threads.  *n_runs runs; run u is entries run_ptr[u] .. run_ptr[u + 1] - 1 of entry[], of group
 * run_group[u] and term run_term[u]; entry[i] is a position in the CSR.  The caller sizes run_ptr for nsel + 1 and run_group / run_term for nsel
 * elements (the worst case: every entry a run of its own), entry for nsel.  M <= 0, V <= 0, G outside [1, 65536], a NULL argument, a bad CSR,
 * a term outside [0, V), a group id outside [-1, G) -> TMVB_EINVAL. */
#ifndef TMVB_GT_SEG
#define TMVB_GT_SEG 512                                     /* entries per segment of a run: one wave adds up a segment */
#endif
#define TMVB_GT_TOP_MAX 64
#define TMVB_GT_GMAX 65536
typedef struct { int64_t nsel, runs, segments; int32_t group_chunks, lanes_per_entry; float ms_index, ms_accum, ms_select, ms_shift; } tmvb_group_topics_info_t;
int tmvb_group_topics(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t M, const double* A, const double* B, const int64_t* doc_ptr,
                      const int32_t* terms, const int32_t* counts, const int32_t* group, int32_t G, double eps, int32_t n,
                      int32_t max_chunk_groups, int64_t* docs, int64_t* tokens, double* mass, int32_t* top_idx, double* top_p,
                      double* shift, double* drift, double* dense, tmvb_group_topics_info_t* info);
int tmvb_group_index(int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* group, int32_t G,
                     int64_t* n_runs, int64_t* run_ptr, int32_t* run_group, int32_t* run_term, int64_t* entry);

#ifdef __cplusplus
}
#endif
#endif /* TMVB_H */
