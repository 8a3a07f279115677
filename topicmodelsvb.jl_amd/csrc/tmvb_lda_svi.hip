// tmvb_lda_svi.hip -- stochastic (minibatch) training for LDA: stepwise EM on the device (include/tmvb.h states the algorithm; the reference
// trains on the whole corpus only, src/LDA.jl:161-187; the closest precedent is the v0.6 batch accumulation, v0.6/src/gpuLDA.jl:200-225).
//
// The driver owns B batch handles (tmvb_lda over the contiguous document slices [cuts[b], cuts[b + 1])), the sharded arrangement of one process:
// every handle is `distributed` with M_total = M, its statistics are bound to ONE buffer of the driver ([S_b | e_b], tmvb_lda_bind_stats), and the
// handles after the first read the first one's alpha / beta pair and fork onto its auxiliary streams (tmvb_lda_share_globals).  Per-document state
// (gamma, Elogtheta, the E rows) stays with the handle of the document's batch.  Device footprint: the corpus's per-document state once, plus
// 2 KP V (beta pair) + 2 (K V + K) (batch statistics, running statistic) floats, plus the per-handle constants.
//
// One step on batch b:   tmvb_lda_estep(h_b) ; tmvb_lda_reduce_docs(h_b)            the existing E-step, unchanged: [S_b | e_b]
//                        svi_blend_kernel                                          Sbar = c0 Sbar + c1 S_b, S_b = 0, per-block partial row sums;
//                                                                                  Ebar = c0 Ebar + c1 e_b (block 0), copied to the tail of the batch buffer
//                        svi_norm_kernel                                           row sums from the partials (fixed order), beta_new = Sbar / rowsum into the
//                                                                                  other buffer of the pair; the pair flips (beta_old <- beta)
//                        tmvb_lda_update_alpha(h_b)                                the existing fp64 Newton, reading the tail (= Ebar) with M_total = M
// The two kernels live in tmvb_svi_kernels.h, which the CTM driver (tmvb_ctm_svi.hip) includes too.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "tmvb_internal.h"
#include "tmvb_handle.h"
#include "tmvb_common_kernels.h"
#include "tmvb_svi_kernels.h"

struct tmvb_lda_svi {
    tmvb_ctx* ctx = nullptr;
    int K = 0, KP = 0, B = 0;
    int64_t M = 0, V = 0, sum_counts = 0;
    std::vector<int64_t> cuts;
    std::vector<tmvb_corpus*> corps;
    std::vector<tmvb_lda*> hs;
    float* d_sb = nullptr;             // [K V + K] the batch's statistics [S_b | e_b], bound to every batch handle
    float* d_sbar = nullptr;           // [K V] running statistic, scaled to the whole corpus
    float* d_ebar = nullptr;           // [K] its tail
    double* d_partial = nullptr;       // [SVI_BLEND_BLOCKS (at least ceil(K / 256))][K]
    float* d_beta[2] = {nullptr, nullptr};   // the first batch handle's pair
    int cur = 0;
    bool sbar_set = false, ebar_set = false;
    int64_t t = 0;
    double tau0 = 1.0, kappa = 0.7, rho = NAN;
    float c0 = NAN, c1 = NAN;
    bool timing = false;               // TMVB_ESTEP_TIMING=1 at create: four events per step of the last run
    std::vector<hipEvent_t> ev;
    int64_t timed_steps = 0;
    tmvb_owned mem;                    // the driver's own buffers and events (tmvb_handle.h)
};

extern "C" int tmvb_lda_svi_destroy(tmvb_lda_svi* h)
{
    if (!h) return TMVB_OK;
    if (h->ctx) { (void)hipSetDevice(h->ctx->device); (void)hipStreamSynchronize(h->ctx->stream); }
    for (size_t b = h->hs.size(); b-- > 0;) (void)tmvb_lda_destroy(h->hs[b]);          // the first handle owns what the others share: last
    for (tmvb_corpus* c : h->corps) (void)tmvb_corpus_destroy(c);
    if (h->ctx) h->mem.release(h->ctx->device, h->ctx->stream);
    delete h;
    return TMVB_OK;
}

extern "C" int tmvb_lda_svi_create(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts, int32_t K,
                                   const int64_t* cuts, int32_t B, tmvb_lda_svi** out)
{
    TMVB_REQUIRE(out != nullptr, TMVB_EINVAL, "tmvb_lda_svi_create: out is NULL");
    *out = nullptr;
    TMVB_REQUIRE(ctx != nullptr, TMVB_EINVAL, "tmvb_lda_svi_create: ctx is NULL");
    TMVB_REQUIRE(K > 0, TMVB_EINVAL, "number of topics must be a positive integer.");
    TMVB_REQUIRE(cuts != nullptr && B >= 1, TMVB_EINVAL, "tmvb_lda_svi_create: at least one batch is needed");
    TMVB_REQUIRE(cuts[0] == 0 && cuts[B] == M, TMVB_EINVAL, "tmvb_lda_svi_create: the batch cuts must run from 0 to M");
    for (int b = 0; b < B; ++b) TMVB_REQUIRE(cuts[b] < cuts[b + 1], TMVB_EINVAL, "tmvb_lda_svi_create: the batch cuts must be strictly increasing (batch %d is empty)", b);
    TMVB_HIP(hipSetDevice(ctx->device));
    int rc;
    {   // the corpus as a whole: tmvb_corpus_create's checks and error codes, and the token count of the initial statistic
        tmvb_corpus* whole = nullptr;
        if ((rc = tmvb_corpus_create(ctx, M, V, 0, doc_ptr, terms, counts, nullptr, nullptr, nullptr, &whole))) return rc;
        tmvb_corpus_info_t info;
        rc = tmvb_corpus_info(whole, &info);
        (void)tmvb_corpus_destroy(whole);
        if (rc) return rc;
        TMVB_REQUIRE(V > 0, TMVB_EINVAL, "tmvb_lda_svi_create: V must be positive");
        tmvb_lda_svi* h = new tmvb_lda_svi();
        tmvb_create_guard<tmvb_lda_svi, tmvb_lda_svi_destroy> guard{h};
        h->ctx = ctx; h->K = K; h->B = B; h->M = M; h->V = V; h->sum_counts = info.sum_counts;
        h->cuts.assign(cuts, cuts + B + 1);
        const size_t KV = (size_t)K * (size_t)V;
        const size_t nbmax = std::max<size_t>(SVI_BLEND_BLOCKS, ((size_t)K + SVI_WG - 1) / SVI_WG);
        if ((rc = h->mem.alloc(&h->d_sb, KV + K)) || (rc = h->mem.alloc(&h->d_sbar, KV)) || (rc = h->mem.alloc(&h->d_ebar, (size_t)K)) || (rc = h->mem.alloc(&h->d_partial, nbmax * K))) return rc;
        TMVB_HIP(hipMemsetAsync(h->d_sb, 0, (KV + K) * sizeof(float), ctx->stream));
        TMVB_HIP(hipMemsetAsync(h->d_sbar, 0, KV * sizeof(float), ctx->stream));
        TMVB_HIP(hipMemsetAsync(h->d_ebar, 0, (size_t)K * sizeof(float), ctx->stream));
        TMVB_HIP(hipStreamSynchronize(ctx->stream));
        std::vector<int64_t> ptr;
        for (int b = 0; b < B; ++b) {
            const int64_t d0 = cuts[b], d1 = cuts[b + 1], off = doc_ptr[d0];
            ptr.resize((size_t)(d1 - d0) + 1);
            for (int64_t d = d0; d <= d1; ++d) ptr[(size_t)(d - d0)] = doc_ptr[d] - off;
            tmvb_corpus* c = nullptr;
            if ((rc = tmvb_corpus_create(ctx, d1 - d0, V, 0, ptr.data(), terms + off, counts + off, nullptr, nullptr, nullptr, &c))) return rc;
            h->corps.push_back(c);
            tmvb_lda* lh = nullptr;
            if ((rc = tmvb_lda_create(ctx, c, K, &lh))) return rc;
            h->hs.push_back(lh);
            if (b > 0 && (rc = tmvb_lda_share_globals(lh, h->hs[0]))) return rc;
            if ((rc = tmvb_lda_bind_stats(lh, h->d_sb, (int64_t)(KV + K)))) return rc;
            if ((rc = tmvb_lda_set_distributed(lh, M, 1))) return rc;
        }
        tmvb_lda_globals_view gv;
        if ((rc = tmvb_lda_globals_view_of(h->hs[0], &gv))) return rc;
        h->d_beta[0] = gv.beta[0]; h->d_beta[1] = gv.beta[1]; h->cur = gv.cur; h->KP = gv.KP;
        h->timing = tmvb_env_on("TMVB_ESTEP_TIMING", false);
        guard.release();
        *out = h;
    }
    return TMVB_OK;
}

// the initial statistic (include/tmvb.h): Sbar_0 = (sum counts / K) beta_0, Ebar_0 = sum_d Elogtheta_0[:, d]; from the host values when the caller
// just handed them in, else from the device state
static int svi_ensure_stat(tmvb_lda_svi* h, const double* beta, const double* Elogtheta)
{
    const size_t K = (size_t)h->K, KV = K * (size_t)h->V, KM = K * (size_t)h->M;
    int rc;
    if (!h->sbar_set) {
        std::vector<double> b;
        if (!beta) {
            b.resize(KV);
            if ((rc = tmvb_lda_set_cur(h->hs[0], h->cur)) || (rc = tmvb_lda_get_state(h->hs[0], nullptr, b.data(), nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
            beta = b.data();
        }
        const double scale = (double)h->sum_counts / (double)h->K;
        std::vector<double> s(KV);
        for (size_t q = 0; q < KV; ++q) s[q] = scale * beta[q];
        if ((rc = upload_f32(h->ctx, h->d_sbar, s.data(), KV))) return rc;
        h->sbar_set = true;
    }
    if (!h->ebar_set) {
        std::vector<double> e;
        if (!Elogtheta) {
            e.resize(KM);
            for (int b = 0; b < h->B; ++b)
                if ((rc = tmvb_lda_get_state(h->hs[(size_t)b], nullptr, nullptr, nullptr, nullptr, e.data() + K * (size_t)h->cuts[(size_t)b], nullptr, nullptr))) return rc;
            Elogtheta = e.data();
        }
        std::vector<double> s(K, 0.0);
        for (int64_t d = 0; d < h->M; ++d)
            for (size_t i = 0; i < K; ++i) s[i] += Elogtheta[(size_t)d * K + i];
        if ((rc = upload_f32(h->ctx, h->d_ebar, s.data(), K))) return rc;
        h->ebar_set = true;
    }
    return TMVB_OK;
}

extern "C" int tmvb_lda_svi_set_state(tmvb_lda_svi* h, const double* alpha, const double* beta, const double* beta_old, const double* gamma,
                                      const double* Elogtheta, const double* sbar, const double* ebar, const int64_t* t)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_lda_svi_set_state: handle is NULL");
    TMVB_REQUIRE(!t || *t >= 0, TMVB_EINVAL, "tmvb_lda_svi_set_state: the step counter must be nonnegative");
    TMVB_HIP(hipSetDevice(h->ctx->device));
    const size_t K = (size_t)h->K, KV = K * (size_t)h->V;
    int rc;
    if ((rc = tmvb_lda_set_cur(h->hs[0], h->cur))) return rc;
    if ((alpha || beta || beta_old) && (rc = tmvb_lda_set_state(h->hs[0], alpha, beta, beta_old, nullptr, nullptr, nullptr, nullptr))) return rc;
    if (gamma || Elogtheta)
        for (int b = 0; b < h->B; ++b) {
            const size_t off = K * (size_t)h->cuts[(size_t)b];
            if ((rc = tmvb_lda_set_state(h->hs[(size_t)b], nullptr, nullptr, nullptr, gamma ? gamma + off : nullptr, Elogtheta ? Elogtheta + off : nullptr, nullptr, nullptr))) return rc;
        }
    if (sbar) {
        for (size_t q = 0; q < KV; ++q) TMVB_REQUIRE(std::isfinite(sbar[q]) && sbar[q] >= 0.0, TMVB_ENONFINITE, "the running statistic must be finite and nonnegative.");
        if ((rc = upload_f32(h->ctx, h->d_sbar, sbar, KV))) return rc;
        h->sbar_set = true;
    }
    if (ebar) {
        for (size_t i = 0; i < K; ++i) TMVB_REQUIRE(std::isfinite(ebar[i]), TMVB_ENONFINITE, "the running Elogtheta sum must be finite.");
        if ((rc = upload_f32(h->ctx, h->d_ebar, ebar, K))) return rc;
        h->ebar_set = true;
    }
    if (t) h->t = *t;
    return svi_ensure_stat(h, beta, Elogtheta);
}

extern "C" int tmvb_lda_svi_get_state(tmvb_lda_svi* h, double* alpha, double* beta, double* beta_old, double* gamma, double* Elogtheta, double* sbar,
                                      double* ebar, int64_t* t)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_lda_svi_get_state: handle is NULL");
    TMVB_HIP(hipSetDevice(h->ctx->device));
    const size_t K = (size_t)h->K, KV = K * (size_t)h->V;
    int rc;
    if ((rc = svi_ensure_stat(h, nullptr, nullptr))) return rc;
    if ((rc = tmvb_lda_set_cur(h->hs[0], h->cur))) return rc;
    if ((alpha || beta || beta_old) && (rc = tmvb_lda_get_state(h->hs[0], alpha, beta, beta_old, nullptr, nullptr, nullptr, nullptr))) return rc;
    if (gamma || Elogtheta)
        for (int b = 0; b < h->B; ++b) {
            const size_t off = K * (size_t)h->cuts[(size_t)b];
            if ((rc = tmvb_lda_get_state(h->hs[(size_t)b], nullptr, nullptr, nullptr, gamma ? gamma + off : nullptr, Elogtheta ? Elogtheta + off : nullptr, nullptr, nullptr))) return rc;
        }
    if (sbar && (rc = download_f32(h->ctx, sbar, h->d_sbar, KV))) return rc;
    if (ebar && (rc = download_f32(h->ctx, ebar, h->d_ebar, K))) return rc;
    if (!sbar && !ebar) TMVB_HIP(hipStreamSynchronize(h->ctx->stream));
    if (t) *t = h->t;
    return TMVB_OK;
}

extern "C" int tmvb_lda_svi_set_schedule(tmvb_lda_svi* h, double tau0, double kappa)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_lda_svi_set_schedule: handle is NULL");
    TMVB_REQUIRE(std::isfinite(tau0) && tau0 >= 0.0, TMVB_EINVAL, "tau0 parameter must be nonnegative.");
    TMVB_REQUIRE(kappa > 0.5 && kappa <= 1.0, TMVB_EINVAL, "kappa parameter must be in (0.5, 1].");
    h->tau0 = tau0; h->kappa = kappa;
    return TMVB_OK;
}

// the fused global update of one step, on the context's stream, behind the batch's E-step and the join of its side chain
static int svi_global_update(tmvb_lda_svi* h, float c0, float c1)
{
    const int64_t n = (int64_t)h->K * h->V;
    int rc = svi_launch_blend_norm(h->ctx->stream, h->d_sbar, h->d_sb, h->K, h->KP, h->V, c0, c1, h->d_partial, h->d_ebar, h->d_sb + n, h->d_beta[h->cur ^ 1]);
    if (rc) return rc;
    h->cur ^= 1;                                                   // beta_old <- beta, beta <- new   (src/LDA.jl:122-123)
    return TMVB_OK;
}

extern "C" int tmvb_lda_svi_run(tmvb_lda_svi* h, const int32_t* batches, int64_t n, int32_t niter, double ntol, int32_t viter, double vtol)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_lda_svi_run: handle is NULL");
    TMVB_REQUIRE(n >= 0 && (batches != nullptr || n == 0), TMVB_EINVAL, "tmvb_lda_svi_run: bad batch list");
    TMVB_REQUIRE(ntol >= 0 && vtol >= 0, TMVB_EINVAL, "tolerance parameters must be nonnegative.");      // src/gpuLDA.jl:349
    TMVB_REQUIRE(niter >= 0 && viter >= 0, TMVB_EINVAL, "iteration parameters must be nonnegative.");    // src/gpuLDA.jl:350
    for (int64_t s = 0; s < n; ++s) TMVB_REQUIRE(batches[s] >= 0 && batches[s] < h->B, TMVB_EINVAL, "tmvb_lda_svi_run: batch id %d outside [0, %d)", batches[s], h->B);
    TMVB_HIP(hipSetDevice(h->ctx->device));
    int rc;
    if ((rc = svi_ensure_stat(h, nullptr, nullptr))) return rc;
    hipStream_t st = h->ctx->stream;
    if (h->timing) {
        while ((int64_t)h->ev.size() < 4 * n) {
            hipEvent_t e = nullptr;
            if ((rc = h->mem.event(&e, hipEventDisableSystemFence))) return rc;
            h->ev.push_back(e);
        }
        h->timed_steps = 0;
    }
    for (int64_t s = 0; s < n; ++s) {
        const int b = batches[s];
        tmvb_lda* lh = h->hs[(size_t)b];
        const int64_t Mb = h->cuts[(size_t)b + 1] - h->cuts[(size_t)b];
        const double rho = std::pow(h->tau0 + (double)(h->t + 1), -h->kappa);
        const float c0 = (float)(1.0 - rho), c1 = (float)(rho * (double)h->M / (double)Mb);
        if (h->timing) TMVB_HIP(hipEventRecord(h->ev[(size_t)(4 * s)], st));
        if ((rc = tmvb_lda_set_cur(lh, h->cur))) return rc;
        if ((rc = tmvb_lda_estep(lh, viter, vtol))) return rc;                       // src/LDA.jl:170-180 on the batch's documents
        if ((rc = tmvb_lda_reduce_docs(lh))) return rc;                             // :98 -- e_b in the tail; the context's stream has joined the side chain
        if (h->timing) TMVB_HIP(hipEventRecord(h->ev[(size_t)(4 * s + 1)], st));
        if ((rc = svi_global_update(h, c0, c1))) return rc;                         // :181 on the running statistic
        if (h->timing) TMVB_HIP(hipEventRecord(h->ev[(size_t)(4 * s + 2)], st));
        if ((rc = tmvb_lda_update_alpha(lh, niter, ntol))) return rc;               // :182, Elogtheta_sum = Ebar, M_total = M
        if ((rc = tmvb_lda_set_cur(lh, h->cur))) return rc;                         // the context's stream waits for the new alpha: the next batch's handle reads it
        if (h->timing) { TMVB_HIP(hipEventRecord(h->ev[(size_t)(4 * s + 3)], st)); h->timed_steps = s + 1; }
        h->t += 1; h->rho = rho; h->c0 = c0; h->c1 = c1;
    }
    return TMVB_OK;
}

extern "C" int tmvb_lda_svi_final_pass(tmvb_lda_svi* h, int32_t viter, double vtol)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_lda_svi_final_pass: handle is NULL");
    TMVB_REQUIRE(vtol >= 0, TMVB_EINVAL, "tolerance parameters must be nonnegative.");
    TMVB_REQUIRE(viter >= 0, TMVB_EINVAL, "iteration parameters must be nonnegative.");
    TMVB_HIP(hipSetDevice(h->ctx->device));
    const size_t KV = (size_t)h->K * (size_t)h->V;
    int rc;
    for (int b = 0; b < h->B; ++b) {
        tmvb_lda* lh = h->hs[(size_t)b];
        if ((rc = tmvb_lda_set_cur(lh, h->cur))) return rc;
        if ((rc = tmvb_lda_estep(lh, viter, vtol))) return rc;
        if ((rc = tmvb_lda_reduce_docs(lh))) return rc;                             // joins the side chain, which writes the tail
        TMVB_HIP(hipMemsetAsync(h->d_sb, 0, KV * sizeof(float), h->ctx->stream));   // the globals stay: the batch's statistics are dropped
        if ((rc = tmvb_lda_set_cur(lh, h->cur))) return rc;
    }
    return TMVB_OK;
}

extern "C" int tmvb_lda_svi_info(tmvb_lda_svi* h, tmvb_lda_svi_info_t* out)
{
    TMVB_REQUIRE(h && out, TMVB_EINVAL, "tmvb_lda_svi_info: NULL argument");
    out->B = h->B; out->K = h->K; out->M = h->M; out->V = h->V; out->t = h->t;
    out->tau0 = h->tau0; out->kappa = h->kappa; out->rho = h->rho; out->c0 = h->c0; out->c1 = h->c1;
    return TMVB_OK;
}

extern "C" int tmvb_lda_svi_doc_sweeps(tmvb_lda_svi* h, uint8_t* out)
{
    TMVB_REQUIRE(h && out, TMVB_EINVAL, "tmvb_lda_svi_doc_sweeps: NULL argument");
    int rc;
    for (int b = 0; b < h->B; ++b)
        if ((rc = tmvb_lda_doc_sweeps(h->hs[(size_t)b], out + h->cuts[(size_t)b]))) return rc;
    return TMVB_OK;
}

extern "C" int tmvb_lda_svi_last_run_ms(tmvb_lda_svi* h, float* ms_estep, float* ms_update, float* ms_alpha, int64_t* steps)
{
    TMVB_REQUIRE(h && ms_estep && ms_update && ms_alpha && steps, TMVB_EINVAL, "tmvb_lda_svi_last_run_ms: NULL argument");
    TMVB_REQUIRE(h->timing, TMVB_EINVAL, "tmvb_lda_svi_last_run_ms: step timing is off (set TMVB_ESTEP_TIMING=1 before creating the model)");
    TMVB_HIP(hipSetDevice(h->ctx->device));
    double e = 0.0, u = 0.0, a = 0.0;
    for (int64_t s = 0; s < h->timed_steps; ++s) {
        float ms = 0.0f;
        TMVB_HIP(hipEventSynchronize(h->ev[(size_t)(4 * s + 3)]));
        TMVB_HIP(hipEventElapsedTime(&ms, h->ev[(size_t)(4 * s)], h->ev[(size_t)(4 * s + 1)])); e += ms;
        TMVB_HIP(hipEventElapsedTime(&ms, h->ev[(size_t)(4 * s + 1)], h->ev[(size_t)(4 * s + 2)])); u += ms;
        TMVB_HIP(hipEventElapsedTime(&ms, h->ev[(size_t)(4 * s + 2)], h->ev[(size_t)(4 * s + 3)])); a += ms;
    }
    *ms_estep = (float)e; *ms_update = (float)u; *ms_alpha = (float)a; *steps = h->timed_steps;
    return TMVB_OK;
}
