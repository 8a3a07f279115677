// tmvb_ctm_svi.hip -- stochastic (minibatch) training for CTM: stepwise EM on the device (include/tmvb.h states the algorithm; the reference trains on
// the whole corpus only, src/CTM.jl:185-217).
//
// The driver owns B batch handles (tmvb_ctm over the contiguous document slices [cuts[b], cuts[b + 1])), the sharded arrangement of one process: every
// handle is `distributed` with M_total = M -- which also switches the E-step's speculative update_sigma! off: a sigma of the BATCH tail is never staged, let
// alone committed --, its statistics are bound to ONE buffer of the driver ([S_b | l_b | v_b | C_b], tmvb_ctm_bind_stats), and the handles after the first
// read the first one's globals proper (tmvb_ctm_share_globals).  Per-document state (lambda, vsq, logzeta) stays with the handle of the document's batch.
// Device footprint: the corpus's per-document state once, plus 2 KP V (beta pair) + 2 K V (batch statistics, running statistic) + 3 T floats
// (T = 2 K + K^2: batch tail, the running tail twice) + 2 K doubles (m_ref twice), plus the per-handle constants and derived tables.
//
// One step on batch b:   tmvb_ctm_estep(h_b) ; tmvb_ctm_reduce_docs(h_b)            the existing E-step, unchanged: [S_b | l_b | v_b | C_b about mu]
//                        tmvb_ctm_stats(h_b)                                       the context's stream joins the handle's side streams
//                        svi_blend_kernel, svi_norm_kernel (tmvb_svi_kernels.h)    Sbar = c0 Sbar + c1 S_b, S_b = 0; beta_new = Sbar row-normalised; the pair flips
//                        ctm_svi_tail_kernel                                       the running tail moved to mu (fp64), blended, written to the other running
//                                                                                  buffer AND over the batch tail; m_ref <- mu
//                        ctm_sigma_mu_kernel (tmvb_ctm_sigma_mu_from_tail)         update_sigma! then update_mu! on the blended tail with M_total = M
//
// ctm_svi_tail_kernel.  T = 2 K + K^2 entries, one lane each, 256 per block (258 blocks at K = 256).  Entry (i, j) of the scatter matrix needs
// a_i, a_j (from lbar and m_ref) and d_i, d_j (from m_ref and mu): 4 K doubles that stay in L2.  The kernel reads the running buffers of this step and
// writes the OTHER pair (ping-pong), so no lane reads what another lane of the same launch writes; the batch tail is read and written by its own lane only.
// No atomics, no reduction: the same inputs give the same bits.  Bound: 4 T floats (two read, two written), 1.06 MB at K = 256 -- launch latency.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "tmvb_internal.h"
#include "tmvb_handle.h"
#include "tmvb_common_kernels.h"
#include "tmvb_svi_kernels.h"

// tbar_in / tbar_out: [lbar (K) | vbar (K) | Cbar (K x K)] the running tail of this step and of the next; tb: the batch's tail, overwritten with the blended
// values for ctm_sigma_mu_kernel; mref_in / mref_out: the vector the running scatter matrix is about; mu: the current (pre-step) mean
static __global__ __launch_bounds__(256) void ctm_svi_tail_kernel(int K, double Md, float c0, float c1, const float* __restrict__ tbar_in, float* __restrict__ tbar_out,
                                                                  float* __restrict__ tb, const double* __restrict__ mref_in, double* __restrict__ mref_out,
                                                                  const double* __restrict__ mu)
{
    const int n = 2 * K + K * K;
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= n) return;
    float r;
    if (q < 2 * K) {
        r = fmaf(c0, tbar_in[q], c1 * tb[q]);
        if (q < K) mref_out[q] = mu[q];
    } else {
        const int e = q - 2 * K, i = e / K, j = e - i * K;
        double c = (double)tbar_in[q];
#ifndef TMVB_MUTANT_CTM_SVI_NO_RECENTRE      // MUTANT (tests/test_ctm_svi_mutant_gpu.py, never in a shipped build): Cbar is blended about m_ref, not about mu
        // C' = Cbar + a d^T + d a^T + M d d^T with a = lbar - M m_ref, d = m_ref - mu; (i, j) and (j, i) evaluate the same expression
        const int lo = min(i, j), hi = max(i, j);
        const double ml = mref_in[lo], mh = mref_in[hi];
        const double dl = ml - mu[lo], dh = mh - mu[hi];
        const double al = (double)tbar_in[lo] - Md * ml, ah = (double)tbar_in[hi] - Md * mh;
        c += (al * dh + dl * ah) + Md * dl * dh;
#endif
        r = (float)((double)c0 * c + (double)c1 * (double)tb[q]);
    }
    tbar_out[q] = r;
    tb[q] = r;
}

struct tmvb_ctm_svi {
    tmvb_ctx* ctx = nullptr;
    int K = 0, KP = 0, B = 0;
    int64_t M = 0, V = 0, sum_counts = 0;
    std::vector<int64_t> cuts;
    std::vector<tmvb_corpus*> corps;
    std::vector<tmvb_ctm*> hs;
    float* d_sb = nullptr;             // [K V + T] the batch's statistics [S_b | l_b | v_b | C_b], bound to every batch handle
    float* d_sbar = nullptr;           // [K V] running statistic, scaled to the whole corpus
    float* d_tbar[2] = {nullptr, nullptr};     // [T] its tail [lbar | vbar | Cbar], this step's and the next one's
    double* d_mref[2] = {nullptr, nullptr};    // [K] the vector Cbar is about
    int tcur = 0;
    double* d_partial = nullptr;       // [SVI_BLEND_BLOCKS (at least ceil(K / 256))][K]
    float* d_beta[2] = {nullptr, nullptr};     // the first batch handle's pair
    double* d_mu = nullptr;            // ... and its fp64 mu
    int cur = 0;
    bool sbar_set = false, tail_set = false;
    int64_t t = 0;
    double tau0 = 1.0, kappa = 0.7, rho = NAN;
    float c0 = NAN, c1 = NAN;
    bool timing = false;               // TMVB_ESTEP_TIMING=1 at create: four events per step of the last run
    std::vector<hipEvent_t> ev;
    int64_t timed_steps = 0;
    tmvb_owned mem;                    // the driver's own buffers and events (tmvb_handle.h)
    size_t T() const { return 2 * (size_t)K + (size_t)K * (size_t)K; }
};

extern "C" int tmvb_ctm_svi_destroy(tmvb_ctm_svi* h)
{
    if (!h) return TMVB_OK;
    if (h->ctx) { (void)hipSetDevice(h->ctx->device); (void)hipDeviceSynchronize(); }       // the handles' side streams included
    for (size_t b = h->hs.size(); b-- > 0;) (void)tmvb_ctm_destroy(h->hs[b]);               // the first handle owns what the others share: last
    for (tmvb_corpus* c : h->corps) (void)tmvb_corpus_destroy(c);
    if (h->ctx) h->mem.release(h->ctx->device, h->ctx->stream);
    delete h;
    return TMVB_OK;
}

extern "C" int tmvb_ctm_svi_create(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts, int32_t K,
                                   const int64_t* cuts, int32_t B, tmvb_ctm_svi** out)
{
    TMVB_REQUIRE(out != nullptr, TMVB_EINVAL, "tmvb_ctm_svi_create: out is NULL");
    *out = nullptr;
    TMVB_REQUIRE(ctx != nullptr, TMVB_EINVAL, "tmvb_ctm_svi_create: ctx is NULL");
    TMVB_REQUIRE(K > 0, TMVB_EINVAL, "number of topics must be a positive integer.");
    TMVB_REQUIRE(cuts != nullptr && B >= 1, TMVB_EINVAL, "tmvb_ctm_svi_create: at least one batch is needed");
    TMVB_REQUIRE(cuts[0] == 0 && cuts[B] == M, TMVB_EINVAL, "tmvb_ctm_svi_create: the batch cuts must run from 0 to M");
    for (int b = 0; b < B; ++b) TMVB_REQUIRE(cuts[b] < cuts[b + 1], TMVB_EINVAL, "tmvb_ctm_svi_create: the batch cuts must be strictly increasing (batch %d is empty)", b);
    TMVB_HIP(hipSetDevice(ctx->device));
    int rc;
    tmvb_corpus* whole = nullptr;           // the corpus as a whole: tmvb_corpus_create's checks and error codes, and the token count of the initial statistic
    if ((rc = tmvb_corpus_create(ctx, M, V, 0, doc_ptr, terms, counts, nullptr, nullptr, nullptr, &whole))) return rc;
    tmvb_corpus_info_t info;
    rc = tmvb_corpus_info(whole, &info);
    (void)tmvb_corpus_destroy(whole);
    if (rc) return rc;
    TMVB_REQUIRE(V > 0, TMVB_EINVAL, "tmvb_ctm_svi_create: V must be positive");
    tmvb_ctm_svi* h = new tmvb_ctm_svi();
    tmvb_create_guard<tmvb_ctm_svi, tmvb_ctm_svi_destroy> guard{h};
    h->ctx = ctx; h->K = K; h->B = B; h->M = M; h->V = V; h->sum_counts = info.sum_counts;
    h->cuts.assign(cuts, cuts + B + 1);
    std::vector<int64_t> ptr;
    for (int b = 0; b < B; ++b) {           // (the first tmvb_ctm_create checks K <= 256 before the driver allocates K^2 anything)
        const int64_t d0 = cuts[b], d1 = cuts[b + 1], off = doc_ptr[d0];
        ptr.resize((size_t)(d1 - d0) + 1);
        for (int64_t d = d0; d <= d1; ++d) ptr[(size_t)(d - d0)] = doc_ptr[d] - off;
        tmvb_corpus* c = nullptr;
        if ((rc = tmvb_corpus_create(ctx, d1 - d0, V, 0, ptr.data(), terms + off, counts + off, nullptr, nullptr, nullptr, &c))) return rc;
        h->corps.push_back(c);
        tmvb_ctm* ch = nullptr;
        if ((rc = tmvb_ctm_create(ctx, c, K, &ch))) return rc;
        h->hs.push_back(ch);
        if (b > 0 && (rc = tmvb_ctm_share_globals(ch, h->hs[0]))) return rc;
    }
    const size_t KV = (size_t)K * (size_t)V, T = h->T();
    const size_t nbmax = std::max<size_t>(SVI_BLEND_BLOCKS, ((size_t)K + SVI_WG - 1) / SVI_WG);
    if ((rc = h->mem.alloc(&h->d_sb, KV + T)) || (rc = h->mem.alloc(&h->d_sbar, KV)) || (rc = h->mem.alloc(&h->d_tbar[0], T)) || (rc = h->mem.alloc(&h->d_tbar[1], T)) ||
        (rc = h->mem.alloc(&h->d_mref[0], (size_t)K)) || (rc = h->mem.alloc(&h->d_mref[1], (size_t)K)) || (rc = h->mem.alloc(&h->d_partial, nbmax * K))) return rc;
    TMVB_HIP(hipMemsetAsync(h->d_sb, 0, (KV + T) * sizeof(float), ctx->stream));
    TMVB_HIP(hipMemsetAsync(h->d_sbar, 0, KV * sizeof(float), ctx->stream));
    for (int q = 0; q < 2; ++q) {
        TMVB_HIP(hipMemsetAsync(h->d_tbar[q], 0, T * sizeof(float), ctx->stream));
        TMVB_HIP(hipMemsetAsync(h->d_mref[q], 0, (size_t)K * sizeof(double), ctx->stream));
    }
    TMVB_HIP(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < B; ++b) {
        if ((rc = tmvb_ctm_bind_stats(h->hs[(size_t)b], h->d_sb, (int64_t)(KV + T)))) return rc;
        if ((rc = tmvb_ctm_set_distributed(h->hs[(size_t)b], M, 1))) return rc;
    }
    TMVB_HIP(hipMemsetAsync(h->d_sb, 0, (KV + T) * sizeof(float), ctx->stream));
    TMVB_HIP(hipStreamSynchronize(ctx->stream));
    tmvb_ctm_globals_view gv;
    if ((rc = tmvb_ctm_globals_view_of(h->hs[0], &gv))) return rc;
    h->d_beta[0] = gv.beta[0]; h->d_beta[1] = gv.beta[1]; h->cur = gv.cur; h->KP = gv.KP; h->d_mu = gv.mu;
    h->timing = tmvb_env_on("TMVB_ESTEP_TIMING", false);
    guard.release();
    *out = h;
    return TMVB_OK;
}

// the initial statistic (include/tmvb.h): Sbar_0 = (sum counts / K) beta_0; lbar_0 = sum_d lambda_d, vbar_0 = sum_d vsq_d, Cbar_0 = sum_d (lambda_d - mu_0)
// (lambda_d - mu_0)^T and m_ref = mu_0, in fp64 on the host; from the host values when the caller just handed them in, else from the device state
static int ctm_svi_ensure_stat(tmvb_ctm_svi* h, const double* beta, const double* mu, const double* lambda, const double* vsq)
{
    const size_t K = (size_t)h->K, KV = K * (size_t)h->V, KM = K * (size_t)h->M, T = h->T();
    int rc;
    if (!h->sbar_set) {
        std::vector<double> b;
        if (!beta) {
            b.resize(KV);
            if ((rc = tmvb_ctm_set_cur(h->hs[0], h->cur)) ||
                (rc = tmvb_ctm_get_state(h->hs[0], nullptr, nullptr, nullptr, b.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
            beta = b.data();
        }
        const double scale = (double)h->sum_counts / (double)h->K;
        std::vector<double> s(KV);
        for (size_t q = 0; q < KV; ++q) s[q] = scale * beta[q];
        if ((rc = upload_f32(h->ctx, h->d_sbar, s.data(), KV))) return rc;
        h->sbar_set = true;
    }
    if (!h->tail_set) {
        std::vector<double> m, l, v;
        if (!mu) {
            m.resize(K);
            if ((rc = tmvb_ctm_get_state(h->hs[0], m.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
            mu = m.data();
        }
        if (!lambda || !vsq) {
            if (!lambda) l.resize(KM);
            if (!vsq) v.resize(KM);
            for (int b = 0; b < h->B; ++b) {
                const size_t off = K * (size_t)h->cuts[(size_t)b];
                if ((rc = tmvb_ctm_get_state(h->hs[(size_t)b], nullptr, nullptr, nullptr, nullptr, nullptr, lambda ? nullptr : l.data() + off, nullptr,
                                             vsq ? nullptr : v.data() + off, nullptr, nullptr))) return rc;
            }
            if (!lambda) lambda = l.data();
            if (!vsq) vsq = v.data();
        }
        std::vector<double> tail(T, 0.0), df(K);
        double* C = tail.data() + 2 * K;
        for (int64_t d = 0; d < h->M; ++d) {
            bool any = false;
            for (size_t i = 0; i < K; ++i) {
                tail[i] += lambda[(size_t)d * K + i];
                tail[K + i] += vsq[(size_t)d * K + i];
                df[i] = lambda[(size_t)d * K + i] - mu[i];
                any = any || df[i] != 0.0;
            }
            if (!any) continue;
            for (size_t i = 0; i < K; ++i)
                for (size_t j = i; j < K; ++j) C[i * K + j] += df[i] * df[j];
        }
        for (size_t i = 0; i < K; ++i)
            for (size_t j = 0; j < i; ++j) C[i * K + j] = C[j * K + i];
        if ((rc = upload_f32(h->ctx, h->d_tbar[h->tcur], tail.data(), T))) return rc;
        TMVB_HIP(hipMemcpyAsync(h->d_mref[h->tcur], mu, K * sizeof(double), hipMemcpyHostToDevice, h->ctx->stream));
        TMVB_HIP(hipStreamSynchronize(h->ctx->stream));
        h->tail_set = true;
    }
    return TMVB_OK;
}

extern "C" int tmvb_ctm_svi_set_state(tmvb_ctm_svi* h, const double* mu, const double* sigma, const double* invsigma, const double* beta, const double* beta_old,
                                      const double* lambda, const double* vsq, const double* logzeta, const double* sbar, const double* lbar,
                                      const double* vbar, const double* cbar, const double* mref, const int64_t* t)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_ctm_svi_set_state: handle is NULL");
    TMVB_REQUIRE(!t || *t >= 0, TMVB_EINVAL, "tmvb_ctm_svi_set_state: the step counter must be nonnegative");
    const bool any_tail = lbar || vbar || cbar || mref, all_tail = lbar && vbar && cbar && mref;
    TMVB_REQUIRE(!any_tail || all_tail, TMVB_EINVAL, "tmvb_ctm_svi_set_state: the running tail (lbar, vbar, cbar, mref) is set as a whole");
    TMVB_HIP(hipSetDevice(h->ctx->device));
    const size_t K = (size_t)h->K, KV = K * (size_t)h->V, T = h->T();
    int rc;
    if ((rc = tmvb_ctm_set_cur(h->hs[0], h->cur))) return rc;
    if ((mu || sigma || invsigma || beta || beta_old) &&
        (rc = tmvb_ctm_set_state(h->hs[0], mu, sigma, invsigma, beta, beta_old, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
    if (lambda || vsq || logzeta)
        for (int b = 0; b < h->B; ++b) {
            const size_t d0 = (size_t)h->cuts[(size_t)b], off = K * d0;
            if ((rc = tmvb_ctm_set_state(h->hs[(size_t)b], nullptr, nullptr, nullptr, nullptr, nullptr, lambda ? lambda + off : nullptr, nullptr,
                                         vsq ? vsq + off : nullptr, logzeta ? logzeta + d0 : nullptr, nullptr))) return rc;
        }
    if (sbar) {
        for (size_t q = 0; q < KV; ++q) TMVB_REQUIRE(std::isfinite(sbar[q]) && sbar[q] >= 0.0, TMVB_ENONFINITE, "the running statistic must be finite and nonnegative.");
        if ((rc = upload_f32(h->ctx, h->d_sbar, sbar, KV))) return rc;
        h->sbar_set = true;
    }
    if (all_tail) {
        for (size_t i = 0; i < K; ++i) TMVB_REQUIRE(std::isfinite(lbar[i]) && std::isfinite(vbar[i]) && std::isfinite(mref[i]), TMVB_ENONFINITE, "the running tail must be finite.");
        for (size_t q = 0; q < K * K; ++q) TMVB_REQUIRE(std::isfinite(cbar[q]), TMVB_ENONFINITE, "the running tail must be finite.");
        std::vector<double> tail(T);
        std::memcpy(tail.data(), lbar, K * sizeof(double));
        std::memcpy(tail.data() + K, vbar, K * sizeof(double));
        std::memcpy(tail.data() + 2 * K, cbar, K * K * sizeof(double));
        if ((rc = upload_f32(h->ctx, h->d_tbar[h->tcur], tail.data(), T))) return rc;
        TMVB_HIP(hipMemcpyAsync(h->d_mref[h->tcur], mref, K * sizeof(double), hipMemcpyHostToDevice, h->ctx->stream));
        TMVB_HIP(hipStreamSynchronize(h->ctx->stream));
        h->tail_set = true;
    }
    if (t) h->t = *t;
    return ctm_svi_ensure_stat(h, beta, mu, lambda, vsq);
}

extern "C" int tmvb_ctm_svi_get_state(tmvb_ctm_svi* h, double* mu, double* sigma, double* invsigma, double* beta, double* beta_old, double* lambda, double* vsq,
                                      double* logzeta, double* sbar, double* lbar, double* vbar, double* cbar, double* mref, int64_t* t)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_ctm_svi_get_state: handle is NULL");
    TMVB_HIP(hipSetDevice(h->ctx->device));
    const size_t K = (size_t)h->K, KV = K * (size_t)h->V, T = h->T();
    int rc;
    if ((rc = ctm_svi_ensure_stat(h, nullptr, nullptr, nullptr, nullptr))) return rc;
    if ((rc = tmvb_ctm_set_cur(h->hs[0], h->cur))) return rc;
    if ((mu || sigma || invsigma || beta || beta_old) &&
        (rc = tmvb_ctm_get_state(h->hs[0], mu, sigma, invsigma, beta, beta_old, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
    if (lambda || vsq || logzeta)
        for (int b = 0; b < h->B; ++b) {
            const size_t d0 = (size_t)h->cuts[(size_t)b], off = K * d0;
            if ((rc = tmvb_ctm_get_state(h->hs[(size_t)b], nullptr, nullptr, nullptr, nullptr, nullptr, lambda ? lambda + off : nullptr, nullptr,
                                         vsq ? vsq + off : nullptr, logzeta ? logzeta + d0 : nullptr, nullptr))) return rc;
        }
    if (sbar && (rc = download_f32(h->ctx, sbar, h->d_sbar, KV))) return rc;
    if (lbar || vbar || cbar) {
        std::vector<double> tail(T);
        if ((rc = download_f32(h->ctx, tail.data(), h->d_tbar[h->tcur], T))) return rc;
        if (lbar) std::memcpy(lbar, tail.data(), K * sizeof(double));
        if (vbar) std::memcpy(vbar, tail.data() + K, K * sizeof(double));
        if (cbar) std::memcpy(cbar, tail.data() + 2 * K, K * K * sizeof(double));
    }
    if (mref) TMVB_HIP(hipMemcpyAsync(mref, h->d_mref[h->tcur], K * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    TMVB_HIP(hipStreamSynchronize(h->ctx->stream));
    if (t) *t = h->t;
    return TMVB_OK;
}

extern "C" int tmvb_ctm_svi_set_schedule(tmvb_ctm_svi* h, double tau0, double kappa)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_ctm_svi_set_schedule: handle is NULL");
    TMVB_REQUIRE(std::isfinite(tau0) && tau0 >= 0.0, TMVB_EINVAL, "tau0 parameter must be nonnegative.");
    TMVB_REQUIRE(kappa > 0.5 && kappa <= 1.0, TMVB_EINVAL, "kappa parameter must be in (0.5, 1].");
    h->tau0 = tau0; h->kappa = kappa;
    return TMVB_OK;
}

// the batch's E-step and document reductions; afterwards the context's stream has joined the handle's side streams (tmvb_ctm_stats) and the handle no
// longer thinks the tail fresh (tmvb_ctm_reduce_docs consumed the flag), so nothing recomputes over what the tail kernel writes there next
static int ctm_svi_estep(tmvb_ctm_svi* h, tmvb_ctm* ch, int32_t niter, double ntol, int32_t viter, double vtol)
{
    int rc;
    void* p = nullptr; int64_t n = 0;
    if ((rc = tmvb_ctm_set_cur(ch, h->cur))) return rc;
    if ((rc = tmvb_ctm_estep(ch, niter, ntol, viter, vtol))) return rc;              // src/CTM.jl:194-205 on the batch's documents
    if ((rc = tmvb_ctm_reduce_docs(ch))) return rc;                                  // l_b, v_b, C_b about the current mu
    return tmvb_ctm_stats(ch, &p, &n);
}

extern "C" int tmvb_ctm_svi_run(tmvb_ctm_svi* h, const int32_t* batches, int64_t n, int32_t niter, double ntol, int32_t viter, double vtol)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_ctm_svi_run: handle is NULL");
    TMVB_REQUIRE(n >= 0 && (batches != nullptr || n == 0), TMVB_EINVAL, "tmvb_ctm_svi_run: bad batch list");
    TMVB_REQUIRE(ntol >= 0 && vtol >= 0, TMVB_EINVAL, "tolerance parameters must be nonnegative.");      // src/gpuCTM.jl:489
    TMVB_REQUIRE(niter >= 0 && viter >= 0, TMVB_EINVAL, "iteration parameters must be nonnegative.");    // src/gpuCTM.jl:490
    for (int64_t s = 0; s < n; ++s) TMVB_REQUIRE(batches[s] >= 0 && batches[s] < h->B, TMVB_EINVAL, "tmvb_ctm_svi_run: batch id %d outside [0, %d)", batches[s], h->B);
    TMVB_HIP(hipSetDevice(h->ctx->device));
    int rc;
    if ((rc = ctm_svi_ensure_stat(h, nullptr, nullptr, nullptr, nullptr))) return rc;
    hipStream_t st = h->ctx->stream;
    if (h->timing) {
        while ((int64_t)h->ev.size() < 4 * n) {
            hipEvent_t e = nullptr;
            if ((rc = h->mem.event(&e, hipEventDisableSystemFence))) return rc;
            h->ev.push_back(e);
        }
        h->timed_steps = 0;
    }
    const int64_t KV = (int64_t)h->K * h->V;
    const int T = (int)h->T();
    for (int64_t s = 0; s < n; ++s) {
        const int b = batches[s];
        tmvb_ctm* ch = h->hs[(size_t)b];
        const int64_t Mb = h->cuts[(size_t)b + 1] - h->cuts[(size_t)b];
        const double rho = std::pow(h->tau0 + (double)(h->t + 1), -h->kappa);
        const float c0 = (float)(1.0 - rho), c1 = (float)(rho * (double)h->M / (double)Mb);
        if (h->timing) TMVB_HIP(hipEventRecord(h->ev[(size_t)(4 * s)], st));
        if ((rc = ctm_svi_estep(h, ch, niter, ntol, viter, vtol))) return rc;
        if (h->timing) TMVB_HIP(hipEventRecord(h->ev[(size_t)(4 * s + 1)], st));
        // the fused global update: beta from the blended Sbar (update_beta!, src/CTM.jl:114-119), then the tail
        if ((rc = svi_launch_blend_norm(st, h->d_sbar, h->d_sb, h->K, h->KP, h->V, c0, c1, h->d_partial, nullptr, nullptr, h->d_beta[h->cur ^ 1]))) return rc;
        h->cur ^= 1;                                                                // beta_old <- beta, beta <- new
        hipLaunchKernelGGL(ctm_svi_tail_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, h->K, (double)h->M, c0, c1, (const float*)h->d_tbar[h->tcur],
                           h->d_tbar[h->tcur ^ 1], h->d_sb + KV, (const double*)h->d_mref[h->tcur], h->d_mref[h->tcur ^ 1], (const double*)h->d_mu);
        TMVB_HIP(hipGetLastError());
        h->tcur ^= 1;
        if (h->timing) TMVB_HIP(hipEventRecord(h->ev[(size_t)(4 * s + 2)], st));
        if ((rc = tmvb_ctm_sigma_mu_from_tail(ch))) return rc;                      // :207-208: sigma about the pre-step mu, then mu
        if (h->timing) { TMVB_HIP(hipEventRecord(h->ev[(size_t)(4 * s + 3)], st)); h->timed_steps = s + 1; }
        h->t += 1; h->rho = rho; h->c0 = c0; h->c1 = c1;
    }
    return TMVB_OK;
}

extern "C" int tmvb_ctm_svi_final_pass(tmvb_ctm_svi* h, int32_t niter, double ntol, int32_t viter, double vtol)
{
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "tmvb_ctm_svi_final_pass: handle is NULL");
    TMVB_REQUIRE(ntol >= 0 && vtol >= 0, TMVB_EINVAL, "tolerance parameters must be nonnegative.");
    TMVB_REQUIRE(niter >= 0 && viter >= 0, TMVB_EINVAL, "iteration parameters must be nonnegative.");
    TMVB_HIP(hipSetDevice(h->ctx->device));
    const size_t n = (size_t)h->K * (size_t)h->V + h->T();
    int rc;
    for (int b = 0; b < h->B; ++b) {
        if ((rc = ctm_svi_estep(h, h->hs[(size_t)b], niter, ntol, viter, vtol))) return rc;
        TMVB_HIP(hipMemsetAsync(h->d_sb, 0, n * sizeof(float), h->ctx->stream));    // the globals stay: the batch's statistics are dropped
    }
    return TMVB_OK;
}

extern "C" int tmvb_ctm_svi_info(tmvb_ctm_svi* h, tmvb_ctm_svi_info_t* out)
{
    TMVB_REQUIRE(h && out, TMVB_EINVAL, "tmvb_ctm_svi_info: NULL argument");
    out->B = h->B; out->K = h->K; out->M = h->M; out->V = h->V; out->t = h->t;
    out->tau0 = h->tau0; out->kappa = h->kappa; out->rho = h->rho; out->c0 = h->c0; out->c1 = h->c1;
    return TMVB_OK;
}

extern "C" int tmvb_ctm_svi_doc_sweeps(tmvb_ctm_svi* h, uint8_t* out)
{
    TMVB_REQUIRE(h && out, TMVB_EINVAL, "tmvb_ctm_svi_doc_sweeps: NULL argument");
    int rc;
    for (int b = 0; b < h->B; ++b)
        if ((rc = tmvb_ctm_doc_sweeps(h->hs[(size_t)b], out + h->cuts[(size_t)b]))) return rc;
    return TMVB_OK;
}

extern "C" int tmvb_ctm_svi_last_run_ms(tmvb_ctm_svi* h, float* ms_estep, float* ms_update, float* ms_sigma_mu, int64_t* steps)
{
    TMVB_REQUIRE(h && ms_estep && ms_update && ms_sigma_mu && steps, TMVB_EINVAL, "tmvb_ctm_svi_last_run_ms: NULL argument");
    TMVB_REQUIRE(h->timing, TMVB_EINVAL, "tmvb_ctm_svi_last_run_ms: step timing is off (set TMVB_ESTEP_TIMING=1 before creating the model)");
    TMVB_HIP(hipSetDevice(h->ctx->device));
    double e = 0.0, u = 0.0, a = 0.0;
    for (int64_t s = 0; s < h->timed_steps; ++s) {
        float ms = 0.0f;
        TMVB_HIP(hipEventSynchronize(h->ev[(size_t)(4 * s + 3)]));
        TMVB_HIP(hipEventElapsedTime(&ms, h->ev[(size_t)(4 * s)], h->ev[(size_t)(4 * s + 1)])); e += ms;
        TMVB_HIP(hipEventElapsedTime(&ms, h->ev[(size_t)(4 * s + 1)], h->ev[(size_t)(4 * s + 2)])); u += ms;
        TMVB_HIP(hipEventElapsedTime(&ms, h->ev[(size_t)(4 * s + 2)], h->ev[(size_t)(4 * s + 3)])); a += ms;
    }
    *ms_estep = (float)e; *ms_update = (float)u; *ms_sigma_mu = (float)a; *steps = h->timed_steps;
    return TMVB_OK;
}
