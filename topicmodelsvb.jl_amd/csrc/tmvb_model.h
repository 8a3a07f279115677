// tmvb_model.h -- what the five model handles share: the fields every family has (tmvb_model_base), the entry points that were the same function with
// another prefix, and the members of the train loop's Ops that never differed (tmvb_base_train_ops).  Each shared entry point takes the C function's
// name for its messages.  Host code only.
#pragma once

#include "tmvb_handle.h"
#include "tmvb_internal.h"

// which form the last update_elbo! took, and what train! asks of the coming iteration (tmvb_train.h).  fCTM keeps its own next to the CTM handle it wraps.
struct tmvb_elbo_form {
    int parts_env = 1;                 // TMVB_<MODEL>_ELBO_PARTS at creation: 0 never, 1 the iterations train! will check, 2 every E-step collects
    bool want_parts = false;           // the coming iteration ends in check_elbo!
    bool force_walk = false;           // train!'s like-with-like evaluation at the switch of forms
    int elbo_form = 0;                 // the last update_elbo!: 1 decomposed, 0 token walk
};

struct tmvb_model_base : tmvb_elbo_form {
    tmvb_ctx* ctx = nullptr;
    tmvb_corpus* corp = nullptr;
    int K = 0, KP = 0, nslot = 1;      // nslot: topic slots per lane of the lane = topic kernels ((K + 63) / 64)
    int64_t M = 0, V = 0, M_total = 0;
    bool distributed = false;
    tmvb_comm* comm = nullptr;         // document-sharded train!: the all-reduce of the packed statistics (not owned)
    float* d_stats = nullptr;          // the packed statistics, the library's own buffer or one the host bound (tmvb_*_bind_stats: not owned then)
    double* d_elbo = nullptr;
    double elbo = 0.0;
    uint8_t* d_sweeps = nullptr;       // [M] sweep count of each document's last E-step
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;                // ev0 / ev1 bracket an E-step
    bool timing = false;               // TMVB_ESTEP_TIMING=1 at creation (LDA, CTPF: the two events are recorded only then)
    tmvb_owned mem;                    // every device allocation, event and auxiliary stream of the handle (tmvb_handle.h)

    void release() { if (ctx) mem.release(ctx->device, ctx->stream); }
};

static inline int tmvb_model_elbo_form(const char* fn, const tmvb_elbo_form* h, int32_t* form)
{
    TMVB_REQUIRE(h && form, TMVB_EINVAL, "%s: NULL argument", fn);
    *form = h->elbo_form;
    return TMVB_OK;
}

// per-document sweep counts of the last E-step (document order of the corpus), for parity tests that compare the state of exactly those documents
// whose exit sweep agrees with the oracle's
static inline int tmvb_model_doc_sweeps(const char* fn, tmvb_model_base* h, uint8_t* out)
{
    TMVB_REQUIRE(h && (out || h->M == 0), TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_HIP(hipSetDevice(h->ctx->device));
    if (h->M) TMVB_HIP(hipMemcpyAsync(out, h->d_sweeps, (size_t)h->M, hipMemcpyDeviceToHost, h->ctx->stream));
    TMVB_HIP(hipStreamSynchronize(h->ctx->stream));
    return TMVB_OK;
}

static inline int tmvb_model_sweep_hist(const char* fn, tmvb_model_base* h, int64_t* hist, int32_t nbins)
{
    TMVB_REQUIRE(h && hist && nbins > 0, TMVB_EINVAL, "%s: bad argument", fn);
    std::vector<uint8_t> sw((size_t)h->M);
    const int rc = tmvb_model_doc_sweeps(fn, h, sw.data());
    if (rc) return rc;
    for (int b = 0; b < nbins; ++b) hist[b] = 0;
    for (uint8_t s : sw) hist[std::min<int>(s, nbins - 1)]++;
    return TMVB_OK;
}

// needs_switch: the family records the two events only under TMVB_ESTEP_TIMING=1 and says so (fLDA and CTM record them always)
static inline int tmvb_model_last_estep_ms(const char* fn, tmvb_model_base* h, float* ms, bool needs_switch)
{
    TMVB_REQUIRE(h && ms, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(!needs_switch || h->timing, TMVB_EINVAL, "%s: E-step timing is off (set TMVB_ESTEP_TIMING=1 before creating the model)", fn);
    TMVB_REQUIRE(h->timed, TMVB_EINVAL, "%s: no E-step has run", fn);
    TMVB_HIP(hipSetDevice(h->ctx->device));
    TMVB_HIP(hipEventSynchronize(h->ev1));
    TMVB_HIP(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return TMVB_OK;
}

// The statistics move to a buffer of the host's (need = the family's stats_len): `flush` first brings everything the handle still owes the buffer onto
// the context's stream, then the contents are copied over and the handle's own buffer goes; the bound one is not owned.
template <class Flush>
static int tmvb_model_bind_stats(const char* fn, tmvb_model_base* h, void* dev_ptr, int64_t n_f32, int64_t need, Flush flush)
{
    TMVB_REQUIRE(h && dev_ptr, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(n_f32 >= need, TMVB_ESHAPE, "%s: buffer holds %lld floats, need %lld", fn, (long long)n_f32, (long long)need);
    TMVB_HIP(hipSetDevice(h->ctx->device));
    { const int frc = flush(); if (frc) return frc; }
    TMVB_HIP(hipMemcpyAsync(dev_ptr, h->d_stats, (size_t)need * sizeof(float), hipMemcpyDeviceToDevice, h->ctx->stream));
    TMVB_HIP(hipStreamSynchronize(h->ctx->stream));
    h->mem.drop(&h->d_stats);
    h->d_stats = (float*)dev_ptr;
    return TMVB_OK;
}

// host K x V (column-major) <-> device [V][KP] padded
static inline int tmvb_model_upload_beta(tmvb_model_base* h, float* dst, const double* src)
{
    const size_t K = h->K, KP = h->KP, V = h->V;
    std::vector<float> tmp(V * KP + 4, 0.0f);
    for (size_t j = 0; j < V; ++j)
        for (size_t i = 0; i < K; ++i) tmp[j * KP + i] = (float)src[j * K + i];
    TMVB_HIP(hipMemcpyAsync(dst, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice, h->ctx->stream));
    TMVB_HIP(hipStreamSynchronize(h->ctx->stream));
    return TMVB_OK;
}

static inline int tmvb_model_download_beta(tmvb_model_base* h, double* dst, const float* src)
{
    const size_t K = h->K, KP = h->KP, V = h->V;
    std::vector<float> tmp(V * KP);
    TMVB_HIP(hipMemcpyAsync(tmp.data(), src, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, h->ctx->stream));
    TMVB_HIP(hipStreamSynchronize(h->ctx->stream));
    for (size_t j = 0; j < V; ++j)
        for (size_t i = 0; i < K; ++i) dst[j * K + i] = (double)tmp[j * KP + i];
    return TMVB_OK;
}

// The members of the train loop's Ops (tmvb_train.h) that are the same for every family.  A family's Ops derive from this and add estep, reduce,
// before_allreduce, stats_len, mstep, elbo_local and its optional members.  H holds the ELBO-form fields itself; the rest is read through
// tmvb_model_core(h), which a handle that wraps another (fCTM) overloads.
static inline tmvb_model_base* tmvb_model_core(tmvb_model_base* h) { return h; }

template <class H>
struct tmvb_base_train_ops {
    float* stats(H* h) { return tmvb_model_core(h)->d_stats; }
    int elbo_form(H* h) { return h->elbo_form; }
    void force_walk(H* h, bool on, bool doubled = true) { h->force_walk = on; if (!on && doubled) h->elbo_form = 1; }   // (switched off behind the one evaluation that doubled a decomposed one)
    void will_check(H* h, bool checked) { h->want_parts = checked; }                  // the coming iteration ends in check_elbo!: collect update_elbo!'s parts on the way
    double* elbo_dev(H* h) { return tmvb_model_core(h)->d_elbo; }
    tmvb_comm* comm(H* h) { return tmvb_model_core(h)->comm; }
    bool distributed(H* h) { return tmvb_model_core(h)->distributed; }
    tmvb_ctx* ctx(H* h) { return tmvb_model_core(h)->ctx; }
    int64_t nnz(H* h) { return tmvb_model_core(h)->corp->info.nnz; }
    void set_elbo(H* h, double v) { tmvb_model_core(h)->elbo = v; }
    double get_elbo(H* h) { return tmvb_model_core(h)->elbo; }
    int finish(H* h)
    {
        tmvb_ctx* c = ctx(h);
        TMVB_HIP(hipSetDevice(c->device));
        TMVB_HIP(hipStreamSynchronize(c->stream));
        return TMVB_OK;
    }
};
