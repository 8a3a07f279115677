// tmvb_call.h -- the device scratch of ONE call of a stateless entry point (tmvb_corpus_split, tmvb_heldout_loglik, tmvb_*_gencorp,
// tmvb_corpus_codocfreq, tmvb_topic_neighbors, tmvb_topic_order, tmvb_ctpf_recommend, tmvb_score_ranks, tmvb_score_topn, tmvb_ctpf_foldin_users, tmvb_ctpf_foldin_users_on, tmvb_topic_search, tmvb_token_topics, tmvb_topic_kmeans, tmvb_map_affinity, tmvb_map_layout, tmvb_topic_divergence, tmvb_term_relevance).  Host code only: no device code, no tmvb_internal.h.
// (Memory that a handle owns for its lifetime is not this: tmvb_owned in tmvb_handle.h.)
//
// Release order.  A call declares, in this order,
//     1. the guard of its malloc'd result struct (tmvb_result_guard) and every host staging buffer (std::vector) that a copy reads or writes,
//     2. its tmvb_call,
// and leaves early only through TMVB_CALL_HIP / TMVB_CALL_TRY / `return c.fail(rc)`.  Then, on every failure: fail() waits for the stream (copies
// already issued may still target host buffers), the tmvb_call's destructor frees the device memory and the events, and only after that do the
// host buffers and the result struct of 1. go -- locals are destroyed in reverse order of declaration.  The success path waits only where the call
// itself does.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "tmvb.h"

void tmvb_set_error(const char* fmt, ...);

struct tmvb_call {
    const char* what;               // prefix of the messages: "heldout", "gencorp", ...
    int device;
    hipStream_t stream;
    std::vector<void*> ptrs;
    std::vector<hipEvent_t> evs;

    tmvb_call(const char* what_, int device_, hipStream_t stream_) : what(what_), device(device_), stream(stream_) {}
    tmvb_call(const tmvb_call&) = delete;
    tmvb_call& operator=(const tmvb_call&) = delete;
    ~tmvb_call()
    {
        for (void* p : ptrs) (void)hipFree(p);
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
    }

    int begin()
    {
        const hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { tmvb_set_error("%s: hipSetDevice(%d) failed: %s", what, device, hipGetErrorString(e)); return TMVB_EHIP; }
        return TMVB_OK;
    }
    // max(n, 1) elements, so that an empty array still has an address
    template <typename T>
    int alloc(T** p, size_t n)
    {
        *p = nullptr;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        const hipError_t e = hipMalloc((void**)p, bytes);
        if (e != hipSuccess) { tmvb_set_error("%s: hipMalloc(%zu bytes) failed: %s", what, bytes, hipGetErrorString(e)); return TMVB_ENOMEM; }
        ptrs.push_back(*p);
        return TMVB_OK;
    }
    // alloc + asynchronous copy of n host elements on the call's stream
    template <typename T>
    int upload(T** d, const T* h, size_t n)
    {
        const int rc = alloc(d, n);
        if (rc != TMVB_OK || n == 0) return rc;
        const hipError_t e = hipMemcpyAsync(*d, h, n * sizeof(T), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) { tmvb_set_error("%s: hipMemcpyAsync(%zu bytes to the device) failed: %s", what, n * sizeof(T), hipGetErrorString(e)); return TMVB_EHIP; }
        return TMVB_OK;
    }
    int events(int n)
    {
        for (int i = 0; i < n; i++) {
            hipEvent_t e;
            const hipError_t err = hipEventCreate(&e);
            if (err != hipSuccess) { tmvb_set_error("%s: hipEventCreate failed: %s", what, hipGetErrorString(err)); return TMVB_EHIP; }
            evs.push_back(e);
        }
        return TMVB_OK;
    }
    hipEvent_t ev(int i) const { return evs[(size_t)i]; }
    int elapsed(float* ms, int i, int j) const
    {
        const hipError_t e = hipEventElapsedTime(ms, ev(i), ev(j));
        if (e != hipSuccess) { tmvb_set_error("%s: hipEventElapsedTime failed: %s", what, hipGetErrorString(e)); return TMVB_EHIP; }
        return TMVB_OK;
    }
    // every early return goes through here: nothing is released while the stream still works on it (the wait's own status is of no interest)
    int fail(int rc)
    {
        (void)hipStreamSynchronize(stream);
        return rc;
    }
};

#define TMVB_CALL_HIP(c, call)                                                                                            \
    do {                                                                                                                  \
        const hipError_t e_ = (call);                                                                                     \
        if (e_ != hipSuccess) {                                                                                           \
            tmvb_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);                    \
            return (c).fail(TMVB_EHIP);                                                                                   \
        }                                                                                                                 \
    } while (0)

#define TMVB_CALL_TRY(c, expr)                                                                                            \
    do {                                                                                                                  \
        const int rc_ = (expr);                                                                                           \
        if (rc_ != TMVB_OK) return (c).fail(rc_);                                                                         \
    } while (0)

// a buffer of a malloc'd result struct: max(n, 1) elements
template <typename T>
int tmvb_host_alloc(const char* what, T** p, size_t n)
{
    *p = (T*)malloc(std::max<size_t>(n, 1) * sizeof(T));
    if (!*p) { tmvb_set_error("%s: out of host memory", what); return TMVB_ENOMEM; }
    return TMVB_OK;
}

// Frees a half-filled result struct (tmvb_split_t, tmvb_gencorp_t) on every early return; release() on success.  Declared BEFORE the tmvb_call.
template <class S, void (*Free)(S*)>
struct tmvb_result_guard {
    S* s;
    ~tmvb_result_guard() { if (s) Free(s); }
    void release() { s = nullptr; }
};
