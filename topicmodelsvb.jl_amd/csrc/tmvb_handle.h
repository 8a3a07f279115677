// tmvb_handle.h -- what a model handle (tmvb_lda, tmvb_flda, tmvb_ctm, tmvb_fctm, tmvb_ctpf, the two stochastic drivers) keeps on the device for its
// lifetime: memory, events, auxiliary streams.  Host code only: no device code, no tmvb_internal.h.  (The scratch of ONE call is tmvb_call.h.)
//
// A handle registers everything it creates with its tmvb_owned; its *_destroy -- and the create guard, from the middle of a *_create -- calls release(),
// which waits for the handle's streams and the context's stream BEFORE the first free (a side stream may still work on a buffer), then frees every
// pointer, destroys every event and gives back every stream of its own, each once.  What a handle only uses -- a statistics buffer bound by the host,
// the globals and streams of a stochastic driver's first batch handle -- is never registered, or dropped when it is adopted, and so is never released.
// Not thread-safe (the index builds that tmvb_lda_create runs on threads own their memory through tmvb_inv_index).
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <vector>

#include "tmvb.h"

void tmvb_set_error(const char* fmt, ...);
hipStream_t tmvb_pool_stream(int device, int slot, bool high_priority);
void tmvb_release_stream(hipStream_t st);

struct tmvb_owned {
    struct stream { hipStream_t st; bool own; };
    std::vector<void*> ptrs;
    std::vector<hipEvent_t> evs;
    std::vector<stream> streams;

    tmvb_owned() = default;
    tmvb_owned(const tmvb_owned&) = delete;
    tmvb_owned& operator=(const tmvb_owned&) = delete;

    // max(n, 1) elements, so that an empty array still has an address; *p = nullptr on failure
    template <typename T>
    int alloc(T** p, size_t n)
    {
        *p = nullptr;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        const hipError_t e = hipMalloc((void**)p, bytes);
        if (e != hipSuccess) {
            tmvb_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
            return TMVB_ENOMEM;
        }
        ptrs.push_back(*p);
        return TMVB_OK;
    }
    // frees *p now (hipFree waits for the device) and nulls it; a pointer this owner does not hold -- bound, shared, never allocated -- is left alone
    template <typename T>
    void drop(T** p)
    {
        const auto it = std::find(ptrs.begin(), ptrs.end(), (void*)*p);
        if (it == ptrs.end()) return;
        ptrs.erase(it);
        (void)hipFree(*p);
        *p = nullptr;
    }
    // the owner keeps the event's value, not its address: members of a std::vector<hipEvent_t> register like any other
    int event(hipEvent_t* e, unsigned flags)
    {
        *e = nullptr;
        const hipError_t err = hipEventCreateWithFlags(e, flags);
        if (err != hipSuccess) {
            *e = nullptr;
            tmvb_set_error("hipEventCreateWithFlags(%u) failed: %s", flags, hipGetErrorString(err));
            return TMVB_EHIP;
        }
        evs.push_back(*e);
        return TMVB_OK;
    }
    // the same event with other flags (nothing may be pending on it); an event that was never made stays unmade
    int remake(hipEvent_t* e, unsigned flags)
    {
        const auto it = std::find(evs.begin(), evs.end(), *e);
        if (!*e || it == evs.end()) return TMVB_OK;
        evs.erase(it);
        (void)hipEventDestroy(*e);
        return event(e, flags);
    }
    // an auxiliary stream of the handle's own (tmvb_pool_stream: created, or the device's pooled one)
    int aux(hipStream_t* s, int device, int slot, bool high_priority)
    {
        *s = tmvb_pool_stream(device, slot, high_priority);
        if (!*s) { tmvb_set_error("hipStreamCreate failed"); return TMVB_EHIP; }
        streams.push_back({*s, true});
        return TMVB_OK;
    }
    // *s gives way to another handle's stream: the own one goes back now, the borrowed one is waited for at release() and never given back
    void borrow(hipStream_t* s, hipStream_t from)
    {
        for (stream& x : streams)
            if (x.st == *s && x.own) { tmvb_release_stream(x.st); x = {from, false}; break; }
        *s = from;
    }
    // idempotent, and safe on a half-built handle: whatever was registered so far goes, once
    void release(int device, hipStream_t ctx_stream)
    {
        if (ptrs.empty() && evs.empty() && streams.empty()) return;
        (void)hipSetDevice(device);
        for (const stream& x : streams) (void)hipStreamSynchronize(x.st);
        (void)hipStreamSynchronize(ctx_stream);
        for (void* p : ptrs) (void)hipFree(p);
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
        for (const stream& x : streams) if (x.own) tmvb_release_stream(x.st);      // pooled streams stay (tmvb_pool_stream)
        ptrs.clear(); evs.clear(); streams.clear();
    }
};
