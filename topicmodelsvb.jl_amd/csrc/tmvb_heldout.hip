// tmvb_heldout.hip -- held-out evaluation on the device: a deterministic per-token split of a corpus and the per-document log predictive
// likelihood of held-out words (document completion; SURVEY section 8(f) item 1 -- the purpose of predict; the reference has no such function).
//
// tmvb_corpus_split.  The token occurrences of document d are numbered t = 0 .. C_d - 1 in CSR order; occurrence t is held out iff word
// x[t & 3] of Philox4x32-10(key = seed, counter = (doc_offset + d, TMVB_RNG_SPLIT, t >> 2)) is below floor(frac 2^32).  Nothing depends on the
// launch geometry: the same seed gives the same bytes and doc_offset reproduces any slice.
//   draw      one wave per document, lane = Philox BLOCK of four occurrences (b, b + 64, ...), not CSR entry: counts are skewed (one entry of
//             5 000 occurrences is 1 250 blocks spread over the wave) and one block serves four occurrences.  A lane finds the entry of its
//             first occurrence by a binary search in the scanned counts, walks on from there, and adds its held occurrences to the entry's
//             counter with an INTEGER atomic (order-independent: the result is bit-exact).
//   compact   flags (count left > 0 on either side), two hipcub::DeviceScan::ExclusiveSum, one scatter; the new doc_ptr is the scan read at
//             the old doc_ptr.
//
// tmvb_heldout_loglik.  ll[d] = sum_n c_n log(theta_d . beta'[:, w_n]): per nonzero one gather of a beta row (the [V][KP] gather layout of the
// engine, 16-byte loads) against the document's theta, K FMAs -- the access pattern of the first sweep of the LDA E-step.
//   theta_d sits in LDS (KP floats); L = 2^logL lanes share a nonzero (lane r takes the 16-byte chunks r, r + L, ... of the row: L adjacent
//   lanes read 16 L consecutive bytes), L grows with K so that a lane has at most ~4 chunks (K = 50: L = 4; K = 1024: L = 64); the L partial
//   dots meet in a fixed xor butterfly.  A workgroup works on one document: 64 lanes for documents of at most 4 trips, 256 lanes for longer
//   ones (host-built lists), so a 5 000-entry document is spread over four waves.  fp32 dot, fp64 log and fp64 sums, reduced in a fixed order:
//   no atomics, bitwise reproducible.
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_philox.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <hipcub/hipcub.hpp>

#define HO_MAX_K 1024
#define HO_MAX_KP 1028              // tmvb_kpad(1024)
#define HO_SHORT_TRIPS 4            // documents of at most this many trips of a wave stay on one wave

// ------------------------------------------------------------------------------------------------------------------ split: draw
struct ho_widen {
    __host__ __device__ int64_t operator()(const int32_t& c) const { return (int64_t)c; }
};

// one wave per document; cum = exclusive scan of counts over the whole CSR ([nnz + 1]); held[j] starts at 0
static __global__ __launch_bounds__(64) void split_draw_kernel(int64_t doc_offset, uint64_t seed, uint64_t thr, const int64_t* __restrict__ doc_ptr,
                                                               const int64_t* __restrict__ cum, int32_t* __restrict__ held)
{
    const int64_t d = blockIdx.x;
    const int64_t a = doc_ptr[d], b = doc_ptr[d + 1];
    if (a == b) return;
    const int64_t base = cum[a], C = cum[b] - base, nblk = (C + 3) >> 2;
    const uint64_t g = (uint64_t)(doc_offset + d);
    for (int64_t blk = threadIdx.x; blk < nblk; blk += 64) {
        const int64_t t0 = blk << 2;
        int64_t lo = a, hi = b - 1;                    // last entry whose first occurrence is <= t0
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (cum[mid] - base <= t0) lo = mid; else hi = mid - 1;
        }
        int64_t j = lo, end = cum[j + 1] - base;
        const tmvb_philox4 r = tmvb_rng(seed, g, TMVB_RNG_SPLIT, 0, (uint32_t)blk);
        int acc = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int64_t t = t0 + q;
            if (t < C) {
                while (t >= end) {                     // counts >= 1: every step is a real entry of this document
                    if (acc) atomicAdd(&held[j], acc);
                    acc = 0;
                    j++;
                    end = cum[j + 1] - base;
                }
                acc += (uint64_t)r.x[q] < thr ? 1 : 0;
            }
        }
        if (acc) atomicAdd(&held[j], acc);
    }
}

// ------------------------------------------------------------------------------------------------------------------ split: compact
// flag arrays have n + 1 entries (the last is 0), so that the exclusive scans end in the totals
static __global__ void split_flags_kernel(int64_t n, const int32_t* __restrict__ counts, const int32_t* __restrict__ held, int32_t* __restrict__ fo,
                                          int32_t* __restrict__ fh)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    fo[j] = j < n && counts[j] - held[j] > 0 ? 1 : 0;
    fh[j] = j < n && held[j] > 0 ? 1 : 0;
}

static __global__ void split_scatter_kernel(int64_t n, const int32_t* __restrict__ terms, const int32_t* __restrict__ counts, const int32_t* __restrict__ held,
                                            const int32_t* __restrict__ po, const int32_t* __restrict__ ph, int32_t* __restrict__ oterms,
                                            int32_t* __restrict__ ocounts, int32_t* __restrict__ hterms, int32_t* __restrict__ hcounts)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t w = terms[j], h = held[j], o = counts[j] - h;
    if (o > 0) { oterms[po[j]] = w; ocounts[po[j]] = o; }
    if (h > 0) { hterms[ph[j]] = w; hcounts[ph[j]] = h; }
}

static __global__ void split_ptr_kernel(int64_t M, const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ po, const int32_t* __restrict__ ph,
                                        int64_t* __restrict__ optr, int64_t* __restrict__ hptr)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > M) return;
    optr[d] = po[doc_ptr[d]];
    hptr[d] = ph[doc_ptr[d]];
}

// ------------------------------------------------------------------------------------------------------------------ log-likelihood
// One workgroup of WG lanes per document docs[blockIdx.x].  theta: [M][KP], beta: [V][KP] (smoothed, pads 0), both 16-byte aligned rows.
template <int WG>
static __global__ __launch_bounds__(WG) void heldout_loglik_kernel(int K, int KP, int logL, const int32_t* __restrict__ docs, const float* __restrict__ theta,
                                                                   const float* __restrict__ beta, const int64_t* __restrict__ doc_ptr,
                                                                   const int32_t* __restrict__ terms, const int32_t* __restrict__ counts,
                                                                   double* __restrict__ ll, long long* __restrict__ tokens, long long* __restrict__ zero)
{
    __shared__ __attribute__((aligned(16))) float s_theta[HO_MAX_KP];
    __shared__ double s_ll[WG / 64];
    __shared__ long long s_tok[WG / 64], s_zero[WG / 64];
    const int tid = threadIdx.x, L = 1 << logL, r = tid & (L - 1), g = tid >> logL, G = WG >> logL;
    const int64_t d = docs[blockIdx.x];
    const int64_t a = doc_ptr[d], n = doc_ptr[d + 1] - a;
#ifdef TMVB_MUTANT_HELDOUT_DROP_TAIL
    const int nch = K >> 2;                            // MUTANT: the last, partial 16-byte chunk of a row is dropped
#else
    const int nch = (K + 3) >> 2;                      // chunks that hold topics; a chunk of pads only (KP = 4 * odd) is never read
#endif
    const float4* th4 = reinterpret_cast<const float4*>(theta + d * KP);
    float4* s4 = reinterpret_cast<float4*>(s_theta);
    for (int c = tid; c < (KP >> 2); c += WG) s4[c] = th4[c];
    __syncthreads();
    double acc = 0.0;
    long long tok = 0, zp = 0;
    for (int64_t i0 = 0; i0 < n; i0 += G) {            // uniform trip count: every lane takes part in the butterfly
        const int64_t i = i0 + g;
        const bool live = i < n;
        float p = 0.0f;
        int c_n = 0;
        if (live) {
            c_n = counts[a + i];
            const float4* row = reinterpret_cast<const float4*>(beta + (int64_t)terms[a + i] * KP);
            float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
            for (int c = r; c < nch; c += L) {
                const float4 bv = row[c], tv = s4[c];
                p0 = fmaf(bv.x, tv.x, p0); p1 = fmaf(bv.y, tv.y, p1); p2 = fmaf(bv.z, tv.z, p2); p3 = fmaf(bv.w, tv.w, p3);
            }
            p = (p0 + p1) + (p2 + p3);
        }
        for (int o = L >> 1; o; o >>= 1) p += __shfl_xor(p, o);
        if (live && r == 0) {
            tok += c_n;
            if (p == 0.0f) zp += c_n;
            acc += (double)c_n * log((double)p);       // log(0) = -inf: the document's sum stays -inf
        }
    }
    for (int o = 32; o; o >>= 1) {                     // lanes that led no nonzero hold 0
        acc += __shfl_xor(acc, o);
        tok += __shfl_xor(tok, o);
        zp += __shfl_xor(zp, o);
    }
    if (WG == 64) {
        if (tid == 0) { ll[d] = acc; tokens[d] = tok; zero[d] = zp; }
    } else {
        if ((tid & 63) == 0) { s_ll[tid >> 6] = acc; s_tok[tid >> 6] = tok; s_zero[tid >> 6] = zp; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < WG / 64; w++) { acc += s_ll[w]; tok += s_tok[w]; zp += s_zero[w]; }
            ll[d] = acc; tokens[d] = tok; zero[d] = zp;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
int ho_split_run(tmvb_ctx* ctx, int64_t M, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts, uint64_t thr, uint64_t seed,
                 int64_t doc_offset, tmvb_split_t* out)
{
    tmvb_result_guard<tmvb_split_t, tmvb_split_free> guard{out};
    hipStream_t st = ctx->stream;
    tmvb_call c("heldout", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(4));
    const int64_t n = doc_ptr[M];
    int64_t *d_ptr, *d_cum, *d_optr, *d_hptr;
    int32_t *d_terms, *d_counts, *d_held, *d_fo, *d_fh, *d_po, *d_ph, *d_ot, *d_oc, *d_ht, *d_hc;
    TMVB_CALL_TRY(c, c.alloc(&d_ptr, (size_t)M + 1)); TMVB_CALL_TRY(c, c.alloc(&d_cum, (size_t)n + 1)); TMVB_CALL_TRY(c, c.alloc(&d_optr, (size_t)M + 1));
    TMVB_CALL_TRY(c, c.alloc(&d_hptr, (size_t)M + 1)); TMVB_CALL_TRY(c, c.alloc(&d_terms, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(&d_counts, (size_t)n + 1));
    TMVB_CALL_TRY(c, c.alloc(&d_held, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(&d_fo, (size_t)n + 1)); TMVB_CALL_TRY(c, c.alloc(&d_fh, (size_t)n + 1));
    TMVB_CALL_TRY(c, c.alloc(&d_po, (size_t)n + 1)); TMVB_CALL_TRY(c, c.alloc(&d_ph, (size_t)n + 1)); TMVB_CALL_TRY(c, c.alloc(&d_ot, (size_t)n));
    TMVB_CALL_TRY(c, c.alloc(&d_oc, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(&d_ht, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(&d_hc, (size_t)n));
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_ptr, doc_ptr, ((size_t)M + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_counts, 0, ((size_t)n + 1) * sizeof(int32_t), st));        // entry n of the scanned array is read as 0
    if (n > 0) {
        TMVB_CALL_HIP(c, hipMemcpyAsync(d_terms, terms, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(d_counts, counts, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    TMVB_CALL_HIP(c, hipMemsetAsync(d_held, 0, std::max<size_t>((size_t)n, 1) * sizeof(int32_t), st));
    hipcub::TransformInputIterator<int64_t, ho_widen, const int32_t*> wide((const int32_t*)d_counts, ho_widen());
    size_t b1 = 0, b2 = 0;
    TMVB_CALL_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b1, wide, d_cum, (int)(n + 1), st));
    TMVB_CALL_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (const int32_t*)d_fo, d_po, (int)(n + 1), st));
    char* d_scan;
    const size_t scan_bytes = std::max<size_t>(std::max(b1, b2), 16);
    TMVB_CALL_TRY(c, c.alloc(&d_scan, scan_bytes));

    // Stage times: each pair of events brackets kernels and hipcub calls only; allocations, copies and memsets lie outside.
    // ---- draw
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    b1 = scan_bytes;
    TMVB_CALL_HIP(c, hipcub::DeviceScan::ExclusiveSum((void*)d_scan, b1, wide, d_cum, (int)(n + 1), st));
    hipLaunchKernelGGL(split_draw_kernel, dim3((unsigned)M), dim3(64), 0, st, doc_offset, seed, thr, (const int64_t*)d_ptr, (const int64_t*)d_cum, d_held);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    // ---- compact
    const unsigned nb = (unsigned)((n + 256) / 256);
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    hipLaunchKernelGGL(split_flags_kernel, dim3(nb), dim3(256), 0, st, n, (const int32_t*)d_counts, (const int32_t*)d_held, d_fo, d_fh);
    TMVB_CALL_HIP(c, hipGetLastError());
    b2 = scan_bytes;
    TMVB_CALL_HIP(c, hipcub::DeviceScan::ExclusiveSum((void*)d_scan, b2, (const int32_t*)d_fo, d_po, (int)(n + 1), st));
    b2 = scan_bytes;
    TMVB_CALL_HIP(c, hipcub::DeviceScan::ExclusiveSum((void*)d_scan, b2, (const int32_t*)d_fh, d_ph, (int)(n + 1), st));
    hipLaunchKernelGGL(split_scatter_kernel, dim3(nb), dim3(256), 0, st, n, (const int32_t*)d_terms, (const int32_t*)d_counts, (const int32_t*)d_held,
                       (const int32_t*)d_po, (const int32_t*)d_ph, d_ot, d_oc, d_ht, d_hc);
    hipLaunchKernelGGL(split_ptr_kernel, dim3((unsigned)((M + 256) / 256)), dim3(256), 0, st, M, (const int64_t*)d_ptr, (const int32_t*)d_po, (const int32_t*)d_ph,
                       d_optr, d_hptr);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));

    // ---- results
    out->M = M;
    TMVB_CALL_TRY(c, tmvb_host_alloc("heldout", &out->obs_ptr, (size_t)M + 1));
    TMVB_CALL_TRY(c, tmvb_host_alloc("heldout", &out->held_ptr, (size_t)M + 1));
    TMVB_CALL_HIP(c, hipMemcpyAsync(out->obs_ptr, d_optr, ((size_t)M + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(out->held_ptr, d_hptr, ((size_t)M + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    out->nnz_obs = out->obs_ptr[M]; out->nnz_held = out->held_ptr[M];
    TMVB_CALL_TRY(c, tmvb_host_alloc("heldout", &out->obs_terms, (size_t)out->nnz_obs));
    TMVB_CALL_TRY(c, tmvb_host_alloc("heldout", &out->obs_counts, (size_t)out->nnz_obs));
    TMVB_CALL_TRY(c, tmvb_host_alloc("heldout", &out->held_terms, (size_t)out->nnz_held));
    TMVB_CALL_TRY(c, tmvb_host_alloc("heldout", &out->held_counts, (size_t)out->nnz_held));
    if (out->nnz_obs > 0) {
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->obs_terms, d_ot, (size_t)out->nnz_obs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->obs_counts, d_oc, (size_t)out->nnz_obs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (out->nnz_held > 0) {
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->held_terms, d_ht, (size_t)out->nnz_held * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->held_counts, d_hc, (size_t)out->nnz_held * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    for (int64_t j = 0; j < out->nnz_obs; j++) out->sum_obs += out->obs_counts[j];
    for (int64_t j = 0; j < out->nnz_held; j++) out->sum_held += out->held_counts[j];
    TMVB_CALL_TRY(c, c.elapsed(&out->ms_draw, 0, 1));
    TMVB_CALL_TRY(c, c.elapsed(&out->ms_compact, 2, 3));
    guard.release();
    return TMVB_OK;
}

// lanes per nonzero: the smallest power of two that leaves a lane at most four 16-byte chunks of the row, at most a wave
int ho_log_lanes(int K)
{
    const int nch = (K + 3) / 4;
    int logL = 0;
    while (logL < 6 && (4 << logL) < nch) logL++;
    return logL;
}

int ho_loglik_run(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t M, const double* theta, const double* beta, const int64_t* doc_ptr, const int32_t* terms,
                  const int32_t* counts, double a, double* ll, int64_t* tokens, int64_t* zero_prob_tokens, float* ms_kernel)
{
    const int KP = tmvb_kpad(K), logL = ho_log_lanes(K);
    const int64_t n = doc_ptr[M];
    // host staging, declared in front of the call's scope: fp32 theta [M][KP], smoothed fp32 beta [V][KP], the two document lists, the read-back
    std::vector<float> h_theta((size_t)M * KP, 0.0f), h_beta((size_t)V * KP, 0.0f);
    std::vector<long long> h_zero((size_t)M);
    const double denom = 1.0 + a * (double)V;
    for (int64_t d = 0; d < M; d++)
        for (int k = 0; k < K; k++) h_theta[(size_t)d * KP + k] = (float)theta[k + (int64_t)K * d];
    for (int64_t v = 0; v < V; v++)
        for (int k = 0; k < K; k++) h_beta[(size_t)v * KP + k] = (float)((beta[k + (int64_t)K * v] + a) / denom);
    const int64_t short_max = (int64_t)HO_SHORT_TRIPS * (64 >> logL);
    std::vector<int32_t> h_docs((size_t)M);
    int64_t n_short = 0, n_long = 0;
    for (int64_t d = 0; d < M; d++)
        if (doc_ptr[d + 1] - doc_ptr[d] <= short_max) h_docs[(size_t)n_short++] = (int32_t)d;
    for (int64_t d = 0; d < M; d++)
        if (doc_ptr[d + 1] - doc_ptr[d] > short_max) h_docs[(size_t)(n_short + n_long++)] = (int32_t)d;

    hipStream_t st = ctx->stream;
    tmvb_call c("heldout", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(2));
    float *d_theta, *d_beta;
    int64_t* d_ptr;
    int32_t *d_terms, *d_counts, *d_docs;
    double* d_ll;
    long long *d_tok, *d_zero;
    TMVB_CALL_TRY(c, c.alloc(&d_theta, h_theta.size())); TMVB_CALL_TRY(c, c.alloc(&d_beta, h_beta.size())); TMVB_CALL_TRY(c, c.alloc(&d_ptr, (size_t)M + 1));
    TMVB_CALL_TRY(c, c.alloc(&d_terms, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(&d_counts, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(&d_docs, (size_t)M));
    TMVB_CALL_TRY(c, c.alloc(&d_ll, (size_t)M)); TMVB_CALL_TRY(c, c.alloc(&d_tok, (size_t)M)); TMVB_CALL_TRY(c, c.alloc(&d_zero, (size_t)M));
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_theta, h_theta.data(), h_theta.size() * sizeof(float), hipMemcpyHostToDevice, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_beta, h_beta.data(), h_beta.size() * sizeof(float), hipMemcpyHostToDevice, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_ptr, doc_ptr, ((size_t)M + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_docs, h_docs.data(), (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (n > 0) {
        TMVB_CALL_HIP(c, hipMemcpyAsync(d_terms, terms, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(d_counts, counts, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    if (n_short > 0)
        hipLaunchKernelGGL(heldout_loglik_kernel<64>, dim3((unsigned)n_short), dim3(64), 0, st, (int)K, KP, logL, (const int32_t*)d_docs, (const float*)d_theta,
                           (const float*)d_beta, (const int64_t*)d_ptr, (const int32_t*)d_terms, (const int32_t*)d_counts, d_ll, d_tok, d_zero);
    if (n_long > 0)
        hipLaunchKernelGGL(heldout_loglik_kernel<256>, dim3((unsigned)n_long), dim3(256), 0, st, (int)K, KP, logL, (const int32_t*)d_docs + n_short,
                           (const float*)d_theta, (const float*)d_beta, (const int64_t*)d_ptr, (const int32_t*)d_terms, (const int32_t*)d_counts, d_ll, d_tok, d_zero);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    static_assert(sizeof(long long) == sizeof(int64_t), "tokens travel as 64-bit integers");
    TMVB_CALL_HIP(c, hipMemcpyAsync(ll, d_ll, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(tokens, d_tok, (size_t)M * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(h_zero.data(), d_zero, (size_t)M * sizeof(long long), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    int64_t z = 0;
    for (int64_t d = 0; d < M; d++) z += h_zero[(size_t)d];
    *zero_prob_tokens = z;
    if (ms_kernel) TMVB_CALL_TRY(c, c.elapsed(ms_kernel, 0, 1));
    return TMVB_OK;
}
}  // namespace

extern "C" void tmvb_split_free(tmvb_split_t* s)
{
    if (!s) return;
    free(s->obs_ptr); free(s->obs_terms); free(s->obs_counts); free(s->held_ptr); free(s->held_terms); free(s->held_counts);
    memset(s, 0, sizeof(*s));
}

extern "C" int tmvb_corpus_split(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts, double frac,
                                 int64_t seed, int64_t doc_offset, tmvb_split_t* out)
{
    TMVB_REQUIRE(out != nullptr, TMVB_EINVAL, "tmvb_corpus_split: out is NULL");
    memset(out, 0, sizeof(*out));
    TMVB_REQUIRE(std::isfinite(frac) && frac >= 0.0 && frac <= 1.0, TMVB_EINVAL, "tmvb_corpus_split: frac must lie in [0, 1]");
    TMVB_REQUIRE(doc_offset >= 0, TMVB_EINVAL, "tmvb_corpus_split: doc_offset must be nonnegative");
    int rc = tmvb_check_host_csr("tmvb_corpus_split", M, V, doc_ptr, terms, counts, true);
    if (rc != TMVB_OK) return rc;
    if ((rc = tmvb_check_ctx_or_device("tmvb_corpus_split", ctx)) != TMVB_OK) return rc;
    const uint64_t thr = (uint64_t)std::floor(frac * 4294967296.0);
    return ho_split_run(ctx, M, doc_ptr, terms, counts, thr, (uint64_t)seed, doc_offset, out);
}

extern "C" int tmvb_heldout_loglik(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t M, const double* theta, const double* beta, const int64_t* doc_ptr,
                                   const int32_t* terms, const int32_t* counts, double laplace_smooth, double* ll, int64_t* tokens,
                                   int64_t* zero_prob_tokens, float* ms_kernel)
{
    const char* fn = "tmvb_heldout_loglik";
    TMVB_REQUIRE(K >= 1 && K <= HO_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, HO_MAX_K);
    TMVB_REQUIRE(laplace_smooth >= 0.0 && std::isfinite(laplace_smooth), TMVB_EINVAL, "laplace_smooth parameter must be nonnegative.");
    TMVB_REQUIRE(theta && beta && ll && tokens && zero_prob_tokens, TMVB_EINVAL, "%s: NULL argument", fn);
    int rc = tmvb_check_host_csr(fn, M, V, doc_ptr, terms, counts, false);
    if (rc != TMVB_OK) return rc;
    if ((rc = tmvb_check_stochastic_beta(K, V, beta)) != TMVB_OK) return rc;
    for (int64_t d = 0; d < M; d++) {
        double s = 0.0;
        bool good = true;
        for (int k = 0; k < K; k++) {
            const double x = theta[k + (int64_t)K * d];
            if (!(x >= 0.0) || !std::isfinite(x)) { good = false; break; }
            s += x;
        }
        TMVB_REQUIRE(good && std::fabs(s - 1.0) <= 1e-6, TMVB_ESHAPE, "%s: \xce\xb8 not a probability vector (document %lld)", fn, (long long)d);
    }
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    return ho_loglik_run(ctx, K, V, M, theta, beta, doc_ptr, terms, counts, laplace_smooth, ll, tokens, zero_prob_tokens, ms_kernel);
}
