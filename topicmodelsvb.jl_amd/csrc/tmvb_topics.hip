// tmvb_topics.hip -- model.topics behind train!, on the device.
//
// Every train! of the reference ends with
//     model.topics = [reverse(sortperm(vec(model.beta[i,:]))) for i in 1:model.K]          src/gpuLDA.jl:374 (CTM, CTPF, fLDA, fCTM alike)
// K stable ascending sorts of V values, read backwards.  On the host that was the largest single item of a train!(iter=150) call next to the
// loop itself (K = 50, V = 25 319: 65 ms of 209, profiles/r6_train_end_to_end.txt).  Here: one segmented radix sort of (value, column) pairs
// (rocPRIM through hipcub -- a library sort is what this is; stable, so ties keep the order sortperm gives them), written out reversed and 1-based.
#include "tmvb_internal.h"
#include "tmvb_call.h"

#include <algorithm>
#include <hipcub/hipcub.hpp>

// keys[i][j] = B[i + K j] (the model's column-major K x V field), vals[i][j] = j
static __global__ __launch_bounds__(256) void topics_keys_kernel(const double* __restrict__ B, int K, int64_t V, double* __restrict__ keys, int32_t* __restrict__ vals)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)K * V) return;
    const int64_t i = q / V, j = q - i * V;
    keys[q] = B[i + (int64_t)K * j];
    vals[q] = (int32_t)j;
}

// out[i][j] = 1 + (column of the j-th LARGEST value of row i) = the ascending order read backwards
static __global__ __launch_bounds__(256) void topics_reverse_kernel(const int32_t* __restrict__ sorted, int K, int64_t V, int32_t* __restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)K * V) return;
    const int64_t i = q / V, j = q - i * V;
    out[q] = sorted[i * V + (V - 1 - j)] + 1;
}

static __global__ void topics_offsets_kernel(int* __restrict__ off, int K, int64_t V)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= K) off[i] = (int)((int64_t)i * V);
}

// K segments of V pairs, one library sort; stable either way (tmvb_internal.h).  tmvb_topic_order sorts ascending and reads backwards, as the reference does;
// tmvb_term_relevance (tmvb_topic_compare.hip) sorts descending, so that equal scores keep ascending term ids.
int tmvb_segmented_sort_pairs(tmvb_call& c, int K, int64_t V, const double* d_keys, const int32_t* d_vals, bool descending, double** d_sorted_keys,
                              int32_t** d_sorted_vals)
{
    const int64_t n = (int64_t)K * V;
    hipStream_t st = c.stream;
    int* d_off;
    char* d_tmp;
    TMVB_CALL_TRY(c, c.alloc(d_sorted_keys, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(d_sorted_vals, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(&d_off, (size_t)K + 1));
    hipLaunchKernelGGL(topics_offsets_kernel, dim3((unsigned)((K + 256) / 256)), dim3(256), 0, st, d_off, (int)K, V);
    TMVB_CALL_HIP(c, hipGetLastError());
    size_t tmp_bytes = 0;
    if (descending) {
        TMVB_CALL_HIP(c, hipcub::DeviceSegmentedRadixSort::SortPairsDescending(nullptr, tmp_bytes, d_keys, *d_sorted_keys, d_vals, *d_sorted_vals, (int)n, (int)K,
                                                                               (const int*)d_off, (const int*)d_off + 1, 0, 64, st));
        TMVB_CALL_TRY(c, c.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 16)));
        TMVB_CALL_HIP(c, hipcub::DeviceSegmentedRadixSort::SortPairsDescending((void*)d_tmp, tmp_bytes, d_keys, *d_sorted_keys, d_vals, *d_sorted_vals, (int)n, (int)K,
                                                                               (const int*)d_off, (const int*)d_off + 1, 0, 64, st));
    } else {
        TMVB_CALL_HIP(c, hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, tmp_bytes, d_keys, *d_sorted_keys, d_vals, *d_sorted_vals, (int)n, (int)K,
                                                                     (const int*)d_off, (const int*)d_off + 1, 0, 64, st));
        TMVB_CALL_TRY(c, c.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 16)));
        TMVB_CALL_HIP(c, hipcub::DeviceSegmentedRadixSort::SortPairs((void*)d_tmp, tmp_bytes, d_keys, *d_sorted_keys, d_vals, *d_sorted_vals, (int)n, (int)K,
                                                                     (const int*)d_off, (const int*)d_off + 1, 0, 64, st));
    }
    return TMVB_OK;
}

extern "C" int tmvb_topic_order(tmvb_ctx* ctx, const double* beta, int32_t K, int64_t V, int32_t* topics)
{
    TMVB_REQUIRE(ctx != nullptr, TMVB_EINVAL, "tmvb_topic_order: ctx is NULL");
    TMVB_REQUIRE(K > 0 && V >= 0, TMVB_EINVAL, "tmvb_topic_order: K must be positive, V nonnegative");
    if (V == 0) return TMVB_OK;
    TMVB_REQUIRE(beta && topics, TMVB_EINVAL, "tmvb_topic_order: NULL argument");
    const int64_t n = (int64_t)K * V;
    TMVB_REQUIRE(n < (int64_t)INT32_MAX, TMVB_EINVAL, "tmvb_topic_order: K * V must fit int32");
    hipStream_t st = ctx->stream;
    tmvb_call c("topic_order", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    double *d_in, *d_keys, *d_keys2;
    int32_t *d_vals, *d_vals2;
    TMVB_CALL_TRY(c, c.alloc(&d_keys, (size_t)n)); TMVB_CALL_TRY(c, c.alloc(&d_vals, (size_t)n)); TMVB_CALL_TRY(c, c.upload(&d_in, beta, (size_t)n));
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(topics_keys_kernel, dim3(nb), dim3(256), 0, st, (const double*)d_in, (int)K, V, d_keys, d_vals);
    TMVB_CALL_HIP(c, hipGetLastError());
    const int rc = tmvb_segmented_sort_pairs(c, (int)K, V, d_keys, d_vals, false, &d_keys2, &d_vals2);
    if (rc != TMVB_OK) return rc;
    hipLaunchKernelGGL(topics_reverse_kernel, dim3(nb), dim3(256), 0, st, (const int32_t*)d_vals2, (int)K, V, d_vals);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipMemcpyAsync(topics, d_vals, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    return TMVB_OK;
}
