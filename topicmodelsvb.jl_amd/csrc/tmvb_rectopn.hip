// tmvb_rectopn.hip -- top-n recommendations: for every query the n best database rows outside the query's exclusion list, the exclusions fused
// into the score scan (include/tmvb.h states the definition; the reference's consumers are showurecs / showdrecs, which read 15 entries of a
// full ranking).
//
// tmvb_score_topn.  The n first rows of [0, Md) \ excl(q) under the total order of the reference's reverse(sortperm(.)): s_e > s_t, or
//   s_e == s_t and e > t.  No score matrix, no sort.
//   prep      rt_feature_kernel: fp64 -> fp32 [M][kp], the layout of tmvb_nbtile.h (shared with tmvb_neighbors.hip and tmvb_recranks.hip).
//   scan      rt_scan_kernel: the tile loop of nb_scan_kernel / rk_scan_kernel (nb_tile_scores, so a pair's score has the same bits in all three
//             units) with the epilogue of nb_scan_kernel under the other order.  Grid (query tile of 128, database split).  Every query has a
//             sorted list of its n best so far in LDS -- empty slots are (-inf, -1), the worst key under this order -- and its threshold = slot
//             n - 1.  A lane tests each of its 64 accumulator entries (masked first: query >= Mq, row >= Md) against the threshold of the
//             entry's query: one LDS read.  Only a survivor is looked up in its query's exclusion list, a binary search over
//             excl_idx[excl_ptr[q] .. excl_ptr[q + 1]) in global memory, and only a survivor that is not listed is marked pending: an excluded
//             row never enters a round.  Every (query, row) pair is met once per call, so an excluded row costs at most one search; the rows of
//             a library are exactly the high scorers -- they pass the threshold whenever they are met --, which is why the search sits behind
//             the threshold and not in front of it: in front, every one of the Mq x Md entries would pay for it.  The rounds are those of
//             nb_scan_kernel: survivors are tested again (the threshold moves between rounds, the list membership does not) and appended to
//             a buffer of RT_CAND entries through an LDS counter; wave w inserts the buffered entries of the queries q with (q & 3) == w, lane
//             j holding slot j.  A list is touched by one wave only, an entry is appended once, and the n best of a set do not depend on the
//             order of insertion.
//   merge     rt_merge_kernel: one wave per query, the splits x n partial entries into a register list by the same insertion.  Skipped with
//             one split.
// No atomics on global memory (the append counter is LDS), no scratch: the 64 accumulator entries are walked by fully unrolled loops.
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_nbtile.h"

#include <algorithm>
#include <cstring>
#include <limits>

#define RT_CAND 1024                // survivors buffered per round

// the total order of reverse(sortperm(.)): (s, i) comes before (t, j)
__host__ __device__ __forceinline__ bool rt_before(float s, int i, float t, int j) { return s > t || (s == t && i > j); }

// ------------------------------------------------------------------------------------------------------------------ prep
static __global__ __launch_bounds__(NB_WG) void rt_feature_kernel(int K, int kp, int64_t M, const double* __restrict__ x, float* __restrict__ f)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6);
    if (r >= M) return;                                 // wave-uniform
    nb_feature_row(K, kp, TMVB_NB_DOT, x + r * K, f + r * kp, lane);
}

// ------------------------------------------------------------------------------------------------------------------ scan
// is e among xi[lo .. lo + n), strictly ascending?
__device__ __forceinline__ bool rt_listed(const int32_t* __restrict__ xi, int lo, int n, int e)
{
#ifdef TMVB_MUTANT_TOPN_MISS_LAST_EXCL
    n -= 1;                                             // MUTANT: the last id of every list is never found
#endif
    while (n > 0) {
        const int h = n >> 1;
        const int v = xi[lo + h];
        if (v == e) return true;
        if (v < e) { lo += h + 1; n -= h + 1; }
        else n = h;
    }
    return false;
}

// one wave, lane j = slot j of list[n] (sorted, LDS): insert (cs, ci) if it is among the n best; the threshold follows slot n - 1
__device__ __forceinline__ void rt_insert(float2* list, int n, float cs, int ci, float2* thr, int lane)
{
    float s = -INFINITY;
    int i = -1;
    if (lane < n) { const float2 v = list[lane]; s = v.x; i = __float_as_int(v.y); }
    const bool ahead = lane < n && rt_before(s, i, cs, ci);
    const int p = __popcll(__ballot(ahead));            // the list is sorted: slots 0 .. p - 1 stay
    if (p >= n) return;                                 // wave-uniform
    const float ps = __shfl_up(s, 1);
    const int pi = __shfl_up(i, 1);
    if (lane < n && lane >= p) {
        const float2 w = lane == p ? make_float2(cs, __int_as_float(ci)) : make_float2(ps, __int_as_float(pi));
        list[lane] = w;
        if (lane == n - 1) *thr = w;
    }
}

// Fq: [Mq][kp], Fd: [Md][kp]; excl_ptr[Mq + 1] (below 2^31 - 1), excl_idx: the exclusion lists.  out_s / out_i: [gridDim.y][Mq][n].
static __global__ __launch_bounds__(NB_WG) void rt_scan_kernel(int kp, int kc_max, int n, int64_t Mq, int64_t Md, int64_t tiles_per_split,
                                                               const float* __restrict__ Fq, const float* __restrict__ Fd,
                                                               const int64_t* __restrict__ excl_ptr, const int32_t* __restrict__ excl_idx,
                                                               float* __restrict__ out_s, int32_t* __restrict__ out_i)
{
    extern __shared__ __attribute__((aligned(16))) float rt_lds[];
    const int S = kc_max + 2;
    float* sA = rt_lds;                                                  // [128][S] queries
    float* sB = sA + NB_QT * S;                                          // [128][S] database rows
    float2* lists = reinterpret_cast<float2*>(sB + NB_TD * S);           // [128][n]  (128 S floats = a multiple of 8 bytes)
    float2* thr = lists + NB_QT * n;                                     // [128]
    float* cand_s = reinterpret_cast<float*>(thr + NB_QT);               // [RT_CAND]
    int* cand_e = reinterpret_cast<int*>(cand_s + RT_CAND);              // [RT_CAND]
    int* cand_q = cand_e + RT_CAND;                                      // [RT_CAND]
    int* x_lo = cand_q + RT_CAND;                                        // [128] first entry of a query's exclusion list
    int* x_n = x_lo + NB_QT;                                             // [128] its length
    int* s_cnt = x_n + NB_QT;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave >> 1, wd = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int64_t qt0 = (int64_t)blockIdx.x * NB_QT;
    const int64_t ntiles = (Md + NB_TD - 1) / NB_TD;
    const int64_t t_begin = (int64_t)blockIdx.y * tiles_per_split, t_end = min(t_begin + tiles_per_split, ntiles);
    const bool one_chunk = kp <= kc_max;

    const float2 empty = make_float2(-INFINITY, __int_as_float(-1));
    for (int u = tid; u < NB_QT * n; u += NB_WG) lists[u] = empty;
    if (tid < NB_QT) {
        thr[tid] = empty;
        int lo = 0, len = 0;
        if (qt0 + tid < Mq) { lo = (int)excl_ptr[qt0 + tid]; len = (int)(excl_ptr[qt0 + tid + 1] - excl_ptr[qt0 + tid]); }
        x_lo[tid] = lo; x_n[tid] = len;
    }
    if (one_chunk && t_begin < t_end) nb_stage(sA, S, Fq, qt0, Mq, kp, 0, kp);
    // (the first barrier of the tile loop orders these writes before any read)

    for (int64_t t = t_begin; t < t_end; t++) {
        const int64_t e0 = t * NB_TD;
        nb_f32x16 acc[2][2];
        nb_tile_scores(acc, sA, sB, S, kp, kc_max, one_chunk, Fq, qt0, Mq, Fd, e0, Md, wq, wd, l31, half);
        // ---- epilogue.  C/D layout: column (database row) = lane & 31, row (query) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        unsigned long long pend = 0ull;
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int q = 64 * wq + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const int64_t e = e0 + 64 * wd + 32 * b + l31;
                    if (qt0 + q < Mq && e < Md) {                                // masked before the test
                        const float2 th = thr[q];
                        if (rt_before(acc[a][b][r], (int)e, th.x, __float_as_int(th.y)) && !rt_listed(excl_idx, x_lo[q], x_n[q], (int)e))
                            pend |= 1ull << (32 * a + 16 * b + r);
                    }
                }
        while (__syncthreads_or(pend != 0ull)) {
            if (tid == 0) *s_cnt = 0;
            __syncthreads();
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const unsigned long long bit = 1ull << (32 * a + 16 * b + r);
                        if (pend & bit) {
                            const int q = 64 * wq + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * half;
                            const int e = (int)(e0 + 64 * wd + 32 * b + l31);
                            const float2 th = thr[q];
                            if (!rt_before(acc[a][b][r], e, th.x, __float_as_int(th.y))) pend &= ~bit;
                            else {
                                const int pos = atomicAdd(s_cnt, 1);             // LDS
                                if (pos < RT_CAND) { cand_s[pos] = acc[a][b][r]; cand_e[pos] = e; cand_q[pos] = q; pend &= ~bit; }
                            }
                        }
                    }
            __syncthreads();
            const int nc = min(*s_cnt, RT_CAND);
            for (int c = 0; c < nc; c++) {
                const int q = cand_q[c];
                if ((q & 3) == wave) rt_insert(lists + q * n, n, cand_s[c], cand_e[c], thr + q, lane);
            }
            // the barrier of the loop condition ends the round: lists, thresholds and the counter are settled before the next one
        }
    }
    __syncthreads();
    for (int u = tid; u < NB_QT * n; u += NB_WG) {
        const int q = u / n;
        if (qt0 + q < Mq) {
            const float2 v = lists[u];
            const int64_t o = ((int64_t)blockIdx.y * Mq + qt0 + q) * n + (u - q * n);
            out_s[o] = v.x;
            out_i[o] = __float_as_int(v.y);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ merge
// in_s / in_i: [splits][Mq][n], each list sorted; out: [Mq][n].  One wave per query.
static __global__ __launch_bounds__(NB_WG) void rt_merge_kernel(int n, int splits, int64_t Mq, const float* __restrict__ in_s, const int32_t* __restrict__ in_i,
                                                                float* __restrict__ out_s, int32_t* __restrict__ out_i)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6);
    if (q >= Mq) return;                                // wave-uniform
    float s = -INFINITY;
    int i = -1;
    for (int sp = 0; sp < splits; sp++) {
        const int64_t o = ((int64_t)sp * Mq + q) * n;
        for (int j = 0; j < n; j++) {
            const float cs = in_s[o + j];
            const int ci = in_i[o + j];
            const float ts = __shfl(s, n - 1);
            const int ti = __shfl(i, n - 1);
            if (!rt_before(cs, ci, ts, ti)) break;      // wave-uniform; the rest of this list comes after cs (an empty slot comes before nothing)
            const bool ahead = lane < n && rt_before(s, i, cs, ci);
            const int p = __popcll(__ballot(ahead));
            const float ps = __shfl_up(s, 1);
            const int pi = __shfl_up(i, 1);
            if (lane == p) { s = cs; i = ci; }
            else if (lane > p) { s = ps; i = pi; }
        }
    }
    if (lane < n) { out_s[q * n + lane] = s; out_i[q * n + lane] = i; }
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
int rt_check_rows(const char* fn, const char* side, int32_t K, int64_t M, const double* x)
{
    for (int64_t r = 0; r < M; r++)
        for (int k = 0; k < K; k++)
            TMVB_REQUIRE(std::isfinite(x[k + (int64_t)K * r]), TMVB_ESHAPE, "%s: non-finite entry (%s row %lld)", fn, side, (long long)r);
    return TMVB_OK;
}

size_t rt_scan_lds(int kc, int n)
{
    return (size_t)2 * 128 * (kc + 2) * sizeof(float) + (size_t)NB_QT * n * sizeof(float2) + NB_QT * sizeof(float2) + (size_t)RT_CAND * 12 +
           2 * NB_QT * sizeof(int) + 16;
}

int rt_run(tmvb_ctx* ctx, int32_t K, int64_t Md, const double* xd, int64_t Mq, const double* xq, const int64_t* excl_ptr, const int32_t* excl_idx,
           int32_t n, int32_t splits_arg, int32_t* idx, float* score, int32_t* count, tmvb_rectopn_info_t* info)
{
    const int kp = (K + 3) & ~3, kc = kp <= NB_KC_ONE ? kp : NB_KC;
    const int64_t ntiles = (Md + NB_TD - 1) / NB_TD, qtiles = (Mq + NB_QT - 1) / NB_QT, nE = excl_ptr[Mq];
    // splits: forced, or enough workgroups for two per CU; never more than there are database tiles (or than a grid's y extent)
    int64_t splits = splits_arg;
    if (splits <= 0) {
        const int64_t want = 2 * (int64_t)ctx->num_cu;
        splits = qtiles >= want ? 1 : (want + qtiles - 1) / qtiles;
    }
    splits = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(splits, ntiles), 65535));
    const int64_t tps = (ntiles + splits - 1) / splits;
    splits = (ntiles + tps - 1) / tps;                  // no empty split

    hipStream_t st = ctx->stream;
    tmvb_call c("score_topn", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(6));
    double *d_xd, *d_xq;
    float *d_fd, *d_fq, *d_ps, *d_os = nullptr;
    int32_t *d_xi, *d_pi, *d_oi = nullptr;
    int64_t* d_xp;
    const size_t out_n = (size_t)Mq * n;
    TMVB_CALL_TRY(c, c.upload(&d_xd, xd, (size_t)Md * K)); TMVB_CALL_TRY(c, c.upload(&d_xq, xq, (size_t)Mq * K));
    TMVB_CALL_TRY(c, c.upload(&d_xp, excl_ptr, (size_t)Mq + 1)); TMVB_CALL_TRY(c, c.upload(&d_xi, excl_idx, (size_t)nE));
    TMVB_CALL_TRY(c, c.alloc(&d_fd, (size_t)Md * kp)); TMVB_CALL_TRY(c, c.alloc(&d_fq, (size_t)Mq * kp));
    TMVB_CALL_TRY(c, c.alloc(&d_ps, (size_t)splits * out_n)); TMVB_CALL_TRY(c, c.alloc(&d_pi, (size_t)splits * out_n));
    if (splits > 1) { TMVB_CALL_TRY(c, c.alloc(&d_os, out_n)); TMVB_CALL_TRY(c, c.alloc(&d_oi, out_n)); }
    const size_t lds = rt_scan_lds(kc, n);
    if (lds > 48 * 1024) TMVB_CALL_HIP(c, hipFuncSetAttribute((const void*)rt_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    // stage times: the events bracket the kernels only; allocations and copies lie outside
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(rt_feature_kernel, dim3((unsigned)((Md + 3) / 4)), dim3(NB_WG), 0, st, (int)K, kp, Md, (const double*)d_xd, d_fd);
    hipLaunchKernelGGL(rt_feature_kernel, dim3((unsigned)((Mq + 3) / 4)), dim3(NB_WG), 0, st, (int)K, kp, Mq, (const double*)d_xq, d_fq);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    hipLaunchKernelGGL(rt_scan_kernel, dim3((unsigned)qtiles, (unsigned)splits), dim3(NB_WG), lds, st, kp, kc, (int)n, Mq, Md, tps, (const float*)d_fq,
                       (const float*)d_fd, (const int64_t*)d_xp, (const int32_t*)d_xi, d_ps, d_pi);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
    if (splits > 1) {
        hipLaunchKernelGGL(rt_merge_kernel, dim3((unsigned)((Mq + 3) / 4)), dim3(NB_WG), 0, st, (int)n, (int)splits, Mq, (const float*)d_ps, (const int32_t*)d_pi, d_os,
                           d_oi);
        TMVB_CALL_HIP(c, hipGetLastError());
    }
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(score, splits > 1 ? d_os : d_ps, out_n * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(idx, splits > 1 ? d_oi : d_pi, out_n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    for (int64_t q = 0; q < Mq; q++) {                  // a list is full from the front: the empty slots (-1, -inf) follow the entries
        int32_t k = 0;
        while (k < n && idx[q * n + k] >= 0) k++;
        count[q] = k;
    }
    if (info) {
        info->splits = (int32_t)splits; info->kp = kp;
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_prep, 0, 1));
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_scan, 2, 3));
        if (splits > 1) TMVB_CALL_TRY(c, c.elapsed(&info->ms_merge, 4, 5));
    }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_score_topn(tmvb_ctx* ctx, int32_t K, int64_t Md, const double* xd, int64_t Mq, const double* xq, const int64_t* excl_ptr,
                               const int32_t* excl_idx, int32_t n, int32_t splits, int32_t* idx, float* score, int32_t* count, tmvb_rectopn_info_t* info)
{
    const char* fn = "tmvb_score_topn";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(K >= 1 && K <= NB_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, NB_MAX_K);
    TMVB_REQUIRE(n >= 1 && n <= TMVB_NB_TOPN_MAX, TMVB_EINVAL, "%s: n = %d outside [1, %d]", fn, n, TMVB_NB_TOPN_MAX);
    TMVB_REQUIRE(Md > 0 && Mq > 0, TMVB_EINVAL, "%s: Md and Mq must be positive integers", fn);
    TMVB_REQUIRE(Md < ((int64_t)1 << 31), TMVB_EINVAL, "%s: Md = %lld is 2^31 or more", fn, (long long)Md);
    TMVB_REQUIRE((Mq + NB_QT - 1) / NB_QT <= 0x7fffffffLL, TMVB_EINVAL, "%s: Mq = %lld is more than one call takes (shard the queries)", fn, (long long)Mq);
    TMVB_REQUIRE(splits >= 0 && (int64_t)splits <= Md, TMVB_EINVAL, "%s: splits = %d outside [0, Md]", fn, splits);
    TMVB_REQUIRE(xd && xq && excl_ptr && idx && score && count, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(excl_ptr[0] == 0, TMVB_ESHAPE, "%s: excl_ptr must start at 0", fn);
    for (int64_t q = 0; q < Mq; q++) TMVB_REQUIRE(excl_ptr[q + 1] >= excl_ptr[q], TMVB_ESHAPE, "%s: excl_ptr decreases at query %lld", fn, (long long)q);
    TMVB_REQUIRE(excl_ptr[Mq] < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: %lld excluded ids in one call (limit 2^31 - 2); shard the queries", fn, (long long)excl_ptr[Mq]);
    TMVB_REQUIRE(excl_idx || excl_ptr[Mq] == 0, TMVB_EINVAL, "%s: NULL argument", fn);
    int rc;
    if ((rc = rt_check_rows(fn, "database", K, Md, xd)) != TMVB_OK) return rc;
    if ((rc = rt_check_rows(fn, "query", K, Mq, xq)) != TMVB_OK) return rc;
    for (int64_t q = 0; q < Mq; q++)
        for (int64_t j = excl_ptr[q]; j < excl_ptr[q + 1]; j++) {
            TMVB_REQUIRE(excl_idx[j] >= 0 && excl_idx[j] < Md, TMVB_ESHAPE, "%s: query %lld holds excluded id %d outside [0, %lld)", fn, (long long)q, excl_idx[j], (long long)Md);
            TMVB_REQUIRE(j == excl_ptr[q] || excl_idx[j] > excl_idx[j - 1], TMVB_ESHAPE, "%s: the excluded ids of query %lld are not strictly ascending", fn, (long long)q);
        }
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    return rt_run(ctx, K, Md, xd, Mq, xq, excl_ptr, excl_idx, n, splits, idx, score, count, info);
}
