// tmvb_neighbors.hip -- nearest documents in topic space: f32-MFMA scores with the top-n selection fused into the epilogue (include/tmvb.h
// states the definition; the reference stops at topicdist(model, d)).
//
// tmvb_topic_neighbors.  For every query row the n database rows of highest score under the total order (score descending, index ascending).
//   features  fp64 in (column-major K x M = one row of K doubles per document), transform in fp64, one rounding to fp32, out [M][kp],
//             kp = K rounded up to a multiple of 4, pads zero.  One wave per row; COSINE's norm is a fixed-order sum (lane-strided partial sums,
//             xor butterfly).  Inside every group of four the values sit in the order k = 0, 2, 1, 3: a lane of the lower half of a wave then
//             reads the k = 4t and 4t + 2 of its row with ONE 8-byte LDS read and a lane of the upper half k = 4t + 1 and 4t + 3 -- the operands of
//             two consecutive v_mfma_f32_32x32x2_f32 (lane l holds A[i = l & 31][k = l >> 5]), whose accumulator chain so runs over k in
//             ascending order.
//   scan      grid (query tile, database split), 256 lanes = 2 x 2 waves.  A workgroup owns NB_QT = 128 queries and one split = a run of whole
//             database tiles of TMVB_NB_TILE_DB = 128 rows; a wave owns 64 x 64 of a tile = 2 x 2 accumulators of 32 x 32 (four independent
//             chains).  Both operands go through LDS in K-chunks of kc <= 64 floats with 16-byte global loads (rows past the end read as zero and
//             are never loaded); row stride kc + 2 floats: 8-byte reads of 32 consecutive rows fall on 64 distinct banks.  kp <= 64: one chunk,
//             the query tile is staged once; else chunks of 32, restaged per database tile (the chain order is kept: chunks ascend).
//             Epilogue: every query has a sorted list of its n best so far in LDS -- empty slots are (-inf, INT32_MAX), the worst key there is --
//             and its threshold = slot n - 1.  A lane tests each of its 64 accumulator entries (masked first: query >= Mq, row >= Md, the self
//             row) against the threshold of the entry's query under the total order, and keeps a 64-bit mask of the survivors.  Rounds, until no
//             lane has one left: survivors are tested again (the threshold moves between rounds) and appended to a buffer of NB_CAND entries
//             through an LDS counter -- those that find it full wait for the next round --; then wave w inserts the buffered entries of the
//             queries q with (q & 3) == w: lane j holds slot j, a ballot counts the slots that beat the entry, the rest shift down by one.  A
//             list is touched by one wave only, an entry is appended once, and the n best of a set do not depend on the order of insertion: any
//             visiting order gives the same list (a database sorted ascending makes every entry survive and costs 16 rounds per tile).
//             A threshold read before a round is stale at worst = too low: it admits too much, never too little.
//   merge     one wave per query: the splits x n partial entries, each list in order, into a register list (lane j = slot j) by the same
//             insertion; a partial list is left at its first entry that does not beat the threshold.  Skipped with one split.
// No atomics on global memory (the append counter is LDS), no scratch: the 64 accumulator entries are walked by a fully unrolled loop.
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_nbtile.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <limits>

#define NB_CAND 1024                // survivors buffered per round

// the total order: (s, i) comes before (t, j)
__device__ __forceinline__ bool nb_before(float s, int i, float t, int j) { return s > t || (s == t && i < j); }

// ------------------------------------------------------------------------------------------------------------------ features
// x: column-major K x M fp64 (row r = x[K r ..]); f: [M][kp].  One wave per row.
static __global__ __launch_bounds__(NB_WG) void nb_feature_kernel(int K, int kp, int metric, int64_t M, const double* __restrict__ x, float* __restrict__ f)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6);
    if (r >= M) return;                                 // wave-uniform
    nb_feature_row(K, kp, metric, x + r * K, f + r * kp, lane);
}

// ------------------------------------------------------------------------------------------------------------------ scan
// one wave, lane j = slot j of list[n] (sorted, LDS): insert (cs, ci) if it is among the n best; the threshold follows slot n - 1
__device__ __forceinline__ void nb_insert(float2* list, int n, float cs, int ci, float2* thr, int lane)
{
    float s = -INFINITY;
    int i = INT_MAX;
    if (lane < n) { const float2 v = list[lane]; s = v.x; i = __float_as_int(v.y); }
    const bool ahead = lane < n && nb_before(s, i, cs, ci);
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

// Fq: [>= qbase + Mq][kp] query features (qbase = q0 when the queries are database rows), Fd: [Md][kp]; self0: database row of query 0, or
// a negative number when nothing is excluded.  out_s / out_i: [gridDim.y][Mq][n].
static __global__ __launch_bounds__(NB_WG) void nb_scan_kernel(int kp, int kc_max, int n, int64_t Mq, int64_t Md, int64_t self0, int64_t tiles_per_split,
                                                               const float* __restrict__ Fq, const float* __restrict__ Fd, float* __restrict__ out_s,
                                                               int32_t* __restrict__ out_i)
{
    extern __shared__ __attribute__((aligned(16))) float nb_lds[];
    const int S = kc_max + 2;
    float* sA = nb_lds;                                                  // [128][S] queries
    float* sB = sA + NB_QT * S;                                          // [128][S] database rows
    float2* lists = reinterpret_cast<float2*>(sB + NB_TD * S);           // [128][n]  (128 S floats = a multiple of 8 bytes)
    float2* thr = lists + NB_QT * n;                                     // [128]
    float* cand_s = reinterpret_cast<float*>(thr + NB_QT);               // [NB_CAND]
    int* cand_e = reinterpret_cast<int*>(cand_s + NB_CAND);              // [NB_CAND]
    int* cand_q = cand_e + NB_CAND;                                      // [NB_CAND]
    int* s_cnt = cand_q + NB_CAND;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave >> 1, wd = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int64_t qt0 = (int64_t)blockIdx.x * NB_QT;
#ifdef TMVB_MUTANT_NB_DROP_TAIL
    const int64_t ntiles = Md / NB_TD;                                   // MUTANT: the last, partial database tile is skipped
#else
    const int64_t ntiles = (Md + NB_TD - 1) / NB_TD;
#endif
    const int64_t t_begin = (int64_t)blockIdx.y * tiles_per_split, t_end = min(t_begin + tiles_per_split, ntiles);
    const bool one_chunk = kp <= kc_max;

    const float2 empty = make_float2(-INFINITY, __int_as_float(INT_MAX));
    for (int u = tid; u < NB_QT * n; u += NB_WG) lists[u] = empty;
    if (tid < NB_QT) thr[tid] = empty;
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
                    if (qt0 + q < Mq && e < Md && e != self0 + qt0 + q) {        // masked before the test
                        const float2 th = thr[q];
                        if (nb_before(acc[a][b][r], (int)e, th.x, __float_as_int(th.y))) pend |= 1ull << (32 * a + 16 * b + r);
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
                            if (!nb_before(acc[a][b][r], e, th.x, __float_as_int(th.y))) pend &= ~bit;
                            else {
                                const int pos = atomicAdd(s_cnt, 1);             // LDS
                                if (pos < NB_CAND) { cand_s[pos] = acc[a][b][r]; cand_e[pos] = e; cand_q[pos] = q; pend &= ~bit; }
                            }
                        }
                    }
            __syncthreads();
            const int nc = min(*s_cnt, NB_CAND);
            for (int c = 0; c < nc; c++) {
                const int q = cand_q[c];
                if ((q & 3) == wave) nb_insert(lists + q * n, n, cand_s[c], cand_e[c], thr + q, lane);
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
static __global__ __launch_bounds__(NB_WG) void nb_merge_kernel(int n, int splits, int64_t Mq, const float* __restrict__ in_s, const int32_t* __restrict__ in_i,
                                                                float* __restrict__ out_s, int32_t* __restrict__ out_i)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6);
    if (q >= Mq) return;                                // wave-uniform
    float s = -INFINITY;
    int i = INT_MAX;
    for (int sp = 0; sp < splits; sp++) {
        const int64_t o = ((int64_t)sp * Mq + q) * n;
        for (int j = 0; j < n; j++) {
            const float cs = in_s[o + j];
            const int ci = in_i[o + j];
            const float ts = __shfl(s, n - 1);
            const int ti = __shfl(i, n - 1);
            if (!nb_before(cs, ci, ts, ti)) break;      // wave-uniform; the rest of this list comes after cs
            const bool ahead = lane < n && nb_before(s, i, cs, ci);
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
// the rows of one side, judged on the host
int nb_check_rows(const char* fn, const char* side, int32_t K, int32_t metric, int64_t M, const double* x)
{
    for (int64_t r = 0; r < M; r++) {
        double s = 0.0;
        bool finite = true, nonneg = true, any = false;
        for (int k = 0; k < K; k++) {
            const double v = x[k + (int64_t)K * r];
            if (!std::isfinite(v)) { finite = false; break; }
            if (v < 0.0) nonneg = false;
            if (v != 0.0) any = true;
            s += v;
        }
        TMVB_REQUIRE(finite, TMVB_ESHAPE, "%s: non-finite entry (%s row %lld)", fn, side, (long long)r);
        if (metric == TMVB_NB_HELLINGER)
            TMVB_REQUIRE(nonneg && std::fabs(s - 1.0) <= 1e-6, TMVB_ESHAPE, "%s: \xce\xb8 not a probability vector (%s row %lld)", fn, side, (long long)r);
        if (metric == TMVB_NB_COSINE) {
            TMVB_REQUIRE(nonneg, TMVB_ESHAPE, "%s: negative entry (%s row %lld)", fn, side, (long long)r);
            TMVB_REQUIRE(any, TMVB_ESHAPE, "%s: all-zero row (%s row %lld)", fn, side, (long long)r);
        }
    }
    return TMVB_OK;
}

size_t nb_scan_lds(int kc, int n)
{
    return (size_t)2 * 128 * (kc + 2) * sizeof(float) + (size_t)NB_QT * n * sizeof(float2) + NB_QT * sizeof(float2) + (size_t)NB_CAND * 12 + 16;
}

int nb_run(tmvb_ctx* ctx, int32_t K, int32_t metric, int64_t Md, const double* xd, int64_t Mq, const double* xq, int64_t q0, int32_t n, int32_t splits_arg,
           int32_t* idx, float* score, int32_t* count, tmvb_neighbors_info_t* info)
{
    const int kp = (K + 3) & ~3, kc = kp <= NB_KC_ONE ? kp : NB_KC;
    const int64_t ntiles = (Md + NB_TD - 1) / NB_TD, qtiles = (Mq + NB_QT - 1) / NB_QT;
    TMVB_REQUIRE(qtiles <= 0x7fffffffLL, TMVB_EINVAL, "tmvb_topic_neighbors: Mq = %lld is more than one call takes (shard the queries through q0)", (long long)Mq);
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
    tmvb_call c("topic_neighbors", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(6));
    double *d_xd, *d_xq = nullptr;
    float *d_fd, *d_fq = nullptr, *d_ps, *d_os = nullptr;
    int32_t *d_pi, *d_oi = nullptr;
    const size_t out_n = (size_t)Mq * n;
    TMVB_CALL_TRY(c, c.alloc(&d_xd, (size_t)Md * K)); TMVB_CALL_TRY(c, c.alloc(&d_fd, (size_t)Md * kp));
    TMVB_CALL_TRY(c, c.alloc(&d_ps, (size_t)splits * out_n)); TMVB_CALL_TRY(c, c.alloc(&d_pi, (size_t)splits * out_n));
    if (xq) { TMVB_CALL_TRY(c, c.alloc(&d_xq, (size_t)Mq * K)); TMVB_CALL_TRY(c, c.alloc(&d_fq, (size_t)Mq * kp)); }
    if (splits > 1) { TMVB_CALL_TRY(c, c.alloc(&d_os, out_n)); TMVB_CALL_TRY(c, c.alloc(&d_oi, out_n)); }
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_xd, xd, (size_t)Md * K * sizeof(double), hipMemcpyHostToDevice, st));
    if (xq) TMVB_CALL_HIP(c, hipMemcpyAsync(d_xq, xq, (size_t)Mq * K * sizeof(double), hipMemcpyHostToDevice, st));
    const size_t lds = nb_scan_lds(kc, n);
    if (lds > 48 * 1024) TMVB_CALL_HIP(c, hipFuncSetAttribute((const void*)nb_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    // stage times: the events bracket the kernels only; allocations and copies lie outside
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(nb_feature_kernel, dim3((unsigned)((Md + 3) / 4)), dim3(NB_WG), 0, st, (int)K, kp, (int)metric, Md, (const double*)d_xd, d_fd);
    if (xq) hipLaunchKernelGGL(nb_feature_kernel, dim3((unsigned)((Mq + 3) / 4)), dim3(NB_WG), 0, st, (int)K, kp, (int)metric, Mq, (const double*)d_xq, d_fq);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    const float* fq = xq ? d_fq : d_fd + q0 * kp;
    const int64_t self0 = xq ? -((int64_t)1 << 40) : q0;
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    hipLaunchKernelGGL(nb_scan_kernel, dim3((unsigned)qtiles, (unsigned)splits), dim3(NB_WG), lds, st, kp, kc, (int)n, Mq, Md, self0, tps, fq, (const float*)d_fd,
                       d_ps, d_pi);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
    if (splits > 1) {
        hipLaunchKernelGGL(nb_merge_kernel, dim3((unsigned)((Mq + 3) / 4)), dim3(NB_WG), 0, st, (int)n, (int)splits, Mq, (const float*)d_ps, (const int32_t*)d_pi, d_os,
                           d_oi);
        TMVB_CALL_HIP(c, hipGetLastError());
    }
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(score, splits > 1 ? d_os : d_ps, out_n * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(idx, splits > 1 ? d_oi : d_pi, out_n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    for (int64_t q = 0; q < Mq; q++) {                  // empty slots: idx = -1, score = -inf (the device's sentinel index is INT32_MAX)
        int32_t c = 0;
        for (int j = 0; j < n; j++) {
            int32_t& e = idx[q * n + j];
            if (e == INT_MAX) { e = -1; score[q * n + j] = -std::numeric_limits<float>::infinity(); }
            else c++;
        }
        count[q] = c;
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

extern "C" int tmvb_topic_neighbors(tmvb_ctx* ctx, int32_t K, int32_t metric, int64_t Md, const double* xd, int64_t Mq, const double* xq, int64_t q0, int32_t n,
                                    int32_t splits, int32_t* idx, float* score, int32_t* count, tmvb_neighbors_info_t* info)
{
    const char* fn = "tmvb_topic_neighbors";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(K >= 1 && K <= NB_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, NB_MAX_K);
    TMVB_REQUIRE(n >= 1 && n <= TMVB_NB_TOPN_MAX, TMVB_EINVAL, "%s: n = %d outside [1, %d]", fn, n, TMVB_NB_TOPN_MAX);
    TMVB_REQUIRE(metric == TMVB_NB_DOT || metric == TMVB_NB_HELLINGER || metric == TMVB_NB_COSINE, TMVB_EINVAL, "%s: unknown metric %d", fn, metric);
    TMVB_REQUIRE(Md > 0 && Mq > 0, TMVB_EINVAL, "%s: Md and Mq must be positive integers", fn);
    TMVB_REQUIRE(Md < ((int64_t)1 << 31), TMVB_EINVAL, "%s: Md = %lld is 2^31 or more", fn, (long long)Md);
    TMVB_REQUIRE(splits >= 0 && (int64_t)splits <= Md, TMVB_EINVAL, "%s: splits = %d outside [0, Md]", fn, splits);
    TMVB_REQUIRE(q0 >= 0, TMVB_EINVAL, "%s: q0 must be nonnegative", fn);
    if (xq) TMVB_REQUIRE(q0 == 0, TMVB_EINVAL, "%s: q0 must be 0 with explicit queries", fn);
    else TMVB_REQUIRE(Mq <= Md && q0 <= Md - Mq, TMVB_EINVAL, "%s: queries [%lld, %lld) are not rows of a database of %lld", fn, (long long)q0, (long long)(q0 + Mq), (long long)Md);
    TMVB_REQUIRE(xd && idx && score && count, TMVB_EINVAL, "%s: NULL argument", fn);
    int rc = nb_check_rows(fn, "database", K, metric, Md, xd);
    if (rc != TMVB_OK) return rc;
    if (xq && (rc = nb_check_rows(fn, "query", K, metric, Mq, xq)) != TMVB_OK) return rc;
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    return nb_run(ctx, K, metric, Md, xd, Mq, xq, q0, n, splits, idx, score, count, info);
}
