// tmvb_search.hip -- search documents by words: the query likelihood of LDA-based retrieval with the top-n selection fused into the epilogue
// (include/tmvb.h states the definition; the reference has no such function).
//
// tmvb_topic_search.  score(q, d) = (float) sum_j c_j log((double) p(d, j)), p(d, j) = the fp32 fmaf chain of theta_d . beta'_{w_j} over k ascending;
//   for every query the n documents of highest score under the total order of tmvb_topic_neighbors (score descending, index ascending).
//   host      beta' = (beta + s) / (1 + s V) in fp64, rounded once, ONLY the columns the queries name, in the feature layout of tmvb_nbtile.h.  Whole
//             queries are packed in order into column tiles of TMVB_SEARCH_TILE_COLS = 128 entries; no query straddles a tile; pad columns are
//             zero rows with count 0 and belong to no query's segment: they are never looked at.
//   prep      sr_feature_kernel: theta fp64 -> fp32 [Md][kp] (nb_feature_row, DOT).
//   scan      sr_scan_kernel: grid (column tile, database split), 256 lanes = 2 x 2 waves.  Per database tile of 128 rows
//             1. nb_tile_scores: the 128 x 128 tile of p in accumulators -- the tile loop of nb_scan_kernel, so p has the bits of
//                tmvb_topic_neighbors (DOT) for that pair.  Both operands are restaged per tile (the p tile below lies over the staging area);
//             2. the p tile goes to LDS as fp32 [column][row], 64 KB, over the operand staging area, which is dead after the tile's last MFMA
//                (one barrier in between);
//             3. lane (row d = tid & 127, parity h = tid >> 7) takes the pairs (d, q) of the tile's queries q = h, h + 2, ...: it walks the
//                query's column segment in j order, takes the fp64 log of p and accumulates fma(c_j, log p, acc) in ONE fp64 register, rounds once
//                to fp32 and tests the score against the query's threshold (slot n - 1 of its sorted list in LDS).  Rows >= Md are masked first.
//                A survivor is appended to a buffer of SR_CAND entries through an LDS counter; then wave w inserts the buffered entries of
//                the queries with (q & 3) == w (nb_scan_kernel's insertion).  A pair that found the buffer full keeps its bit in a 64-bit mask
//                and is scored again in the next round (the same operations on the same LDS words: the same bits); rounds repeat until no lane
//                has a bit left.  After the first tiles of a split almost nothing survives the threshold and a tile is one round.
//             A list is touched by one wave only, an entry is appended once, and the n best of a set do not depend on the order of insertion.
//   merge     sr_merge_kernel: one wave per query, the splits x n partial entries into a register list by the same insertion.  Skipped with one
//             split.
// No atomics on global memory (the append counter is LDS), no scratch: the scores are never kept, a 64-bit mask says which are still owed.
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_nbtile.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <limits>

#define SR_CAND 1024                // survivors buffered per round
#define SR_TC TMVB_SEARCH_TILE_COLS
static_assert(SR_TC == NB_QT, "a column tile is the query side of the 2 x 2 wave tile");

// the total order of tmvb_topic_neighbors: (s, i) comes before (t, j)
__device__ __forceinline__ bool sr_before(float s, int i, float t, int j) { return s > t || (s == t && i < j); }

// ------------------------------------------------------------------------------------------------------------------ prep
static __global__ __launch_bounds__(NB_WG) void sr_feature_kernel(int K, int kp, int64_t M, const double* __restrict__ x, float* __restrict__ f)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6);
    if (r >= M) return;                                 // wave-uniform
    nb_feature_row(K, kp, TMVB_NB_DOT, x + r * K, f + r * kp, lane);
}

// ------------------------------------------------------------------------------------------------------------------ scan
// one wave, lane j = slot j of list[n] (sorted, LDS): insert (cs, ci) if it is among the n best; the threshold follows slot n - 1
__device__ __forceinline__ void sr_insert(float2* list, int n, float cs, int ci, float2* thr, int lane)
{
    float s = -INFINITY;
    int i = INT_MAX;
    if (lane < n) { const float2 v = list[lane]; s = v.x; i = __float_as_int(v.y); }
    const bool ahead = lane < n && sr_before(s, i, cs, ci);
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

// floats of the area that holds the operand staging [2][128][S] during the MFMAs and the p tile [128][128] after them
__host__ __device__ __forceinline__ int sr_area_floats(int S) { return 2 * 128 * S > SR_TC * NB_TD ? 2 * 128 * S : SR_TC * NB_TD; }

// Fb: [ncols][kp] beta' features of the packed query entries (ncols = 128 x column tiles), Fd: [Md][kp]; tile_q0[column tiles + 1]: first query
// of a tile; qmeta[Q]: first column of a query inside its tile | (entries << 8); colcnt[ncols]: the entries' counts (0 on pad columns).
// out_s / out_i: [gridDim.y][Q][n].
static __global__ __launch_bounds__(NB_WG) void sr_scan_kernel(int kp, int kc_max, int n, int64_t Q, int64_t Md, int64_t tiles_per_split, int64_t ncols,
                                                               const float* __restrict__ Fb, const float* __restrict__ Fd,
                                                               const int32_t* __restrict__ tile_q0, const int32_t* __restrict__ qmeta,
                                                               const int32_t* __restrict__ colcnt, float* __restrict__ out_s, int32_t* __restrict__ out_i)
{
    extern __shared__ __attribute__((aligned(16))) float sr_lds[];
    const int S = kc_max + 2;
    float* sA = sr_lds;                                                  // [128][S] query entries (beta' columns)
    float* sB = sA + SR_TC * S;                                          // [128][S] database rows
    float* P = sr_lds;                                                   // [128 columns][128 rows], over sA / sB once the tile's MFMAs are done
    float2* lists = reinterpret_cast<float2*>(sr_lds + sr_area_floats(S));   // [128][n]  (an even number of floats in front)
    float2* thr = lists + SR_TC * n;                                     // [128]
    float* cand_s = reinterpret_cast<float*>(thr + SR_TC);               // [SR_CAND]
    int* cand_e = reinterpret_cast<int*>(cand_s + SR_CAND);              // [SR_CAND]
    int* cand_q = cand_e + SR_CAND;                                      // [SR_CAND]
    int* seg_lo = cand_q + SR_CAND;                                      // [128] first column of a query of this tile
    int* seg_n = seg_lo + SR_TC;                                         // [128] its entries
    int* ccnt = seg_n + SR_TC;                                           // [128] count of a column
    int* s_cnt = ccnt + SR_TC;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave >> 1, wd = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int64_t c0 = (int64_t)blockIdx.x * SR_TC;                      // first column of this tile in Fb
    const int q0 = tile_q0[blockIdx.x], nq = tile_q0[blockIdx.x + 1] - q0;   // 1 <= nq <= 128: every query has an entry
    const int64_t ntiles = (Md + NB_TD - 1) / NB_TD;
    const int64_t t_begin = (int64_t)blockIdx.y * tiles_per_split, t_end = min(t_begin + tiles_per_split, ntiles);

    const float2 empty = make_float2(-INFINITY, __int_as_float(INT_MAX));
    for (int u = tid; u < SR_TC * n; u += NB_WG) lists[u] = empty;
    if (tid < SR_TC) {
        thr[tid] = empty;
        ccnt[tid] = colcnt[c0 + tid];
        int lo = 0, len = 0;
        if (tid < nq) { const int m = qmeta[q0 + tid]; lo = m & 255; len = m >> 8; }
        seg_lo[tid] = lo; seg_n[tid] = len;
    }
    // (the first barrier of the tile loop orders these writes before any read)

    const int d = tid & 127, qh = tid >> 7;             // this lane's row of a tile; its queries are qh, qh + 2, ...
    const int nit = (nq - qh + 1) >> 1;                 // how many of them: at most 64
    for (int64_t t = t_begin; t < t_end; t++) {
        const int64_t e0 = t * NB_TD;
        {
            nb_f32x16 acc[2][2];
            nb_tile_scores(acc, sA, sB, S, kp, kc_max, false, Fb, c0, ncols, Fd, e0, Md, wq, wd, l31, half);
            __syncthreads();                                             // every wave has read its operands: the area is free
            // C/D layout: column (database row) = lane & 31, row (query entry) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int j = 64 * wq + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * half;
                        P[j * NB_TD + 64 * wd + 32 * b + l31] = acc[a][b][r];
                    }
        }
        // bit i: the pair (row d, query qh + 2 i) is still owed.  Rows past the end are masked here, before anything is scored.
        unsigned long long pend = 0ull;
        if (e0 + d < Md && nit > 0) pend = nit >= 64 ? ~0ull : (1ull << nit) - 1ull;
        const int e = (int)(e0 + d);
        while (__syncthreads_or(pend != 0ull)) {                         // (its first barrier: the p tile is written)
            if (tid == 0) *s_cnt = 0;
            __syncthreads();
            for (int it = 0; it < nit; it++) {
                const unsigned long long bit = 1ull << it;
                if (!(pend & bit)) continue;
                const int q = qh + 2 * it;
                const int lo = seg_lo[q];
#ifdef TMVB_MUTANT_SEARCH_DROP_LAST_ENTRY
                const int hi = lo + seg_n[q] - 1;                        // MUTANT: the segment walk stops one entry early
#else
                const int hi = lo + seg_n[q];
#endif
                double a = 0.0;
                for (int j = lo; j < hi; j++) a = fma((double)ccnt[j], log((double)P[j * NB_TD + d]), a);
                const float s = (float)a;
                const float2 th = thr[q];
                if (!sr_before(s, e, th.x, __float_as_int(th.y))) pend &= ~bit;
                else {
                    const int pos = atomicAdd(s_cnt, 1);                 // LDS
                    if (pos < SR_CAND) { cand_s[pos] = s; cand_e[pos] = e; cand_q[pos] = q; pend &= ~bit; }
                }
            }
            __syncthreads();
            const int nc = min(*s_cnt, SR_CAND);
            for (int c = 0; c < nc; c++) {
                const int q = cand_q[c];
                if ((q & 3) == wave) sr_insert(lists + q * n, n, cand_s[c], cand_e[c], thr + q, lane);
            }
            // the barrier of the loop condition ends the round: lists, thresholds and the counter are settled before the next one
        }
        // (the first barrier of nb_tile_scores orders the last reads of the p tile before the next staging)
    }
    __syncthreads();
    for (int u = tid; u < nq * n; u += NB_WG) {
        const int q = u / n;
        const float2 v = lists[u];
        const int64_t o = ((int64_t)blockIdx.y * Q + q0 + q) * n + (u - q * n);
        out_s[o] = v.x;
        out_i[o] = __float_as_int(v.y);
    }
}

// ------------------------------------------------------------------------------------------------------------------ merge
// in_s / in_i: [splits][Q][n], each list sorted; out: [Q][n].  One wave per query.
static __global__ __launch_bounds__(NB_WG) void sr_merge_kernel(int n, int splits, int64_t Q, const float* __restrict__ in_s, const int32_t* __restrict__ in_i,
                                                                float* __restrict__ out_s, int32_t* __restrict__ out_i)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6);
    if (q >= Q) return;                                 // wave-uniform
    float s = -INFINITY;
    int i = INT_MAX;
    for (int sp = 0; sp < splits; sp++) {
        const int64_t o = ((int64_t)sp * Q + q) * n;
        for (int j = 0; j < n; j++) {
            const float cs = in_s[o + j];
            const int ci = in_i[o + j];
            const float ts = __shfl(s, n - 1);
            const int ti = __shfl(i, n - 1);
            if (!sr_before(cs, ci, ts, ti)) break;      // wave-uniform; the rest of this list comes after cs
            const bool ahead = lane < n && sr_before(s, i, cs, ci);
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
size_t sr_scan_lds(int kc, int n)
{
    return (size_t)sr_area_floats(kc + 2) * sizeof(float) + (size_t)SR_TC * n * sizeof(float2) + SR_TC * sizeof(float2) + (size_t)SR_CAND * 12 +
           3 * SR_TC * sizeof(int) + 16;
}

int sr_run(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t Md, const double* theta, const double* beta, double a, int64_t Q, const int64_t* q_ptr,
           const int32_t* q_terms, const int32_t* q_counts, int32_t n, int32_t splits_arg, int32_t* idx, float* score, int32_t* count, tmvb_search_info_t* info)
{
    const int kp = (K + 3) & ~3, kc = kp <= NB_KC_ONE ? kp : NB_KC;
    // ---- packing: whole queries, in order, into column tiles; a query that does not fit opens the next tile
    std::vector<int32_t> h_tq0, h_meta((size_t)Q);
    std::vector<int64_t> h_col((size_t)Q);              // first column of a query in the packed array
    int64_t tiles = 0;
    int fill = SR_TC;                                   // columns used in the open tile (none is open yet)
    for (int64_t q = 0; q < Q; q++) {
        const int len = (int)(q_ptr[q + 1] - q_ptr[q]);
        if (fill + len > SR_TC) { h_tq0.push_back((int32_t)q); tiles++; fill = 0; }
        h_meta[(size_t)q] = fill | (len << 8);
        h_col[(size_t)q] = (tiles - 1) * SR_TC + fill;
        fill += len;
    }
    h_tq0.push_back((int32_t)Q);
    const int64_t ncols = tiles * SR_TC;
    std::vector<float> h_fb((size_t)ncols * kp, 0.0f);
    std::vector<int32_t> h_cnt((size_t)ncols, 0);
    const double denom = 1.0 + a * (double)V;
    for (int64_t q = 0; q < Q; q++)
        for (int64_t j = q_ptr[q]; j < q_ptr[q + 1]; j++) {
            const int64_t c = h_col[(size_t)q] + (j - q_ptr[q]);
            const double* b = beta + (int64_t)K * q_terms[j];
            float* f = h_fb.data() + (size_t)c * kp;
            for (int p = 0; p < kp; p++) {
                const int k = nb_perm(p);
                if (k < K) f[p] = (float)((b[k] + a) / denom);
            }
            h_cnt[(size_t)c] = q_counts[j];
        }

    const int64_t ntiles = (Md + NB_TD - 1) / NB_TD;
    // splits: forced, or enough workgroups for two per CU; never more than there are database tiles (or than a grid's y extent)
    int64_t splits = splits_arg;
    if (splits <= 0) {
        const int64_t want = 2 * (int64_t)ctx->num_cu;
        splits = tiles >= want ? 1 : (want + tiles - 1) / tiles;
    }
    splits = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(splits, ntiles), 65535));
    const int64_t tps = (ntiles + splits - 1) / splits;
    splits = (ntiles + tps - 1) / tps;                  // no empty split

    hipStream_t st = ctx->stream;
    tmvb_call c("topic_search", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(6));
    double* d_xd;
    float *d_fd, *d_fb, *d_ps, *d_os = nullptr;
    int32_t *d_tq0, *d_meta, *d_cnt, *d_pi, *d_oi = nullptr;
    const size_t out_n = (size_t)Q * n;
    TMVB_CALL_TRY(c, c.upload(&d_xd, theta, (size_t)Md * K)); TMVB_CALL_TRY(c, c.upload(&d_fb, (const float*)h_fb.data(), h_fb.size()));
    TMVB_CALL_TRY(c, c.upload(&d_tq0, (const int32_t*)h_tq0.data(), h_tq0.size())); TMVB_CALL_TRY(c, c.upload(&d_meta, (const int32_t*)h_meta.data(), h_meta.size()));
    TMVB_CALL_TRY(c, c.upload(&d_cnt, (const int32_t*)h_cnt.data(), h_cnt.size()));
    TMVB_CALL_TRY(c, c.alloc(&d_fd, (size_t)Md * kp));
    TMVB_CALL_TRY(c, c.alloc(&d_ps, (size_t)splits * out_n)); TMVB_CALL_TRY(c, c.alloc(&d_pi, (size_t)splits * out_n));
    if (splits > 1) { TMVB_CALL_TRY(c, c.alloc(&d_os, out_n)); TMVB_CALL_TRY(c, c.alloc(&d_oi, out_n)); }
    const size_t lds = sr_scan_lds(kc, n);
    if (lds > 48 * 1024) TMVB_CALL_HIP(c, hipFuncSetAttribute((const void*)sr_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    // stage times: the events bracket the kernels only; allocations and copies lie outside
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(sr_feature_kernel, dim3((unsigned)((Md + 3) / 4)), dim3(NB_WG), 0, st, (int)K, kp, Md, (const double*)d_xd, d_fd);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    hipLaunchKernelGGL(sr_scan_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(NB_WG), lds, st, kp, kc, (int)n, Q, Md, tps, ncols, (const float*)d_fb,
                       (const float*)d_fd, (const int32_t*)d_tq0, (const int32_t*)d_meta, (const int32_t*)d_cnt, d_ps, d_pi);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
    if (splits > 1) {
        hipLaunchKernelGGL(sr_merge_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(NB_WG), 0, st, (int)n, (int)splits, Q, (const float*)d_ps, (const int32_t*)d_pi, d_os,
                           d_oi);
        TMVB_CALL_HIP(c, hipGetLastError());
    }
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(score, splits > 1 ? d_os : d_ps, out_n * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(idx, splits > 1 ? d_oi : d_pi, out_n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    for (int64_t q = 0; q < Q; q++) {                   // empty slots: idx = -1, score = -inf (the device's sentinel index is INT32_MAX)
        int32_t k = 0;
        for (int j = 0; j < n; j++) {
            int32_t& e = idx[q * n + j];
            if (e == INT_MAX) { e = -1; score[q * n + j] = -std::numeric_limits<float>::infinity(); }
            else k++;
        }
        count[q] = k;
    }
    if (info) {
        info->splits = (int32_t)splits; info->kp = kp; info->col_tiles = (int32_t)tiles;
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_prep, 0, 1));
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_scan, 2, 3));
        if (splits > 1) TMVB_CALL_TRY(c, c.elapsed(&info->ms_merge, 4, 5));
    }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_topic_search(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t Md, const double* theta, const double* beta, double laplace_smooth, int64_t Q,
                                 const int64_t* q_ptr, const int32_t* q_terms, const int32_t* q_counts, int32_t n, int32_t splits, int32_t* idx, float* score,
                                 int32_t* count, tmvb_search_info_t* info)
{
    const char* fn = "tmvb_topic_search";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(K >= 1 && K <= NB_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, NB_MAX_K);
    TMVB_REQUIRE(n >= 1 && n <= TMVB_NB_TOPN_MAX, TMVB_EINVAL, "%s: n = %d outside [1, %d]", fn, n, TMVB_NB_TOPN_MAX);
    TMVB_REQUIRE(Md > 0 && V > 0 && Q > 0, TMVB_EINVAL, "%s: Md, V and Q must be positive integers", fn);
    TMVB_REQUIRE(Md < ((int64_t)1 << 31), TMVB_EINVAL, "%s: Md = %lld is 2^31 or more", fn, (long long)Md);
    TMVB_REQUIRE(V < ((int64_t)1 << 31), TMVB_EINVAL, "%s: V = %lld is 2^31 or more", fn, (long long)V);
    TMVB_REQUIRE(splits >= 0 && (int64_t)splits <= Md, TMVB_EINVAL, "%s: splits = %d outside [0, Md]", fn, splits);
    TMVB_REQUIRE(laplace_smooth >= 0.0 && std::isfinite(laplace_smooth), TMVB_EINVAL, "laplace_smooth parameter must be nonnegative.");
    TMVB_REQUIRE(theta && beta && q_ptr && q_terms && q_counts && idx && score && count, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(q_ptr[0] == 0, TMVB_ESHAPE, "%s: q_ptr must start at 0", fn);
    for (int64_t q = 0; q < Q; q++) {
        TMVB_REQUIRE(q_ptr[q + 1] >= q_ptr[q], TMVB_ESHAPE, "%s: q_ptr decreases at query %lld", fn, (long long)q);
        TMVB_REQUIRE(q_ptr[q + 1] > q_ptr[q], TMVB_ESHAPE, "%s: query %lld is empty", fn, (long long)q);
        TMVB_REQUIRE(q_ptr[q + 1] - q_ptr[q] <= SR_TC, TMVB_ESHAPE, "%s: query %lld has %lld entries (limit %d)", fn, (long long)q,
                     (long long)(q_ptr[q + 1] - q_ptr[q]), SR_TC);
    }
    TMVB_REQUIRE(q_ptr[Q] < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: %lld entries in one call (limit 2^31 - 2); shard the queries", fn, (long long)q_ptr[Q]);
    for (int64_t q = 0; q < Q; q++)
        for (int64_t j = q_ptr[q]; j < q_ptr[q + 1]; j++) {
            TMVB_REQUIRE(q_terms[j] >= 0 && q_terms[j] < V, TMVB_ESHAPE, "%s: query %lld holds term %d outside [0, %lld)", fn, (long long)q, q_terms[j], (long long)V);
            TMVB_REQUIRE(q_counts[j] >= 1, TMVB_ESHAPE, "%s: query %lld holds a count below 1 (all counts must be positive integers)", fn, (long long)q);
        }
    int rc;
    if ((rc = tmvb_check_stochastic_beta(K, V, beta)) != TMVB_OK) return rc;
    for (int64_t d = 0; d < Md; d++) {
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
    return sr_run(ctx, K, V, Md, theta, beta, laplace_smooth, Q, q_ptr, q_terms, q_counts, n, splits, idx, score, count, info);
}
