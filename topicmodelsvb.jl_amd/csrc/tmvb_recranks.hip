// tmvb_recranks.hip -- held-out recommendation metrics: the split of the reader lists, the rank of every held-out pair fused into the score
// GEMM, and the metrics on the ranks (include/tmvb.h states the definitions; the reference stops at showdrecs / showurecs).
//
// tmvb_readers_split, tmvb_rank_metrics: host only, no device.
// tmvb_score_ranks.  rank of target t of query q = how many candidates e (not excluded, e != t) come before t under the total order of the
//   reference's reverse(sortperm(.)): s_e > s_t, or s_e == s_t and e > t.  No score matrix, no sort of candidates.
//   prep      rk_feature_kernel: fp64 -> fp32 [M][kp], the layout of tmvb_nbtile.h (shared with tmvb_neighbors.hip).
//   pairs     rk_pairs_kernel: the score of every listed (query, id) pair, targets first, then exclusions.  One wave takes 32 pairs: lane l holds
//             the operands of pair l & 31 for k-half l >> 5, read straight from the two feature rows, and runs the same two MFMAs per group of four
//             k as the scan; the diagonal of the 32 x 32 tile is kept.  Same instruction, same operand values, same k order: a pair's score has
//             the same bits here as in the scan.  rk_sort_kernel then orders the targets of each query (best first) by counting, one lane per
//             target.
//   scan      rk_scan_kernel: the tile loop of nb_scan_kernel with another epilogue.  Grid (query tile of 128, database split).  The targets of the
//             tile's queries sit in LDS, each query's sorted; register r of an accumulator holds 32 database rows of one query per half-wave, and
//             that half walks the query's targets from worst to best: compare, ballot restricted to the half, popcount, LDS add into the target's
//             counter; it stops at the first empty ballot (a row that does not come before target i comes before no better one).  Rows >= Md are
//             masked, queries >= Mq have no targets.  Exclusions are NOT tested here.  A target never counts itself: its own row has the same
//             score bits and fails e > t.  If a tile has more targets than the LDS slots, the tile runs in passes over slices of them.  The
//             counters are integers: the LDS adds and the global adds of the splits' partial counts give the same sums in any order.
//   fix       rk_fix_kernel: rank = count - #{o in excl(q): o before t}, one lane per target over the query's excluded scores.
// No scratch: the 64 accumulator entries are walked by a fully unrolled loop.
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_nbtile.h"
#include "tmvb_philox.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#define RK_TGT_SLOTS 2048           // targets of a query tile held in LDS per pass (12 bytes each)

// the total order of reverse(sortperm(.)): (s, i) comes before (t, j)
__host__ __device__ __forceinline__ bool rk_before(float s, int i, float t, int j) { return s > t || (s == t && i > j); }

// ------------------------------------------------------------------------------------------------------------------ prep
static __global__ __launch_bounds__(NB_WG) void rk_feature_kernel(int K, int kp, int64_t M, const double* __restrict__ x, float* __restrict__ f)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6);
    if (r >= M) return;                                 // wave-uniform
    nb_feature_row(K, kp, TMVB_NB_DOT, x + r * K, f + r * kp, lane);
}

// ------------------------------------------------------------------------------------------------------------------ pairs
// pair p = (query pq[p], database row pe[p]) -> ps[p].  One wave per 32 pairs.
static __global__ __launch_bounds__(NB_WG) void rk_pairs_kernel(int kp, int64_t nP, const int32_t* __restrict__ pq, const int32_t* __restrict__ pe,
                                                                const float* __restrict__ Fq, const float* __restrict__ Fd, float* __restrict__ ps)
{
    const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
    const int64_t p0 = ((int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6)) * 32;
    if (p0 >= nP) return;                               // wave-uniform
    const int64_t p = p0 + l31;
    const bool live = p < nP;
    const float* a = Fq + (live ? (int64_t)pq[p] : 0) * kp + 2 * half;     // a dead lane reads row 0: its column and row of the tile are never kept
    const float* b = Fd + (live ? (int64_t)pe[p] : 0) * kp + 2 * half;
    nb_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    for (int kk = 0; kk < kp; kk += 4) {
        const float2 av = *reinterpret_cast<const float2*>(a + kk), bv = *reinterpret_cast<const float2*>(b + kk);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
    }
    // C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): the diagonal entry of column j lies in half (j >> 2) & 1
    const int rsel = (l31 & 3) + 4 * (l31 >> 3);
    float v = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++)
        if (r == rsel) v = acc[r];
    if (live && half == ((l31 >> 2) & 1)) ps[p] = v;
}

// One lane per target g (query tq[g], row te[g], score ts[g]): its place among its query's targets, best first -> the sorted copies ss / se and
// so[place] = g.  The order is total (ids are distinct), so the places of a query are a permutation.
static __global__ __launch_bounds__(NB_WG) void rk_sort_kernel(int64_t nT, const int64_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tq,
                                                               const int32_t* __restrict__ te, const float* __restrict__ ts, float* __restrict__ ss,
                                                               int32_t* __restrict__ se, int32_t* __restrict__ so)
{
    const int64_t g = (int64_t)blockIdx.x * NB_WG + threadIdx.x;
    if (g >= nT) return;
    const int q = tq[g], e = te[g];
    const float s = ts[g];
    const int64_t lo = tgt_ptr[q], hi = tgt_ptr[q + 1];
    int64_t place = lo;
    for (int64_t j = lo; j < hi; j++) place += rk_before(ts[j], te[j], s, e) ? 1 : 0;
    ss[place] = s; se[place] = e; so[place] = (int32_t)g;
}

// ------------------------------------------------------------------------------------------------------------------ scan
// Fq: [Mq][kp], Fd: [Md][kp]; ss / se / so: the sorted targets; cnt[g] += number of rows of this split's tiles that come before target g.
static __global__ __launch_bounds__(NB_WG) void rk_scan_kernel(int kp, int kc_max, int slots, int64_t Mq, int64_t Md, int64_t tiles_per_split,
                                                               const float* __restrict__ Fq, const float* __restrict__ Fd, const int64_t* __restrict__ tgt_ptr,
                                                               const float* __restrict__ ss, const int32_t* __restrict__ se, const int32_t* __restrict__ so,
                                                               int32_t* __restrict__ cnt)
{
    extern __shared__ __attribute__((aligned(16))) float rk_lds[];
    const int S = kc_max + 2;
    float* sA = rk_lds;                                                  // [128][S] queries
    float* sB = sA + NB_QT * S;                                          // [128][S] database rows
    float* t_s = sB + NB_TD * S;                                         // [slots] target scores of this pass
    int* t_e = reinterpret_cast<int*>(t_s + slots);                      // [slots] their rows
    int* t_c = t_e + slots;                                              // [slots] their counters
    int* q_lo = t_c + slots;                                             // [128] first slot of a query's targets in this pass
    int* q_n = q_lo + NB_QT;                                             // [128] how many

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave >> 1, wd = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int64_t qt0 = (int64_t)blockIdx.x * NB_QT, qt1 = min(qt0 + NB_QT, Mq);
#ifdef TMVB_MUTANT_RK_DROP_TAIL
    const int64_t ntiles = Md / NB_TD;                                   // MUTANT: the last, partial database tile is skipped
#else
    const int64_t ntiles = (Md + NB_TD - 1) / NB_TD;
#endif
    const int64_t t_begin = (int64_t)blockIdx.y * tiles_per_split, t_end = min(t_begin + tiles_per_split, ntiles);
    const bool one_chunk = kp <= kc_max;
    const int64_t g_begin = tgt_ptr[qt0], g_end = tgt_ptr[qt1];          // the tile's targets, contiguous in the sorted arrays
    if (g_begin == g_end || t_begin >= t_end) return;                    // uniform over the workgroup

    if (one_chunk) nb_stage(sA, S, Fq, qt0, Mq, kp, 0, kp);
    for (int64_t p0 = g_begin; p0 < g_end; p0 += slots) {                // passes
        const int64_t p1 = min(p0 + (int64_t)slots, g_end);
        __syncthreads();                                                 // the previous pass has flushed its counters
        for (int u = tid; u < (int)(p1 - p0); u += NB_WG) { t_s[u] = ss[p0 + u]; t_e[u] = se[p0 + u]; t_c[u] = 0; }
        if (tid < NB_QT) {
            int lo = 0, n = 0;
            if (qt0 + tid < Mq) {
                const int64_t a = max(tgt_ptr[qt0 + tid], p0), b = min(tgt_ptr[qt0 + tid + 1], p1);
                if (b > a) { lo = (int)(a - p0); n = (int)(b - a); }
            }
            q_lo[tid] = lo; q_n[tid] = n;
        }
        // (the first barrier of the tile's chunk loop orders these writes before any read)
        for (int64_t t = t_begin; t < t_end; t++) {
            const int64_t e0 = t * NB_TD;
            nb_f32x16 acc[2][2];
            nb_tile_scores(acc, sA, sB, S, kp, kc_max, one_chunk, Fq, qt0, Mq, Fd, e0, Md, wq, wd, l31, half);
            // ---- epilogue.  C/D layout: column (database row) = lane & 31, row (query) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    const int64_t e64 = e0 + 64 * wd + 32 * b + l31;
                    const bool row_ok = e64 < Md;
                    const int e = (int)e64;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int q = 64 * wq + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * half;      // uniform over the half-wave
                        const int lo = q_lo[q];
                        const float s = acc[a][b][r];
                        for (int i = q_n[q] - 1; i >= 0; i--) {                                 // worst target first
                            const bool bef = row_ok && rk_before(s, e, t_s[lo + i], t_e[lo + i]);
                            const unsigned long long bal = __ballot(bef);
                            const unsigned mine = (unsigned)(half ? (bal >> 32) : bal);
                            if (mine == 0u) break;
                            if (l31 == 0) atomicAdd(&t_c[lo + i], __popc(mine));               // LDS
                        }
                    }
                }
        }
        __syncthreads();
        for (int u = tid; u < (int)(p1 - p0); u += NB_WG)
            if (t_c[u] != 0) atomicAdd(&cnt[so[p0 + u]], t_c[u]);
    }
}

// ------------------------------------------------------------------------------------------------------------------ fix
// One lane per target g: rank[g] = cnt[g] - the excluded rows of its query that come before it.  xs / xe: scores and rows of the exclusions.
static __global__ __launch_bounds__(NB_WG) void rk_fix_kernel(int64_t nT, const int32_t* __restrict__ tq, const int32_t* __restrict__ te,
                                                              const float* __restrict__ ts, const int64_t* __restrict__ excl_ptr,
                                                              const int32_t* __restrict__ xe, const float* __restrict__ xs, const int32_t* __restrict__ cnt,
                                                              int32_t* __restrict__ rank)
{
    const int64_t g = (int64_t)blockIdx.x * NB_WG + threadIdx.x;
    if (g >= nT) return;
    const int q = tq[g], e = te[g];
    const float s = ts[g];
    int c = 0;
    for (int64_t j = excl_ptr[q]; j < excl_ptr[q + 1]; j++) c += rk_before(xs[j], xe[j], s, e) ? 1 : 0;
    rank[g] = cnt[g] - c;
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
int rk_check_rows(const char* fn, const char* side, int32_t K, int64_t M, const double* x)
{
    for (int64_t r = 0; r < M; r++)
        for (int k = 0; k < K; k++)
            TMVB_REQUIRE(std::isfinite(x[k + (int64_t)K * r]), TMVB_ESHAPE, "%s: non-finite entry (%s row %lld)", fn, side, (long long)r);
    return TMVB_OK;
}

int rk_check_ptr(const char* fn, const char* what, int64_t Mq, const int64_t* ptr)
{
    TMVB_REQUIRE(ptr[0] == 0, TMVB_ESHAPE, "%s: %s_ptr must start at 0", fn, what);
    for (int64_t q = 0; q < Mq; q++) TMVB_REQUIRE(ptr[q + 1] >= ptr[q], TMVB_ESHAPE, "%s: %s_ptr decreases at query %lld", fn, what, (long long)q);
    TMVB_REQUIRE(ptr[Mq] < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: %lld %s entries in one call (limit 2^31 - 2); shard the queries", fn, (long long)ptr[Mq], what);
    return TMVB_OK;
}

int rk_check_ids(const char* fn, const char* what, int64_t Mq, int64_t Md, const int64_t* ptr, const int32_t* idx)
{
    for (int64_t q = 0; q < Mq; q++)
        for (int64_t j = ptr[q]; j < ptr[q + 1]; j++) {
            TMVB_REQUIRE(idx[j] >= 0 && idx[j] < Md, TMVB_ESHAPE, "%s: query %lld holds %s id %d outside [0, %lld)", fn, (long long)q, what, idx[j], (long long)Md);
            TMVB_REQUIRE(j == ptr[q] || idx[j] > idx[j - 1], TMVB_ESHAPE, "%s: the %s ids of query %lld are not strictly ascending", fn, what, (long long)q);
        }
    return TMVB_OK;
}

size_t rk_scan_lds(int kc, int slots) { return (size_t)2 * 128 * (kc + 2) * sizeof(float) + (size_t)slots * 12 + 2 * NB_QT * sizeof(int); }

int rk_run(tmvb_ctx* ctx, int32_t K, int64_t Md, const double* xd, int64_t Mq, const double* xq, const int64_t* excl_ptr, const int32_t* excl_idx,
           const int64_t* tgt_ptr, const int32_t* tgt_idx, int32_t splits_arg, int32_t* rank, float* score, tmvb_recranks_info_t* info)
{
    const int kp = (K + 3) & ~3, kc = kp <= NB_KC_ONE ? kp : NB_KC;
    const int64_t ntiles = (Md + NB_TD - 1) / NB_TD, qtiles = (Mq + NB_QT - 1) / NB_QT, nT = tgt_ptr[Mq], nE = excl_ptr[Mq], nP = nT + nE;
    if (info) { info->kp = kp; info->splits = 0; }
    if (nT == 0) return TMVB_OK;                        // nothing to rank
    // splits: forced, or enough workgroups for two per CU; never more than there are database tiles (or than a grid's y extent)
    int64_t splits = splits_arg;
    if (splits <= 0) {
        const int64_t want = 2 * (int64_t)ctx->num_cu;
        splits = qtiles >= want ? 1 : (want + qtiles - 1) / qtiles;
    }
    splits = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(splits, ntiles), 65535));
    const int64_t tps = (ntiles + splits - 1) / splits;
    splits = (ntiles + tps - 1) / tps;                  // no empty split
    // the LDS slots of a pass: the default, a smaller number for tests (TMVB_RK_TARGET_SLOTS), never more than the fullest tile needs
    int64_t slots = RK_TGT_SLOTS, need = 1;
    { const long v = tmvb_env_int("TMVB_RK_TARGET_SLOTS", 0); if (v >= 1 && v <= RK_TGT_SLOTS) slots = v; }
    for (int64_t t = 0; t < qtiles; t++) need = std::max(need, tgt_ptr[std::min((t + 1) * NB_QT, Mq)] - tgt_ptr[t * NB_QT]);
    slots = std::min(slots, need);

    // host staging, declared in front of the call's scope: the pairs (targets, then exclusions) as (query, row)
    std::vector<int32_t> h_pq((size_t)nP), h_pe((size_t)nP);
    for (int64_t q = 0; q < Mq; q++) {
        for (int64_t j = tgt_ptr[q]; j < tgt_ptr[q + 1]; j++) { h_pq[(size_t)j] = (int32_t)q; h_pe[(size_t)j] = tgt_idx[j]; }
        for (int64_t j = excl_ptr[q]; j < excl_ptr[q + 1]; j++) { h_pq[(size_t)(nT + j)] = (int32_t)q; h_pe[(size_t)(nT + j)] = excl_idx[j]; }
    }

    hipStream_t st = ctx->stream;
    tmvb_call c("score_ranks", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(8));
    double *d_xd, *d_xq;
    float *d_fd, *d_fq, *d_ps, *d_ss;
    int32_t *d_pq, *d_pe, *d_se, *d_so, *d_cnt, *d_rank;
    int64_t *d_tptr, *d_eptr;
    TMVB_CALL_TRY(c, c.upload(&d_xd, xd, (size_t)Md * K)); TMVB_CALL_TRY(c, c.upload(&d_xq, xq, (size_t)Mq * K));
    TMVB_CALL_TRY(c, c.upload(&d_pq, (const int32_t*)h_pq.data(), (size_t)nP)); TMVB_CALL_TRY(c, c.upload(&d_pe, (const int32_t*)h_pe.data(), (size_t)nP));
    TMVB_CALL_TRY(c, c.upload(&d_tptr, tgt_ptr, (size_t)Mq + 1)); TMVB_CALL_TRY(c, c.upload(&d_eptr, excl_ptr, (size_t)Mq + 1));
    TMVB_CALL_TRY(c, c.alloc(&d_fd, (size_t)Md * kp)); TMVB_CALL_TRY(c, c.alloc(&d_fq, (size_t)Mq * kp));
    TMVB_CALL_TRY(c, c.alloc(&d_ps, (size_t)nP)); TMVB_CALL_TRY(c, c.alloc(&d_ss, (size_t)nT)); TMVB_CALL_TRY(c, c.alloc(&d_se, (size_t)nT));
    TMVB_CALL_TRY(c, c.alloc(&d_so, (size_t)nT)); TMVB_CALL_TRY(c, c.alloc(&d_cnt, (size_t)nT)); TMVB_CALL_TRY(c, c.alloc(&d_rank, (size_t)nT));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_cnt, 0, (size_t)nT * sizeof(int32_t), st));
    const size_t lds = rk_scan_lds(kc, (int)slots);
    if (lds > 48 * 1024) TMVB_CALL_HIP(c, hipFuncSetAttribute((const void*)rk_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    // stage times: the events bracket the kernels only; allocations and copies lie outside
    const unsigned tblocks = (unsigned)((nT + NB_WG - 1) / NB_WG);
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(rk_feature_kernel, dim3((unsigned)((Md + 3) / 4)), dim3(NB_WG), 0, st, (int)K, kp, Md, (const double*)d_xd, d_fd);
    hipLaunchKernelGGL(rk_feature_kernel, dim3((unsigned)((Mq + 3) / 4)), dim3(NB_WG), 0, st, (int)K, kp, Mq, (const double*)d_xq, d_fq);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    hipLaunchKernelGGL(rk_pairs_kernel, dim3((unsigned)((nP + 127) / 128)), dim3(NB_WG), 0, st, kp, nP, (const int32_t*)d_pq, (const int32_t*)d_pe, (const float*)d_fq,
                       (const float*)d_fd, d_ps);
    hipLaunchKernelGGL(rk_sort_kernel, dim3(tblocks), dim3(NB_WG), 0, st, nT, (const int64_t*)d_tptr, (const int32_t*)d_pq, (const int32_t*)d_pe, (const float*)d_ps, d_ss,
                       d_se, d_so);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
    hipLaunchKernelGGL(rk_scan_kernel, dim3((unsigned)qtiles, (unsigned)splits), dim3(NB_WG), lds, st, kp, kc, (int)slots, Mq, Md, tps, (const float*)d_fq,
                       (const float*)d_fd, (const int64_t*)d_tptr, (const float*)d_ss, (const int32_t*)d_se, (const int32_t*)d_so, d_cnt);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(6), st));
    hipLaunchKernelGGL(rk_fix_kernel, dim3(tblocks), dim3(NB_WG), 0, st, nT, (const int32_t*)d_pq, (const int32_t*)d_pe, (const float*)d_ps, (const int64_t*)d_eptr,
                       (const int32_t*)d_pe + nT, (const float*)d_ps + nT, (const int32_t*)d_cnt, d_rank);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(7), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(rank, d_rank, (size_t)nT * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (score) TMVB_CALL_HIP(c, hipMemcpyAsync(score, d_ps, (size_t)nT * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    if (info) {
        info->splits = (int32_t)splits;
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_prep, 0, 1));
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_pairs, 2, 3));
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_scan, 4, 5));
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_fix, 6, 7));
    }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_score_ranks(tmvb_ctx* ctx, int32_t K, int64_t Md, const double* xd, int64_t Mq, const double* xq, const int64_t* excl_ptr,
                                const int32_t* excl_idx, const int64_t* tgt_ptr, const int32_t* tgt_idx, int32_t splits, int32_t* rank, int32_t* n_cand,
                                float* score, tmvb_recranks_info_t* info)
{
    const char* fn = "tmvb_score_ranks";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(K >= 1 && K <= NB_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, NB_MAX_K);
    TMVB_REQUIRE(Md > 0 && Mq > 0, TMVB_EINVAL, "%s: Md and Mq must be positive integers", fn);
    TMVB_REQUIRE(Md < ((int64_t)1 << 31), TMVB_EINVAL, "%s: Md = %lld is 2^31 or more", fn, (long long)Md);
    TMVB_REQUIRE((Mq + NB_QT - 1) / NB_QT <= 0x7fffffffLL, TMVB_EINVAL, "%s: Mq = %lld is more than one call takes (shard the queries)", fn, (long long)Mq);
    TMVB_REQUIRE(splits >= 0 && (int64_t)splits <= Md, TMVB_EINVAL, "%s: splits = %d outside [0, Md]", fn, splits);
    TMVB_REQUIRE(xd && xq && excl_ptr && tgt_ptr && rank && n_cand, TMVB_EINVAL, "%s: NULL argument", fn);
    int rc;
    if ((rc = rk_check_ptr(fn, "excl", Mq, excl_ptr)) != TMVB_OK) return rc;
    if ((rc = rk_check_ptr(fn, "tgt", Mq, tgt_ptr)) != TMVB_OK) return rc;
    TMVB_REQUIRE((excl_idx || excl_ptr[Mq] == 0) && (tgt_idx || tgt_ptr[Mq] == 0), TMVB_EINVAL, "%s: NULL argument", fn);
    if ((rc = rk_check_rows(fn, "database", K, Md, xd)) != TMVB_OK) return rc;
    if ((rc = rk_check_rows(fn, "query", K, Mq, xq)) != TMVB_OK) return rc;
    if ((rc = rk_check_ids(fn, "excluded", Mq, Md, excl_ptr, excl_idx)) != TMVB_OK) return rc;
    if ((rc = rk_check_ids(fn, "target", Mq, Md, tgt_ptr, tgt_idx)) != TMVB_OK) return rc;
    for (int64_t q = 0; q < Mq; q++) {                  // both lists ascend: one merge walk finds a shared id
        int64_t i = excl_ptr[q], j = tgt_ptr[q];
        while (i < excl_ptr[q + 1] && j < tgt_ptr[q + 1]) {
            TMVB_REQUIRE(excl_idx[i] != tgt_idx[j], TMVB_ESHAPE, "%s: id %d of query %lld is both excluded and a target", fn, tgt_idx[j], (long long)q);
            if (excl_idx[i] < tgt_idx[j]) i++; else j++;
        }
    }
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    for (int64_t q = 0; q < Mq; q++) n_cand[q] = (int32_t)(Md - (excl_ptr[q + 1] - excl_ptr[q]));
    return rk_run(ctx, K, Md, xd, Mq, xq, excl_ptr, excl_idx, tgt_ptr, tgt_idx, splits, rank, score, info);
}

// ------------------------------------------------------------------------------------------------------------------ the split of the reader lists
extern "C" void tmvb_rsplit_free(tmvb_rsplit_t* s)
{
    if (!s) return;
    free(s->obs_ptr); free(s->obs_readers); free(s->obs_ratings); free(s->held_ptr); free(s->held_readers); free(s->held_ratings);
    memset(s, 0, sizeof(*s));
}

extern "C" int tmvb_readers_split(int64_t M, int64_t U, const int64_t* rdr_ptr, const int32_t* readers, const int32_t* ratings, double frac, int64_t seed,
                                  int64_t doc_offset, int32_t mode, tmvb_rsplit_t* out)
{
    const char* fn = "tmvb_readers_split";
    TMVB_REQUIRE(out != nullptr, TMVB_EINVAL, "%s: out is NULL", fn);
    memset(out, 0, sizeof(*out));
    TMVB_REQUIRE(std::isfinite(frac) && frac >= 0.0 && frac <= 1.0, TMVB_EINVAL, "%s: frac must lie in [0, 1]", fn);
    TMVB_REQUIRE(doc_offset >= 0, TMVB_EINVAL, "%s: doc_offset must be nonnegative", fn);
    TMVB_REQUIRE(mode == TMVB_RSPLIT_ENTRY || mode == TMVB_RSPLIT_DOCUMENT, TMVB_EINVAL, "%s: unknown mode %d", fn, mode);
    TMVB_REQUIRE(M > 0, TMVB_EINVAL, "%s: M must be a positive integer", fn);
    TMVB_REQUIRE(U > 0, TMVB_EINVAL, "%s: U must be a positive integer", fn);
    TMVB_REQUIRE(M < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: M = %lld above 2^31 - 2 documents per call", fn, (long long)M);
    TMVB_REQUIRE(rdr_ptr && readers && ratings, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(rdr_ptr[0] == 0, TMVB_ESHAPE, "%s: rdr_ptr must start at 0", fn);
    for (int64_t d = 0; d < M; d++) TMVB_REQUIRE(rdr_ptr[d + 1] >= rdr_ptr[d], TMVB_ESHAPE, "%s: rdr_ptr decreases at document %lld", fn, (long long)d);
    for (int64_t d = 0; d < M; d++)
        for (int64_t j = rdr_ptr[d]; j < rdr_ptr[d + 1]; j++) {
            TMVB_REQUIRE(readers[j] >= 0 && readers[j] < U, TMVB_ESHAPE, "%s: document %lld holds reader %d outside [0, %lld)", fn, (long long)d, readers[j], (long long)U);
            TMVB_REQUIRE(ratings[j] >= 1, TMVB_ESHAPE, "%s: document %lld holds a rating below 1 (all ratings must be positive integers)", fn, (long long)d);
        }
    const uint64_t thr = (uint64_t)std::floor(frac * 4294967296.0);
    const int64_t n = rdr_ptr[M];
    tmvb_result_guard<tmvb_rsplit_t, tmvb_rsplit_free> guard{out};
    std::vector<uint8_t> held((size_t)n);
    int64_t n_held = 0;
    for (int64_t d = 0; d < M; d++) {
        const int64_t lo = rdr_ptr[d], len = rdr_ptr[d + 1] - lo;
        if (mode == TMVB_RSPLIT_DOCUMENT) {
            const bool h = (uint64_t)tmvb_rng((uint64_t)seed, (uint64_t)(doc_offset + d), TMVB_RNG_RSPLIT_DOCUMENT, 0, 0).x[0] < thr;
            for (int64_t j = 0; j < len; j++) held[(size_t)(lo + j)] = h;
            if (h) n_held += len;
            continue;
        }
        tmvb_philox4 x{};
        for (int64_t j = 0; j < len; j++) {
            if ((j & 3) == 0) x = tmvb_rng((uint64_t)seed, (uint64_t)(doc_offset + d), TMVB_RNG_RSPLIT_ENTRY, 0, (uint32_t)(j >> 2));
            const bool h = (uint64_t)x.x[j & 3] < thr;
            held[(size_t)(lo + j)] = h;
            n_held += h;
        }
    }
    out->M = M; out->n_held = n_held; out->n_obs = n - n_held;
    int rc;
    if ((rc = tmvb_host_alloc("readers_split", &out->obs_ptr, (size_t)M + 1)) != TMVB_OK) return rc;
    if ((rc = tmvb_host_alloc("readers_split", &out->held_ptr, (size_t)M + 1)) != TMVB_OK) return rc;
    if ((rc = tmvb_host_alloc("readers_split", &out->obs_readers, (size_t)out->n_obs)) != TMVB_OK) return rc;
    if ((rc = tmvb_host_alloc("readers_split", &out->obs_ratings, (size_t)out->n_obs)) != TMVB_OK) return rc;
    if ((rc = tmvb_host_alloc("readers_split", &out->held_readers, (size_t)out->n_held)) != TMVB_OK) return rc;
    if ((rc = tmvb_host_alloc("readers_split", &out->held_ratings, (size_t)out->n_held)) != TMVB_OK) return rc;
    int64_t o = 0, h = 0;
    out->obs_ptr[0] = out->held_ptr[0] = 0;
    for (int64_t d = 0; d < M; d++) {
        for (int64_t j = rdr_ptr[d]; j < rdr_ptr[d + 1]; j++) {
            if (held[(size_t)j]) { out->held_readers[h] = readers[j]; out->held_ratings[h++] = ratings[j]; }
            else { out->obs_readers[o] = readers[j]; out->obs_ratings[o++] = ratings[j]; }
        }
        out->obs_ptr[d + 1] = o; out->held_ptr[d + 1] = h;
    }
    guard.release();
    return TMVB_OK;
}

// ------------------------------------------------------------------------------------------------------------------ metrics on the ranks
extern "C" int tmvb_rank_metrics(int64_t Mq, const int64_t* tgt_ptr, const int32_t* rank, const int32_t* n_cand, int32_t nN, const int32_t* Ns, double* recall,
                                 double* precision, double* ndcg, double* mrr, double* pct_rank, double* mean, int64_t* counts)
{
    const char* fn = "tmvb_rank_metrics";
    TMVB_REQUIRE(Mq > 0, TMVB_EINVAL, "%s: Mq must be a positive integer", fn);
    TMVB_REQUIRE(nN >= 1, TMVB_EINVAL, "%s: nN = %d: at least one cut-off is needed", fn, nN);
    TMVB_REQUIRE(tgt_ptr && n_cand && Ns && recall && precision && ndcg && mrr && pct_rank && mean && counts, TMVB_EINVAL, "%s: NULL argument", fn);
    for (int a = 0; a < nN; a++) TMVB_REQUIRE(Ns[a] >= 1, TMVB_EINVAL, "%s: N = %d below 1", fn, Ns[a]);
    TMVB_REQUIRE(tgt_ptr[0] == 0, TMVB_ESHAPE, "%s: tgt_ptr must start at 0", fn);
    for (int64_t q = 0; q < Mq; q++) TMVB_REQUIRE(tgt_ptr[q + 1] >= tgt_ptr[q], TMVB_ESHAPE, "%s: tgt_ptr decreases at query %lld", fn, (long long)q);
    TMVB_REQUIRE(rank || tgt_ptr[Mq] == 0, TMVB_EINVAL, "%s: NULL argument", fn);
    for (int64_t q = 0; q < Mq; q++)
        for (int64_t j = tgt_ptr[q]; j < tgt_ptr[q + 1]; j++)
            TMVB_REQUIRE(rank[j] >= 0 && rank[j] < n_cand[q], TMVB_ESHAPE, "%s: query %lld holds rank %d outside [0, %d)", fn, (long long)q, rank[j], n_cand[q]);
    const int nm = 3 * nN + 2;
    std::vector<double> sum((size_t)nm, 0.0);
    int64_t nq = 0;
    for (int64_t q = 0; q < Mq; q++) {
        const int64_t lo = tgt_ptr[q], T = tgt_ptr[q + 1] - lo;
        double* rec = recall + q * nN; double* pre = precision + q * nN; double* nd = ndcg + q * nN;
        if (T == 0) {
            for (int a = 0; a < nN; a++) rec[a] = pre[a] = nd[a] = NAN;
            mrr[q] = pct_rank[q] = NAN;
            continue;
        }
        int32_t best = rank[lo];
        double rsum = 0.0;
        for (int64_t j = 0; j < T; j++) { best = std::min(best, rank[lo + j]); rsum += (double)rank[lo + j]; }
        for (int a = 0; a < nN; a++) {
            const int32_t N = Ns[a];
            int64_t hits = 0;
            double dcg = 0.0, ideal = 0.0;
            for (int64_t j = 0; j < T; j++)
                if (rank[lo + j] < N) { hits++; dcg += 1.0 / std::log2((double)rank[lo + j] + 2.0); }
            for (int64_t i = 0; i < std::min<int64_t>(T, N); i++) ideal += 1.0 / std::log2((double)i + 2.0);
            rec[a] = (double)hits / (double)T; pre[a] = (double)hits / (double)N; nd[a] = dcg / ideal;
            sum[(size_t)a] += rec[a]; sum[(size_t)(nN + a)] += pre[a]; sum[(size_t)(2 * nN + a)] += nd[a];
        }
        mrr[q] = 1.0 / ((double)best + 1.0);
        pct_rank[q] = rsum / (double)T / (double)std::max(n_cand[q] - 1, 1);
        sum[(size_t)(3 * nN)] += mrr[q]; sum[(size_t)(3 * nN + 1)] += pct_rank[q];
        nq++;
    }
    for (int a = 0; a < nm; a++) mean[a] = nq ? sum[(size_t)a] / (double)nq : NAN;
    counts[0] = nq; counts[1] = tgt_ptr[Mq];
    return TMVB_OK;
}
