// tmvb_kmeans.hip -- cluster documents in topic space: Lloyd's k-means whose assignment step is the f32-MFMA score GEMM of tmvb_neighbors.hip
// with another epilogue -- the best column per row instead of the n best rows per query (include/tmvb.h states the definition; the reference
// has no such function).
//
// tmvb_topic_kmeans.
//   features  nb_feature_row of tmvb_nbtile.h: fp64 in, one rounding, F[M][kp].  A second kernel, one lane per row, takes n_d = the fp32 fmaf
//             chain of f^2 over k ascending (and, for the seeding, N_d = the same sum in fp64); the same kernel gives n_c and b_c = -n_c / 2
//             of the centroids Cf[C][kp].
//   assign    grid = tiles of NB_QT = 128 documents, 256 lanes = 2 x 2 waves.  The documents are the resident operand, the centroid tiles of 128
//             stream through nb_tile_scores (the chain of a(d, c) is therefore the neighbours' chain bit for bit).  Epilogue: s = a + b_c (one fp32
//             add); a lane holds two columns of each of its 32 rows: it takes the better one, an xor butterfly over the 32 lanes of its half
//             (offsets 1 .. 16) leaves the best of the wave's 64 columns under the total order (s descending, c ascending), and lane 0 of the
//             half folds it into the running best of (column half wd, row) in LDS -- a slot only its own wave touches.  After the last tile
//             lane q merges the two halves of row q and writes label, dist2 = max(0, fmaf(-2, s, n_d)), the label histogram (LDS bins, then one
//             integer atomic per used bin) and the count of labels that differ from the previous assignment (one integer atomic per wave).
//   inertia   J: one lane per block of TMVB_KM_RUN documents sums its dist2 sequentially in fp64; one workgroup adds the block sums
//             sequentially (staged through LDS in chunks, lane 0 walks them).
//   update    a stable radix sort of (label, document id) (rocPRIM through hipcub) lists every cluster's members ascending; one workgroup
//             takes the exclusive prefixes of the counts and of the run counts; one wave per run of TMVB_KM_RUN sorted positions, lanes over kp,
//             sums its rows of F sequentially in fp64; one wave per cluster adds its run sums in order, divides (COSINE: by the fp64 norm, a
//             fixed-order lane-strided sum and xor butterfly), rounds once and rebuilds n_c and b_c.
//   seeding   k-means++: per round one kernel -- a workgroup = one block of TMVB_KM_RUN documents, a lane per document: D2 to the last seed in fp64,
//             m = min(m, D2), lane 0 sums the block sequentially -- and one workgroup that adds the block sums, finds the first block whose
//             running sum passes u_j total, walks that block, and copies the picked row to Cf.  The rounds follow each other on the stream
//             without the host: the uniforms are uploaded, a round reads the previous pick from device memory.
// No floating-point atomics.  Every sum has one order that depends on M, C and the labels alone.
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_nbtile.h"
#include "tmvb_philox.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <hipcub/hipcub.hpp>
#include <limits>
#include <vector>

#define KM_RUN TMVB_KM_RUN
#define KM_CHUNK 2048               // block sums staged per pass of the sequential adds
static_assert(KM_RUN == NB_WG, "a workgroup of the seeding kernel is one block of TMVB_KM_RUN documents");
static_assert(TMVB_KM_EUCLID == TMVB_NB_DOT && TMVB_KM_HELLINGER == TMVB_NB_HELLINGER && TMVB_KM_COSINE == TMVB_NB_COSINE, "nb_feature_row takes the metric as it is");

// the total order: (s, i) comes before (t, j)
__device__ __forceinline__ bool km_before(float s, int i, float t, int j) { return s > t || (s == t && i < j); }

// ------------------------------------------------------------------------------------------------------------------ features, norms
static __global__ __launch_bounds__(NB_WG) void km_feature_kernel(int K, int kp, int metric, int64_t M, const double* __restrict__ x, float* __restrict__ f)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (NB_WG / 64) + (threadIdx.x >> 6);
    if (r >= M) return;                                 // wave-uniform
    nb_feature_row(K, kp, metric, x + r * K, f + r * kp, lane);
}

// one lane per row of f[rows][kp]: n32 = fp32 fmaf chain of f^2 over k ascending; b32 = -n32 / 2 and N64 = the fp64 sum, where asked for
static __global__ __launch_bounds__(256) void km_norm_kernel(int K, int kp, int64_t rows, const float* __restrict__ f, float* __restrict__ n32, float* __restrict__ b32,
                                                             double* __restrict__ N64)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float* fr = f + r * kp;
    float n = 0.0f;
    double N = 0.0;
    for (int k = 0; k < K; k++) {
        const float v = fr[nb_perm(k)];
        n = fmaf(v, v, n);
        N = fma((double)v, (double)v, N);
    }
    n32[r] = n;
    if (b32) b32[r] = -0.5f * n;
    if (N64) N64[r] = N;
}

// ------------------------------------------------------------------------------------------------------------------ assign
// F: [M][kp], nd: [M], Cf: [C][kp], bc: [C]; prev: the previous labels or NULL.  count[C] and *changed are zero on entry.
static __global__ __launch_bounds__(NB_WG) void km_assign_kernel(int kp, int kc_max, int64_t M, int C, const float* __restrict__ F, const float* __restrict__ nd,
                                                                 const float* __restrict__ Cf, const float* __restrict__ bc, const int32_t* __restrict__ prev,
                                                                 int32_t* __restrict__ label, float* __restrict__ dist2, int* __restrict__ count, int* __restrict__ changed)
{
    extern __shared__ __attribute__((aligned(16))) float km_lds[];
    const int S = kc_max + 2;
    float* sA = km_lds;                                                  // [128][S] documents
    float* sB = sA + NB_QT * S;                                          // [128][S] centroids
    float* best_s = sB + NB_TD * S;                                      // [2][128]: column half wd, row
    int* best_i = reinterpret_cast<int*>(best_s + 2 * NB_QT);            // [2][128]
    int* hist = best_i + 2 * NB_QT;                                      // [C]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave >> 1, wd = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int64_t qt0 = (int64_t)blockIdx.x * NB_QT;
    const int ntiles = (C + NB_TD - 1) / NB_TD;
    const bool one_chunk = kp <= kc_max;

    for (int u = tid; u < C; u += NB_WG) hist[u] = 0;
    best_s[tid] = -INFINITY;                                             // NB_WG = 2 * NB_QT slots
    best_i[tid] = INT_MAX;
    if (one_chunk) nb_stage(sA, S, F, qt0, M, kp, 0, kp);
    // (the first barrier of the tile loop orders these writes before any read)

    for (int t = 0; t < ntiles; t++) {
        const int64_t e0 = (int64_t)t * NB_TD;
        nb_f32x16 acc[2][2];
        nb_tile_scores(acc, sA, sB, S, kp, kc_max, one_chunk, F, qt0, M, Cf, e0, (int64_t)C, wq, wd, l31, half);
        // ---- epilogue.  C/D layout: column (centroid) = lane & 31, row (document) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const int c0 = (int)e0 + 64 * wd + l31, c1 = c0 + 32;
        const bool ok0 = c0 < C, ok1 = c1 < C;
#ifdef TMVB_MUTANT_KM_NO_BIAS
        const float b0 = 0.0f, b1 = 0.0f;                                // MUTANT: the arg-max of the dot product alone
#else
        const float b0 = ok0 ? bc[c0] : 0.0f, b1 = ok1 ? bc[c1] : 0.0f;
#endif
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                float s = ok0 ? acc[a][0][r] + b0 : -INFINITY;
                int i = ok0 ? c0 : INT_MAX;
                const float s1 = ok1 ? acc[a][1][r] + b1 : -INFINITY;
                const int i1 = ok1 ? c1 : INT_MAX;
                if (km_before(s1, i1, s, i)) { s = s1; i = i1; }
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) {                       // stays inside the half: 32 lanes, one row
                    const float os = __shfl_xor(s, o, 64);
                    const int oi = __shfl_xor(i, o, 64);
                    if (km_before(os, oi, s, i)) { s = os; i = oi; }
                }
                if (l31 == 0) {
                    const int slot = wd * NB_QT + 64 * wq + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (km_before(s, i, best_s[slot], best_i[slot])) { best_s[slot] = s; best_i[slot] = i; }
                }
            }
    }
    __syncthreads();
    bool moved = false;
    if (tid < NB_QT && qt0 + tid < M) {
        const int64_t d = qt0 + tid;
        float s = best_s[tid];
        int i = best_i[tid];
        if (km_before(best_s[NB_QT + tid], best_i[NB_QT + tid], s, i)) { s = best_s[NB_QT + tid]; i = best_i[NB_QT + tid]; }
        if (i < 0 || i >= C) i = 0;                                      // unreachable with finite scores; keeps every index in range
#ifdef TMVB_MUTANT_KM_NO_BIAS
        s += bc[i];                                                      // MUTANT: b_c reaches the distance, not the comparison
#endif
        label[d] = i;
        dist2[d] = fmaxf(0.0f, fmaf(-2.0f, s, nd[d]));
        atomicAdd(&hist[i], 1);                                          // LDS, integer
        moved = prev != nullptr && prev[d] != i;
    }
    const int nmoved = __popcll(__ballot(moved));
    if (lane == 0 && nmoved) atomicAdd(changed, nmoved);
    __syncthreads();
    for (int u = tid; u < C; u += NB_WG)
        if (hist[u]) atomicAdd(&count[u], hist[u]);
}

// ------------------------------------------------------------------------------------------------------------------ fixed-order sums
// part[b] = dist2 of documents [KM_RUN b, KM_RUN (b + 1)) added sequentially ascending in fp64
static __global__ __launch_bounds__(256) void km_block_sum_kernel(int64_t M, int64_t nblk, const float* __restrict__ dist2, double* __restrict__ part)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblk) return;
    const int64_t d0 = b * KM_RUN, d1 = min(d0 + KM_RUN, M);
    double s = 0.0;
    for (int64_t d = d0; d < d1; d++) s += (double)dist2[d];
    part[b] = s;
}

// one workgroup of 256, buf = KM_CHUNK doubles of LDS: part[0 .. n) added sequentially ascending from 0; returned to lane 0 only
__device__ __forceinline__ double km_seq_total(const double* __restrict__ part, int64_t n, double* buf)
{
    double s = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += KM_CHUNK) {
        const int m = (int)min((int64_t)KM_CHUNK, n - c0);
        __syncthreads();
        for (int u = threadIdx.x; u < m; u += 256) buf[u] = part[c0 + u];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int u = 0; u < m; u++) s += buf[u];
    }
    return s;
}

static __global__ __launch_bounds__(256) void km_total_kernel(int64_t n, const double* __restrict__ part, double* __restrict__ out)
{
    __shared__ double buf[KM_CHUNK];
    const double s = km_seq_total(part, n, buf);
    if (threadIdx.x == 0) *out = s;
}

// ------------------------------------------------------------------------------------------------------------------ update
static __global__ __launch_bounds__(256) void km_iota_kernel(int64_t M, int32_t* __restrict__ ids)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d < M) ids[d] = (int32_t)d;
}

// one workgroup: off[c] = members before cluster c in the sorted list, roff[c] = runs before cluster c; off[C], roff[C] = the totals
static __global__ __launch_bounds__(256) void km_offsets_kernel(int C, const int* __restrict__ count, int* __restrict__ off, int* __restrict__ roff)
{
    __shared__ int sc[TMVB_KM_CMAX];
    for (int u = threadIdx.x; u < C; u += 256) sc[u] = count[u];
    __syncthreads();
    if (threadIdx.x == 0) {
        int o = 0, r = 0;
        for (int c = 0; c < C; c++) {
            off[c] = o; roff[c] = r;
            o += sc[c];
            r += (sc[c] + KM_RUN - 1) / KM_RUN;
        }
        off[C] = o; roff[C] = r;
    }
}

// one wave per run: part[run][kp] = the run's rows of F added sequentially ascending in fp64
static __global__ __launch_bounds__(256) void km_run_sum_kernel(int kp, int C, const float* __restrict__ F, const int32_t* __restrict__ sorted_ids, const int* __restrict__ off,
                                                                const int* __restrict__ roff, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= roff[C]) return;                           // wave-uniform
    int lo = 0, hi = C;                                 // the cluster c with roff[c] <= w < roff[c + 1]: the last c with roff[c] <= w
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (roff[mid] <= w) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int begin = off[c] + ((int)w - roff[c]) * KM_RUN, end = min(off[c + 1], begin + KM_RUN);
    for (int p = lane; p < kp; p += 64) {
        double s = 0.0;
        for (int i = begin; i < end; i++) s += (double)F[(int64_t)sorted_ids[i] * kp + p];
        part[w * kp + p] = s;
    }
}

// one wave per cluster: the run sums in order, the division, one rounding; n_c and b_c.  A cluster without members keeps its centroid.
static __global__ __launch_bounds__(64) void km_finalize_kernel(int K, int kp, int metric, const int* __restrict__ count, const int* __restrict__ roff,
                                                                const double* __restrict__ part, float* __restrict__ Cf, float* __restrict__ nc, float* __restrict__ bc)
{
    __shared__ double sd[NB_MAX_K];
    __shared__ float sf[NB_MAX_K];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int cnt = count[c], r0 = roff[c], r1 = roff[c + 1];
    double ss = 0.0;
    if (cnt > 0)
        for (int p = lane; p < kp; p += 64) {
            double tot = 0.0;
            for (int r = r0; r < r1; r++) tot += part[(int64_t)r * kp + p];
            sd[p] = tot;
            ss = fma(tot, tot, ss);
        }
    const double norm = sqrt(wave_sum_d(ss));
    for (int p = lane; p < kp; p += 64) {
        float f = Cf[c * kp + p];
        if (cnt > 0) {
            f = (float)(metric == TMVB_KM_COSINE ? sd[p] / norm : sd[p] / (double)cnt);
            Cf[c * kp + p] = f;
        }
        sf[nb_perm(p)] = f;
    }
    __syncthreads();
    if (lane == 0) {
        float n = 0.0f;
        for (int k = 0; k < K; k++) n = fmaf(sf[k], sf[k], n);
        nc[c] = n;
        bc[c] = -0.5f * n;
    }
}

// ------------------------------------------------------------------------------------------------------------------ seeding
// round j >= 1, one workgroup per block of KM_RUN documents: m[d] = min(m[d], D2(d, seeds[j - 1])) (round 1: = D2), bsum[block] = the block's m
// added sequentially ascending
static __global__ __launch_bounds__(NB_WG) void km_seed_dist_kernel(int kp, int64_t M, int j, const float* __restrict__ F, const double* __restrict__ N64,
                                                                    const int32_t* __restrict__ seeds, double* __restrict__ m, double* __restrict__ bsum)
{
    __shared__ __attribute__((aligned(16))) float fs[NB_MAX_K];
    __shared__ double sm[KM_RUN];
    const int tid = threadIdx.x;
    const int64_t s = seeds[j - 1], d = (int64_t)blockIdx.x * KM_RUN + tid;
    for (int u = tid; u < kp; u += NB_WG) fs[u] = F[s * kp + u];
    __syncthreads();
    double v = 0.0;
    if (d < M) {
        const float4* fr = reinterpret_cast<const float4*>(F + d * kp);
        const float4* sr = reinterpret_cast<const float4*>(fs);
        double dot = 0.0;
        for (int g = 0; g < (kp >> 2); g++) {           // memory order inside a group: k = 0, 2, 1, 3 -> x, z, y, w ascend in k
            const float4 a = fr[g], b = sr[g];
            dot = fma((double)a.x, (double)b.x, dot);
            dot = fma((double)a.z, (double)b.z, dot);
            dot = fma((double)a.y, (double)b.y, dot);
            dot = fma((double)a.w, (double)b.w, dot);
        }
        v = fmax(0.0, (N64[d] + N64[s]) - 2.0 * dot);
        if (j > 1) v = fmin(m[d], v);
        m[d] = v;
    }
    sm[tid] = v;
    __syncthreads();
    if (tid == 0) {
        const int n = (int)min((int64_t)KM_RUN, M - (int64_t)blockIdx.x * KM_RUN);
        double t = 0.0;
        for (int u = 0; u < n; u++) t += sm[u];
        bsum[blockIdx.x] = t;
    }
}

// one workgroup.  Round 0: the pick is first_pick.  Round j >= 1: total = the block sums in order; the first d with cum(d) > u[j] total, else the
// lowest document not yet chosen.  seeds[j] = pick, chosen[pick] = 1, Cf[j] = F[pick].
static __global__ __launch_bounds__(256) void km_seed_pick_kernel(int kp, int64_t M, int64_t nblk, int j, int64_t first_pick, const double* __restrict__ u,
                                                                  const float* __restrict__ F, const double* __restrict__ m, const double* __restrict__ bsum,
                                                                  int32_t* __restrict__ seeds, unsigned char* __restrict__ chosen, float* __restrict__ Cf)
{
    __shared__ double buf[KM_CHUNK];
    __shared__ long long s_pick, s_blk;
    __shared__ double s_before;
    const int tid = threadIdx.x;
    if (j == 0) {
        if (tid == 0) s_pick = first_pick;
    } else {
        const double total = km_seq_total(bsum, nblk, buf);             // lane 0
        const double thr = u[j] * total;
        if (tid == 0) { s_blk = -1; s_pick = -1; }
        double P = 0.0;
        bool found = false;
        for (int64_t c0 = 0; c0 < nblk; c0 += KM_CHUNK) {               // the first block b with P_(b+1) > thr
            const int n = (int)min((int64_t)KM_CHUNK, nblk - c0);
            __syncthreads();
            for (int q = tid; q < n; q += 256) buf[q] = bsum[c0 + q];
            __syncthreads();
            if (tid == 0 && !found && total > 0.0)
                for (int q = 0; q < n; q++) {
                    const double Pn = P + buf[q];
                    if (Pn > thr) { found = true; s_blk = c0 + q; s_before = P; break; }
                    P = Pn;
                }
        }
        __syncthreads();
        const int64_t blk = s_blk;
        if (blk >= 0) {                                                  // inside it the first d with P_b + (m up to d) > thr: its last d passes
            const int n = (int)min((int64_t)KM_RUN, M - blk * KM_RUN);
            if (tid < n) buf[tid] = m[blk * KM_RUN + tid];
            __syncthreads();
            if (tid == 0) {
                double q = 0.0;
                for (int i = 0; i < n; i++) {
                    q += buf[i];
                    if (s_before + q > thr) { s_pick = blk * KM_RUN + i; break; }
                }
            }
        }
        if (tid == 0 && s_pick < 0) {
            int64_t d = 0;
            while (d < M - 1 && chosen[d]) d++;                          // j < C <= M: one is free
            s_pick = d;
        }
    }
    __syncthreads();
    const int64_t pick = s_pick;
    if (tid == 0) { seeds[j] = (int32_t)pick; chosen[pick] = 1; }
    for (int p = tid; p < kp; p += 256) Cf[(int64_t)j * kp + p] = F[pick * kp + p];
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
int km_check_rows(const char* fn, const char* what, int32_t K, int32_t metric, int64_t M, const double* x, bool sums)
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
        TMVB_REQUIRE(finite, TMVB_ESHAPE, "%s: non-finite entry (%s %lld)", fn, what, (long long)r);
        if (metric == TMVB_KM_HELLINGER) {
            TMVB_REQUIRE(nonneg, TMVB_ESHAPE, "%s: negative entry (%s %lld)", fn, what, (long long)r);
            if (sums) TMVB_REQUIRE(std::fabs(s - 1.0) <= 1e-6, TMVB_ESHAPE, "%s: \xce\xb8 not a probability vector (%s %lld)", fn, what, (long long)r);
        }
        if (metric == TMVB_KM_COSINE) {
            TMVB_REQUIRE(nonneg, TMVB_ESHAPE, "%s: negative entry (%s %lld)", fn, what, (long long)r);
            TMVB_REQUIRE(any, TMVB_ESHAPE, "%s: all-zero row (%s %lld)", fn, what, (long long)r);
        }
    }
    return TMVB_OK;
}

size_t km_assign_lds(int kc, int C) { return (size_t)2 * 128 * (kc + 2) * sizeof(float) + (size_t)2 * NB_QT * 8 + (size_t)C * sizeof(int); }

int km_run(tmvb_ctx* ctx, int32_t K, int32_t metric, int64_t M, const double* x, int32_t C, const double* init, int64_t seed, int32_t max_iter, double tol,
           int32_t* label, double* centroid, int64_t* count, float* dist2, double* inertia, int32_t* seeds, tmvb_kmeans_info_t* info)
{
    const int kp = (K + 3) & ~3, kc = kp <= NB_KC_ONE ? kp : NB_KC;
    const int64_t qtiles = (M + NB_QT - 1) / NB_QT, nblk = (M + KM_RUN - 1) / KM_RUN, max_runs = nblk + C;
    int end_bit = 1;
    while (end_bit < 31 && ((int64_t)1 << end_bit) < C) end_bit++;

    std::vector<float> h_cf((size_t)C * kp, 0.0f);
    std::vector<int32_t> h_count((size_t)C);
    std::vector<double> h_u((size_t)C);
    hipStream_t st = ctx->stream;
    tmvb_call c("topic_kmeans", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(8));
    double *d_x, *d_N64 = nullptr, *d_m = nullptr, *d_bsum, *d_part = nullptr, *d_J, *d_u = nullptr;
    float *d_f, *d_nd, *d_cf, *d_nc, *d_bc, *d_dist2;
    int32_t *d_lab[2], *d_ids = nullptr, *d_keys = nullptr, *d_sorted = nullptr, *d_seeds = nullptr;
    int *d_count, *d_changed, *d_off = nullptr, *d_roff = nullptr;
    unsigned char* d_chosen = nullptr;
    char* d_tmp = nullptr;
    TMVB_CALL_TRY(c, c.upload(&d_x, x, (size_t)M * K));
    TMVB_CALL_TRY(c, c.alloc(&d_f, (size_t)M * kp)); TMVB_CALL_TRY(c, c.alloc(&d_nd, (size_t)M)); TMVB_CALL_TRY(c, c.alloc(&d_dist2, (size_t)M));
    TMVB_CALL_TRY(c, c.alloc(&d_cf, (size_t)C * kp)); TMVB_CALL_TRY(c, c.alloc(&d_nc, (size_t)C)); TMVB_CALL_TRY(c, c.alloc(&d_bc, (size_t)C));
    TMVB_CALL_TRY(c, c.alloc(&d_lab[0], (size_t)M)); TMVB_CALL_TRY(c, c.alloc(&d_lab[1], (size_t)M));
    TMVB_CALL_TRY(c, c.alloc(&d_count, (size_t)C)); TMVB_CALL_TRY(c, c.alloc(&d_changed, 1)); TMVB_CALL_TRY(c, c.alloc(&d_J, 1));
    TMVB_CALL_TRY(c, c.alloc(&d_bsum, (size_t)nblk));
    size_t tmp_bytes = 0;
    if (max_iter > 0) {
        TMVB_CALL_TRY(c, c.alloc(&d_ids, (size_t)M)); TMVB_CALL_TRY(c, c.alloc(&d_keys, (size_t)M)); TMVB_CALL_TRY(c, c.alloc(&d_sorted, (size_t)M));
        TMVB_CALL_TRY(c, c.alloc(&d_off, (size_t)C + 1)); TMVB_CALL_TRY(c, c.alloc(&d_roff, (size_t)C + 1));
        TMVB_CALL_TRY(c, c.alloc(&d_part, (size_t)max_runs * kp));
        TMVB_CALL_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const int32_t*)d_lab[0], d_keys, (const int32_t*)d_ids, d_sorted, (int)M, 0, end_bit, st));
        TMVB_CALL_TRY(c, c.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 16)));
        hipLaunchKernelGGL(km_iota_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, M, d_ids);
        TMVB_CALL_HIP(c, hipGetLastError());
    }
    const size_t lds = km_assign_lds(kc, C);
    if (lds > 48 * 1024) TMVB_CALL_HIP(c, hipFuncSetAttribute((const void*)km_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    // ---- features
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(km_feature_kernel, dim3((unsigned)((M + 3) / 4)), dim3(NB_WG), 0, st, (int)K, kp, (int)metric, M, (const double*)d_x, d_f);
    if (!init) TMVB_CALL_TRY(c, c.alloc(&d_N64, (size_t)M));
    hipLaunchKernelGGL(km_norm_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (int)K, kp, M, (const float*)d_f, d_nd, (float*)nullptr, d_N64);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));

    // ---- c^0
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    if (init) {
        for (int cc = 0; cc < C; cc++)
            for (int p = 0; p < kp; p++) {
                const int k = nb_perm(p);
                if (k < K) h_cf[(size_t)cc * kp + p] = (float)init[k + (size_t)K * cc];
            }
        TMVB_CALL_HIP(c, hipMemcpyAsync(d_cf, h_cf.data(), h_cf.size() * sizeof(float), hipMemcpyHostToDevice, st));
    } else {
        for (int j = 0; j < C; j++) {
            const tmvb_philox4 r = tmvb_rng((uint64_t)seed, (uint64_t)j, TMVB_RNG_KMEANS, 0, 0);
            h_u[(size_t)j] = tmvb_u53(r.x[0], r.x[1]);
        }
        const int64_t first = std::min<int64_t>(M - 1, (int64_t)std::floor(h_u[0] * (double)M));
        TMVB_CALL_TRY(c, c.upload(&d_u, (const double*)h_u.data(), (size_t)C));
        TMVB_CALL_TRY(c, c.alloc(&d_m, (size_t)M)); TMVB_CALL_TRY(c, c.alloc(&d_seeds, (size_t)C)); TMVB_CALL_TRY(c, c.alloc(&d_chosen, (size_t)M));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_chosen, 0, (size_t)M, st));
        for (int j = 0; j < C; j++) {
            if (j > 0)
                hipLaunchKernelGGL(km_seed_dist_kernel, dim3((unsigned)nblk), dim3(NB_WG), 0, st, kp, M, j, (const float*)d_f, (const double*)d_N64, (const int32_t*)d_seeds,
                                   d_m, d_bsum);
            hipLaunchKernelGGL(km_seed_pick_kernel, dim3(1), dim3(256), 0, st, kp, M, nblk, j, first, (const double*)d_u, (const float*)d_f, (const double*)d_m,
                               (const double*)d_bsum, d_seeds, d_chosen, d_cf);
        }
        TMVB_CALL_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(km_norm_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (int)K, kp, (int64_t)C, (const float*)d_cf, d_nc, d_bc, (double*)nullptr);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));

    // ---- Lloyd
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int t = 0; t <= max_iter; t++) inertia[t] = nan;
    float ms_assign = 0.0f, ms_update = 0.0f, ms = 0.0f;
    int t = 0, stop = 0, cur = 0;
    int64_t moved = M;
    bool update_pending = false;
    for (;;) {
        TMVB_CALL_HIP(c, hipMemsetAsync(d_count, 0, (size_t)C * sizeof(int), st));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_changed, 0, sizeof(int), st));
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
        hipLaunchKernelGGL(km_assign_kernel, dim3((unsigned)qtiles), dim3(NB_WG), lds, st, kp, kc, M, (int)C, (const float*)d_f, (const float*)d_nd, (const float*)d_cf,
                           (const float*)d_bc, (const int32_t*)(t > 0 ? d_lab[cur ^ 1] : nullptr), d_lab[cur], d_dist2, d_count, d_changed);
        hipLaunchKernelGGL(km_block_sum_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, M, nblk, (const float*)d_dist2, d_bsum);
        hipLaunchKernelGGL(km_total_kernel, dim3(1), dim3(256), 0, st, nblk, (const double*)d_bsum, d_J);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
        int h_changed = 0;
        double J = 0.0;
        TMVB_CALL_HIP(c, hipMemcpyAsync(&h_changed, d_changed, sizeof(int), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(&J, d_J, sizeof(double), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipStreamSynchronize(st));
        TMVB_CALL_TRY(c, c.elapsed(&ms, 4, 5));
        ms_assign += ms;
        if (update_pending) { TMVB_CALL_TRY(c, c.elapsed(&ms, 6, 7)); ms_update += ms; update_pending = false; }
        inertia[t] = J;
        if (t >= 1) moved = h_changed;
        if (t >= 1 && h_changed == 0) { stop = 1; break; }
        if (t == max_iter) { stop = 0; break; }
        if (tol > 0.0 && t >= 1 && inertia[t - 1] - J <= tol * inertia[t - 1]) { stop = 2; break; }
        // ---- update
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(6), st));
        TMVB_CALL_HIP(c, hipcub::DeviceRadixSort::SortPairs((void*)d_tmp, tmp_bytes, (const int32_t*)d_lab[cur], d_keys, (const int32_t*)d_ids, d_sorted, (int)M, 0, end_bit, st));
        hipLaunchKernelGGL(km_offsets_kernel, dim3(1), dim3(256), 0, st, (int)C, (const int*)d_count, d_off, d_roff);
        hipLaunchKernelGGL(km_run_sum_kernel, dim3((unsigned)((max_runs + 3) / 4)), dim3(256), 0, st, kp, (int)C, (const float*)d_f, (const int32_t*)d_sorted, (const int*)d_off,
                           (const int*)d_roff, d_part);
        hipLaunchKernelGGL(km_finalize_kernel, dim3((unsigned)C), dim3(64), 0, st, (int)K, kp, (int)metric, (const int*)d_count, (const int*)d_roff, (const double*)d_part, d_cf,
                           d_nc, d_bc);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(7), st));
        update_pending = true;
        t++;
        cur ^= 1;
    }

    // ---- results
    TMVB_CALL_HIP(c, hipMemcpyAsync(label, d_lab[cur], (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(dist2, d_dist2, (size_t)M * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(h_count.data(), d_count, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(h_cf.data(), d_cf, h_cf.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    if (!init) TMVB_CALL_HIP(c, hipMemcpyAsync(seeds, d_seeds, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    int n_empty = 0;
    for (int cc = 0; cc < C; cc++) {
        count[cc] = h_count[(size_t)cc];
        if (h_count[(size_t)cc] == 0) n_empty++;
        if (init) seeds[cc] = -1;
        for (int k = 0; k < K; k++) centroid[k + (size_t)K * cc] = (double)h_cf[(size_t)cc * kp + nb_perm(k)];
    }
    if (info) {
        info->iters = t; info->stop = stop; info->n_empty = n_empty; info->kp = kp; info->moved_last = moved;
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_prep, 0, 1));
        if (!init) TMVB_CALL_TRY(c, c.elapsed(&info->ms_seed, 2, 3));
        info->ms_assign = ms_assign; info->ms_update = ms_update;
    }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_topic_kmeans(tmvb_ctx* ctx, int32_t K, int32_t metric, int64_t M, const double* x, int32_t C, const double* init, int64_t seed, int32_t max_iter,
                                 double tol, int32_t* label, double* centroid, int64_t* count, float* dist2, double* inertia, int32_t* seeds, tmvb_kmeans_info_t* info)
{
    const char* fn = "tmvb_topic_kmeans";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(K >= 1 && K <= NB_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, NB_MAX_K);
    TMVB_REQUIRE(metric == TMVB_KM_EUCLID || metric == TMVB_KM_HELLINGER || metric == TMVB_KM_COSINE, TMVB_EINVAL, "%s: unknown metric %d", fn, metric);
    TMVB_REQUIRE(M > 0 && M < ((int64_t)1 << 31), TMVB_EINVAL, "%s: M = %lld outside [1, 2^31)", fn, (long long)M);
    TMVB_REQUIRE(C >= 1 && C <= TMVB_KM_CMAX && (int64_t)C <= M, TMVB_EINVAL, "%s: C = %d outside [1, min(M, %d)]", fn, C, TMVB_KM_CMAX);
    TMVB_REQUIRE(max_iter >= 0 && max_iter <= 10000, TMVB_EINVAL, "%s: max_iter = %d outside [0, 10000]", fn, max_iter);
    TMVB_REQUIRE(std::isfinite(tol) && tol >= 0.0, TMVB_EINVAL, "%s: tol must be a finite nonnegative number", fn);
    TMVB_REQUIRE(x && label && centroid && count && dist2 && inertia && seeds, TMVB_EINVAL, "%s: NULL argument", fn);
    int rc = km_check_rows(fn, "row", K, metric, M, x, true);
    if (rc != TMVB_OK) return rc;
    if (init && (rc = km_check_rows(fn, "init centroid", K, metric, C, init, false)) != TMVB_OK) return rc;
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    return km_run(ctx, K, metric, M, x, C, init, seed, max_iter, tol, label, centroid, count, dist2, inertia, seeds, info);
}
