// tmvb_topic_compare.hip -- the topic side of a trained model: pairwise divergences of topic-word rows, minimum-cost matching of the topics of two
// runs, relevance / distinctiveness / saliency of terms (include/tmvb.h states the definitions; the reference has none of them).
//
// tmvb_topic_divergence.  The library's first fp64 hot path: KA x KB x V terms with up to two logarithms and two divisions each.
//   prep      x: column-major K x V -> X[kp][vp] row-major, kp = K rounded up to TD_T, vp = V rounded up to TMVB_TD_RUN, pads zero; a 32 x 32 transpose
//             through LDS, reads coalesced along k, writes along w.  HELLINGER: sqrt, KL: (x + smooth) / den, once per element.  A zero pad adds
//             exactly +0 to every sum under every metric (x + 0 = x bit for bit: no sum here is ever -0), so pads need no masks in the pair kernel.
//   pairs     grid (tile j, tile i, group of runs), 256 lanes = 16 x 16.  A workgroup owns TD_T x TD_T pairs; lane (ty, tx) keeps the sums of rows
//             {ty, ty + 16} x {tx, tx + 16}.  A run of TMVB_TD_RUN terms is staged in chunks of TD_CH: both row panels go to LDS with one 16-byte global
//             load per lane and piece, row stride TD_CH + 2 doubles = 132 dwords: the 16 distinct B rows of a wave's 8-byte read fall on banks 0, 4, ..
//             60, two dwords each; the A rows are 4 broadcasts.  Inside a run the lane adds its terms sequentially in ascending w; at the run's end the
//             run sum is added to the total (one group) or stored (several): part[run][i][j].  With b == NULL and a symmetric metric the tiles below
//             the diagonal leave at once; their pairs are mirrored by whoever writes D.
//   merge     one lane per pair: the run sums ascending from 0, then max(0, .) for JS and KL.  Skipped with one group.  sqrt of HELLINGER: the host,
//             on the copied matrix (correctly rounded, and a test can bracket the sum through it).
// The build keeps fp contraction OFF in this unit: a fused multiply-add in 0.5 * (x + y) or acc += term would break the stated arithmetic and,
// with it, the transpose symmetry.  No atomics; no scratch (tools/kernel_resources.py holds the pair kernel to that).
//
// tmvb_term_relevance.  score kernel: one lane per element of the column-major input, r written row-major with its column id beside it;
// tmvb_segmented_sort_pairs (tmvb_topics.hip) descending and stable; a select kernel copies the n heads.  Per-term kernel: a workgroup loads the
// contiguous columns of TR_W consecutive terms into LDS, then one lane per term walks its column twice in ascending k.
//
// tmvb_assignment.  Host: shortest augmenting paths with potentials (Jonker & Volgenant 1987 in its dense row-by-row form), +inf = forbidden.
#include "tmvb_internal.h"
#include "tmvb_call.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#pragma clang fp contract(off)
#include "tmvb_divergence_terms.h"

#define TD_T 32                     // pairs per tile edge
#define TD_CH 64                    // terms per staged chunk
#define TD_LD (TD_CH + 2)           // LDS row stride in doubles
#define TD_WG 256

// ------------------------------------------------------------------------------------------------------------------ divergence: prep
static __global__ __launch_bounds__(256) void td_prep_kernel(int metric, int K, int64_t V, int64_t vp, double smooth, double den, const double* __restrict__ x,
                                                             double* __restrict__ X)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    const int64_t w0 = (int64_t)blockIdx.x * 32;
    const int k0 = blockIdx.y * 32;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t w = w0 + ty + 8 * r;
        const int k = k0 + tx;
        double v = 0.0;
        if (k < K && w < V) {
            v = x[k + (int64_t)K * w];
            if (metric == TMVB_TD_HELLINGER) v = sqrt(v);
            else if (metric == TMVB_TD_KL) v = (v + smooth) / den;
        }
        tile[ty + 8 * r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) X[(int64_t)(k0 + ty + 8 * r) * vp + w0 + tx] = tile[tx][ty + 8 * r];      // every element of [kp][vp] is written
}

// ------------------------------------------------------------------------------------------------------------------ divergence: pairs
// the addend td_term<METRIC>(p, q) and the clamp td_finish<METRIC>(s): tmvb_divergence_terms.h (shared with tmvb_group_topics.hip)
// A: [>= TD_T gridDim.y][vp], B: [>= TD_T gridDim.x][vp].  nruns: runs the kernel walks; rps: runs per group (blockIdx.z).  split == 0: out = D[KA][KB];
// else out = part[run][KA][KB].
template <int METRIC>
static __global__ __launch_bounds__(TD_WG) void td_pairs_kernel(const double* __restrict__ A, const double* __restrict__ B, int64_t vp, int nruns, int rps, int KA,
                                                                int KB, int sym, int split, double* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) double sA[TD_T * TD_LD];
    __shared__ __attribute__((aligned(16))) double sB[TD_T * TD_LD];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (sym && tj < ti) return;                                      // workgroup-uniform
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int r0 = blockIdx.z * rps, r1 = min(r0 + rps, nruns);
    const double* Ap = A + (int64_t)ti * TD_T * vp;
    const double* Bp = B + (int64_t)tj * TD_T * vp;
    const int i0 = ti * TD_T + ty, j0 = tj * TD_T + tx;
    double t00 = 0.0, t01 = 0.0, t10 = 0.0, t11 = 0.0;
    for (int r = r0; r < r1; r++) {
        double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
        for (int ch = 0; ch < TMVB_TD_RUN / TD_CH; ch++) {
            const int64_t w0 = (int64_t)r * TMVB_TD_RUN + ch * TD_CH;
            __syncthreads();                                         // the previous chunk has been read
#pragma unroll
            for (int u = tid; u < TD_T * TD_CH / 2; u += TD_WG) {    // 32 pieces of 16 bytes per row
                const int row = u >> 5, c2 = (u & 31) * 2;
                const double2 va = *reinterpret_cast<const double2*>(Ap + (int64_t)row * vp + w0 + c2);
                const double2 vb = *reinterpret_cast<const double2*>(Bp + (int64_t)row * vp + w0 + c2);
                *reinterpret_cast<double2*>(sA + row * TD_LD + c2) = va;
                *reinterpret_cast<double2*>(sB + row * TD_LD + c2) = vb;
            }
            __syncthreads();
#pragma unroll 2
            for (int w = 0; w < TD_CH; w++) {
                const double p0 = sA[ty * TD_LD + w], p1 = sA[(ty + 16) * TD_LD + w];
                const double q0 = sB[tx * TD_LD + w], q1 = sB[(tx + 16) * TD_LD + w];
                a00 += td_term<METRIC>(p0, q0);
                a01 += td_term<METRIC>(p0, q1);
                a10 += td_term<METRIC>(p1, q0);
                a11 += td_term<METRIC>(p1, q1);
            }
        }
        if (split) {
            double* o = out + (int64_t)r * KA * KB;
            if (i0 < KA && j0 < KB) o[(int64_t)i0 * KB + j0] = a00;
            if (i0 < KA && j0 + 16 < KB) o[(int64_t)i0 * KB + j0 + 16] = a01;
            if (i0 + 16 < KA && j0 < KB) o[(int64_t)(i0 + 16) * KB + j0] = a10;
            if (i0 + 16 < KA && j0 + 16 < KB) o[(int64_t)(i0 + 16) * KB + j0 + 16] = a11;
        } else {
            t00 += a00; t01 += a01; t10 += a10; t11 += a11;
        }
    }
    if (split) return;
    const bool mirror = sym && ti != tj;                             // KA == KB then
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int i = i0 + 16 * (e >> 1), j = j0 + 16 * (e & 1);
        const double v = td_finish<METRIC>(e == 0 ? t00 : e == 1 ? t01 : e == 2 ? t10 : t11);
        if (i < KA && j < KB) {
            out[(int64_t)i * KB + j] = v;
            if (mirror) out[(int64_t)j * KB + i] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ divergence: merge
template <int METRIC>
static __global__ __launch_bounds__(256) void td_merge_kernel(const double* __restrict__ part, int nruns, int KA, int KB, int sym, double* __restrict__ D)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)KA * KB) return;
    int i = (int)(q / KB), j = (int)(q - (int64_t)i * KB);
    if (sym && i / TD_T > j / TD_T) { const int t = i; i = j; j = t; }       // a tile below the diagonal: its mirror was computed
    double s = 0.0;
    for (int r = 0; r < nruns; r++) s += part[((int64_t)r * KA + i) * KB + j];
    D[q] = td_finish<METRIC>(s);
}

// ------------------------------------------------------------------------------------------------------------------ relevance
// beta: column-major K x V.  keys[k][w] = r(k, w), vals[k][w] = w.
static __global__ __launch_bounds__(256) void tr_score_kernel(int K, int64_t V, double lambda, double mu, const double* __restrict__ beta, const double* __restrict__ pw,
                                                              double* __restrict__ keys, int32_t* __restrict__ vals)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)K * V) return;
    const int64_t w = q / K;
    const int k = (int)(q - w * K);
    const double phi = beta[q], p = pw[w];
    double r = -INFINITY;
    if (phi > 0.0 && p > 0.0) {
        const double t1 = lambda * log(phi), t2 = mu * log(phi / p);
        r = (t1 + t2) + 0.0;                                        // + 0.0: a zero score is +0 (the radix sort tells the two zeros apart)
    }
    keys[(int64_t)k * V + w] = r;
    vals[(int64_t)k * V + w] = (int32_t)w;
}

static __global__ __launch_bounds__(256) void tr_select_kernel(int K, int64_t V, int n, const double* __restrict__ skeys, const int32_t* __restrict__ svals,
                                                               int32_t* __restrict__ idx, double* __restrict__ score)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)K * n) return;
    const int64_t k = q / n, s = q - k * n;
    const double v = skeys[k * V + s];
    const bool fin = v > -INFINITY;
    idx[q] = fin ? svals[k * V + s] : -1;
    score[q] = fin ? v : -INFINITY;
}

#define TR_WG 256
// A workgroup takes W consecutive terms = W K contiguous doubles of beta, W = tr_terms_per_wg(K); lane t < W walks column t of the LDS copy (stride K | 1).
static __host__ __device__ inline int tr_terms_per_wg(int K) { return K >= 4096 ? 1 : (4096 / K < TR_WG ? 4096 / K : TR_WG); }

static __global__ __launch_bounds__(TR_WG) void tr_terms_kernel(int K, int64_t V, const double* __restrict__ beta, const double* __restrict__ pw,
                                                                const double* __restrict__ pi, double* __restrict__ distinct, double* __restrict__ saliency)
{
    extern __shared__ double tr_lds[];
    const int W = tr_terms_per_wg(K), ld = K | 1;
    const int64_t w0 = (int64_t)blockIdx.x * W;
    const int nw = (int)min((int64_t)W, V - w0);
    const double* src = beta + w0 * K;
    for (int u = threadIdx.x; u < nw * K; u += TR_WG) {
        const int c = u / K;
        tr_lds[c * ld + (u - c * K)] = src[u];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= nw) return;
    const double* col = tr_lds + t * ld;
    double den = 0.0;
    for (int k = 0; k < K; k++) den += pi[k] * col[k];
    double d = 0.0;
    if (den > 0.0)
        for (int k = 0; k < K; k++) {
            const double P = (pi[k] * col[k]) / den;
            d += P > 0.0 ? P * log(P / pi[k]) : 0.0;
        }
    distinct[w0 + t] = d;
    saliency[w0 + t] = pw[w0 + t] * d;
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
// rows of a column-major K x V matrix: finite, nonnegative, each summing to 1 within 1e-6
int tc_check_rows(const char* fn, const char* side, int32_t K, int64_t V, const double* x)
{
    std::vector<double> sum((size_t)K, 0.0);
    for (int64_t w = 0; w < V; w++)
        for (int k = 0; k < K; k++) {
            const double v = x[k + (int64_t)K * w];
            TMVB_REQUIRE(std::isfinite(v), TMVB_ESHAPE, "%s: non-finite entry (%s row %d, term %lld)", fn, side, k, (long long)w);
            TMVB_REQUIRE(v >= 0.0, TMVB_ESHAPE, "%s: negative entry (%s row %d, term %lld)", fn, side, k, (long long)w);
            sum[(size_t)k] += v;
        }
    for (int k = 0; k < K; k++)
        TMVB_REQUIRE(std::fabs(sum[(size_t)k] - 1.0) <= 1e-6, TMVB_ESHAPE, "%s: %s row %d does not sum to 1", fn, side, k);
    return TMVB_OK;
}

int tc_check_dist(const char* fn, const char* what, int64_t n, const double* x)
{
    double s = 0.0;
    for (int64_t i = 0; i < n; i++) {
        TMVB_REQUIRE(std::isfinite(x[i]) && x[i] >= 0.0, TMVB_ESHAPE, "%s: non-finite or negative entry of %s (%lld)", fn, what, (long long)i);
        s += x[i];
    }
    TMVB_REQUIRE(std::fabs(s - 1.0) <= 1e-6, TMVB_ESHAPE, "%s: %s does not sum to 1", fn, what);
    return TMVB_OK;
}

template <int METRIC>
void td_launch(hipStream_t st, dim3 grid, const double* A, const double* B, int64_t vp, int nruns, int rps, int KA, int KB, int sym, int split, double* out)
{
    hipLaunchKernelGGL(td_pairs_kernel<METRIC>, grid, dim3(TD_WG), 0, st, A, B, vp, nruns, rps, KA, KB, sym, split, out);
}

template <int METRIC>
void td_merge(hipStream_t st, const double* part, int nruns, int KA, int KB, int sym, double* D)
{
    const int64_t n = (int64_t)KA * KB;
    hipLaunchKernelGGL(td_merge_kernel<METRIC>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, nruns, KA, KB, sym, D);
}

int td_run(tmvb_ctx* ctx, int32_t metric, int64_t V, int32_t KA, const double* a, int32_t KB, const double* b, double smooth, int32_t splits_arg, double* D,
           tmvb_topicdiv_info_t* info)
{
    const int64_t runs = (V + TMVB_TD_RUN - 1) / TMVB_TD_RUN, vp = runs * TMVB_TD_RUN;
#ifdef TMVB_MUTANT_TD_DROP_TAIL
    const int nruns = (int)(V / TMVB_TD_RUN);                        // MUTANT: the last, partial run is left out
#else
    const int nruns = (int)runs;
#endif
    const int ta = (KA + TD_T - 1) / TD_T, tb = (KB + TD_T - 1) / TD_T;
    const int sym = (!b && metric != TMVB_TD_KL) ? 1 : 0;
    // groups of runs: forced, or enough workgroups for four per CU (what the LDS of a tile pair allows); whole runs only, no empty group
    const int64_t tiles = sym ? (int64_t)ta * (ta + 1) / 2 : (int64_t)ta * tb;
    int64_t splits = splits_arg;
    if (splits <= 0) {
        const int64_t want = 4 * (int64_t)ctx->num_cu;
        splits = tiles >= want ? 1 : (want + tiles - 1) / tiles;
    }
    splits = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(splits, runs), 65535));
    const int64_t rps = (runs + splits - 1) / splits;
    splits = (runs + rps - 1) / rps;
    const int split = splits > 1 ? 1 : 0;

    hipStream_t st = ctx->stream;
    tmvb_call c("topic_divergence", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(6));
    double *d_a, *d_b = nullptr, *d_A, *d_B, *d_D, *d_part = nullptr;
    const size_t nD = (size_t)KA * KB;
    TMVB_CALL_TRY(c, c.upload(&d_a, a, (size_t)KA * V));
    TMVB_CALL_TRY(c, c.alloc(&d_A, (size_t)ta * TD_T * vp));
    d_B = d_A;
    if (b) { TMVB_CALL_TRY(c, c.upload(&d_b, b, (size_t)KB * V)); TMVB_CALL_TRY(c, c.alloc(&d_B, (size_t)tb * TD_T * vp)); }
    TMVB_CALL_TRY(c, c.alloc(&d_D, nD));
    if (split) TMVB_CALL_TRY(c, c.alloc(&d_part, (size_t)runs * nD));
    const double den = 1.0 + (double)V * smooth;

    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(td_prep_kernel, dim3((unsigned)(vp / 32), (unsigned)ta), dim3(256), 0, st, (int)metric, (int)KA, V, vp, smooth, den, (const double*)d_a, d_A);
    if (b) hipLaunchKernelGGL(td_prep_kernel, dim3((unsigned)(vp / 32), (unsigned)tb), dim3(256), 0, st, (int)metric, (int)KB, V, vp, smooth, den, (const double*)d_b, d_B);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    const dim3 grid((unsigned)tb, (unsigned)ta, (unsigned)splits);
    double* out = split ? d_part : d_D;
    switch (metric) {
    case TMVB_TD_JS: td_launch<TMVB_TD_JS>(st, grid, d_A, d_B, vp, nruns, (int)rps, KA, KB, sym, split, out); break;
    case TMVB_TD_HELLINGER: td_launch<TMVB_TD_HELLINGER>(st, grid, d_A, d_B, vp, nruns, (int)rps, KA, KB, sym, split, out); break;
    case TMVB_TD_TV: td_launch<TMVB_TD_TV>(st, grid, d_A, d_B, vp, nruns, (int)rps, KA, KB, sym, split, out); break;
    default: td_launch<TMVB_TD_KL>(st, grid, d_A, d_B, vp, nruns, (int)rps, KA, KB, sym, split, out); break;
    }
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
    if (split) {
        switch (metric) {
        case TMVB_TD_JS: td_merge<TMVB_TD_JS>(st, d_part, nruns, KA, KB, sym, d_D); break;
        case TMVB_TD_HELLINGER: td_merge<TMVB_TD_HELLINGER>(st, d_part, nruns, KA, KB, sym, d_D); break;
        case TMVB_TD_TV: td_merge<TMVB_TD_TV>(st, d_part, nruns, KA, KB, sym, d_D); break;
        default: td_merge<TMVB_TD_KL>(st, d_part, nruns, KA, KB, sym, d_D); break;
        }
        TMVB_CALL_HIP(c, hipGetLastError());
    }
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(D, d_D, nD * sizeof(double), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    if (metric == TMVB_TD_HELLINGER)
        for (size_t q = 0; q < nD; q++) D[q] = std::sqrt(D[q]);
    if (info) {
        info->splits = (int32_t)splits; info->runs = (int32_t)runs;
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_prep, 0, 1));
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_pairs, 2, 3));
        if (split) TMVB_CALL_TRY(c, c.elapsed(&info->ms_merge, 4, 5));
    }
    return TMVB_OK;
}

int tr_run(tmvb_ctx* ctx, int32_t K, int64_t V, const double* beta, const double* pw, const double* pi, double lambda, int32_t n, int32_t* idx, double* score,
           int32_t* count, double* dense, double* distinct, double* saliency, tmvb_relevance_info_t* info)
{
    const int64_t N = (int64_t)K * V;
    hipStream_t st = ctx->stream;
    tmvb_call c("term_relevance", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(6));
    double *d_beta, *d_pw, *d_pi, *d_keys, *d_skeys, *d_score, *d_dist = nullptr, *d_sal = nullptr;
    int32_t *d_vals, *d_svals, *d_idx;
    TMVB_CALL_TRY(c, c.upload(&d_beta, beta, (size_t)N)); TMVB_CALL_TRY(c, c.upload(&d_pw, pw, (size_t)V)); TMVB_CALL_TRY(c, c.upload(&d_pi, pi, (size_t)K));
    TMVB_CALL_TRY(c, c.alloc(&d_keys, (size_t)N)); TMVB_CALL_TRY(c, c.alloc(&d_vals, (size_t)N));
    TMVB_CALL_TRY(c, c.alloc(&d_idx, (size_t)K * n)); TMVB_CALL_TRY(c, c.alloc(&d_score, (size_t)K * n));
    if (distinct) { TMVB_CALL_TRY(c, c.alloc(&d_dist, (size_t)V)); TMVB_CALL_TRY(c, c.alloc(&d_sal, (size_t)V)); }
    const unsigned nb = (unsigned)((N + 255) / 256);
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(tr_score_kernel, dim3(nb), dim3(256), 0, st, (int)K, V, lambda, 1.0 - lambda, (const double*)d_beta, (const double*)d_pw, d_keys, d_vals);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    if (dense) TMVB_CALL_HIP(c, hipMemcpyAsync(dense, d_keys, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    const int rc = tmvb_segmented_sort_pairs(c, (int)K, V, d_keys, d_vals, true, &d_skeys, &d_svals);
    if (rc != TMVB_OK) return rc;
    hipLaunchKernelGGL(tr_select_kernel, dim3((unsigned)(((int64_t)K * n + 255) / 256)), dim3(256), 0, st, (int)K, V, (int)n, (const double*)d_skeys,
                       (const int32_t*)d_svals, d_idx, d_score);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
    if (distinct) {
        const int W = tr_terms_per_wg(K);
        const size_t lds = (size_t)W * (K | 1) * sizeof(double);
        hipLaunchKernelGGL(tr_terms_kernel, dim3((unsigned)((V + W - 1) / W)), dim3(TR_WG), lds, st, (int)K, V, (const double*)d_beta, (const double*)d_pw,
                           (const double*)d_pi, d_dist, d_sal);
        TMVB_CALL_HIP(c, hipGetLastError());
    }
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(idx, d_idx, (size_t)K * n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(score, d_score, (size_t)K * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (distinct) {
        TMVB_CALL_HIP(c, hipMemcpyAsync(distinct, d_dist, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(saliency, d_sal, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    for (int k = 0; k < K; k++) {                                    // the finite scores are the head of a row
        int32_t m = 0;
        while (m < n && idx[(int64_t)k * n + m] >= 0) m++;
        count[k] = m;
    }
    if (info) {
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_score, 0, 1));
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_select, 2, 3));
        if (distinct) TMVB_CALL_TRY(c, c.elapsed(&info->ms_terms, 4, 5));
    }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_topic_divergence(tmvb_ctx* ctx, int32_t metric, int64_t V, int32_t KA, const double* a, int32_t KB, const double* b, double smooth,
                                     int32_t splits, double* D, tmvb_topicdiv_info_t* info)
{
    const char* fn = "tmvb_topic_divergence";
    if (info) memset(info, 0, sizeof(*info));
    if (!b) KB = KA;
    TMVB_REQUIRE(KA >= 1 && KA <= TMVB_TD_KMAX && KB >= 1 && KB <= TMVB_TD_KMAX, TMVB_EINVAL, "%s: KA = %d or KB = %d outside [1, %d]", fn, KA, KB, TMVB_TD_KMAX);
    TMVB_REQUIRE(V > 0, TMVB_EINVAL, "%s: V must be a positive integer", fn);
    TMVB_REQUIRE((int64_t)KA * V < ((int64_t)1 << 31) && (int64_t)KB * V < ((int64_t)1 << 31), TMVB_EINVAL, "%s: K V is 2^31 or more", fn);
    TMVB_REQUIRE(metric == TMVB_TD_JS || metric == TMVB_TD_HELLINGER || metric == TMVB_TD_TV || metric == TMVB_TD_KL, TMVB_EINVAL, "%s: unknown metric %d", fn, metric);
    TMVB_REQUIRE(splits >= 0 && (int64_t)splits <= (V + TMVB_TD_RUN - 1) / TMVB_TD_RUN, TMVB_EINVAL, "%s: splits = %d outside [0, number of runs]", fn, splits);
    TMVB_REQUIRE(std::isfinite(smooth) && smooth >= 0.0, TMVB_EINVAL, "%s: smooth must be finite and nonnegative", fn);
    TMVB_REQUIRE(metric == TMVB_TD_KL || smooth == 0.0, TMVB_EINVAL, "%s: smooth must be 0 for every metric but KL", fn);
    TMVB_REQUIRE(a && D, TMVB_EINVAL, "%s: NULL argument", fn);
    int rc = tc_check_rows(fn, "a", KA, V, a);
    if (rc != TMVB_OK) return rc;
    if (b && (rc = tc_check_rows(fn, "b", KB, V, b)) != TMVB_OK) return rc;
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    return td_run(ctx, metric, V, KA, a, KB, b, smooth, splits, D, info);
}

extern "C" int tmvb_term_relevance(tmvb_ctx* ctx, int32_t K, int64_t V, const double* beta, const double* pw, const double* pi, double lambda, int32_t n,
                                   int32_t* idx, double* score, int32_t* count, double* dense, double* distinct, double* saliency, tmvb_relevance_info_t* info)
{
    const char* fn = "tmvb_term_relevance";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(K >= 1 && K <= TMVB_TD_KMAX, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, TMVB_TD_KMAX);
    TMVB_REQUIRE(V > 0, TMVB_EINVAL, "%s: V must be a positive integer", fn);
    TMVB_REQUIRE((int64_t)K * V < ((int64_t)1 << 31), TMVB_EINVAL, "%s: K V is 2^31 or more", fn);
    TMVB_REQUIRE(std::isfinite(lambda) && lambda >= 0.0 && lambda <= 1.0, TMVB_EINVAL, "%s: lambda outside [0, 1]", fn);
    TMVB_REQUIRE(n >= 1 && (int64_t)n <= V, TMVB_EINVAL, "%s: n = %d outside [1, V]", fn, n);
    TMVB_REQUIRE(beta && pw && pi && idx && score && count, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE((distinct == nullptr) == (saliency == nullptr), TMVB_EINVAL, "%s: distinct and saliency are given together or not at all", fn);
    int rc = tc_check_rows(fn, "beta", K, V, beta);
    if (rc != TMVB_OK) return rc;
    if ((rc = tc_check_dist(fn, "pw", V, pw)) != TMVB_OK) return rc;
    if ((rc = tc_check_dist(fn, "pi", K, pi)) != TMVB_OK) return rc;
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    return tr_run(ctx, K, V, beta, pw, pi, lambda, n, idx, score, count, dense, distinct, saliency, info);
}

// Rows are inserted one at a time; each insertion grows the shortest alternating path tree from the new row (Dijkstra on the reduced costs
// cost - u - v, dense: O(n m) per row) and augments along it.  The potentials stay finite: a step of infinite length means that no column of finite
// cost is reachable, so no finite assignment exists.
extern "C" int tmvb_assignment(int32_t n, int32_t m, const double* cost, int32_t* row_to_col, double* total)
{
    const char* fn = "tmvb_assignment";
    TMVB_REQUIRE(n >= 1 && n <= m && m <= TMVB_TD_KMAX, TMVB_EINVAL, "%s: need 1 <= n <= m <= %d (n = %d, m = %d)", fn, TMVB_TD_KMAX, n, m);
    TMVB_REQUIRE(cost && row_to_col, TMVB_EINVAL, "%s: NULL argument", fn);
    const double inf = std::numeric_limits<double>::infinity();
    for (int64_t q = 0; q < (int64_t)n * m; q++)
        TMVB_REQUIRE(!std::isnan(cost[q]) && cost[q] != -inf, TMVB_ESHAPE, "%s: cost %lld is NaN or -inf", fn, (long long)q);
    std::vector<double> u((size_t)n + 1, 0.0), v((size_t)m + 1, 0.0), minv((size_t)m + 1);
    std::vector<int> p((size_t)m + 1, 0), way((size_t)m + 1, 0);     // p[j]: the row (1-based) matched to column j; column 0 is the virtual start
    std::vector<char> used((size_t)m + 1);
    for (int i = 1; i <= n; i++) {
        p[0] = i;
        int j0 = 0;
        std::fill(minv.begin(), minv.end(), inf);
        std::fill(used.begin(), used.end(), (char)0);
        do {
            used[(size_t)j0] = 1;
            const int i0 = p[(size_t)j0];
            double delta = inf;
            int j1 = 0;
            for (int j = 1; j <= m; j++) {
                if (used[(size_t)j]) continue;
                const double cur = cost[(int64_t)(i0 - 1) * m + (j - 1)] - u[(size_t)i0] - v[(size_t)j];
                if (cur < minv[(size_t)j]) { minv[(size_t)j] = cur; way[(size_t)j] = j0; }
                if (minv[(size_t)j] < delta) { delta = minv[(size_t)j]; j1 = j; }
            }
            TMVB_REQUIRE(delta < inf, TMVB_ESHAPE, "%s: no assignment of finite cost exists (row %d cannot be placed)", fn, i - 1);
            for (int j = 0; j <= m; j++) {
                if (used[(size_t)j]) { u[(size_t)p[(size_t)j]] += delta; v[(size_t)j] -= delta; }
                else minv[(size_t)j] -= delta;
            }
            j0 = j1;
        } while (p[(size_t)j0] != 0);
        do {
            const int j1 = way[(size_t)j0];
            p[(size_t)j0] = p[(size_t)j1];
            j0 = j1;
        } while (j0);
    }
    for (int j = 1; j <= m; j++)
        if (p[(size_t)j]) row_to_col[p[(size_t)j] - 1] = j - 1;
    if (total) {
        double s = 0.0;
        for (int i = 0; i < n; i++) s += cost[(int64_t)i * m + row_to_col[i]];
        *total = s;
    }
    return TMVB_OK;
}
