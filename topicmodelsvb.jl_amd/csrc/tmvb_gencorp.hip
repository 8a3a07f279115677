// tmvb_gencorp.hip -- gendoc / gencorp (src/modelutils.jl:594-649) on the device: a trained model run as a generative process.
//
// For document d:  C_d ~ Poisson(mean_C);  theta_d ~ Dirichlet(alpha) (LDA, fLDA; :598)  or  additive_logistic(N(mu, sigma)) (CTM, fCTM; :619);
// C_d tokens  z ~ Cat(theta_d), w ~ Cat((beta[z,:] + a) / (1 + a V))  (:601-607);  the document is its unique terms with their counts (:610).
// Two differences from the reference as written:
//   * its CTM method draws `rand(topicdist)` at :626, a typo for `topic_dist` that throws as written; the intent (:605) is implemented;
//   * it returns a Dict's keys / values, unique terms in arbitrary order; here terms come out sorted ascending with summed counts (the
//     condensed CSR the engine uses everywhere), 0-based.
//
// Every random number is Philox4x32-10 of (seed, global document index, stage, draw index) (tmvb_philox.h), so the corpus does not depend on the
// launch geometry, documents [d0, d0 + m) of a large call equal a call with doc_offset = d0, and the same seed gives the same bytes.
//
// Stages (device time of each is reported):
//   tables    per topic a two-level sampling table from the fp64 beta: V is cut into blocks of 64 terms; block masses are summed and scanned in
//             fp64 (53-bit uniform against them), and inside a block a prefix normalised by the block's own mass is kept in fp32 (24-bit
//             uniform).  A flat fp32 CDF over V = 25 k terms cannot resolve entries under 6e-8, which most of a trained beta is.  All sums run
//             left to right, so a zero entry repeats its left neighbour's CDF value exactly and is never drawn (searches take the first
//             entry STRICTLY above the uniform).
//   docs      one wave per document: lane = topic.  Dirichlet through log-space Gamma variates (Marsaglia-Tsang at shape alpha + 1, plus
//             log(u) / alpha, then a log-sum-exp; u^(1/alpha) underflows in linear space at the trained alpha of 0.007), or mu + L eps with
//             Box-Muller normals; C_d by multiplication (mean < 10) or PTRS transformed rejection (Hoermann 1993).  fp64 throughout.
//   tokens    one wave per document: theta's CDF in LDS, lane = token; two binary searches per token in the topic's table.
//   condense  segmented radix sort of each document's term ids (rocPRIM through hipcub), run-length encode, scan, write.
// No floating-point atomics; the diagnostic count matrices use integer atomics (order-independent).
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_philox.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <hipcub/hipcub.hpp>

#define GC_BLOCK 64                 // terms per table block = lanes of a wave
#define GC_LDA_MAX_K 1024
#define GC_CTM_MAX_K 256
#define GC_MAX_M ((int64_t)(1 << 26) - 1)

extern "C" int tmvb_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out)
{
    TMVB_REQUIRE(counter && key && out, TMVB_EINVAL, "tmvb_philox4x32_10: NULL argument");
    const tmvb_philox4 r = tmvb_philox4x32_10_raw(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
    memcpy(out, r.x, sizeof(r.x));
    return TMVB_OK;
}

// ------------------------------------------------------------------------------------------------------------------ device draws
static __device__ inline double gc_wave_max(double v)
{
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
static __device__ inline double gc_wave_sum(double v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// standard normal from two 32-bit words (Box-Muller; the radius uniform is in (0, 1])
static __device__ inline double gc_normal(uint32_t a, uint32_t b)
{
    const double u1 = ((double)a + 1.0) * (1.0 / 4294967296.0), u2 = (double)b * (1.0 / 4294967296.0);
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// log of a Gamma(alpha, 1) variate, alpha > 0: log G(alpha + 1) + log(u) / alpha (Marsaglia & Tsang 2000, section 6)
static __device__ double gc_log_gamma_variate(uint64_t seed, uint64_t doc, uint32_t k, double alpha)
{
    const double d = alpha + 1.0 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double lg = 0.0;
    for (uint32_t attempt = 0;; attempt++) {
        const tmvb_philox4 r = tmvb_rng(seed, doc, TMVB_RNG_GAMMA, k, attempt);
        const double x = gc_normal(r.x[0], r.x[1]);
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double u = tmvb_u53_open(r.x[2], r.x[3]);
        if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) { lg = log(d * v); break; }
    }
    const tmvb_philox4 r = tmvb_rng(seed, doc, TMVB_RNG_BOOST, k, 0);
    return lg + log(tmvb_u53_open(r.x[0], r.x[1])) / alpha;
}

// Poisson(lam), exact: multiplication of uniforms below 10 (Knuth), PTRS above (Hoermann 1993, "The transformed rejection method for
// generating Poisson random variables")
static __device__ int64_t gc_poisson(uint64_t seed, uint64_t doc, double lam)
{
    if (lam < 10.0) {
        const double L = exp(-lam);
        double p = 1.0;
        int64_t k = 0;
        for (uint32_t j = 0;; j++) {
            const tmvb_philox4 r = tmvb_rng(seed, doc, TMVB_RNG_POISSON, 0, j);
            for (int q = 0; q < 4; q++) {
                p *= ((double)r.x[q] + 0.5) * (1.0 / 4294967296.0);
                if (p <= L) return k;
                k++;
            }
        }
    }
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    for (uint32_t j = 0;; j++) {
        const tmvb_philox4 r = tmvb_rng(seed, doc, TMVB_RNG_POISSON, 0, j);
        const double U = tmvb_u53_open(r.x[0], r.x[1]) - 0.5, V = tmvb_u53_open(r.x[2], r.x[3]);
        const double us = 0.5 - fabs(U);
        const double kf = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return (int64_t)kf;
        if (kf < 0.0 || kf > 9.0e15 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + kf * loglam - lgamma(kf + 1.0)) return (int64_t)kf;
    }
}

// ------------------------------------------------------------------------------------------------------------------ tables
// grid (nb, K), one wave: block b of topic k.  beta is the model's column-major K x V field.
static __global__ __launch_bounds__(64) void gencorp_blocks_kernel(const double* __restrict__ beta, int K, int64_t V, int nb, double a, double denom,
                                                                   double* __restrict__ bsum, float* __restrict__ wcdf)
{
    __shared__ double s_p[GC_BLOCK];
    const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const int64_t v = (int64_t)b * GC_BLOCK + lane;
    s_p[lane] = v < V ? (beta[k + (int64_t)K * v] + a) / denom : 0.0;
    __syncthreads();
    double acc = 0.0, tot = 0.0;
    for (int j = 0; j < GC_BLOCK; j++) {           // every lane adds in the same left-to-right order: acc of lane 63 IS tot, bit for bit
        const double p = s_p[j];
        tot += p;
        acc += j <= lane ? p : 0.0;
    }
    wcdf[((int64_t)k * nb + b) * GC_BLOCK + lane] = tot > 0.0 ? (float)(acc / tot) : 1.0f;
    if (lane == 0) bsum[(int64_t)k * nb + b] = tot;
}

// one thread per topic: block CDF = left-to-right fp64 scan of the block masses over their total (the last entry is exactly 1)
static __global__ __launch_bounds__(64) void gencorp_blockcdf_kernel(const double* __restrict__ bsum, int K, int nb, double* __restrict__ bcdf)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const double* s = bsum + (int64_t)k * nb;
    double tot = 0.0;
    for (int b = 0; b < nb; b++) tot += s[b];
    double run = 0.0;
    for (int b = 0; b < nb; b++) {
        run += s[b];
        bcdf[(int64_t)k * nb + b] = run / tot;
    }
}

// ------------------------------------------------------------------------------------------------------------------ documents
// one wave per document.  CTM = false: par = alpha[K].  CTM = true: par = mu[K], L = lower Cholesky factor of sigma, row-major K x K.
template <bool CTM>
static __global__ __launch_bounds__(64) void gencorp_docs_kernel(int K, int64_t doc_offset, uint64_t seed, double mean_C, const double* __restrict__ par,
                                                                 const double* __restrict__ L, float* __restrict__ log_theta, int64_t* __restrict__ C)
{
    __shared__ double s_v[GC_LDA_MAX_K];
    __shared__ double s_eps[CTM ? GC_CTM_MAX_K : 1];
    const int64_t d = blockIdx.x;
    const uint64_t g = (uint64_t)(doc_offset + d);
    const int lane = threadIdx.x;
    if (CTM) {
        for (int k = lane; k < K; k += 64) {
            const tmvb_philox4 r = tmvb_rng(seed, g, TMVB_RNG_NORMAL, (uint32_t)k, 0);
            s_eps[k] = gc_normal(r.x[0], r.x[1]);
        }
        __syncthreads();
        for (int k = lane; k < K; k += 64) {
            double eta = par[k];
            for (int j = 0; j <= k; j++) eta += L[(int64_t)k * K + j] * s_eps[j];
            s_v[k] = eta;
        }
    } else {
        for (int k = lane; k < K; k += 64) s_v[k] = gc_log_gamma_variate(seed, g, (uint32_t)k, par[k]);
    }
    __syncthreads();
    double m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmax(m, s_v[k]);
    m = gc_wave_max(m);
    double s = 0.0;
    for (int k = lane; k < K; k += 64) s += exp(s_v[k] - m);
    const double lse = m + log(gc_wave_sum(s));
    for (int k = lane; k < K; k += 64) log_theta[d * K + k] = (float)(s_v[k] - lse);
    if (lane == 0) C[d] = gc_poisson(seed, g, mean_C);
}

// ------------------------------------------------------------------------------------------------------------------ tokens
// first index in [0, n) whose value is strictly above x; the caller guarantees a[n - 1] > x
template <typename T>
static __device__ inline int gc_first_above(const T* __restrict__ a, int n, T x)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// one wave per document, lane = token (t, t + 64, ...).  theta's CDF sits in LDS; a document's tokens concentrate on its few heavy topics,
// so the lanes of a wave walk the same topics' tables.
static __global__ __launch_bounds__(64) void gencorp_tokens_kernel(int K, int64_t V, int nb, int64_t doc_offset, uint64_t seed, const float* __restrict__ log_theta,
                                                                   const int64_t* __restrict__ tok_ptr, const double* __restrict__ bcdf,
                                                                   const float* __restrict__ wcdf, int32_t* __restrict__ tok, int32_t* __restrict__ doc_topic,
                                                                   unsigned long long* __restrict__ topic_term)
{
    __shared__ float s_cdf[GC_LDA_MAX_K];
    const int64_t d = blockIdx.x;
    const int64_t base = tok_ptr[d], n = tok_ptr[d + 1] - base;
    if (n == 0) return;
    const uint64_t g = (uint64_t)(doc_offset + d);
    const int lane = threadIdx.x;
    float carry = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        float v = k < K ? expf(log_theta[d * K + k]) : 0.0f;
        for (int o = 1; o < 64; o <<= 1) {
            const float t = __shfl_up(v, o);
            if (lane >= o) v += t;
        }
        v += carry;
        if (k < K) s_cdf[k] = v;
        carry = __shfl(v, 63);
    }
    __syncthreads();
    const float total = carry;
    for (int64_t t = lane; t < n; t += 64) {
        const tmvb_philox4 r = tmvb_rng(seed, g, TMVB_RNG_TOKEN, 0, (uint32_t)t);
        float x = tmvb_u24(r.x[0]) * total;
        if (x >= total) x = nextafterf(total, 0.0f);
        const int z = gc_first_above(s_cdf, K, x);
        const int b = gc_first_above(bcdf + (int64_t)z * nb, nb, tmvb_u53(r.x[1], r.x[2]));
        const int i = gc_first_above(wcdf + ((int64_t)z * nb + b) * GC_BLOCK, GC_BLOCK, tmvb_u24(r.x[3]));
        const int64_t w = min((int64_t)b * GC_BLOCK + i, V - 1);          // padding terms have no mass; the clamp only guards the stores
        tok[base + t] = (int32_t)w;
        if (doc_topic) {
            atomicAdd(&doc_topic[d * K + z], 1);
            atomicAdd(&topic_term[(int64_t)z * V + w], 1ull);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ condense
static __global__ void gencorp_offsets32_kernel(const int64_t* __restrict__ p, int64_t n, int* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int)p[i];
}

// one wave per document over its sorted tokens: number of distinct terms
static __global__ __launch_bounds__(64) void gencorp_unique_kernel(const int32_t* __restrict__ s, const int64_t* __restrict__ tok_ptr, int64_t* __restrict__ nuniq)
{
    const int64_t d = blockIdx.x;
    const int64_t base = tok_ptr[d], n = tok_ptr[d + 1] - base;
    int c = 0;
    for (int64_t i = threadIdx.x; i < n; i += 64) c += (i == 0 || s[base + i] != s[base + i - 1]) ? 1 : 0;
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
    if (threadIdx.x == 0) nuniq[d] = c;
}

static __global__ __launch_bounds__(64) void gencorp_rle_kernel(const int32_t* __restrict__ s, const int64_t* __restrict__ tok_ptr, const int64_t* __restrict__ doc_ptr,
                                                                int32_t* __restrict__ terms, int32_t* __restrict__ counts)
{
    const int64_t d = blockIdx.x;
    const int64_t base = tok_ptr[d], n = tok_ptr[d + 1] - base;
    const int lane = threadIdx.x;
    int64_t o = doc_ptr[d];
    for (int64_t c0 = 0; c0 < n; c0 += 64) {
        const int64_t i = c0 + lane;
        const bool head = i < n && (i == 0 || s[base + i] != s[base + i - 1]);
        const unsigned long long mask = __ballot(head);
        if (head) {
            const int64_t pos = o + __popcll(mask & ((1ull << lane) - 1ull));
            const int32_t w = s[base + i];
            int64_t j = i + 1;
            while (j < n && s[base + j] == w) j++;
            terms[pos] = w;
            counts[pos] = (int32_t)(j - i);
        }
        o += __popcll(mask);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
// lower Cholesky factor of the column-major (symmetric) K x K sigma, row-major; false if sigma is not positive-definite
bool gc_cholesky(const double* sigma, int K, std::vector<double>& L)
{
    L.assign((size_t)K * K, 0.0);
    for (int i = 0; i < K; i++)
        for (int j = 0; j <= i; j++) {
            double s = sigma[i + (size_t)K * j];
            for (int q = 0; q < j; q++) s -= L[(size_t)i * K + q] * L[(size_t)j * K + q];
            if (i == j) {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                L[(size_t)i * K + i] = std::sqrt(s);
            } else {
                L[(size_t)i * K + j] = s / L[(size_t)j * K + j];
            }
        }
    return true;
}

int gc_check_common(const char* fn, int32_t K, int32_t maxK, int64_t V, const double* beta, int64_t M, int64_t doc_offset, double mean_C,
                    double a, tmvb_gencorp_t* out)
{
    TMVB_REQUIRE(out != nullptr, TMVB_EINVAL, "%s: out is NULL", fn);
    memset(out, 0, sizeof(*out));
    TMVB_REQUIRE(M > 0, TMVB_EINVAL, "corp_size parameter must be a positive integer.");                       // src/modelutils.jl:643
    TMVB_REQUIRE(a >= 0.0 && std::isfinite(a), TMVB_EINVAL, "laplace_smooth parameter must be nonnegative.");   // :595, :644
    TMVB_REQUIRE(std::isfinite(mean_C) && mean_C > 0.0, TMVB_EINVAL, "%s: mean_C must be positive and finite", fn);
    TMVB_REQUIRE(K > 0 && K <= maxK, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, maxK);
    TMVB_REQUIRE(V > 0 && doc_offset >= 0, TMVB_EINVAL, "%s: V must be positive, doc_offset nonnegative", fn);
    // one 64-lane workgroup per document: the grid must stay below 2^32 threads
    TMVB_REQUIRE(M <= GC_MAX_M, TMVB_EINVAL, "%s: M = %lld above %lld documents per call; generate in shards through doc_offset", fn, (long long)M, (long long)GC_MAX_M);
    TMVB_REQUIRE(beta != nullptr, TMVB_EINVAL, "%s: NULL argument", fn);
    return tmvb_check_stochastic_beta(K, V, beta);
}

// par: alpha (chol == NULL) or mu; chol: row-major lower factor of sigma
int gc_run(tmvb_ctx* ctx, int32_t K, int64_t V, const double* par, const double* chol, const double* beta, int64_t M, int64_t doc_offset, double mean_C,
           double a, uint64_t seed, int32_t flags, tmvb_gencorp_t* out)
{
    tmvb_result_guard<tmvb_gencorp_t, tmvb_gencorp_free> guard{out};
    int64_t T = 0, nnz = 0;         // read back from the device: in front of the call's scope
    hipStream_t st = ctx->stream;
    tmvb_call c("gencorp", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    const bool diag = (flags & 1) != 0;
    const int nb = (int)((V + GC_BLOCK - 1) / GC_BLOCK);
    const int64_t KV = (int64_t)K * V, Knb = (int64_t)K * nb;
    TMVB_CALL_TRY(c, c.events(8));
    double *d_beta, *d_bsum, *d_bcdf, *d_par, *d_chol = nullptr;
    float *d_wcdf, *d_lt;
    int64_t *d_C, *d_tokptr, *d_nu, *d_docptr;
    TMVB_CALL_TRY(c, c.alloc(&d_beta, (size_t)KV)); TMVB_CALL_TRY(c, c.alloc(&d_bsum, (size_t)Knb)); TMVB_CALL_TRY(c, c.alloc(&d_bcdf, (size_t)Knb));
    TMVB_CALL_TRY(c, c.alloc(&d_wcdf, (size_t)Knb * GC_BLOCK)); TMVB_CALL_TRY(c, c.alloc(&d_par, (size_t)K)); TMVB_CALL_TRY(c, c.alloc(&d_lt, (size_t)M * K));
    TMVB_CALL_TRY(c, c.alloc(&d_C, (size_t)M + 1)); TMVB_CALL_TRY(c, c.alloc(&d_tokptr, (size_t)M + 1)); TMVB_CALL_TRY(c, c.alloc(&d_nu, (size_t)M + 1));
    TMVB_CALL_TRY(c, c.alloc(&d_docptr, (size_t)M + 1));
    if (chol) TMVB_CALL_TRY(c, c.alloc(&d_chol, (size_t)K * K));
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_beta, beta, (size_t)KV * sizeof(double), hipMemcpyHostToDevice, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_par, par, (size_t)K * sizeof(double), hipMemcpyHostToDevice, st));
    if (chol) TMVB_CALL_HIP(c, hipMemcpyAsync(d_chol, chol, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice, st));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_C, 0, ((size_t)M + 1) * sizeof(int64_t), st));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_nu, 0, ((size_t)M + 1) * sizeof(int64_t), st));
    size_t scan_bytes = 0;
    TMVB_CALL_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const int64_t*)d_C, d_tokptr, (int)(M + 1), st));
    char* d_scan;
    TMVB_CALL_TRY(c, c.alloc(&d_scan, std::max<size_t>(scan_bytes, 16)));

    // Stage times: every pair of events brackets kernels and hipcub calls only; allocations, memsets, the two 8-byte read-backs and
    // their stream synchronisations lie outside the pairs (ms_condense adds its two pairs).
    // ---- tables
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(gencorp_blocks_kernel, dim3((unsigned)nb, (unsigned)K), dim3(64), 0, st, (const double*)d_beta, (int)K, V, nb, a, 1.0 + a * (double)V, d_bsum, d_wcdf);
    hipLaunchKernelGGL(gencorp_blockcdf_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, (const double*)d_bsum, (int)K, nb, d_bcdf);
    TMVB_CALL_HIP(c, hipGetLastError());
    // ---- documents: theta and C_d, then the token offsets
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    if (chol)
        hipLaunchKernelGGL(gencorp_docs_kernel<true>, dim3((unsigned)M), dim3(64), 0, st, (int)K, doc_offset, seed, mean_C, (const double*)d_par, (const double*)d_chol, d_lt, d_C);
    else
        hipLaunchKernelGGL(gencorp_docs_kernel<false>, dim3((unsigned)M), dim3(64), 0, st, (int)K, doc_offset, seed, mean_C, (const double*)d_par, (const double*)nullptr, d_lt, d_C);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, (const int64_t*)d_C, d_tokptr, (int)(M + 1), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(&T, d_tokptr + M, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    if (T >= (int64_t)INT32_MAX) {
        tmvb_set_error("gencorp: %lld tokens in one call; generate in shards of fewer than 2^31 tokens through doc_offset", (long long)T);
        return c.fail(TMVB_EINVAL);
    }

    // ---- tokens
    int32_t *d_tok, *d_sorted, *d_dt = nullptr;
    unsigned long long* d_tt = nullptr;
    int* d_off;
    char* d_tmp = nullptr;
    size_t sort_bytes = 0;
    TMVB_CALL_TRY(c, c.alloc(&d_tok, (size_t)T)); TMVB_CALL_TRY(c, c.alloc(&d_sorted, (size_t)T)); TMVB_CALL_TRY(c, c.alloc(&d_off, (size_t)M + 1));
    int end_bit = 1;
    while (end_bit < 31 && ((int64_t)1 << end_bit) < V) end_bit++;
    if (T > 0) {
        TMVB_CALL_HIP(c, hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, sort_bytes, (const int32_t*)d_tok, d_sorted, (int)T, (int)M, (const int*)d_off, (const int*)d_off + 1, 0, end_bit, st));
        TMVB_CALL_TRY(c, c.alloc(&d_tmp, std::max<size_t>(sort_bytes, 16)));
    }
    if (diag) {
        TMVB_CALL_TRY(c, c.alloc(&d_dt, (size_t)M * K)); TMVB_CALL_TRY(c, c.alloc(&d_tt, (size_t)KV));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_dt, 0, (size_t)M * K * sizeof(int32_t), st));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_tt, 0, (size_t)KV * sizeof(unsigned long long), st));
    }
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
    hipLaunchKernelGGL(gencorp_tokens_kernel, dim3((unsigned)M), dim3(64), 0, st, (int)K, V, nb, doc_offset, seed, (const float*)d_lt, (const int64_t*)d_tokptr,
                       (const double*)d_bcdf, (const float*)d_wcdf, d_tok, d_dt, d_tt);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));

    // ---- condense
    hipLaunchKernelGGL(gencorp_offsets32_kernel, dim3((unsigned)((M + 256) / 256)), dim3(256), 0, st, (const int64_t*)d_tokptr, M + 1, d_off);
    if (T > 0)
        TMVB_CALL_HIP(c, hipcub::DeviceSegmentedRadixSort::SortKeys((void*)d_tmp, sort_bytes, (const int32_t*)d_tok, d_sorted, (int)T, (int)M, (const int*)d_off, (const int*)d_off + 1, 0, end_bit, st));
    hipLaunchKernelGGL(gencorp_unique_kernel, dim3((unsigned)M), dim3(64), 0, st, (const int32_t*)d_sorted, (const int64_t*)d_tokptr, d_nu);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, (const int64_t*)d_nu, d_docptr, (int)(M + 1), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(&nnz, d_docptr + M, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    int32_t *d_terms, *d_counts;
    TMVB_CALL_TRY(c, c.alloc(&d_terms, (size_t)nnz)); TMVB_CALL_TRY(c, c.alloc(&d_counts, (size_t)nnz));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(6), st));
    hipLaunchKernelGGL(gencorp_rle_kernel, dim3((unsigned)M), dim3(64), 0, st, (const int32_t*)d_sorted, (const int64_t*)d_tokptr, (const int64_t*)d_docptr, d_terms, d_counts);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(7), st));

    // ---- results
    out->M = M; out->nnz = nnz; out->sum_counts = T;
    TMVB_CALL_TRY(c, tmvb_host_alloc("gencorp", &out->doc_ptr, (size_t)M + 1));
    TMVB_CALL_TRY(c, tmvb_host_alloc("gencorp", &out->terms, (size_t)nnz));
    TMVB_CALL_TRY(c, tmvb_host_alloc("gencorp", &out->counts, (size_t)nnz));
    TMVB_CALL_HIP(c, hipMemcpyAsync(out->doc_ptr, d_docptr, ((size_t)M + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (nnz > 0) {
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->terms, d_terms, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->counts, d_counts, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (diag) {
        TMVB_CALL_TRY(c, tmvb_host_alloc("gencorp", &out->log_theta, (size_t)M * K));
        TMVB_CALL_TRY(c, tmvb_host_alloc("gencorp", &out->doc_topic, (size_t)M * K));
        TMVB_CALL_TRY(c, tmvb_host_alloc("gencorp", &out->topic_term, (size_t)KV));
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->log_theta, d_lt, (size_t)M * K * sizeof(float), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->doc_topic, d_dt, (size_t)M * K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(out->topic_term, d_tt, (size_t)KV * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    TMVB_CALL_TRY(c, c.elapsed(&out->ms_tables, 0, 1));
    TMVB_CALL_TRY(c, c.elapsed(&out->ms_docs, 1, 2));
    TMVB_CALL_TRY(c, c.elapsed(&out->ms_tokens, 3, 4));
    float ms_sort = 0.0f, ms_rle = 0.0f;
    TMVB_CALL_TRY(c, c.elapsed(&ms_sort, 4, 5));
    TMVB_CALL_TRY(c, c.elapsed(&ms_rle, 6, 7));
    out->ms_condense = ms_sort + ms_rle;
    guard.release();
    return TMVB_OK;
}
}  // namespace

extern "C" void tmvb_gencorp_free(tmvb_gencorp_t* g)
{
    if (!g) return;
    free(g->doc_ptr); free(g->terms); free(g->counts); free(g->log_theta); free(g->doc_topic); free(g->topic_term);
    memset(g, 0, sizeof(*g));
}

extern "C" int tmvb_lda_gencorp(tmvb_ctx* ctx, int32_t K, int64_t V, const double* alpha, const double* beta, int64_t M, int64_t doc_offset, double mean_C,
                                double laplace_smooth, int64_t seed, int32_t flags, tmvb_gencorp_t* out)
{
    int rc = gc_check_common("tmvb_lda_gencorp", K, GC_LDA_MAX_K, V, beta, M, doc_offset, mean_C, laplace_smooth, out);
    if (rc != TMVB_OK) return rc;
    TMVB_REQUIRE(alpha != nullptr, TMVB_EINVAL, "tmvb_lda_gencorp: NULL argument");
    for (int k = 0; k < K; k++) TMVB_REQUIRE(std::isfinite(alpha[k]) && alpha[k] > 0.0, TMVB_ESHAPE, "alpha must be positive.");     // src/modelutils.jl:47
    if ((rc = tmvb_check_ctx_or_device("tmvb_lda_gencorp", ctx)) != TMVB_OK) return rc;
    return gc_run(ctx, K, V, alpha, nullptr, beta, M, doc_offset, mean_C, laplace_smooth, (uint64_t)seed, flags, out);
}

extern "C" int tmvb_ctm_gencorp(tmvb_ctx* ctx, int32_t K, int64_t V, const double* mu, const double* sigma, const double* beta, int64_t M, int64_t doc_offset,
                                double mean_C, double laplace_smooth, int64_t seed, int32_t flags, tmvb_gencorp_t* out)
{
    int rc = gc_check_common("tmvb_ctm_gencorp", K, GC_CTM_MAX_K, V, beta, M, doc_offset, mean_C, laplace_smooth, out);
    if (rc != TMVB_OK) return rc;
    TMVB_REQUIRE(mu != nullptr && sigma != nullptr, TMVB_EINVAL, "tmvb_ctm_gencorp: NULL argument");
    for (int k = 0; k < K; k++) TMVB_REQUIRE(std::isfinite(mu[k]), TMVB_ESHAPE, "mu must be finite.");                                // src/modelutils.jl:114
    std::vector<double> L;
    TMVB_REQUIRE(gc_cholesky(sigma, K, L), TMVB_ESHAPE, "sigma must be positive-definite.");                                          // :116
    if ((rc = tmvb_check_ctx_or_device("tmvb_ctm_gencorp", ctx)) != TMVB_OK) return rc;
    return gc_run(ctx, K, V, mu, L.data(), beta, M, doc_offset, mean_C, laplace_smooth, (uint64_t)seed, flags, out);
}
