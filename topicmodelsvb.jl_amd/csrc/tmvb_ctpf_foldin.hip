// tmvb_ctpf_foldin.hip -- CTPF fold-in: he[:, u] of users who were not in training, iterated to its fixed point with every document factor
// frozen (include/tmvb.h states the operator).  The reference moves he once per walk over the corpus (update_he!,
// src/CTPF.jl:266-277) and never iterates it per user: a new operator.
//
// The 2K-way softmax of update_xi! (src/CTPF.jl:334-337) for the pair (d, u) holds psi(he[i, u]) in both halves at index i, so that
//     xi[i] + xi[K + i] = exp(psi(h_i)) W[i, d] / sum_j exp(psi(h_j)) W[j, d],   W[i, d] = (exp(psi(gimel[i, d])) / dalet[i] + exp(psi(zayin[i, d])) / het[i]) / vav[i]
// and W does not move while h does.  A user is then a document whose tokens are its library entries and whose beta columns are W[:, d].
//   prep      foldin_w_kernel: W as [M][kp] fp32, kp = K rounded up to a multiple of 4, the pads 0; one kernel for both forms (fp32 state in).  No max-subtraction: exp(psi(x)) <= x for x > 0
//             (psi(x) < log x), gimel <= c + the document's counts + ratings and zayin <= g + its ratings, each far below 2^31, and the rates
//             are positive and finite (checked on the host), so W <= 2 x / (rate vav) stays far inside fp32; at the low end exp(psi(x)) is a normal
//             fp32 number down to x = 0.012 (psi(x) ~ -1 / x), an order of magnitude under the shape hyperparameters c = g = 0.1 that bound gimel
//             and zayin from below.  A smaller shape flushes its term to 0 and the entry's normaliser is held at FLT_MIN.
//   sweeps    Layout of both user kernels: topic i = lane + 64 s, slot s < NS (NS = 1, 2, 4, 8 for K <= 64, 128, 256, 512): a W row is one coalesced
//             load per slot, the normaliser of an entry one wave_sum, the new h one fmaf per slot.  exp(psi(h)) is taken relative to its largest
//             entry (one wave_max per sweep; p is unchanged by a common factor), so h itself needs no range argument.
//             foldin_users_kernel: one wave per user, the library's rows gathered ONCE into a register tile of CAP x NS floats (CAP = 32, 16 for NS = 8:
//             at most 128 VGPRs of tile) that stays put over all sweeps; the entry loop is fully unrolled under wave-uniform guards c < R.
//             foldin_users_long_kernel: a workgroup of four waves per user; wave w takes entries w, w + 4, ..., gathers their rows again in every
//             sweep (L2), the four partial sums meet in LDS and EVERY wave adds them in the order 0, 1, 2, 3 and runs the tail itself -- four
//             identical tails, no broadcast of h and a workgroup-uniform exit.
//             Why lane = topic and not the 16 x 4 grid of tmvb_gridtile.h or the lane = entry tile of tmvb_regtile.h: read off the instructions per
//             entry and sweep.  Here 2 NS fmaf + one wave_sum (6 DPP adds, 1 readlane) + 1 reciprocal; the entry's rating comes from a readlane.
//             Lane = entry needs K registers per lane for the row (K <= 512 does not fit) and trades the per-entry sum for a per-topic one; the grid
//             halves the reduction to a 16-lane one but needs the reduce-scatter tables and the KP <= 60 restriction of the document kernels.
//             Nothing here rests on a measurement: tools/ctpf_foldin_bench.py measures.
//   tail      one topic per lane-slot: h_new = fmaf(exp(t_i - max t), acc_i, e), the squared change summed over the wave, the exit test of
//             src/CTPF.jl:359 with he in the place of gimel, digamma_f for the next sweep.
// No atomics, no scratch, one fixed summation order per path; a user's path depends on its own library length and K alone.
#include "tmvb_internal.h"
#include "tmvb_call.h"

#include <algorithm>
#include <cfloat>
#include <cstring>

#define FI_LONG_WAVES 4

// ------------------------------------------------------------------------------------------------------------------ prep
// gimel / zayin: [M][K] (= column-major K x M) in fp32 -- the state of a handle, or the host's fp64 arrays rounded once on the host, as tmvb_ctpf_set_state
// rounds them: ONE kernel for both forms, hence the same bits.  The rates arrive in fp64 (the handle keeps them so) and are rounded once here.
static __global__ __launch_bounds__(256) void foldin_w_kernel(int K, int kp, int64_t M, const float* __restrict__ gimel, const float* __restrict__ zayin,
                                                              const double* __restrict__ dalet, const double* __restrict__ het,
                                                              const double* __restrict__ vav, float* __restrict__ W)
{
    const int64_t n = M * kp, step = (int64_t)gridDim.x * 256;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += step) {
        const int64_t d = idx / kp;
        const int i = (int)(idx - d * kp);
        float w = 0.0f;
        if (i < K) {
            const float g = gimel[d * K + i], z = zayin[d * K + i];
            w = expf(digamma_f(g)) / (float)dalet[i];
#ifndef TMVB_MUTANT_FOLDIN_DROP_ZAYIN
            w += expf(digamma_f(z)) / (float)het[i];
#else
            (void)z;                                    // MUTANT: the users are folded in against gimel alone
#endif
            w /= (float)vav[i];
        }
        W[idx] = w;
    }
}

// ------------------------------------------------------------------------------------------------------------------ sweeps
struct FoldinParams {
    int K, kp, viter;
    float vtol, e;
    const float* W;                 // [M][kp]
    const int64_t* lib_ptr;         // [Un + 1]
    const int32_t* lib_docs;
    const int32_t* lib_ratings;
    const double* he0;              // [Un][K] or NULL: all ones
    const int32_t* users;           // the users of this launch, one per wave / workgroup
    double* he;                     // [Un][K]
    int32_t* sweeps;                // [Un]
};

template <int NS>
__device__ __forceinline__ void fi_load_h(const FoldinParams& p, int u, int lane, float (&h)[NS])
{
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int i = lane + 64 * s;
        h[s] = (i < p.K && p.he0) ? (float)p.he0[(int64_t)u * p.K + i] : 1.0f;       // a lane without a topic keeps 1: digamma_f needs x > 0
    }
}

// et_i = exp(psi(h_i) - max_j psi(h_j)); 0 for a lane-slot without a topic
template <int NS>
__device__ __forceinline__ void fi_weights(int K, int lane, const float (&h)[NS], float (&et)[NS])
{
    float t[NS], m = -INFINITY;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        t[s] = digamma_f(h[s]);
        if (lane + 64 * s < K) m = fmaxf(m, t[s]);
    }
    m = wave_max(m);
#pragma unroll
    for (int s = 0; s < NS; s++) et[s] = lane + 64 * s < K ? expf(t[s] - m) : 0.0f;
}

// one entry: acc += r w / sum_j et_j w_j.  All 64 lanes are active (the callers' guards are wave-uniform).
template <int NS>
__device__ __forceinline__ void fi_entry(const float (&et)[NS], const float (&w)[NS], float r, float (&acc)[NS])
{
    float part = 0.0f;
#pragma unroll
    for (int s = 0; s < NS; s++) part = fmaf(et[s], w[s], part);
    const float q = r * fast_rcp(fmaxf(wave_sum(part), FLT_MIN));
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = fmaf(q, w[s], acc[s]);
}

// h <- e + et .* acc; returns ||h_new - h||_2
template <int NS>
__device__ __forceinline__ float fi_tail(int K, int lane, float e, const float (&et)[NS], const float (&acc)[NS], float (&h)[NS])
{
    float dn = 0.0f;
#pragma unroll
    for (int s = 0; s < NS; s++)
        if (lane + 64 * s < K) {
            const float hn = fmaf(et[s], acc[s], e);
            const float df = hn - h[s];
            dn = fmaf(df, df, dn);
            h[s] = hn;
        }
    return sqrtf(wave_sum(dn));
}

template <int NS>
__device__ __forceinline__ void fi_store(const FoldinParams& p, int u, int lane, const float (&h)[NS], int sweeps)
{
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int i = lane + 64 * s;
        if (i < p.K) p.he[(int64_t)u * p.K + i] = (double)h[s];
    }
    if (lane == 0) p.sweeps[u] = sweeps;
}

// one wave per user, R <= CAP entries: the W rows of the library live in registers over all sweeps
template <int NS, int CAP>
static __global__ __launch_bounds__(64) void foldin_users_kernel(FoldinParams p)
{
    const int lane = threadIdx.x;
    const int u = p.users[blockIdx.x];
    const int64_t lo = p.lib_ptr[u];
    const int R = (int)(p.lib_ptr[u + 1] - lo);                         // <= CAP <= 64 (the host's classes)
    float w[CAP][NS];
    float myr = 0.0f;                                                    // lane c holds the rating of entry c
    if (lane < R) myr = (float)p.lib_ratings[lo + lane];
#pragma unroll
    for (int c = 0; c < CAP; c++)
        if (c < R) {                                                     // wave-uniform
            const float* row = p.W + (int64_t)p.lib_docs[lo + c] * p.kp;
#pragma unroll
            for (int s = 0; s < NS; s++) w[c][s] = lane + 64 * s < p.K ? row[lane + 64 * s] : 0.0f;
        } else {
#pragma unroll
            for (int s = 0; s < NS; s++) w[c][s] = 0.0f;
        }
    float h[NS], et[NS], acc[NS];
    fi_load_h<NS>(p, u, lane, h);
    int sweeps = 0;
    for (int it = 0; it < p.viter; it++) {
        fi_weights<NS>(p.K, lane, h, et);
#pragma unroll
        for (int s = 0; s < NS; s++) acc[s] = 0.0f;
#pragma unroll
        for (int c = 0; c < CAP; c++)
            if (c < R) fi_entry<NS>(et, w[c], __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, myr), c)), acc);
        const float norm = fi_tail<NS>(p.K, lane, p.e, et, acc, h);
        sweeps++;
        if (norm < p.vtol) break;                                        // wave-uniform: norm comes out of wave_sum
    }
    fi_store<NS>(p, u, lane, h, sweeps);
}

// a workgroup of FI_LONG_WAVES waves per user: wave w takes entries w, w + 4, ... and gathers their rows again in every sweep
template <int NS>
static __global__ __launch_bounds__(64 * FI_LONG_WAVES) void foldin_users_long_kernel(FoldinParams p)
{
    __shared__ float part[FI_LONG_WAVES][NS * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = p.users[blockIdx.x];
    const int64_t lo = p.lib_ptr[u];
    const int R = (int)(p.lib_ptr[u + 1] - lo);
    float h[NS], et[NS], acc[NS], w[NS];
    fi_load_h<NS>(p, u, lane, h);
    int sweeps = 0;
    for (int it = 0; it < p.viter; it++) {
        fi_weights<NS>(p.K, lane, h, et);
#pragma unroll
        for (int s = 0; s < NS; s++) acc[s] = 0.0f;
        for (int c = wave; c < R; c += FI_LONG_WAVES) {                  // wave-uniform
            const float* row = p.W + (int64_t)p.lib_docs[lo + c] * p.kp;
#pragma unroll
            for (int s = 0; s < NS; s++) w[s] = lane + 64 * s < p.K ? row[lane + 64 * s] : 0.0f;
            fi_entry<NS>(et, w, (float)p.lib_ratings[lo + c], acc);
        }
#pragma unroll
        for (int s = 0; s < NS; s++) part[wave][64 * s + lane] = acc[s];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; s++) acc[s] = ((part[0][64 * s + lane] + part[1][64 * s + lane]) + part[2][64 * s + lane]) + part[3][64 * s + lane];
        __syncthreads();                                                 // the next sweep writes `part` again
        const float norm = fi_tail<NS>(p.K, lane, p.e, et, acc, h);      // the same bits in all four waves
        sweeps++;
        if (norm < p.vtol) break;                                        // workgroup-uniform
    }
    if (wave == 0) fi_store<NS>(p, u, lane, h, sweeps);
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
struct fi_state {                       // the frozen state: host fp64 arrays (stateless form) or a handle's device arrays
    const double *h_gimel = nullptr, *h_zayin = nullptr, *h_dalet = nullptr, *h_het = nullptr, *h_vav = nullptr;
    const float *d_gimel = nullptr, *d_zayin = nullptr;
    const double *d_dalet = nullptr, *d_het = nullptr, *d_vav = nullptr;
};

int fi_capacity(int K) { return K > 256 ? TMVB_FOLDIN_REG_CAP_BIGK : TMVB_FOLDIN_REG_CAP; }

int fi_check_positive(const char* fn, const char* name, const double* x, int64_t n)
{
    for (int64_t j = 0; j < n; j++) TMVB_REQUIRE(std::isfinite(x[j]) && x[j] > 0.0, TMVB_ESHAPE, "%s: %s holds a value that is not positive and finite (entry %lld)", fn, name, (long long)j);
    return TMVB_OK;
}

// everything but the state: the checks shared by both forms
int fi_check_args(const char* fn, int32_t K, int64_t M, double e, int64_t Un, const int64_t* lib_ptr, const int32_t* lib_docs, const int32_t* lib_ratings,
                  const double* he0, int32_t viter, double vtol, const double* he_out, const int32_t* sweeps_out)
{
    TMVB_REQUIRE(K >= 1 && K <= 512, TMVB_EINVAL, "%s: K = %d outside [1, 512]", fn, K);
    TMVB_REQUIRE(M > 0, TMVB_EINVAL, "%s: M must be a positive integer", fn);
    TMVB_REQUIRE(M < ((int64_t)1 << 31), TMVB_EINVAL, "%s: M = %lld is 2^31 or more", fn, (long long)M);
    TMVB_REQUIRE(Un >= 0 && Un < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: Un = %lld outside [0, 2^31 - 1)", fn, (long long)Un);
    TMVB_REQUIRE(viter >= 0, TMVB_EINVAL, "%s: viter must be nonnegative", fn);
    TMVB_REQUIRE(std::isfinite(vtol) && vtol >= 0.0, TMVB_EINVAL, "%s: vtol must be nonnegative and finite", fn);
    TMVB_REQUIRE(std::isfinite(e) && e > 0.0, TMVB_EINVAL, "%s: e must be positive and finite", fn);
    TMVB_REQUIRE(lib_ptr && (he_out || Un == 0) && (sweeps_out || Un == 0), TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(lib_ptr[0] == 0, TMVB_ESHAPE, "%s: lib_ptr must start at 0", fn);
    for (int64_t u = 0; u < Un; u++) TMVB_REQUIRE(lib_ptr[u + 1] >= lib_ptr[u], TMVB_ESHAPE, "%s: lib_ptr decreases at user %lld", fn, (long long)u);
    TMVB_REQUIRE(lib_ptr[Un] < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: %lld library entries in one call (limit 2^31 - 2); shard the users", fn, (long long)lib_ptr[Un]);
    TMVB_REQUIRE((lib_docs && lib_ratings) || lib_ptr[Un] == 0, TMVB_EINVAL, "%s: NULL argument", fn);
    for (int64_t u = 0; u < Un; u++)
        for (int64_t j = lib_ptr[u]; j < lib_ptr[u + 1]; j++) {
            TMVB_REQUIRE(lib_docs[j] >= 0 && lib_docs[j] < M, TMVB_ESHAPE, "%s: user %lld holds document id %d outside [0, %lld)", fn, (long long)u, lib_docs[j], (long long)M);
            TMVB_REQUIRE(j == lib_ptr[u] || lib_docs[j] > lib_docs[j - 1], TMVB_ESHAPE, "%s: the document ids of user %lld are not strictly ascending", fn, (long long)u);
            TMVB_REQUIRE(lib_ratings[j] >= 1, TMVB_ESHAPE, "%s: user %lld holds a rating below 1", fn, (long long)u);
        }
    if (he0) return fi_check_positive(fn, "he0", he0, (int64_t)K * Un);
    return TMVB_OK;
}

// NS = 8 is K > 256: the capacity of fi_capacity
template <int NS>
void fi_launch(const FoldinParams& p, int64_t n_reg, const int32_t* d_reg, int64_t n_long, const int32_t* d_long, hipStream_t st)
{
    constexpr int CAP = NS == 8 ? TMVB_FOLDIN_REG_CAP_BIGK : TMVB_FOLDIN_REG_CAP;
    FoldinParams q = p;
    if (n_reg > 0) {
        q.users = d_reg;
        hipLaunchKernelGGL((foldin_users_kernel<NS, CAP>), dim3((unsigned)n_reg), dim3(64), 0, st, q);
    }
    if (n_long > 0) {
        q.users = d_long;
        hipLaunchKernelGGL(foldin_users_long_kernel<NS>, dim3((unsigned)n_long), dim3(64 * FI_LONG_WAVES), 0, st, q);
    }
}

int fi_run(tmvb_ctx* ctx, int32_t K, int64_t M, const fi_state& s, double e, int64_t Un, const int64_t* lib_ptr, const int32_t* lib_docs,
           const int32_t* lib_ratings, const double* he0, int32_t viter, double vtol, double* he_out, int32_t* sweeps_out, tmvb_foldin_info_t* info)
{
    const int kp = (K + 3) & ~3, cap = fi_capacity(K);
    if (info) { info->kp = kp; info->capacity = cap; }
    if (Un == 0) return TMVB_OK;
    // launch classes by library length; the order inside a class is the caller's
    std::vector<int32_t> reg, lng;
    for (int64_t u = 0; u < Un; u++) (lib_ptr[u + 1] - lib_ptr[u] <= cap ? reg : lng).push_back((int32_t)u);
    const int64_t nE = lib_ptr[Un];
    const size_t KM = (size_t)K * M;
    std::vector<float> g32, z32;                        // stateless form: the state rounded once to fp32, as a handle holds it
    if (s.h_gimel) {
        g32.resize(KM); z32.resize(KM);
        for (size_t j = 0; j < KM; j++) { g32[j] = (float)s.h_gimel[j]; z32[j] = (float)s.h_zayin[j]; }
    }

    hipStream_t st = ctx->stream;
    tmvb_call c("ctpf_foldin_users", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(4));
    float* d_W;
    int64_t* d_lp;
    int32_t *d_ld, *d_lr, *d_reg, *d_lng, *d_sw;
    double *d_he0 = nullptr, *d_he;
    TMVB_CALL_TRY(c, c.alloc(&d_W, (size_t)M * kp));
    TMVB_CALL_TRY(c, c.upload(&d_lp, lib_ptr, (size_t)Un + 1)); TMVB_CALL_TRY(c, c.upload(&d_ld, lib_docs, (size_t)nE));
    TMVB_CALL_TRY(c, c.upload(&d_lr, lib_ratings, (size_t)nE));
    TMVB_CALL_TRY(c, c.upload(&d_reg, (const int32_t*)reg.data(), reg.size())); TMVB_CALL_TRY(c, c.upload(&d_lng, (const int32_t*)lng.data(), lng.size()));
    if (he0) TMVB_CALL_TRY(c, c.upload(&d_he0, he0, (size_t)K * Un));
    TMVB_CALL_TRY(c, c.alloc(&d_he, (size_t)K * Un)); TMVB_CALL_TRY(c, c.alloc(&d_sw, (size_t)Un));
    const unsigned wblocks = (unsigned)std::min<int64_t>(((int64_t)M * kp + 255) / 256, (int64_t)ctx->num_cu * 64);

    // stage times: the events bracket the kernels only; allocations and copies lie outside
    const float *d_g = s.d_gimel, *d_z = s.d_zayin;
    const double *d_da = s.d_dalet, *d_ht = s.d_het, *d_va = s.d_vav;
    if (s.h_gimel) {
        float *u_g, *u_z;
        double *u_da, *u_ht, *u_va;
        TMVB_CALL_TRY(c, c.upload(&u_g, (const float*)g32.data(), KM)); TMVB_CALL_TRY(c, c.upload(&u_z, (const float*)z32.data(), KM));
        TMVB_CALL_TRY(c, c.upload(&u_da, s.h_dalet, (size_t)K)); TMVB_CALL_TRY(c, c.upload(&u_ht, s.h_het, (size_t)K)); TMVB_CALL_TRY(c, c.upload(&u_va, s.h_vav, (size_t)K));
        d_g = u_g; d_z = u_z; d_da = u_da; d_ht = u_ht; d_va = u_va;
    }
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    hipLaunchKernelGGL(foldin_w_kernel, dim3(wblocks), dim3(256), 0, st, (int)K, kp, M, d_g, d_z, d_da, d_ht, d_va, d_W);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));

    FoldinParams p;
    p.K = K; p.kp = kp; p.viter = viter; p.vtol = (float)vtol; p.e = (float)e;
    p.W = d_W; p.lib_ptr = d_lp; p.lib_docs = d_ld; p.lib_ratings = d_lr; p.he0 = d_he0; p.users = nullptr; p.he = d_he; p.sweeps = d_sw;
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
    const int64_t nr = (int64_t)reg.size(), nl = (int64_t)lng.size();
    if (K <= 64) fi_launch<1>(p, nr, d_reg, nl, d_lng, st);
    else if (K <= 128) fi_launch<2>(p, nr, d_reg, nl, d_lng, st);
    else if (K <= 256) fi_launch<4>(p, nr, d_reg, nl, d_lng, st);
    else fi_launch<8>(p, nr, d_reg, nl, d_lng, st);
    TMVB_CALL_HIP(c, hipGetLastError());
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(he_out, d_he, (size_t)K * Un * sizeof(double), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(sweeps_out, d_sw, (size_t)Un * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    if (info) {
        info->n_reg = nr; info->n_long = nl;
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_prep, 0, 1));
        TMVB_CALL_TRY(c, c.elapsed(&info->ms_sweeps, 2, 3));
    }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_ctpf_foldin_users(tmvb_ctx* ctx, int32_t K, int64_t M, const double* gimel, const double* zayin, const double* dalet, const double* het,
                                      const double* vav, double e, int64_t Un, const int64_t* lib_ptr, const int32_t* lib_docs, const int32_t* lib_ratings,
                                      const double* he0, int32_t viter, double vtol, double* he_out, int32_t* sweeps_out, tmvb_foldin_info_t* info)
{
    const char* fn = "tmvb_ctpf_foldin_users";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(gimel && zayin && dalet && het && vav, TMVB_EINVAL, "%s: NULL argument", fn);
    int rc;
    if ((rc = fi_check_args(fn, K, M, e, Un, lib_ptr, lib_docs, lib_ratings, he0, viter, vtol, he_out, sweeps_out)) != TMVB_OK) return rc;
    if ((rc = fi_check_positive(fn, "gimel", gimel, (int64_t)K * M)) != TMVB_OK || (rc = fi_check_positive(fn, "zayin", zayin, (int64_t)K * M)) != TMVB_OK ||
        (rc = fi_check_positive(fn, "dalet", dalet, K)) != TMVB_OK || (rc = fi_check_positive(fn, "het", het, K)) != TMVB_OK ||
        (rc = fi_check_positive(fn, "vav", vav, K)) != TMVB_OK)
        return rc;
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    fi_state s;
    s.h_gimel = gimel; s.h_zayin = zayin; s.h_dalet = dalet; s.h_het = het; s.h_vav = vav;
    return fi_run(ctx, K, M, s, e, Un, lib_ptr, lib_docs, lib_ratings, he0, viter, vtol, he_out, sweeps_out, info);
}

extern "C" int tmvb_ctpf_foldin_users_on(tmvb_ctpf* h, int64_t Un, const int64_t* lib_ptr, const int32_t* lib_docs, const int32_t* lib_ratings,
                                         const double* he0, int32_t viter, double vtol, double* he_out, int32_t* sweeps_out, tmvb_foldin_info_t* info)
{
    const char* fn = "tmvb_ctpf_foldin_users_on";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(h != nullptr, TMVB_EINVAL, "%s: handle is NULL", fn);
    tmvb_ctpf_view v;
    int rc;
    if ((rc = tmvb_ctpf_view_of(h, &v)) != TMVB_OK) return rc;
    if ((rc = fi_check_args(fn, v.K, v.M, v.e, Un, lib_ptr, lib_docs, lib_ratings, he0, viter, vtol, he_out, sweeps_out)) != TMVB_OK) return rc;
    fi_state s;                                         // rates: [8][K] = bet, vav, dalet, het, *_old
    s.d_gimel = v.gimel; s.d_zayin = v.zayin; s.d_vav = v.rates + v.K; s.d_dalet = v.rates + 2 * v.K; s.d_het = v.rates + 3 * v.K;
    return fi_run(v.ctx, v.K, v.M, s, v.e, Un, lib_ptr, lib_docs, lib_ratings, he0, viter, vtol, he_out, sweeps_out, info);
}
