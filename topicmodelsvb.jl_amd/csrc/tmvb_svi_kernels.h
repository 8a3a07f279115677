// tmvb_svi_kernels.h -- the K x V part of the fused global update of stochastic (minibatch) training, shared by its drivers (tmvb_lda_svi.hip,
// tmvb_ctm_svi.hip): blend the running statistic with the batch's, clear the batch's, and row-normalise into beta as update_beta! does.
//
// svi_blend_kernel.  The K x V statistic is column-major, i.e. ONE flat array of n = K V floats whose element q belongs to row q mod K.  A lane walks
// the array in 16-byte units (4-byte units when n is no multiple of 4) with a grid stride that is a multiple of K units: the rows of the lane's
// components never change, so it keeps one fp64 accumulator per component, and consecutive lanes touch consecutive units (coalesced; 2 reads and
// 2 writes of 16 bytes per unit).  The block then lays its 256 x VEC accumulators out in LDS in flat order, where the entries of row i are
// e0(i), e0(i) + K, ...; 256 / K lanes per row add strided shares of them and one lane per row adds the shares: a fixed order, no floating-point
// atomics, the same bits for the same inputs.  Bound: 4 n floats of traffic, HBM (or L2 when 2 n floats fit) -- 20 MB at K = 50, V = 25 319.
// svi_norm_kernel.  Every block adds the blocks' partials per row in the same fixed order (K x at most SVI_BLEND_BLOCKS fp64 values, L2-resident) and
// writes its share of the padded [V][KP] layout with 16-byte stores; the normalisation is update_beta!'s: (float)((double)S * (1.0 / rowsum)).
#pragma once
#include <algorithm>

#include "tmvb_internal.h"

#define SVI_WG 256
#define SVI_BLEND_BLOCKS 128          // partials per row that every block of svi_norm_kernel adds again
#define SVI_NORM_BLOCKS 512

template <int VEC> struct svi_unit;
template <> struct svi_unit<4> { typedef float4 type; };
template <> struct svi_unit<1> { typedef float type; };

__device__ __forceinline__ void svi_blend_unit(float4& a, const float4& b, float c0, float c1, double* acc)
{
    a.x = fmaf(c0, a.x, c1 * b.x); a.y = fmaf(c0, a.y, c1 * b.y); a.z = fmaf(c0, a.z, c1 * b.z); a.w = fmaf(c0, a.w, c1 * b.w);
    acc[0] += (double)a.x; acc[1] += (double)a.y; acc[2] += (double)a.z; acc[3] += (double)a.w;
}
__device__ __forceinline__ void svi_blend_unit(float& a, const float& b, float c0, float c1, double* acc)
{
    a = fmaf(c0, a, c1 * b);
    acc[0] += (double)a;
}
__device__ __forceinline__ void svi_zero(float4& z) { z = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ void svi_zero(float& z) { z = 0.0f; }

// sbar, sb: n = units * VEC floats; stride: lanes that take part (a multiple of K, <= gridDim.x * SVI_WG); partial: [gridDim.x][K];
// ebar: [K] or NULL (a driver whose tail has a kernel of its own); eb: [K] the batch's Elogtheta sums (the tail of the batch buffer), overwritten
// with the blended values for update_alpha!
template <int VEC>
static __global__ __launch_bounds__(SVI_WG) void svi_blend_kernel(float* __restrict__ sbar, float* __restrict__ sb, int64_t units, int K, float c0, float c1,
                                                                  int64_t stride, double* __restrict__ partial, float* __restrict__ ebar, float* __restrict__ eb)
{
    typedef typename svi_unit<VEC>::type U;
    __shared__ double sm[SVI_WG * VEC];
    __shared__ double sm2[SVI_WG];
    const int t = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * SVI_WG, gid = g0 + t;
    double acc[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[c] = 0.0;
    if (gid < stride) {
        U* __restrict__ A = reinterpret_cast<U*>(sbar);
        U* __restrict__ Bv = reinterpret_cast<U*>(sb);
        for (int64_t u = gid; u < units; u += stride) {
            U a = A[u];
            const U b = Bv[u];
            svi_blend_unit(a, b, c0, c1, acc);
            A[u] = a;
#ifndef TMVB_MUTANT_SVI_KEEP_BATCH_STATS     // MUTANT (tests/test_svi_mutant_gpu.py, never in a shipped build): the batch's statistics are not cleared
            U z; svi_zero(z);
            Bv[u] = z;
#endif
        }
    }
    if (blockIdx.x == 0 && ebar)
        for (int i = t; i < K; i += SVI_WG) {
            const float e = fmaf(c0, ebar[i], c1 * eb[i]);
            ebar[i] = e; eb[i] = e;
        }
#pragma unroll
    for (int c = 0; c < VEC; ++c) sm[t * VEC + c] = acc[c];
    __syncthreads();
    // entry e of sm is flat element VEC * g0 + e (mod the walk's stride): row (VEC * g0 + e) mod K
    const int off = (int)((VEC * g0) % K);
    if (K <= SVI_WG) {
        const int P = SVI_WG / K, part = t / K, i = t - part * K;
        if (part < P) {
            double s = 0.0;
            for (int e = (i - off + K) % K + part * K; e < SVI_WG * VEC; e += P * K) s += sm[e];
            sm2[part * K + i] = s;
        }
        __syncthreads();
        if (t < K) {
            double s = 0.0;
            for (int p = 0; p < P; ++p) s += sm2[p * K + t];
            partial[(int64_t)blockIdx.x * K + t] = s;
        }
    } else {
        for (int i = t; i < K; i += SVI_WG) {
            double s = 0.0;
            for (int e = (i - off + K) % K; e < SVI_WG * VEC; e += K) s += sm[e];
            partial[(int64_t)blockIdx.x * K + i] = s;
        }
    }
}

// beta_new: padded [V][KP] (pad columns zero); dynamic LDS: K doubles
static __global__ __launch_bounds__(SVI_WG) void svi_norm_kernel(const float* __restrict__ sbar, const double* __restrict__ partial, int nb, int K, int KP, int64_t V,
                                                                 float* __restrict__ beta_new)
{
    extern __shared__ double rinv[];
    __shared__ double sm2[SVI_WG];
    const int t = threadIdx.x;
    if (K <= SVI_WG) {
        const int P = SVI_WG / K, part = t / K, i = t - part * K;
        const int len = (nb + P - 1) / P;
        if (part < P) {
            double s = 0.0;
            const int b1 = min(nb, (part + 1) * len);
            for (int b = part * len; b < b1; ++b) s += partial[(int64_t)b * K + i];
            sm2[part * K + i] = s;
        }
        __syncthreads();
        if (t < K) {
            double s = 0.0;
            for (int p = 0; p < P; ++p) s += sm2[p * K + t];
            rinv[t] = 1.0 / s;
        }
    } else {
        for (int i = t; i < K; i += SVI_WG) {
            double s = 0.0;
            for (int b = 0; b < nb; ++b) s += partial[(int64_t)b * K + i];
            rinv[i] = 1.0 / s;
        }
    }
    __syncthreads();
    const int64_t units = V * (int64_t)(KP / 4);
    const int64_t stride = (int64_t)gridDim.x * SVI_WG;
    float4* __restrict__ out = reinterpret_cast<float4*>(beta_new);
    const int lpr = KP / 4;
    for (int64_t u = (int64_t)blockIdx.x * SVI_WG + t; u < units; u += stride) {
        const int64_t j = u / lpr;
        const int i = 4 * (int)(u - j * lpr);
        const float* __restrict__ s = sbar + j * K;
        float4 o;
        o.x = i < K ? (float)((double)s[i] * rinv[i]) : 0.0f;
        o.y = i + 1 < K ? (float)((double)s[i + 1] * rinv[i + 1]) : 0.0f;
        o.z = i + 2 < K ? (float)((double)s[i + 2] * rinv[i + 2]) : 0.0f;
        o.w = i + 3 < K ? (float)((double)s[i + 3] * rinv[i + 3]) : 0.0f;
        out[u] = o;
    }
}

// the two launches of the K x V update on stream st (d_partial holds max(SVI_BLEND_BLOCKS, ceil(K / 256)) x K doubles); ebar / eb as
// svi_blend_kernel takes them
static inline int svi_launch_blend_norm(hipStream_t st, float* d_sbar, float* d_sb, int K, int KP, int64_t V, float c0, float c1, double* d_partial, float* d_ebar,
                                        float* d_eb, float* d_beta_new)
{
    const int64_t n = (int64_t)K * V;
    const bool vec = (n % 4) == 0;
    const int64_t units = vec ? n / 4 : n;
    int nb = (int)std::min<int64_t>(SVI_BLEND_BLOCKS, std::max<int64_t>(1, (units + SVI_WG - 1) / SVI_WG));
    nb = std::max(nb, (K + SVI_WG - 1) / SVI_WG);
    const int64_t stride = ((int64_t)nb * SVI_WG / K) * K;          // >= K: the lanes [0, stride) walk, whole rows of units at a time
    if (vec) hipLaunchKernelGGL((svi_blend_kernel<4>), dim3(nb), dim3(SVI_WG), 0, st, d_sbar, d_sb, units, K, c0, c1, stride, d_partial, d_ebar, d_eb);
    else hipLaunchKernelGGL((svi_blend_kernel<1>), dim3(nb), dim3(SVI_WG), 0, st, d_sbar, d_sb, units, K, c0, c1, stride, d_partial, d_ebar, d_eb);
    TMVB_HIP(hipGetLastError());
    const int64_t ounits = V * (int64_t)(KP / 4);
    const int nbn = (int)std::min<int64_t>(SVI_NORM_BLOCKS, std::max<int64_t>(1, (ounits + SVI_WG - 1) / SVI_WG));
    hipLaunchKernelGGL(svi_norm_kernel, dim3(nbn), dim3(SVI_WG), (size_t)K * sizeof(double), st, (const float*)d_sbar, (const double*)d_partial, nb, K, KP, V, d_beta_new);
    TMVB_HIP(hipGetLastError());
    return TMVB_OK;
}
