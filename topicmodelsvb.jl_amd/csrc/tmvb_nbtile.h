// tmvb_nbtile.h -- what tmvb_neighbors.hip, tmvb_recranks.hip and tmvb_rectopn.hip share: the fp32 feature layout [M][kp], the LDS staging of a
// 128-row operand tile and the 2 x 2 accumulator K-chunk loop on v_mfma_f32_32x32x2_f32.  Device code only; each unit keeps its own kernels (and their names).
//
// Layout.  kp = K rounded up to a multiple of 4, pads zero.  Inside every group of four the values sit in the order k = 0, 2, 1, 3 (nb_perm): a
// lane of the lower half of a wave then reads the k = 4t and 4t + 2 of its row with ONE 8-byte read and a lane of the upper half k = 4t + 1 and
// 4t + 3 -- the operands of two consecutive v_mfma_f32_32x32x2_f32 (lane l holds A[i = l & 31][k = l >> 5]), whose accumulator chain so runs
// over k in ascending order.  A score is the same bits wherever these pieces compute it: the same instruction, operand values and k order.
#pragma once

#include "tmvb_internal.h"

#define NB_MAX_K 1024
#define NB_WG 256
#define NB_QT 128                   // queries per workgroup
#define NB_TD TMVB_NB_TILE_DB       // database rows per tile
#define NB_KC_ONE 64                // kp up to this: one K-chunk, the query tile stays resident
#define NB_KC 32                    // else chunks of this many floats
static_assert(NB_TD == 128 && NB_QT == 128, "a workgroup is 2 x 2 waves of 64 x 64");

typedef float nb_f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ __forceinline__ int nb_perm(int k) { return (k & ~3) | ((k & 1) << 1) | ((k >> 1) & 1); }

// one wave: row xr[K] (fp64, transformed by `metric`) -> fr[kp] (fp32, each value rounded once, the group order above)
__device__ __forceinline__ void nb_feature_row(int K, int kp, int metric, const double* __restrict__ xr, float* __restrict__ fr, int lane)
{
    double inv = 1.0;
    if (metric == TMVB_NB_COSINE) {
        double s = 0.0;
        for (int k = lane; k < K; k += 64) s = fma(xr[k], xr[k], s);
        inv = sqrt(wave_sum_d(s));
    }
    for (int p = lane; p < kp; p += 64) {
        const int k = nb_perm(p);
        double v = 0.0;
        if (k < K) {
            v = xr[k];
            if (metric == TMVB_NB_HELLINGER) v = sqrt(v);
            else if (metric == TMVB_NB_COSINE) v = v / inv;
        }
        fr[p] = (float)v;
    }
}

// 128 rows [row0, row0 + 128) x floats [k0, k0 + kc) of F[rows][kp] into s[128][S], S = kc + 2; rows at or past `rows` are zero
__device__ __forceinline__ void nb_stage(float* __restrict__ s, int S, const float* __restrict__ F, int64_t row0, int64_t rows, int kp, int k0, int kc)
{
    const int upr = kc >> 2;                            // 16-byte units per row
    for (int u = threadIdx.x; u < 128 * upr; u += NB_WG) {
        const int row = u / upr, c = u - row * upr;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row0 + row < rows) v = *reinterpret_cast<const float4*>(F + (row0 + row) * kp + k0 + 4 * c);
        float2* d = reinterpret_cast<float2*>(s + row * S + 4 * c);
        d[0] = make_float2(v.x, v.y);
        d[1] = make_float2(v.z, v.w);
    }
}

// one K-chunk of kc floats, staged: pa / pb = this lane's row of the wave's first 32-row block of each operand (+ 2 * half); the second block
// lies 32 rows further.  acc[a][b]: query block a x database block b.
__device__ __forceinline__ void nb_chunk_mma(nb_f32x16 (&acc)[2][2], const float* __restrict__ pa, const float* __restrict__ pb, int S, int kc)
{
    for (int kk = 0; kk < kc; kk += 4) {
        const float2 a0 = *reinterpret_cast<const float2*>(pa + kk), a1 = *reinterpret_cast<const float2*>(pa + 32 * S + kk);
        const float2 b0 = *reinterpret_cast<const float2*>(pb + kk), b1 = *reinterpret_cast<const float2*>(pb + 32 * S + kk);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b1.x, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b0.x, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc[1][1], 0, 0, 0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b1.y, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b0.y, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc[1][1], 0, 0, 0);
    }
}

// The scores of one database tile against the workgroup's query tile: acc zeroed, then every K-chunk in ascending order.  sA / sB: [128][S],
// S = kc_max + 2.  With one chunk the query tile is staged by the caller once; else it is restaged per chunk here.  Leaves no barrier behind:
// the caller's next write to sA / sB comes after the first barrier of its next call.
__device__ __forceinline__ void nb_tile_scores(nb_f32x16 (&acc)[2][2], float* __restrict__ sA, float* __restrict__ sB, int S, int kp, int kc_max, bool one_chunk,
                                               const float* __restrict__ Fq, int64_t qt0, int64_t Mq, const float* __restrict__ Fd, int64_t e0, int64_t Md,
                                               int wq, int wd, int l31, int half)
{
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
    for (int k0 = 0; k0 < kp; k0 += kc_max) {
        const int kc = min(kc_max, kp - k0);
        __syncthreads();                                             // the previous chunk / tile has been read
        if (!one_chunk) nb_stage(sA, S, Fq, qt0, Mq, kp, k0, kc);
        nb_stage(sB, S, Fd, e0, Md, kp, k0, kc);
        __syncthreads();
        nb_chunk_mma(acc, sA + (64 * wq + l31) * S + 2 * half, sB + (64 * wd + l31) * S + 2 * half, S, kc);
    }
}
