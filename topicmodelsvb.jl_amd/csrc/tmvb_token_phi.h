// tmvb_token_phi.h -- the responsibilities r of one corpus entry from the two staged factor rows, the ONE place where the arithmetic of
// tmvb_token_topics (include/tmvb.h) is written down.  token_topics_kernel (tmvb_token_topics.hip) and group_topics_kernel
// (tmvb_group_topics.hip) both call it, so that the grouped statistics add up exactly the bits the per-entry call returns.
//
//   L = 2^logL lanes per entry; lane r of the entry holds the 16-byte chunks r, r + L, r + 2 L, r + 3 L of the two rows (at most four: <= 16 topics).
//   y_k = fma(a_k, b_k, eps) on topics, 0 on pads; per lane ((y0 + y1) + (y2 + y3)) per chunk, chunks ascending; the L partial sums meet in a
//   fixed xor butterfly, so every lane of the entry holds the same bits of S; r = y / S is the IEEE fp32 division.
#pragma once

// lanes per entry: the smallest power of two that leaves a lane at most four 16-byte chunks of the row, at most a wave (tmvb_heldout.hip)
static inline int tt_log_lanes(int K)
{
    const int nch = (K + 3) / 4;
    int logL = 0;
    while (logL < 6 && (4 << logL) < nch) logL++;
    return logL;
}

#if defined(__HIPCC__)
// bit 4 q + j: value j of the lane's q-th chunk is a topic
__device__ __forceinline__ unsigned tt_value_mask(int K, int r, int L)
{
    unsigned vmask = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * (r + q * L) + j < K) vmask |= 1u << (4 * q + j);
    return vmask;
}

// av, bv: the lane's chunks of the document's and the term's row (zeros where the lane holds no chunk).  Every lane of the entry calls it: the
// butterfly has a uniform trip count.  live == false: the lane group holds no entry; its y come out finite and are not used.
__device__ __forceinline__ void tt_responsibilities(float (&y)[16], const float4 (&av)[4], const float4 (&bv)[4], unsigned vmask, float eps, int L, bool live)
{
    float S = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        y[4 * q + 0] = (vmask >> (4 * q + 0)) & 1u ? __fmaf_rn(av[q].x, bv[q].x, eps) : 0.0f;
        y[4 * q + 1] = (vmask >> (4 * q + 1)) & 1u ? __fmaf_rn(av[q].y, bv[q].y, eps) : 0.0f;
        y[4 * q + 2] = (vmask >> (4 * q + 2)) & 1u ? __fmaf_rn(av[q].z, bv[q].z, eps) : 0.0f;
        y[4 * q + 3] = (vmask >> (4 * q + 3)) & 1u ? __fmaf_rn(av[q].w, bv[q].w, eps) : 0.0f;
        S += (y[4 * q + 0] + y[4 * q + 1]) + (y[4 * q + 2] + y[4 * q + 3]);
    }
    for (int o = L >> 1; o; o >>= 1) S += __shfl_xor(S, o);
    if (!live) S = 1.0f;
#pragma unroll
    for (int j = 0; j < 16; j++) y[j] = __fdiv_rn(y[j], S);            // y is r from here on
}
#endif
