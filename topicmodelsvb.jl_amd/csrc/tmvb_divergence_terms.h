// tmvb_divergence_terms.h -- the addend and the clamp of the divergences of include/tmvb.h (TMVB_TD_JS, TMVB_TD_HELLINGER, TMVB_TD_TV, TMVB_TD_KL), the ONE
// place where they are written down: the pair kernel of tmvb_topic_divergence (tmvb_topic_compare.hip) and the row kernel of tmvb_group_topics
// (tmvb_group_topics.hip) both call them.
//
// fp contraction is OFF from here to the end of the including unit: a fused multiply-add in 0.5 * (x + y) or acc += term would break the stated
// arithmetic (and the transpose symmetry of the pair kernel).  Both units keep it off anyway; include this header in front of every kernel.
#pragma once

#include "tmvb.h"

#pragma clang fp contract(off)

#if defined(__HIPCC__)
// p, q: the prepared values (HELLINGER: roots; KL: smoothed)
template <int METRIC>
__device__ __forceinline__ double td_term(double p, double q)
{
    if (METRIC == TMVB_TD_JS) {
        const double s = p + q;
        const double x = p > 0.0 ? p * log((2.0 * p) / s) : 0.0;
        const double y = q > 0.0 ? q * log((2.0 * q) / s) : 0.0;
        return 0.5 * (x + y);
    }
    if (METRIC == TMVB_TD_HELLINGER) {
        const double d = p - q;
        return 0.5 * (d * d);
    }
    if (METRIC == TMVB_TD_TV) return 0.5 * fabs(p - q);
    return p > 0.0 ? p * log(p / q) : 0.0;                           // KL: q = 0 < p gives p * log(inf) = +inf
}

template <int METRIC>
__device__ __forceinline__ double td_finish(double s)
{
    return (METRIC == TMVB_TD_JS || METRIC == TMVB_TD_KL) ? (s > 0.0 ? s : 0.0) : s;      // max(0, s); HELLINGER's root is the host's
}
#endif
