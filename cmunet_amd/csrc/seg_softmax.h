// seg_softmax.h -- the per-pixel fp32 softmax of the K-class segmentation statistics (heads.hip: cmu_seg_stats_fwd / _bwd) in one statement
// for every kernel that must see the same probability bits: the counters thresholded at t (heads.hip) and the probability histogram whose
// suffix sums are those counters at every t = j / NB at once (prob_hist.hip).
#pragma once
#include "common.h"

// softmax of one pixel in fp32: p[c] = e^(l[c] - max) / sum, lse = max + log(sum); classes >= K are left alone
template <int KT>
__device__ static inline void seg_softmax(const float (&l)[KT], int K, float (&p)[KT], float& lse) {
    float m = l[0];
#pragma unroll
    for (int c = 1; c < KT; ++c)
        if (c < K) m = fmaxf(m, l[c]);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c)
        if (c < K) {
            // e^(l - m) with the rounding d of the fp32 difference given back (e^(x + d) = e^x (1 + d)): a class far below the
            // maximum would otherwise carry |l - m| roundoffs in its probability, and through sum_c p_c G_c into every gradient
            const float x = l[c] - m;
            const float d = (float)(((double)l[c] - (double)m) - (double)x);
            const float e = expf(x);
            p[c] = fmaf(e, d, e);
            se += p[c];
        }
    lse = m + logf(se);
#pragma unroll
    for (int c = 0; c < KT; ++c)
        if (c < K) p[c] = p[c] / se;
}
