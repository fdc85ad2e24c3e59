// head_math.h -- the per-pixel arithmetic of the 1x1 head's prediction kernels (predict.hip: cmu_head_predict; tiled_predict.hip:
// cmu_head_probs).  head_prob / head_prob_all: the softmax / sigmoid with the maximum subtracted and the accurate expf, one statement
// for both kernels.  head_lane_operands / head_pixel_logits: the logits of cmu_conv1x1_head_fwd (elementwise.hip) in registers -- the
// same 16-byte chunking, the same fmaf order inside a chunk, the same __shfl_xor butterfly over the C/epc lanes of the pixel, then
// + bias -- as head_predict_kernel states them inline (that kernel keeps its own text: behind these functions hipcc allocates its
// registers differently, and its measured timings are on record; tests/test_gpu_tiled_predict.py and tests/test_gpu_predict.py hold
// all three statements to the logits kernel's bits).
#pragma once
#include "common.h"

constexpr int PRED_MAX_K = 8;

// the head's operands of lane ``ch`` (its 16-byte chunk of the C channels): BatchNorm scale / shift, the K weight rows, the biases
template <class TR, int KT>
__device__ static inline void head_lane_operands(const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ w,
                                                 const float* __restrict__ bias, int C, int K, int ch, float* sc, float* sh,
                                                 float (*wk)[TR::EPC], float* bk) {
    constexpr int EPC = TR::EPC;
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        sc[e] = scale ? scale[ch * EPC + e] : 1.f;
        sh[e] = scale ? shift[ch * EPC + e] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        bk[k] = (k < K) ? bias[k] : 0.f;
#pragma unroll
        for (int e = 0; e < EPC; ++e) wk[k][e] = (k < K) ? w[k * C + ch * EPC + e] : 0.f;
    }
}

// the K logits of one pixel from this lane's chunk ``q``: after the butterfly every lane of the pixel's group holds the same sums
template <class TR, int KT>
__device__ static inline void head_pixel_logits(const u32x4& q, const float* sc, const float* sh, const float (*wk)[TR::EPC], const float* bk,
                                                float lo, int nchunk, int K, float* l) {
    constexpr int EPC = TR::EPC;
    float f[EPC];
    TR::unpack(q, f);
    float acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = 0.f;
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const float a = fmaxf(fmaf(f[e], sc[e], sh[e]), lo);
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[k] = fmaf(a, wk[k][e], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < K)
            for (int o = 1; o < nchunk; o <<= 1) acc[k] += __shfl_xor(acc[k], o, 64);
#pragma unroll
    for (int k = 0; k < KT; ++k) l[k] = acc[k] + bk[k];
}

// softmax probability of class pc (K >= 2; m = the maximum logit) or the sigmoid (K == 1), fp32 with the accurate expf
template <int KT>
__device__ static inline float head_prob(const float* l, float m, int K, int pc) {
    if (K == 1) {      // without overflow for either sign: the exponential's argument is never positive
        const float e = expf(-fabsf(l[0]));
        return (l[0] >= 0.f ? 1.f : e) / (1.f + e);
    }
    float s = 0.f, num = 0.f;
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < K) {
            const float e = expf(l[k] - m);
            s += e;
            num = (k == pc) ? e : num;
        }
    return num / s;
}

// every class's probability at once: p[k] is the value head_prob returns for pc = k (the same exponentials, the same sum in the same
// order, the same division); K == 1: p[0] = the sigmoid
template <int KT>
__device__ static inline void head_prob_all(const float* l, float m, int K, float* p) {
    if (K == 1) {
        p[0] = head_prob<KT>(l, m, 1, 0);
        return;
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        p[k] = (k < K) ? expf(l[k] - m) : 0.f;
        s += p[k];      // (+ 0 past K: the sum of the K positive terms is unchanged)
    }
#pragma unroll
    for (int k = 0; k < KT; ++k) p[k] = p[k] / s;
}
