// predict.hip -- the prediction head: 1x1 head + argmax / threshold (+ one class's probability) in one pass over the last activation.
//
// cmu_head_predict computes, per pixel, the K logits of cmu_conv1x1_head_fwd (elementwise.hip) IN REGISTERS -- the same 16-byte chunking,
// the same fmaf order inside a chunk, the same __shfl_xor butterfly over the C/epc lanes of the pixel, then + bias: bit for bit the
// numbers that kernel writes -- and stores only what a segmentation needs: one uint8 label (and optionally one fp32 probability).  The
// fp32 NCHW logits (4 K bytes per pixel), torch.argmax's int64 map (8 bytes) and the cast never reach memory.
//
// Memory shape: HBM-bound like the head it restates.  One lane per 16-byte chunk, four loads in flight per lane, grid-stride under a
// block cap.  Unlike the logits kernel (pixel u * ppb + g: consecutive pixels in consecutive lane groups, one fp32 per class plane),
// a lane group here owns FOUR CONSECUTIVE pixels (4 g + u), so its first lane packs the four labels into one 32-bit store; a load
// instruction still touches whole 16 * C/epc-byte runs (one or two full 128-byte lines at the product's C = 64).
// The probability: after the butterfly every lane of the group holds the logits of all four pixels, so lane u (< 4) keeps pixel u's and
// computes ONE softmax / sigmoid per trip -- the accurate expf and the division run once per lane, not four times in every lane -- and
// the group's first four lanes store four consecutive floats.  (Groups of one or two lanes, C = epc or 2 epc, compute per pixel.)
#include "head_math.h"      // PRED_MAX_K and head_prob: shared with cmu_head_probs (tiled_predict.hip)

#ifndef CMU_HEADP_CAP
#define CMU_HEADP_CAP 8192
#endif

template <class TR, int KT, bool PROB>   // KT = compiled class count (2 for the reference's heads and one-channel heads, PRED_MAX_K otherwise)
// (256 lanes; at least four waves per SIMD without the probability, three with it: the eight-class 16-bit form then takes 141 registers
// instead of spilling at 128)
__global__ void __launch_bounds__(256, PROB ? 3 : 4)
head_predict_kernel(const unsigned char* __restrict__ x, int64_t ldx, const float* __restrict__ scale, const float* __restrict__ shift,
                    const float* __restrict__ w, const float* __restrict__ bias, float thr, const uint8_t* __restrict__ lut,
                    uint8_t* __restrict__ labels, float* __restrict__ prob, int pc, int C, int K, int64_t npix) {
    constexpr int EPC = TR::EPC;
    constexpr int ES = (int)sizeof(typename TR::elem_t);
    constexpr int U = 4;         // consecutive pixels per lane group and trip: four 16-byte loads in flight, one packed label store
    const int nchunk = C / EPC;  // power of two <= 64 (checked on the host)
    const int ch = threadIdx.x % nchunk;
    const int g = threadIdx.x / nchunk;
    const int ppb = blockDim.x / nchunk;
    float sc[EPC], sh[EPC], wk[KT][EPC], bk[KT];
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
    // the byte written for label j (the index itself without a table); one-channel heads have the two labels 0 / 1
    uint32_t val[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) val[k] = (lut != nullptr && k < (K > 2 ? K : 2)) ? (uint32_t)lut[k] : (uint32_t)k;
    const float lo = scale ? 0.f : -__builtin_inff();
    for (int64_t p0 = (int64_t)blockIdx.x * ppb * U; p0 < npix; p0 += (int64_t)gridDim.x * ppb * U) {
        const int64_t pbase = p0 + (int64_t)g * U;      // a multiple of four
        u32x4 q[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            q[u] = (pbase + u < npix) ? ld_global16(x + ((pbase + u) * ldx + ch * EPC) * ES) : u32x4{0u, 0u, 0u, 0u};
        uint32_t packed = 0u;
        float kl[KT], km = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) kl[k] = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float f[EPC];
            TR::unpack(q[u], f);
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
            // every lane of the group now holds the same K sums; the logits
            float l[KT];
#pragma unroll
            for (int k = 0; k < KT; ++k) l[k] = acc[k] + bk[k];
            uint32_t v;
            float m = l[0];
            if (K == 1) {
                v = (l[0] > thr) ? val[1] : val[0];
            } else {
                v = val[0];
#pragma unroll
                for (int k = 1; k < KT; ++k)
                    if (k < K && l[k] > m) {      // strict: the smallest index among equal maxima
                        m = l[k];
                        v = val[k];
                    }
            }
            packed |= v << (8 * u);
            if (PROB) {
                if (nchunk >= U) {      // lane u of the group keeps pixel u
#pragma unroll
                    for (int k = 0; k < KT; ++k) kl[k] = (ch == u) ? l[k] : kl[k];
                    km = (ch == u) ? m : km;
                } else if (ch == 0 && pbase + u < npix) {
                    prob[pbase + u] = head_prob<KT>(l, m, K, pc);
                }
            }
        }
        if (PROB && nchunk >= U) {
            const float p = head_prob<KT>(kl, km, K, pc);
            if (ch < U && pbase + ch < npix) prob[pbase + ch] = p;
        }
        if (ch == 0 && pbase < npix) {
            if (pbase + U <= npix) {
                *reinterpret_cast<uint32_t*>(labels + pbase) = packed;      // labels is 4-byte aligned (host check), pbase % 4 == 0
            } else {      // the last, partial group of the tensor
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (pbase + u < npix) labels[pbase + u] = (uint8_t)(packed >> (8 * u));
            }
        }
    }
}

template <class TR, int KT>
static void head_predict_launch(int grid, hipStream_t st, const void* x, int64_t ldx, const float* scale, const float* shift, const float* w,
                                const float* bias, float thr, const uint8_t* lut, uint8_t* labels, float* prob, int pc, int C, int K,
                                int64_t npix) {
    if (prob != nullptr)
        hipLaunchKernelGGL((head_predict_kernel<TR, KT, true>), dim3(grid), dim3(256), 0, st, (const unsigned char*)x, ldx, scale, shift, w,
                           bias, thr, lut, labels, prob, pc, C, K, npix);
    else
        hipLaunchKernelGGL((head_predict_kernel<TR, KT, false>), dim3(grid), dim3(256), 0, st, (const unsigned char*)x, ldx, scale, shift, w,
                           bias, thr, lut, labels, prob, pc, C, K, npix);
}

template <class TR>
static int head_predict_t(const void* x, int64_t ldx, const float* scale, const float* shift, const float* w, const float* bias, float thr,
                          const uint8_t* lut, uint8_t* labels, float* prob, int pc, int B, int H, int W, int C, int K, hipStream_t st) {
    const int nchunk = C / TR::EPC;
    const int64_t npix = (int64_t)B * H * W;
    const int ppb = 256 / nchunk;
    const int64_t nb = cmu_div_up64(npix, ppb * 4);
    const int grid = (int)(nb < CMU_HEADP_CAP ? nb : CMU_HEADP_CAP);
    if (K <= 2)
        head_predict_launch<TR, 2>(grid, st, x, ldx, scale, shift, w, bias, thr, lut, labels, prob, pc, C, K, npix);
    else
        head_predict_launch<TR, PRED_MAX_K>(grid, st, x, ldx, scale, shift, w, bias, thr, lut, labels, prob, pc, C, K, npix);
    CMU_CHECK_LAUNCH("cmu_head_predict");
    return CMU_OK;
}

static bool pred_is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

extern "C" int cmu_head_predict(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, const float* w, const float* bias,
                                float logit_threshold, const uint8_t* lut, uint8_t* labels, float* prob, int prob_class, int B, int H, int W,
                                int C, int K, int dt, void* stream) {
    const int es = cmu_dtype_size(dt);
    CMU_CHECK_ARG(es > 0 && x && w && bias && labels && B > 0 && H > 0 && W > 0, "cmu_head_predict: bad args");
    const int epc = 16 / es;
    CMU_CHECK_ARG(K >= 1 && K <= PRED_MAX_K, "cmu_head_predict: K=%d must be in 1..%d", K, PRED_MAX_K);
    CMU_CHECK_ARG(C % epc == 0 && pred_is_pow2(C / epc) && C / epc <= 64, "cmu_head_predict: C=%d: C/%d must be a power of two <= 64", C, epc);
    CMU_CHECK_ARG(cmu_aligned16(x) && ldx % epc == 0 && ldx >= C, "cmu_head_predict: x alignment / stride");
    CMU_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "cmu_head_predict: scale/shift must both be set");
    CMU_CHECK_ARG((reinterpret_cast<uintptr_t>(labels) & 3) == 0, "cmu_head_predict: labels must be 4-byte aligned (packed stores)");
    if (prob != nullptr) {
        CMU_CHECK_ARG((reinterpret_cast<uintptr_t>(prob) & 3) == 0, "cmu_head_predict: prob must be 4-byte aligned");
        CMU_CHECK_ARG(prob_class >= 0 && prob_class < (K > 1 ? K : 1), "cmu_head_predict: prob_class=%d outside 0..%d", prob_class, (K > 1 ? K : 1) - 1);
    }
    CMU_DISPATCH_DT(dt, head_predict_t, x, ldx, in_scale, in_shift, w, bias, logit_threshold, lut, labels, prob, prob_class, B, H, W, C, K,
                    (hipStream_t)stream);
}
