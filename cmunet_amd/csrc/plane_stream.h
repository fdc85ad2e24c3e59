// plane_stream.h -- the skeleton of every streaming pass over (B,K,H,W) fp32 planes, 1 <= K <= 8: the segmentation counters (heads.hip),
// the class-index cross entropy (pointwise_loss.hip), the focal and map-weighted losses (map_loss.hip) and the probability histogram
// (prob_hist.hip).  The contract, stated here once:
//   - the class count is compiled in as KT in {2, 4, 8} with classes >= K masked (PLANE_DISPATCH);
//   - a lane takes V = 4 / 4 / 2 consecutive pixels of every plane (16- / 8-byte fp32 accesses) when H*W % V == 0 and every pointer in
//     use is 16-byte aligned, and ONE pixel otherwise (plane_width): the access width is chosen once for the whole tensor, so there is
//     no scalar tail behind a vector body and a vector never straddles a plane;
//   - the grid is capped at CE_MAX_BLOCKS with grid-stride loops (plane_grid); indices are 64-bit, the division that splits a pixel
//     group into (image, offset) is 32-bit below 2^31 groups (plane_group_base);
//   - sums are per-lane fp64 accumulation -> block partials in a caller's fp64 tensor of [columns][CE_MAX_BLOCKS] -> a fixed-order
//     finalisation (plane_final_kernel) that reads the slots of the blocks that were launched, each written by its block in the same
//     call: no floating-point atomics, the same bits on every call;
//   - backward kernels read their upstream gradients from device memory (NULL = zeros): no host synchronisation anywhere.
// What a pass computes per pixel, its softmax formulation included, stays in its own file.
#pragma once
#include "common.h"

template <typename T, int V>
struct alignas(sizeof(T) * V < 16 ? sizeof(T) * V : 16) PlaneVec {
    T v[V];
};
// first pixel of pixel group g in plane 0 of its image; ``small``: fewer than 2^31 groups (a 64-bit division is ~10x the instructions)
__device__ static inline int64_t plane_group_base(int64_t g, int64_t gpi, bool small, int K, int64_t HW, int V) {
    int64_t b, r;
    if (small) {
        const unsigned gu = (unsigned)g, bu = gu / (unsigned)gpi;
        b = bu;
        r = gu - bu * (unsigned)gpi;
    } else {
        b = g / gpi;
        r = g - b * gpi;
    }
    return b * K * HW + r * V;
}
static inline int plane_grid(int64_t ngroups) {
    const int64_t blocks = cmu_div_up64(ngroups, 256);
    return (int)(blocks < CE_MAX_BLOCKS ? blocks : CE_MAX_BLOCKS);
}
// pixels per lane: 4 (2 above four classes, which keeps the KT = 8 kernels clear of scratch) on whole 16- / 8-byte chunks of every plane
// with 16-byte aligned pointers (NULL: not used), else 1
static inline int plane_width(int K, int64_t HW, const void* a, const void* b, const void* c, const void* d) {
    const int V = K > 4 ? 2 : 4;
    return (HW % V == 0 && cmu_aligned16(a) && cmu_aligned16(b) && cmu_aligned16(c) && cmu_aligned16(d)) ? V : 1;
}
// the prologue of an entry point: the launch shape of a pass over B images of K planes that touches the pointers a..d
struct PlaneStream {
    int64_t HW, npix;
    int V, grid;
};
static inline PlaneStream plane_stream(int B, int K, int H, int W, const void* a, const void* b, const void* c, const void* d) {
    PlaneStream s;
    s.HW = (int64_t)H * W;
    s.npix = (int64_t)B * s.HW;
    s.V = plane_width(K, s.HW, a, b, c, d);
    s.grid = plane_grid(s.npix / s.V);
    return s;
}

// one wave per column of partials ([column][CE_MAX_BLOCKS], at most 64 columns), fixed order: lane l takes blocks l, l + 64, ...; then
// the wave's butterfly.  A column outside col_mask gives 0 and reads nothing.  MEAN0: column 0 is divided by div0.
// (A template: a file that includes this and launches none gets none, and the host stubs of those that do cannot collide.)
constexpr unsigned long long PLANE_ALL_COLUMNS = ~0ull;
template <bool MEAN0>
__global__ __launch_bounds__(64) void plane_final_kernel(const double* __restrict__ partials, int nblocks, unsigned long long col_mask,
                                                         double div0, double* __restrict__ out) {
    double s = 0.0;
    if ((col_mask >> blockIdx.x) & 1ull) {
        const double* col = partials + (int64_t)blockIdx.x * CE_MAX_BLOCKS;
        for (int b = threadIdx.x; b < nblocks; b += 64) s += col[b];
        s = wave_sum_d(s);
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (MEAN0 && blockIdx.x == 0) ? s / div0 : s;
}

// the target kinds of the class-index losses (CMU_ICE_*): a label plane (B,H,W) in its own dtype, or K one-hot planes
template <int TK> struct PlaneTarget;
template <> struct PlaneTarget<CMU_ICE_LABEL_I64> { typedef int64_t T; static constexpr bool onehot = false; };
template <> struct PlaneTarget<CMU_ICE_LABEL_I32> { typedef int32_t T; static constexpr bool onehot = false; };
template <> struct PlaneTarget<CMU_ICE_LABEL_U8> { typedef uint8_t T; static constexpr bool onehot = false; };
template <> struct PlaneTarget<CMU_ICE_LABEL_F32> { typedef float T; static constexpr bool onehot = false; };
template <> struct PlaneTarget<CMU_ICE_LABEL_F64> { typedef double T; static constexpr bool onehot = false; };
template <> struct PlaneTarget<CMU_ICE_ONEHOT_F32> { typedef float T; static constexpr bool onehot = true; };
template <> struct PlaneTarget<CMU_ICE_ONEHOT_F64> { typedef double T; static constexpr bool onehot = true; };

// labels of the V pixels of group g: the label plane's values truncated as .long() does, or the arg-max over the one-hot planes of
// keep_mask (the first maximum wins; an all-zero pixel gives the first kept channel, as torch.argmax does).  ``best < 0`` says that no
// kept channel has been seen yet.  ALL_KEPT: the arg-max runs over all K channels and keep_mask is not looked at.  ``best < 0`` then
// holds at channel 0 and nowhere else (K >= 1), so ``c == 0 || y > bv`` picks what ``best < 0 || y > bv`` picks -- also for a NaN in
// plane 0, which stays the maximum in both forms because nothing compares greater than it -- and is what is compiled: neither start
// value is read, and such a pass keeps the code of a decoder without a mask.
template <int KT, int V, int TK, bool ALL_KEPT>
__device__ static inline void plane_labels(const typename PlaneTarget<TK>::T* __restrict__ tgt, int64_t g, int64_t base, int K, int64_t HW,
                                           unsigned keep_mask, int64_t (&lab)[V]) {
    typedef typename PlaneTarget<TK>::T TT;
    if (PlaneTarget<TK>::onehot) {
        int best[V];
        TT bv[V];
        if (!ALL_KEPT) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                best[v] = -1;
                bv[v] = (TT)0;
            }
        }
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K && (ALL_KEPT || ((keep_mask >> c) & 1u))) {
                const PlaneVec<TT, V> yv = *reinterpret_cast<const PlaneVec<TT, V>*>(tgt + base + c * HW);
#pragma unroll
                for (int v = 0; v < V; ++v)
                    if ((ALL_KEPT ? c == 0 : best[v] < 0) || yv.v[v] > bv[v]) {
                        best[v] = c;
                        bv[v] = yv.v[v];
                    }
            }
#pragma unroll
        for (int v = 0; v < V; ++v) lab[v] = best[v];
    } else {
        const PlaneVec<TT, V> tv = *reinterpret_cast<const PlaneVec<TT, V>*>(tgt + g * V);
#pragma unroll
        for (int v = 0; v < V; ++v) lab[v] = (int64_t)tv.v[v];
    }
}

// INNER(KT, V, args...) for the runtime class count and vector width
#define PLANE_DISPATCH(INNER, K, vec, ...)                                                           \
    do {                                                                                             \
        if ((K) <= 2)      { if (vec) INNER(2, 4, __VA_ARGS__); else INNER(2, 1, __VA_ARGS__); }     \
        else if ((K) <= 4) { if (vec) INNER(4, 4, __VA_ARGS__); else INNER(4, 1, __VA_ARGS__); }     \
        else               { if (vec) INNER(8, 2, __VA_ARGS__); else INNER(8, 1, __VA_ARGS__); }     \
    } while (0)
// an INNER of PLANE_DISPATCH: FN<KT, V, TK>(args...) for the runtime target kind
#define PLANE_DISPATCH_TK(KT, V, FN, tk, ...)                                                  \
    do {                                                                                       \
        switch (tk) {                                                                          \
            case CMU_ICE_LABEL_I64: FN<KT, V, CMU_ICE_LABEL_I64>(__VA_ARGS__); break;          \
            case CMU_ICE_LABEL_I32: FN<KT, V, CMU_ICE_LABEL_I32>(__VA_ARGS__); break;          \
            case CMU_ICE_LABEL_U8: FN<KT, V, CMU_ICE_LABEL_U8>(__VA_ARGS__); break;            \
            case CMU_ICE_LABEL_F32: FN<KT, V, CMU_ICE_LABEL_F32>(__VA_ARGS__); break;          \
            case CMU_ICE_LABEL_F64: FN<KT, V, CMU_ICE_LABEL_F64>(__VA_ARGS__); break;          \
            case CMU_ICE_ONEHOT_F32: FN<KT, V, CMU_ICE_ONEHOT_F32>(__VA_ARGS__); break;        \
            default: FN<KT, V, CMU_ICE_ONEHOT_F64>(__VA_ARGS__);                               \
        }                                                                                      \
    } while (0)
