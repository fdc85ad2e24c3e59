// lovasz.hip -- the Lovasz-Softmax loss (Berman et al., 2018) on (B,K,H,W) fp32 logits, 2 <= K <= 8 (no
// reference counterpart).  Per kept class c and per segment (the whole batch, or one image) the errors e_i = 1 - p_c(i) on the class's
// pixels and p_c(i) elsewhere are sorted in descending order and weighted by the gradient of the Jaccard index along that order.
//   cmu_lovasz_keys   one streaming pass under the contract of plane_stream.h builds a 64-bit sort key per (kept class, pixel) and
//                     counts the valid and the foreground pixels of every segment (integer atomics: exact in any order);
//   cmu_sort_u64      (key_sort.hip) sorts every (segment, class) row;
//   cmu_lovasz_grad   scans the foreground bit along the sorted rows, forms the Jaccard gradient g in fp64, scatters -+ coef g into a
//                     weight map for cmu_softmax_map_bwd (kind 0) and sums e g: per-lane fp64 -> block partials -> a fixed-order
//                     finalisation.  No floating-point atomics, no host synchronisation, the same bits on every call.
// p is seg_softmax<>() (seg_softmax.h: the probability bits of the counters); 1 - p is one fp32 subtraction.
#include "common.h"
#include "plane_stream.h"
#include "seg_softmax.h"
#include "key_sort.h"

constexpr int LZ_MAX_K = 8;
constexpr int LZ_THREADS = CMU_KS_THREADS;             // the passes over sorted rows: one tile of the sort per workgroup,
constexpr int LZ_PER_LANE = CMU_KS_PER_LANE;           // LZ_PER_LANE consecutive ranks per lane
constexpr int LZ_WAVES = LZ_THREADS / 64;
// The key, from the top: bit 63 "not valid" (an ignored pixel, or a label outside [0, K): behind every valid key), bits 62..32 the low
// 31 bits of the fp32 error inverted (ascending keys = descending errors; an error is never negative, so its sign bit says nothing),
// bits 31..1 the pixel's index in its segment (fewer than 2^31 pixels per segment), bit 0 the foreground bit -- below the index, so it
// cannot influence the order: keys of a row differ in their index fields.
constexpr uint64_t LZ_NOT_VALID = 1ull << 63;
__device__ static inline uint64_t lz_key(bool valid, float e, uint32_t idx, bool fg) {
    const uint64_t low = ((uint64_t)idx << 1) | (uint64_t)fg;
    if (!valid) return LZ_NOT_VALID | (0x7fffffffull << 32) | ((uint64_t)idx << 1);
    return ((uint64_t)(~__float_as_uint(e) & 0x7fffffffu) << 32) | low;
}
__device__ static inline float lz_key_error(uint64_t k) { return __uint_as_float(~(uint32_t)(k >> 32) & 0x7fffffffu); }
__device__ static inline uint32_t lz_key_index(uint64_t k) { return (uint32_t)(k >> 1) & 0x7fffffffu; }

__device__ static inline int lz_wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// block sum of an int64 over `red` (one slot per wave), the result in every thread; integers: exact in any order
__device__ static inline int64_t lz_block_sum_i64(int64_t v, int64_t* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int64_t a = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) a += red[i];
    return a;
}
// exclusive scan of one int per lane over the block, in lane order
__device__ static inline int lz_block_excl_scan(int v, int* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int off = 0;
    for (int i = 0; i < w; ++i) off += wsum[i];
    return off + inc - v;
}
// the c of the ci-th kept class
__device__ static inline int lz_kept_class(unsigned keep_mask, int ci) {
    int c = 0;
    for (unsigned m = keep_mask; m; m >>= 1, ++c)
        if (m & 1u) {
            if (ci == 0) return c;
            --ci;
        }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// keys and counts.  grid (blocks per image, B): a block stays inside one image, so its counts belong to one segment and leave it as
// K + 2 integer atomics.  counts (int64): [s][0] valid pixels, [s][1 + c] pixels of label c, c < K; [S (K + 1)] labels outside [0, K)
// that are not ignore_index, over the whole batch.
// ---------------------------------------------------------------------------------------------
template <int KT, int V, int TK>
__global__ __launch_bounds__(256) void lz_keys_kernel(const float* __restrict__ x, const typename PlaneTarget<TK>::T* __restrict__ tgt,
                                                     uint64_t* __restrict__ keys, unsigned long long* __restrict__ counts, int B, int K,
                                                     int64_t HW, unsigned keep_mask, int per_image, int64_t ignore_index) {
    __shared__ int cnt[KT + 2];
    const int b = blockIdx.y;
    const int64_t gpi = HW / V, n = per_image ? HW : (int64_t)B * HW;
    const int Kk = __popc(keep_mask), S = per_image ? B : 1;
    const int64_t seg = per_image ? b : 0;
    const uint32_t idx0 = per_image ? 0u : (uint32_t)((int64_t)b * HW);
    uint64_t* krow = keys + seg * Kk * n + idx0;             // row ci of the segment, at this image's first pixel: krow + ci * n
    if (threadIdx.x < KT + 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    int nvalid = 0, nbad = 0, nfg[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) nfg[c] = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < gpi; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = b * gpi + r, base = (int64_t)b * K * HW + r * V;
        PlaneVec<float, V> xv[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) xv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(x + base + c * HW);
        int64_t lab[V];
        plane_labels<KT, V, TK, true>(tgt, g, base, K, HW, 0u, lab);
        PlaneVec<uint64_t, V> kv[KT];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int64_t t = lab[v];
            const bool ignored = !PlaneTarget<TK>::onehot && t == ignore_index;
            const bool ok = !ignored && t >= 0 && t < K;
            nvalid += ok;
            nbad += !ignored && !ok;
            float l[KT], p[KT], lse;
#pragma unroll
            for (int c = 0; c < KT; ++c) l[c] = c < K ? xv[c].v[v] : 0.f;
            seg_softmax<KT>(l, K, p, lse);
            const uint32_t idx = idx0 + (uint32_t)(r * V + v);
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < K) {
                    const bool fg = ok && t == c;
                    nfg[c] += fg;
                    kv[c].v[v] = lz_key(ok, fg ? 1.f - p[c] : p[c], idx, fg);
                }
        }
        int ci = 0;
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K && ((keep_mask >> c) & 1u)) {
                *reinterpret_cast<PlaneVec<uint64_t, V>*>(krow + ci * n + r * V) = kv[c];
                ++ci;
            }
    }
    nvalid = lz_wave_sum_i(nvalid);
    nbad = lz_wave_sum_i(nbad);
#pragma unroll
    for (int c = 0; c < KT; ++c) nfg[c] = lz_wave_sum_i(nfg[c]);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&cnt[0], nvalid);
        atomicAdd(&cnt[KT + 1], nbad);
#pragma unroll
        for (int c = 0; c < KT; ++c) atomicAdd(&cnt[1 + c], nfg[c]);
    }
    __syncthreads();
    if ((int)threadIdx.x <= K) atomicAdd(&counts[seg * (K + 1) + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    if (threadIdx.x == KT + 1) atomicAdd(&counts[(int64_t)S * (K + 1)], (unsigned long long)cnt[KT + 1]);
}
template <int KT, int V, int TK>
static void lz_keys_launch(const float* x, const void* tgt, uint64_t* keys, int64_t* counts, int B, int K, int64_t HW, unsigned keep_mask,
                           int per_image, int64_t ignore_index, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL((lz_keys_kernel<KT, V, TK>), grid, dim3(256), 0, st, x, (const typename PlaneTarget<TK>::T*)tgt, keys,
                       (unsigned long long*)counts, B, K, HW, keep_mask, per_image, ignore_index);
}

static int lz_check(const char* who, int keep_mask, int B, int K, int H, int W, int per_image, int64_t& n, int& S) {
    CMU_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0, "%s: bad args (1 <= B <= 65535)", who);
    CMU_CHECK_ARG(K >= 2 && K <= LZ_MAX_K, "%s: 2 <= K <= %d classes (got %d)", who, LZ_MAX_K, K);
    CMU_CHECK_ARG(keep_mask > 0 && keep_mask < (1 << K), "%s: keep_mask 0x%x names no channel, or one past K = %d", who, keep_mask, K);
    const int64_t HW = (int64_t)H * W;
    S = per_image ? B : 1;
    n = per_image ? HW : (int64_t)B * HW;
    CMU_CHECK_ARG(n < (int64_t(1) << 31), "%s: a segment holds fewer than 2^31 pixels (got %lld)", who, (long long)n);
    CMU_CHECK_ARG((int64_t)S * __builtin_popcount((unsigned)keep_mask) * cmu_ks_tiles(n) < (int64_t(1) << 31), "%s: too many tiles", who);
    return CMU_OK;
}

extern "C" int cmu_lovasz_keys(const float* x, const void* target, int target_kind, int keep_mask, int per_image, int64_t ignore_index,
                               uint64_t* keys, int64_t* counts, int B, int K, int H, int W, void* stream) {
    int64_t n;
    int S;
    if (int rc = lz_check("cmu_lovasz_keys", keep_mask, B, K, H, W, per_image, n, S)) return rc;
    CMU_CHECK_ARG(x && target && keys && counts, "cmu_lovasz_keys: bad args");
    CMU_CHECK_ARG(target_kind >= CMU_ICE_LABEL_I64 && target_kind <= CMU_ICE_ONEHOT_F64, "cmu_lovasz_keys: unknown target kind %d", target_kind);
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    const int V = plane_width(K, HW, x, target, keys, nullptr);
    hipError_t e = hipMemsetAsync(counts, 0, ((size_t)S * (K + 1) + 1) * sizeof(int64_t), st);
    CMU_CHECK_ARG(e == hipSuccess, "cmu_lovasz_keys: clearing the counts: %s", hipGetErrorString(e));
    const int64_t per_img = cmu_div_up64(HW / V, 256), cap = 4096 / B > 0 ? 4096 / B : 1;
    const dim3 grid((unsigned)(per_img < cap ? per_img : cap), (unsigned)B);
    PLANE_DISPATCH(PLANE_DISPATCH_TK, K, V > 1, lz_keys_launch, target_kind, x, target, keys, counts, B, K, HW, (unsigned)keep_mask,
                   per_image != 0, ignore_index, grid, st);
    CMU_CHECK_LAUNCH("cmu_lovasz_keys");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// The Jaccard gradient along a sorted row.  With G the row's foreground count, r the 1-based rank and F_r the foreground count among
// the first r keys, J_r = 1 - (G - F_r) / U_r with the union U_r = G + r - F_r, and g_r = J_r - J_(r-1) (g_1 = J_1).  A foreground key
// leaves the union as it is and takes one from the numerator; a background key leaves the numerator N = G - F_r and adds one to the
// union.  The difference is therefore formed WITHOUT its cancellation (J_r - J_(r-1) loses log2(n) bits far down a row):
//   foreground  g_r = 1 / U_r            background  g_r = N / ((U_r - 1) U_r),  and 1 where U_r = 1 (r = 1 in a row with G = 0)
// -- integers, one fp64 quotient.  g_r >= 0, sum_r g_r <= 1; a row with G = 0 has g = (1, 0, 0, ...).
// ---------------------------------------------------------------------------------------------
__device__ static inline double lz_jaccard_grad(int64_t G, int64_t r, int64_t F, bool fg) {
    const int64_t U = G + r - F;
    if (fg) return 1.0 / (double)U;
    return U == 1 ? 1.0 : (double)(G - F) / ((double)(U - 1) * (double)U);
}
// foreground keys per tile of the sorted rows (a key that is not valid carries no foreground bit)
__global__ __launch_bounds__(LZ_THREADS) void lz_tile_fg_kernel(const uint64_t* __restrict__ keys, int64_t* __restrict__ tile_fg, int64_t n,
                                                               int64_t tiles) {
    __shared__ int64_t red[LZ_WAVES];
    const int64_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const int cnt = cmu_ks_tile_count(n, tile);
    const uint64_t* k = keys + row * n + tile * CMU_KS_TILE;
    int64_t f = 0;
    for (int i = threadIdx.x; i < cnt; i += LZ_THREADS) f += (int64_t)(k[i] & 1ull);
    f = lz_block_sum_i64(f, red);
    if (threadIdx.x == 0) tile_fg[blockIdx.x] = f;
}
// The averaging factor of segment s: 1 / (S x the classes that count in it) -- the kept classes with G > 0, or with classes_all all
// kept classes --, 0 when none counts or a label was out of range.
__device__ static inline double lz_coef(const int64_t* __restrict__ counts, int s, int S, int K, unsigned keep_mask, int classes_all) {
    int counted = 0;
    for (int c = 0; c < K; ++c)
        if (((keep_mask >> c) & 1u) && (classes_all || counts[(int64_t)s * (K + 1) + 1 + c] > 0)) ++counted;
    const bool bad = counts[(int64_t)S * (K + 1)] != 0;
    return (counted > 0 && !bad) ? 1.0 / ((double)S * (double)counted) : 0.0;
}
__global__ __launch_bounds__(LZ_THREADS) void lz_grad_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ counts,
                                                            const int64_t* __restrict__ tile_fg, float* __restrict__ wmap,
                                                            double* __restrict__ partials, int S, int K, int64_t HW, int64_t n, int64_t tiles,
                                                            unsigned keep_mask, int per_image, int classes_all) {
    __shared__ int64_t red_i[LZ_WAVES];
    __shared__ double red_d[LZ_WAVES];
    __shared__ int wsum[LZ_WAVES];
    const int Kk = __popc(keep_mask);
    const int64_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const int s = (int)(row / Kk), c = lz_kept_class(keep_mask, (int)(row - (int64_t)s * Kk));
    const int64_t G = counts[(int64_t)s * (K + 1) + 1 + c];
    const bool counted = classes_all || G > 0;
    const double coef = lz_coef(counts, s, S, K, keep_mask, classes_all);
    // foreground keys of the row in front of this tile: integers, any order
    int64_t f0 = 0;
    for (int64_t i = threadIdx.x; i < tile; i += LZ_THREADS) f0 += tile_fg[row * tiles + i];
    f0 = lz_block_sum_i64(f0, red_i);
    const int64_t pos0 = tile * CMU_KS_TILE + (int64_t)threadIdx.x * LZ_PER_LANE;
    uint64_t k[LZ_PER_LANE];
    int nloc = 0;
#pragma unroll
    for (int i = 0; i < LZ_PER_LANE; ++i) {
        k[i] = pos0 + i < n ? keys[row * n + pos0 + i] : LZ_NOT_VALID;
        nloc += (int)(k[i] & 1ull);
    }
    int64_t F = f0 + lz_block_excl_scan(nloc, wsum);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < LZ_PER_LANE; ++i) {
        if (pos0 + i >= n) continue;
        const bool fg = (k[i] & 1ull) != 0;
        F += fg;
        float w = 0.f;
        if (!(k[i] >> 63) && counted) {
            const double g = lz_jaccard_grad(G, pos0 + i + 1, F, fg);
            acc += (double)lz_key_error(k[i]) * g;
            w = (float)(fg ? -(coef * g) : coef * g);
        }
        const uint32_t idx = lz_key_index(k[i]);
        if (idx >= n) continue;          // (not a key of cmu_lovasz_keys: never an address)
        const uint32_t b = per_image ? (uint32_t)s : idx / (uint32_t)HW, hw = per_image ? idx : idx - b * (uint32_t)HW;
        wmap[((int64_t)b * K + c) * HW + hw] = w;
    }
    acc = block_sum_d(acc, red_d);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}
// out: [0] the loss = sum_s coef_s L_s (NaN when a label was out of range); [1 + s] L_s = the sum of the losses of the classes that
// count in segment s; [1 + S + s] coef_s; [1 + 2 S + s K + c] the loss of class c in segment s (0 for a class that does not count).
// Fixed order: a wave adds a row's tile partials lane-strided and folds the lanes; classes and segments are added in index order.
__global__ __launch_bounds__(256) void lz_final_kernel(const double* __restrict__ partials, const int64_t* __restrict__ counts, double* out,
                                                      int S, int K, int64_t tiles, unsigned keep_mask, int classes_all) {
    const int Kk = __popc(keep_mask), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* Lsc = out + 1 + 2 * (int64_t)S;
    for (int64_t sc = wave; sc < (int64_t)S * K; sc += 4) {
        const int64_t s = sc / K;
        const int c = (int)(sc - s * K);
        double v = 0.0;
        if (((keep_mask >> c) & 1u) && (classes_all || counts[s * (K + 1) + 1 + c] > 0)) {
            const double* p = partials + (s * Kk + __popc(keep_mask & ((1u << c) - 1u))) * tiles;
            for (int64_t i = lane; i < tiles; i += 64) v += p[i];
            v = wave_sum_d(v);
        }
        if (lane == 0) Lsc[sc] = v;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += 256) {
        double L = 0.0;
        for (int c = 0; c < K; ++c) L += Lsc[(int64_t)s * K + c];
        out[1 + s] = L;
        out[1 + S + s] = lz_coef(counts, s, S, K, keep_mask, classes_all);
    }
    __syncthreads();
    if (wave == 0) {
        double v = 0.0;
        for (int s = lane; s < S; s += 64) v += out[1 + S + s] * out[1 + s];
        v = wave_sum_d(v);
        if (lane == 0) out[0] = counts[(int64_t)S * (K + 1)] != 0 ? __builtin_nan("") : v;
    }
}

extern "C" int cmu_lovasz_grad(const uint64_t* sorted_keys, const int64_t* counts, int keep_mask, int per_image, int classes_all, float* wmap,
                               int64_t* tile_fg, double* partials, double* out, int B, int K, int H, int W, void* stream) {
    int64_t n;
    int S;
    if (int rc = lz_check("cmu_lovasz_grad", keep_mask, B, K, H, W, per_image, n, S)) return rc;
    CMU_CHECK_ARG(sorted_keys && counts && wmap && tile_fg && partials && out, "cmu_lovasz_grad: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, tiles = cmu_ks_tiles(n);
    const int Kk = __builtin_popcount((unsigned)keep_mask);
    if (Kk < K) {       // the planes of the classes that are not kept: the scatter below writes the kept ones, every pixel of them
        hipError_t e = hipMemsetAsync(wmap, 0, (size_t)B * K * HW * sizeof(float), st);
        CMU_CHECK_ARG(e == hipSuccess, "cmu_lovasz_grad: clearing the weight map: %s", hipGetErrorString(e));
    }
    const dim3 grid((unsigned)((int64_t)S * Kk * tiles)), block(LZ_THREADS);
    hipLaunchKernelGGL(lz_tile_fg_kernel, grid, block, 0, st, sorted_keys, tile_fg, n, tiles);
    CMU_CHECK_LAUNCH("cmu_lovasz_grad(tile counts)");
    hipLaunchKernelGGL(lz_grad_kernel, grid, block, 0, st, sorted_keys, counts, (const int64_t*)tile_fg, wmap, partials, S, K, HW, n, tiles,
                       (unsigned)keep_mask, per_image != 0, classes_all != 0);
    CMU_CHECK_LAUNCH("cmu_lovasz_grad");
    hipLaunchKernelGGL(lz_final_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, counts, out, S, K, tiles, (unsigned)keep_mask,
                       classes_all != 0);
    CMU_CHECK_LAUNCH("cmu_lovasz_grad(final)");
    return CMU_OK;
}
