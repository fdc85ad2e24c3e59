// preprocess.hip -- the reference's image preprocessing (data_processing/pre_processing.py) on the device: per-image statistics,
// Intensity / MinMax / row-L2 normalisation, skimage's unsharp mask (scipy's separable Gaussian, 'reflect' borders), centre crop and
// mask integration.  DESIGN.md section 4.22.  Planes are contiguous (B,H,W), uint8 or float32; outputs are float32 (masks uint8).
// Everything is deterministic: each sum has one fixed order, nothing is accumulated with atomics.
//
// Built with hipcc's default contraction: no result here is pinned to an unfused multiply-add.  The bit-exact outputs (the uint8 mean,
// min / max, the min-max quotient) are single IEEE operations; the others are checked against float64 with bounds that hold for a
// fused and an unfused a * b + c alike.
#include "common.h"
#include <math.h>

namespace {

constexpr int PRE_THREADS = 256;
constexpr int PRE_MAX_BLOCKS = 1024;      // per image; the element-wise passes stride over the rest
constexpr int STAT_THREADS = 1024;

template <bool U8>
__device__ inline float pre_ld(const void* __restrict__ x, int64_t i) {
    if (U8) return (float)reinterpret_cast<const uint8_t*>(x)[i];
    return reinterpret_cast<const float*>(x)[i];
}

// index i of an axis of n samples under scipy's 'reflect' (half-sample symmetric: d c b a | a b c d), any distance from the axis
__device__ inline int pre_reflect(int i, int n) {
    if (i >= 0 && i < n) return i;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

__device__ inline double block_min_d(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double a = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) a = fmin(a, red[i]);
    return a;
}
__device__ inline double block_max_d(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double a = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) a = fmax(a, red[i]);
    return a;
}

// grid (B): thread t takes pixels t, t + 1024, ...; its sum, then the waves' sums in wave order (block_sum_d).  Two passes, as np.std:
// the mean first, then sum((x - mean)^2).  A uint8 image's sum is carried as an integer (every partial sum below 2^53 is exact in the
// float64 reduction too), so its mean is the exact sum rounded once by the division.
template <bool U8>
__global__ __launch_bounds__(STAT_THREADS) void pre_stats_kernel(const void* __restrict__ x, double* __restrict__ stats, int HW) {
    __shared__ double red[STAT_THREADS / 64];
    const int b = blockIdx.x;
    const int64_t base = (int64_t)b * HW;
    double s = 0.0, mn = INFINITY, mx = -INFINITY;
    unsigned long long si = 0;
    for (int64_t i = threadIdx.x; i < HW; i += STAT_THREADS) {
        if (U8) {
            const unsigned v = reinterpret_cast<const uint8_t*>(x)[base + i];
            si += v;
            mn = fmin(mn, (double)v);
            mx = fmax(mx, (double)v);
        } else {
            const double v = (double)reinterpret_cast<const float*>(x)[base + i];
            s += v;
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
    }
    if (U8) s = (double)si;
    const double mean = block_sum_d(s, red) / (double)HW;
    mn = block_min_d(mn, red);
    mx = block_max_d(mx, red);
    double q = 0.0;
    for (int64_t i = threadIdx.x; i < HW; i += STAT_THREADS) {
        const double d = (double)pre_ld<U8>(x, base + i) - mean;
        q += d * d;
    }
    q = block_sum_d(q, red);
    if (threadIdx.x == 0) {
        stats[4 * b + 0] = mean;
        stats[4 * b + 1] = sqrt(q / (double)HW);
        stats[4 * b + 2] = mn;
        stats[4 * b + 3] = mx;
    }
}

// grid (blocks, B)
template <bool U8>
__global__ __launch_bounds__(PRE_THREADS) void pre_standardize_kernel(const void* __restrict__ x, const double* __restrict__ stats,
                                                                      float* __restrict__ out, int HW) {
    const int b = blockIdx.y;
    const int64_t base = (int64_t)b * HW;
    const double mean = stats[4 * b + 0], sd = stats[4 * b + 1];
    for (int64_t i = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * PRE_THREADS)
        out[base + i] = (float)(((double)pre_ld<U8>(x, base + i) - mean) / sd);
}

template <bool U8>
__global__ __launch_bounds__(PRE_THREADS) void pre_minmax_kernel(const void* __restrict__ x, const double* __restrict__ stats,
                                                                 float* __restrict__ out, int HW) {
    const int b = blockIdx.y;
    const int64_t base = (int64_t)b * HW;
    if (U8) {
        const int lo = (int)stats[4 * b + 2], hi = (int)stats[4 * b + 3];
        const float den = (float)(hi - lo);
        for (int64_t i = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * PRE_THREADS)
            out[base + i] = __fdiv_rn((float)((int)reinterpret_cast<const uint8_t*>(x)[base + i] - lo), den);
    } else {
        const float lo = (float)stats[4 * b + 2], hi = (float)stats[4 * b + 3];
        const float den = __fsub_rn(hi, lo);
        for (int64_t i = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * PRE_THREADS)
            out[base + i] = __fdiv_rn(__fsub_rn(reinterpret_cast<const float*>(x)[base + i], lo), den);
    }
}

// one wave per row: lane l sums columns l, l + 64, ..., then the lanes' sums in the butterfly's fixed order
template <bool U8>
__global__ __launch_bounds__(PRE_THREADS) void pre_row_normalize_kernel(const void* __restrict__ x, float* __restrict__ out, int64_t rows, int W) {
    const int64_t row = (int64_t)blockIdx.x * (PRE_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;      // (whole waves leave: no barrier below)
    const int lane = threadIdx.x & 63;
    const int64_t base = row * W;
    double q = 0.0;
    for (int c = lane; c < W; c += 64) {
        const double v = (double)pre_ld<U8>(x, base + c);
        q += v * v;
    }
    double n = sqrt(wave_sum_d(q));
    if (n == 0.0) n = 1.0;
    for (int c = lane; c < W; c += 64) out[base + c] = (float)((double)pre_ld<U8>(x, base + c) / n);
}

// ---- unsharp mask: two separable passes over LDS tiles with their halo ------------------------------------------------------
// One output per thread and row (column) of the tile; taps are added from the far pair inwards, acc += w[k] * (t[-k] + t[+k]), the
// centre last.  Lanes of a wave read consecutive LDS words (no bank conflict); w[k] is wave-uniform (a scalar load).
constexpr int BR_TW = 256, BR_ROWS = 4;      // row pass: 4 rows x 256 columns per workgroup, halo lw on both sides
constexpr int UC_TW = 64, UC_TR = 32;        // column pass: 32 rows x 64 columns per workgroup, halo lw above and below

// grid (ceil(W / 256), ceil(H / 4), B)
template <bool U8>
__global__ __launch_bounds__(PRE_THREADS) void pre_blur_rows_kernel(const void* __restrict__ x, float scale_div, const float* __restrict__ w, int lw,
                                                                    float* __restrict__ tmp, int H, int W) {
    __shared__ float t[BR_ROWS][BR_TW + 2 * CMU_PRE_MAX_LW];
    const int64_t base = (int64_t)blockIdx.z * H * W;
    const int y0 = blockIdx.y * BR_ROWS, x0 = blockIdx.x * BR_TW;
    const int tw = min(BR_TW, W - x0), span = tw + 2 * lw;
    const int nr = min(BR_ROWS, H - y0);
    for (int r = 0; r < nr; ++r) {
        const int64_t rowp = base + (int64_t)(y0 + r) * W;
        for (int i = threadIdx.x; i < span; i += PRE_THREADS)
            t[r][i] = __fdiv_rn(pre_ld<U8>(x, rowp + pre_reflect(x0 - lw + i, W)), scale_div);
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= tw) return;
    for (int r = 0; r < nr; ++r) {
        const float* tc = &t[r][c + lw];
        float acc = 0.f;
        for (int k = lw; k > 0; --k) acc += w[k] * (tc[-k] + tc[k]);
        acc += w[0] * tc[0];
        tmp[base + (int64_t)(y0 + r) * W + x0 + c] = acc;
    }
}

// grid (ceil(W / 64), ceil(H / 32), B): thread (cx = t & 63, rg = t >> 6) takes column cx and rows rg, rg + 4, ... of the tile
template <bool U8>
__global__ __launch_bounds__(PRE_THREADS) void pre_unsharp_cols_kernel(const void* __restrict__ x, float scale_div, const float* __restrict__ tmp,
                                                                       const float* __restrict__ w, int lw, float amount, int clip,
                                                                       const double* __restrict__ stats, float* __restrict__ out, int H, int W) {
    __shared__ float t[UC_TR + 2 * CMU_PRE_MAX_LW][UC_TW];
    const int b = blockIdx.z;
    const int64_t base = (int64_t)b * H * W;
    const int y0 = blockIdx.y * UC_TR, x0 = blockIdx.x * UC_TW;
    const int cx = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int tr = min(UC_TR, H - y0), span = tr + 2 * lw;
    const int xx = x0 + cx;
    for (int i = rg; i < span; i += PRE_THREADS / 64)
        t[i][cx] = xx < W ? tmp[base + (int64_t)pre_reflect(y0 - lw + i, H) * W + xx] : 0.f;
    __syncthreads();
    if (xx >= W) return;
    const float lo = (stats && stats[4 * b + 2] < 0.0) ? -1.f : 0.f;
    for (int r = rg; r < tr; r += PRE_THREADS / 64) {
        float acc = 0.f;
        for (int k = lw; k > 0; --k) acc += w[k] * (t[r + lw - k][cx] + t[r + lw + k][cx]);
        acc += w[0] * t[r + lw][cx];
        const int64_t p = base + (int64_t)(y0 + r) * W + xx;
        const float f = __fdiv_rn(pre_ld<U8>(x, p), scale_div);
        float res = f + (f - acc) * amount;
        if (clip) res = res < lo ? lo : (res > 1.f ? 1.f : res);      // (a nan stays a nan, as in np.clip)
        out[p] = res;
    }
}

// grid (blocks, B)
template <typename T>
__global__ __launch_bounds__(PRE_THREADS) void pre_crop_kernel(const T* __restrict__ src, T* __restrict__ dst, int H, int W, int y0, int x0, int OH,
                                                               int OW) {
    const int64_t sbase = (int64_t)blockIdx.y * H * W, dbase = (int64_t)blockIdx.y * OH * OW;
    const int n = OH * OW;
    for (int64_t i = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PRE_THREADS) {
        const int oy = (int)((unsigned)i / (unsigned)OW), ox = (int)i - oy * OW;
        dst[dbase + i] = src[sbase + (int64_t)(y0 + oy) * W + x0 + ox];
    }
}

__global__ __launch_bounds__(PRE_THREADS) void pre_integrate_kernel(const uint8_t* __restrict__ masks, uint8_t* __restrict__ out, int M, int64_t HW) {
    const int64_t mbase = (int64_t)blockIdx.y * M * HW, obase = (int64_t)blockIdx.y * HW;
    for (int64_t i = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * PRE_THREADS) {
        unsigned any = 0;
        for (int m = 0; m < M; ++m) any |= masks[mbase + (int64_t)m * HW + i];
        out[obase + i] = any ? 1 : 0;
    }
}

inline bool pre_shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31); }
inline unsigned pre_blocks(int64_t n) {
    const int64_t nb = cmu_div_up64(n, PRE_THREADS);
    return (unsigned)(nb < PRE_MAX_BLOCKS ? nb : PRE_MAX_BLOCKS);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------------------------------------
#define PRE_LAUNCH_U8(kernel, is_u8, grid, block, st, ...)                                   \
    do {                                                                                     \
        if (is_u8) hipLaunchKernelGGL(kernel<true>, grid, block, 0, st, __VA_ARGS__);        \
        else hipLaunchKernelGGL(kernel<false>, grid, block, 0, st, __VA_ARGS__);             \
    } while (0)

extern "C" int cmu_pre_stats(const void* x, int is_u8, double* stats, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(x && stats && pre_shape_ok(B, H, W), "cmu_pre_stats: bad args (1 <= B <= 65535, 1 <= H, W, H * W < 2^31)");
    CMU_CHECK_ARG(is_u8 == 0 || is_u8 == 1, "cmu_pre_stats: is_u8 must be 0 (float32) or 1 (uint8), got %d", is_u8);
    PRE_LAUNCH_U8(pre_stats_kernel, is_u8, dim3(B), dim3(STAT_THREADS), (hipStream_t)stream, x, stats, H * W);
    CMU_CHECK_LAUNCH("cmu_pre_stats");
    return CMU_OK;
}

extern "C" int cmu_pre_standardize(const void* x, int is_u8, const double* stats, float* out, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(x && stats && out && pre_shape_ok(B, H, W), "cmu_pre_standardize: bad args (1 <= B <= 65535, 1 <= H, W, H * W < 2^31)");
    CMU_CHECK_ARG(is_u8 == 0 || is_u8 == 1, "cmu_pre_standardize: is_u8 must be 0 (float32) or 1 (uint8), got %d", is_u8);
    PRE_LAUNCH_U8(pre_standardize_kernel, is_u8, dim3(pre_blocks((int64_t)H * W), B), dim3(PRE_THREADS), (hipStream_t)stream, x, stats, out, H * W);
    CMU_CHECK_LAUNCH("cmu_pre_standardize");
    return CMU_OK;
}

extern "C" int cmu_pre_minmax(const void* x, int is_u8, const double* stats, float* out, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(x && stats && out && pre_shape_ok(B, H, W), "cmu_pre_minmax: bad args (1 <= B <= 65535, 1 <= H, W, H * W < 2^31)");
    CMU_CHECK_ARG(is_u8 == 0 || is_u8 == 1, "cmu_pre_minmax: is_u8 must be 0 (float32) or 1 (uint8), got %d", is_u8);
    PRE_LAUNCH_U8(pre_minmax_kernel, is_u8, dim3(pre_blocks((int64_t)H * W), B), dim3(PRE_THREADS), (hipStream_t)stream, x, stats, out, H * W);
    CMU_CHECK_LAUNCH("cmu_pre_minmax");
    return CMU_OK;
}

extern "C" int cmu_pre_row_normalize(const void* x, int is_u8, float* out, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(x && out && pre_shape_ok(B, H, W), "cmu_pre_row_normalize: bad args (1 <= B <= 65535, 1 <= H, W, H * W < 2^31)");
    CMU_CHECK_ARG(is_u8 == 0 || is_u8 == 1, "cmu_pre_row_normalize: is_u8 must be 0 (float32) or 1 (uint8), got %d", is_u8);
    const int64_t rows = (int64_t)B * H, nb = cmu_div_up64(rows, PRE_THREADS / 64);
    CMU_CHECK_ARG(nb < ((int64_t)1 << 31), "cmu_pre_row_normalize: B * H < 2^33");
    PRE_LAUNCH_U8(pre_row_normalize_kernel, is_u8, dim3((unsigned)nb), dim3(PRE_THREADS), (hipStream_t)stream, x, out, rows, W);
    CMU_CHECK_LAUNCH("cmu_pre_row_normalize");
    return CMU_OK;
}

extern "C" int cmu_pre_blur_rows(const void* x, int is_u8, float scale_div, const float* weights, int lw, float* tmp, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(x && weights && tmp && pre_shape_ok(B, H, W), "cmu_pre_blur_rows: bad args (1 <= B <= 65535, 1 <= H, W, H * W < 2^31)");
    CMU_CHECK_ARG(is_u8 == 0 || is_u8 == 1, "cmu_pre_blur_rows: is_u8 must be 0 (float32) or 1 (uint8), got %d", is_u8);
    CMU_CHECK_ARG(lw >= 0 && lw <= CMU_PRE_MAX_LW, "cmu_pre_blur_rows: half-width %d outside 0..%d", lw, CMU_PRE_MAX_LW);
    CMU_CHECK_ARG(scale_div > 0.f, "cmu_pre_blur_rows: scale_div must be positive");
    const int gy = cmu_div_up(H, BR_ROWS);
    CMU_CHECK_ARG(gy <= 65535, "cmu_pre_blur_rows: H <= %d", 65535 * BR_ROWS);
    PRE_LAUNCH_U8(pre_blur_rows_kernel, is_u8, dim3(cmu_div_up(W, BR_TW), gy, B), dim3(PRE_THREADS), (hipStream_t)stream, x, scale_div, weights, lw, tmp,
                  H, W);
    CMU_CHECK_LAUNCH("cmu_pre_blur_rows");
    return CMU_OK;
}

extern "C" int cmu_pre_unsharp_cols(const void* x, int is_u8, float scale_div, const float* tmp, const float* weights, int lw, float amount, int clip,
                                    const double* stats, float* out, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(x && tmp && weights && out && pre_shape_ok(B, H, W), "cmu_pre_unsharp_cols: bad args (1 <= B <= 65535, 1 <= H, W, H * W < 2^31)");
    CMU_CHECK_ARG(is_u8 == 0 || is_u8 == 1, "cmu_pre_unsharp_cols: is_u8 must be 0 (float32) or 1 (uint8), got %d", is_u8);
    CMU_CHECK_ARG(lw >= 0 && lw <= CMU_PRE_MAX_LW, "cmu_pre_unsharp_cols: half-width %d outside 0..%d", lw, CMU_PRE_MAX_LW);
    CMU_CHECK_ARG(scale_div > 0.f, "cmu_pre_unsharp_cols: scale_div must be positive");
    CMU_CHECK_ARG(clip == 0 || clip == 1, "cmu_pre_unsharp_cols: clip must be 0 or 1, got %d", clip);
    CMU_CHECK_ARG((const void*)tmp != (const void*)out && (const void*)x != (const void*)out, "cmu_pre_unsharp_cols: out must be a buffer of its own");
    const int gy = cmu_div_up(H, UC_TR);
    CMU_CHECK_ARG(gy <= 65535, "cmu_pre_unsharp_cols: H <= %d", 65535 * UC_TR);
    PRE_LAUNCH_U8(pre_unsharp_cols_kernel, is_u8, dim3(cmu_div_up(W, UC_TW), gy, B), dim3(PRE_THREADS), (hipStream_t)stream, x, scale_div, tmp, weights,
                  lw, amount, clip, stats, out, H, W);
    CMU_CHECK_LAUNCH("cmu_pre_unsharp_cols");
    return CMU_OK;
}

extern "C" int cmu_pre_crop(const void* src, int elem_bytes, void* dst, int B, int H, int W, int y0, int x0, int OH, int OW, void* stream) {
    CMU_CHECK_ARG(src && dst && pre_shape_ok(B, H, W), "cmu_pre_crop: bad args (1 <= B <= 65535, 1 <= H, W, H * W < 2^31)");
    CMU_CHECK_ARG(elem_bytes == 1 || elem_bytes == 4, "cmu_pre_crop: elem_bytes must be 1 or 4, got %d", elem_bytes);
    CMU_CHECK_ARG(OH >= 1 && OW >= 1 && y0 >= 0 && x0 >= 0 && (int64_t)y0 + OH <= H && (int64_t)x0 + OW <= W,
                  "cmu_pre_crop: the window (%d, %d) + (%d, %d) leaves the %d x %d image", y0, x0, OH, OW, H, W);
    const dim3 grid(pre_blocks((int64_t)OH * OW), B);
    if (elem_bytes == 1)
        hipLaunchKernelGGL(pre_crop_kernel<uint8_t>, grid, dim3(PRE_THREADS), 0, (hipStream_t)stream, (const uint8_t*)src, (uint8_t*)dst, H, W, y0, x0, OH, OW);
    else
        hipLaunchKernelGGL(pre_crop_kernel<uint32_t>, grid, dim3(PRE_THREADS), 0, (hipStream_t)stream, (const uint32_t*)src, (uint32_t*)dst, H, W, y0, x0, OH,
                           OW);
    CMU_CHECK_LAUNCH("cmu_pre_crop");
    return CMU_OK;
}

extern "C" int cmu_pre_integrate_masks(const uint8_t* masks, uint8_t* out, int B, int M, int64_t HW, void* stream) {
    CMU_CHECK_ARG(masks && out && B > 0 && B <= 65535 && M >= 1 && HW >= 1, "cmu_pre_integrate_masks: bad args (1 <= B <= 65535, M >= 1, HW >= 1)");
    hipLaunchKernelGGL(pre_integrate_kernel, dim3(pre_blocks(HW), B), dim3(PRE_THREADS), 0, (hipStream_t)stream, masks, out, M, HW);
    CMU_CHECK_LAUNCH("cmu_pre_integrate_masks");
    return CMU_OK;
}
