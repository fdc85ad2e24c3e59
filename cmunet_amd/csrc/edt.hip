// edt.hip -- the exact Euclidean distance transform of uint8 maps on the device, the disk morphology fused into it, and the
// surface-distance reductions built on it.  DESIGN.md section 4.23.
//
//   cmu_edt_columns   edt_col_kernel     one thread per column, two sweeps (down, then up): g = vertical distance to the nearest site
//                                        of the column.  A wave reads and writes 64 consecutive pixels of a row: coalesced.
//   cmu_edt_rows      edt_row_kernel     one workgroup per row: the row of g in LDS, one output pixel per thread, a scan outwards
//                                        from x (edt_scan.h).  Lane l reads g[x0 + l - d] and g[x0 + l + d]: consecutive lanes,
//                                        consecutive words -- no bank conflict at any d.  Writes dist2 (int32), its root (float32)
//                                        and / or a thresholded uint8 map (dilation / erosion by a disk without the int32 map).
//   cmu_surface_border   the border map of a mask (the site predicate of the column pass, as a map).
//   cmu_surface_reduce   one workgroup per image over A's border pixels: n, sum of roots (fp64, fixed order), max, count within tol.
//   cmu_surface_select   one workgroup per image: k-th smallest squared distance of both directions' border pixels, by bisection on
//                        the value with one counting pass per step.
// Every value but the fp64 sum is an integer; no atomics anywhere; no kernel reads what it did not write on the same call.
#include "common.h"
#include "edt_scan.h"

namespace {

constexpr int EDT_COL_THREADS = 64;
constexpr int EDT_COL_UNROLL = 8;
constexpr int EDT_ROW_MAX_THREADS = 256;
constexpr int EDT_RED_THREADS = 1024;

// grid (ceil(W / 64), B)
__global__ __launch_bounds__(EDT_COL_THREADS) void edt_col_kernel(const uint8_t* __restrict__ src, int cls, int border, int* __restrict__ g,
                                                                  int H, int W) {
    const int x = blockIdx.x * EDT_COL_THREADS + threadIdx.x;
    if (x >= W) return;
    const int64_t base = (int64_t)blockIdx.y * H * W;
    const uint8_t* img = src + base;
    int* gc = g + base + x;
    int d = CMU_EDT_GINF;
#pragma unroll EDT_COL_UNROLL
    for (int y = 0; y < H; ++y) {
        d = cmu_edt_col_step(d, cmu_edt_site(img, y, x, H, W, cls, border));
        gc[(int64_t)y * W] = d;
    }
    d = CMU_EDT_GINF;
#pragma unroll EDT_COL_UNROLL
    for (int y = H - 1; y >= 0; --y) {
        const int down = gc[(int64_t)y * W];      // (written above by this very thread)
        d = cmu_edt_col_step(d, down == 0);
        if (d < down) gc[(int64_t)y * W] = d;
    }
}

// grid (H, B), dynamic LDS W ints
__global__ __launch_bounds__(EDT_ROW_MAX_THREADS) void edt_row_kernel(const int* __restrict__ g, int* __restrict__ dist2, float* __restrict__ dist,
                                                                      const uint8_t* __restrict__ base_map, uint8_t* __restrict__ out8, int gt, int t,
                                                                      int v_hit, int v_miss, int H, int W) {
    extern __shared__ int row[];
    const int64_t off = ((int64_t)blockIdx.y * H + blockIdx.x) * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) row[x] = g[off + x];
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const int d2 = cmu_edt_row_min(row, x, W);
        if (dist2) dist2[off + x] = d2;
        if (dist) dist[off + x] = d2 < 0 ? __builtin_inff() : (float)sqrt((double)d2);      // fp64 root, one rounding to float32
        if (out8) out8[off + x] = (uint8_t)cmu_edt_select(d2, t, gt, base_map[off + x], v_hit, v_miss);
    }
}

// grid (ceil(H * W / 256), B)
__global__ __launch_bounds__(256) void edt_border_kernel(const uint8_t* __restrict__ src, int cls, uint8_t* __restrict__ out, int H, int W) {
    const int HW = H * W;
    const int64_t base = (int64_t)blockIdx.y * HW;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < HW) out[base + i] = cmu_edt_site(src + base, (int)(i / W), (int)(i % W), H, W, cls, 1);
}

// integer block reductions over `red` (LDS, one word per wave), the result in every thread
__device__ inline int edt_block_sum_i(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int a = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) a += red[i];
    return a;
}
__device__ inline int edt_block_max_i(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int a = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) a = max(a, red[i]);
    return a;
}

// grid (B): thread t takes pixels t, t + 1024, ... (a fixed order), then the waves' sums are added in wave order
__global__ __launch_bounds__(EDT_RED_THREADS) void surface_reduce_kernel(const uint8_t* __restrict__ src, int cls, const int* __restrict__ dist2,
                                                                         int tol2, int* __restrict__ masked, double* __restrict__ sums,
                                                                         int* __restrict__ counts, int H, int W) {
    __shared__ int red_i[EDT_RED_THREADS / 64];
    __shared__ double red_d[EDT_RED_THREADS / 64];
    const int b = blockIdx.x, HW = H * W;
    const int64_t base = (int64_t)b * HW;
    int n = 0, mx = -1, within = 0;
    double sum = 0.0;
    for (int i = threadIdx.x; i < HW; i += EDT_RED_THREADS) {
        const bool on = cmu_edt_site(src + base, i / W, i % W, H, W, cls, 1);
        const int d2 = dist2[base + i];
        if (masked) masked[base + i] = on ? d2 : CMU_EDT_NOT_BORDER;
        if (on) {
            ++n;
            if (d2 < 0) {                       // the other border is empty: infinitely far
                sum += (double)__builtin_inff();
                mx = 0x7fffffff;
            } else {
                sum += sqrt((double)d2);
                mx = max(mx, d2);
                within += d2 <= tol2;
            }
        }
    }
    n = edt_block_sum_i(n, red_i);
    within = edt_block_sum_i(within, red_i);
    mx = edt_block_max_i(mx, red_i);
    sum = block_sum_d(sum, red_d);
    if (threadIdx.x == 0) {
        sums[2 * b] = sum;
        sums[2 * b + 1] = mx < 0 ? 0.0 : (mx == 0x7fffffff ? (double)__builtin_inff() : sqrt((double)mx));
        counts[3 * b] = n;
        counts[3 * b + 1] = mx;
        counts[3 * b + 2] = within;
    }
}

// count(v) over both masked maps of one image, by the whole workgroup: every thread calls it with the same v and gets the same count
struct SurfaceCount {
    const int* a;
    const int* b;
    int HW;
    int* red;
    __device__ int64_t operator()(int v) {
        int c = 0;
        for (int i = threadIdx.x; i < HW; i += EDT_RED_THREADS) {
            const int p = a[i], q = b[i];
            c += (p >= 0 && p <= v) + (q >= 0 && q <= v);
        }
        return edt_block_sum_i(c, red);      // (at most 2 * H * W <= 2^25: no overflow)
    }
};

// grid (B).  A first pass finds how many entries there are and their maximum (the bisection's upper end: 9 bits on a typical mask where
// the bound (H - 1)^2 + (W - 1)^2 has 19); a rank that is not below the one before it starts from that one's answer.
__global__ __launch_bounds__(EDT_RED_THREADS) void surface_select_kernel(const int* __restrict__ ma, const int* __restrict__ mb,
                                                                         const int* __restrict__ ranks, int R, int* __restrict__ vals,
                                                                         double* __restrict__ roots, int H, int W) {
    __shared__ int red_i[EDT_RED_THREADS / 64];
    const int b = blockIdx.x, HW = H * W;
    const int64_t base = (int64_t)b * HW;
    SurfaceCount count{ma + base, mb + base, HW, red_i};
    int mx = -1;
    for (int i = threadIdx.x; i < HW; i += EDT_RED_THREADS) mx = max(mx, max(ma[base + i], mb[base + i]));
    mx = edt_block_max_i(mx, red_i);
    const int64_t total = mx < 0 ? 0 : count(mx);
    int prev_v = 0, prev_k = 0;
    for (int r = 0; r < R; ++r) {
        const int k = ranks[b * R + r];
        const int lo = (r > 0 && prev_v >= 0 && k >= prev_k) ? prev_v : 0;
        const int v = cmu_edt_kth(count, (int64_t)k, lo, mx, total);
        prev_v = v;
        prev_k = k;
        if (threadIdx.x == 0) {
            vals[b * R + r] = v;
            roots[b * R + r] = v < 0 ? (double)__builtin_inff() : sqrt((double)v);
        }
    }
}

inline bool edt_shape_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= 1 && H <= CMU_EDT_MAX_SIDE && W >= 1 && W <= CMU_EDT_MAX_SIDE;
}
inline bool edt_cls_ok(int cls) { return cls >= -257 && cls <= 255; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int cmu_edt_columns(const uint8_t* src, int cls, int border, int32_t* g, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(src && g && edt_shape_ok(B, H, W), "cmu_edt_columns: bad args (1 <= B <= 65535, 1 <= H, W <= %d)", CMU_EDT_MAX_SIDE);
    CMU_CHECK_ARG(edt_cls_ok(cls), "cmu_edt_columns: cls in 0..255, -1 (non-zero) or -2 - c (not class c), got %d", cls);
    hipLaunchKernelGGL(edt_col_kernel, dim3(cmu_div_up(W, EDT_COL_THREADS), B), dim3(EDT_COL_THREADS), 0, (hipStream_t)stream, src, cls, border != 0, g,
                       H, W);
    CMU_CHECK_LAUNCH("cmu_edt_columns");
    return CMU_OK;
}

extern "C" int cmu_edt_rows(const int32_t* g, int32_t* dist2, float* dist, const uint8_t* base, uint8_t* out8, int greater, int t, int v_hit,
                            int v_miss, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(g && edt_shape_ok(B, H, W), "cmu_edt_rows: bad args (1 <= B <= 65535, 1 <= H, W <= %d)", CMU_EDT_MAX_SIDE);
    CMU_CHECK_ARG(dist2 || dist || out8, "cmu_edt_rows: no output given");
    CMU_CHECK_ARG(!out8 == !base, "cmu_edt_rows: base and out8 come together");
    CMU_CHECK_ARG(!out8 || (t >= 0 && v_hit >= -1 && v_hit <= 255 && v_miss >= -1 && v_miss <= 255),
                  "cmu_edt_rows: t >= 0 and v_hit, v_miss in -1 (keep base) .. 255");
    const int threads = min(EDT_ROW_MAX_THREADS, cmu_div_up(W, 64) * 64);
    hipLaunchKernelGGL(edt_row_kernel, dim3(H, B), dim3(threads), (size_t)W * sizeof(int), (hipStream_t)stream, g, dist2, dist, base, out8,
                       greater != 0, t, v_hit, v_miss, H, W);
    CMU_CHECK_LAUNCH("cmu_edt_rows");
    return CMU_OK;
}

extern "C" int cmu_surface_border(const uint8_t* src, int cls, uint8_t* border, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(src && border && edt_shape_ok(B, H, W), "cmu_surface_border: bad args (1 <= B <= 65535, 1 <= H, W <= %d)", CMU_EDT_MAX_SIDE);
    CMU_CHECK_ARG(edt_cls_ok(cls), "cmu_surface_border: cls in 0..255, -1 (non-zero) or -2 - c (not class c), got %d", cls);
    hipLaunchKernelGGL(edt_border_kernel, dim3((unsigned)cmu_div_up64((int64_t)H * W, 256), B), dim3(256), 0, (hipStream_t)stream, src, cls, border, H,
                       W);
    CMU_CHECK_LAUNCH("cmu_surface_border");
    return CMU_OK;
}

extern "C" int cmu_surface_reduce(const uint8_t* src, int cls, const int32_t* dist2, int tol2, int32_t* masked, double* sums, int32_t* counts, int B,
                                  int H, int W, void* stream) {
    CMU_CHECK_ARG(src && dist2 && sums && counts && edt_shape_ok(B, H, W), "cmu_surface_reduce: bad args (1 <= B <= 65535, 1 <= H, W <= %d)",
                  CMU_EDT_MAX_SIDE);
    CMU_CHECK_ARG(edt_cls_ok(cls) && tol2 >= 0, "cmu_surface_reduce: cls in 0..255, -1 or -2 - c, and tol2 >= 0");
    hipLaunchKernelGGL(surface_reduce_kernel, dim3(B), dim3(EDT_RED_THREADS), 0, (hipStream_t)stream, src, cls, dist2, tol2, masked, sums, counts, H, W);
    CMU_CHECK_LAUNCH("cmu_surface_reduce");
    return CMU_OK;
}

extern "C" int cmu_surface_select(const int32_t* masked_a, const int32_t* masked_b, const int32_t* ranks, int n_ranks, int32_t* values, double* roots,
                                  int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(masked_a && masked_b && ranks && values && roots && edt_shape_ok(B, H, W),
                  "cmu_surface_select: bad args (1 <= B <= 65535, 1 <= H, W <= %d)", CMU_EDT_MAX_SIDE);
    CMU_CHECK_ARG(n_ranks >= 1 && n_ranks <= 2, "cmu_surface_select: one or two ranks per image, got %d", n_ranks);
    hipLaunchKernelGGL(surface_select_kernel, dim3(B), dim3(EDT_RED_THREADS), 0, (hipStream_t)stream, masked_a, masked_b, ranks, n_ranks, values, roots,
                       H, W);
    CMU_CHECK_LAUNCH("cmu_surface_select");
    return CMU_OK;
}
