// tiled_predict.hip -- sliding-window (tiled) segmentation with flip / rotation ensembling: three streaming passes around the network.
//
//   cmu_extract_tiles   images (N,H,W) f32 / u8 -> tiles (n,TH,TW) f32: the window at (ystarts[iy], xstarts[ix]) of the zero- or
//                       reflect-padded canvas, in the forward dihedral view of the copy's code.  A pure copy: exact.
//   cmu_head_probs      the 1x1 head of cmu_head_predict (head_math.h: the same logits, the same softmax arithmetic) storing ALL K'
//                       probability planes, fp32 (n,K',TH,TW), each tile put back into the un-augmented frame (the inverse view).
//   cmu_blend_tiles     per canvas pixel, the window-weighted sum of every covering (tile, copy)'s probabilities in the fixed order
//                       iy, ix, a -> argmax / threshold label (+ one class's blended probability).  A gather: no atomics, the same
//                       bits on every call.
//
// Tile index = ((img * ny + iy) * nx + ix) * A + a.  Dihedral code: bit 0 flips W, bit 1 flips H, bit 2 transposes; the forward view is
// flip W, flip H, transpose in that order, so view[r][c] = window[y][x] with (y, x) = (r, c), swapped if bit 2, then y -> TH-1-y if
// bit 1, x -> TW-1-x if bit 0 (view_to_window below; a transposing code needs TH == TW).
//
// Memory shape: all three are HBM-streaming.  extract stores one 16-byte vector per lane (TW % 4 == 0) from four gathered source values
// (a tile row is a source row or column: L2 serves the transposed reads); head_probs walks the pixels in the order of its OUTPUT -- a
// lane group owns four consecutive output pixels and fetches the view pixel each one comes from; a pixel's C channels are one
// contiguous run of 16 * C/epc bytes wherever it lies, so the loads stay whole lines at the product's C = 64 and the K' plane stores
// are consecutive floats for every code; blend reads 4 K' bytes per covering (tile, copy) per pixel with consecutive lanes on consecutive
// x, and stores one byte per lane.  Grid-stride under a block cap.
#include "head_math.h"

constexpr int TILED_CAP = 8192;      // blocks per launch: the rest is a grid-stride loop

// forward view coordinate (r, c) -> window coordinate (y, x)
__device__ static inline void view_to_window(int code, int TH, int TW, int r, int c, int& y, int& x) {
    y = (code & 4) ? c : r;
    x = (code & 4) ? r : c;
    if (code & 2) y = TH - 1 - y;
    if (code & 1) x = TW - 1 - x;
}

// window coordinate (y, x) -> forward view coordinate (r, c): the flips are their own inverses and precede the transpose
__device__ static inline void window_to_view(int code, int TH, int TW, int y, int x, int& r, int& c) {
    if (code & 2) y = TH - 1 - y;
    if (code & 1) x = TW - 1 - x;
    r = (code & 4) ? x : y;
    c = (code & 4) ? y : x;
}

// reflection without repeating the edge (numpy's 'reflect'), for any integer i: the triangle fold of period 2 (L - 1)
__device__ static inline int fold_reflect(int i, int L) {
    if (L == 1) return 0;
    const int m = 2 * (L - 1);
    i %= m;
    if (i < 0) i += m;
    return i >= L ? m - i : i;
}

template <class TS>
__device__ static inline float extract_one(const TS* __restrict__ src, int64_t img, int H, int W, int sy, int sx, int pad_mode) {
    if (sy < 0 || sy >= H || sx < 0 || sx >= W) {
        if (pad_mode == 0) return 0.f;
        sy = fold_reflect(sy, H);
        sx = fold_reflect(sx, W);
    }
    return (float)src[(img * H + sy) * (int64_t)W + sx];
}

template <class TS, int V>      // V = outputs per lane: 4 (one 16-byte store; TW % 4 == 0) or 1
__global__ void __launch_bounds__(256)
extract_tiles_kernel(const TS* __restrict__ src, const int* __restrict__ ystarts, const int* __restrict__ xstarts,
                     const uint8_t* __restrict__ codes, float* __restrict__ out, int H, int W, int ny, int nx, int A, int TH, int TW,
                     int pad_mode, int64_t nvec) {
    const int rowv = TW / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        const int cv = (int)(i % rowv);
        int64_t t = i / rowv;
        const int r = (int)(t % TH);
        t /= TH;                               // the tile
        const int a = (int)(t % A);
        int64_t s = t / A;
        const int ix = (int)(s % nx);
        s /= nx;
        const int iy = (int)(s % ny);
        const int64_t img = s / ny;
        const int code = codes ? codes[a] & (TH == TW ? 7 : 3) : 0;      // (a transposing code on a non-square tile: refused by the caller)
        const int y0 = ystarts[iy], x0 = xstarts[ix];
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            int y, x;
            view_to_window(code, TH, TW, r, cv * V + j, y, x);
            v[j] = extract_one<TS>(src, img, H, W, y0 + y, x0 + x, pad_mode);
        }
        if (V == 4) {
            st_global16(out + i * 4, u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])});
        } else {
            out[i] = v[0];
        }
    }
}

extern "C" int cmu_extract_tiles(const void* src, int src_u8, int N, int H, int W, const int* ystarts, int ny, const int* xstarts, int nx,
                                 const uint8_t* codes, int A, int TH, int TW, int pad_mode, float* out, void* stream) {
    CMU_CHECK_ARG(src && out && ystarts && xstarts, "cmu_extract_tiles: null pointer");
    CMU_CHECK_ARG(src_u8 == 0 || src_u8 == 1, "cmu_extract_tiles: src_u8=%d must be 0 (float32) or 1 (uint8)", src_u8);
    CMU_CHECK_ARG(N > 0 && H > 0 && W > 0 && ny > 0 && nx > 0 && A > 0 && TH > 0 && TW > 0, "cmu_extract_tiles: sizes must be positive");
    CMU_CHECK_ARG(pad_mode == 0 || pad_mode == 1, "cmu_extract_tiles: pad_mode=%d must be 0 (zero) or 1 (reflect)", pad_mode);
    CMU_CHECK_ARG(codes != nullptr || A == 1, "cmu_extract_tiles: A=%d copies need a code array", A);
    CMU_CHECK_ARG(src_u8 == 1 || (reinterpret_cast<uintptr_t>(src) & 3) == 0, "cmu_extract_tiles: float32 source must be 4-byte aligned");
    CMU_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "cmu_extract_tiles: out must be 4-byte aligned");
    CMU_CHECK_ARG(TH <= (1 << 20) && TW <= (1 << 20) && H <= (1 << 24) && W <= (1 << 24), "cmu_extract_tiles: side too large");
    const int64_t n = (int64_t)N * ny * nx * A;
    const int64_t total = n * TH * TW;
    CMU_CHECK_ARG(n < ((int64_t)1 << 31) && total < ((int64_t)1 << 40), "cmu_extract_tiles: too many tiles");
    const bool vec = (TW % 4 == 0) && cmu_aligned16(out);
    const int64_t nvec = vec ? total / 4 : total;
    const int64_t nb = cmu_div_up64(nvec, 256);
    const int grid = (int)(nb < TILED_CAP ? nb : TILED_CAP);
    hipStream_t st = (hipStream_t)stream;
#define CMU_EXTRACT_LAUNCH(TS, V)                                                                                                      \
    hipLaunchKernelGGL((extract_tiles_kernel<TS, V>), dim3(grid), dim3(256), 0, st, (const TS*)src, ystarts, xstarts, codes, out, H, W, \
                       ny, nx, A, TH, TW, pad_mode, nvec)
    if (src_u8) {
        if (vec) CMU_EXTRACT_LAUNCH(uint8_t, 4); else CMU_EXTRACT_LAUNCH(uint8_t, 1);
    } else {
        if (vec) CMU_EXTRACT_LAUNCH(float, 4); else CMU_EXTRACT_LAUNCH(float, 1);
    }
#undef CMU_EXTRACT_LAUNCH
    CMU_CHECK_LAUNCH("cmu_extract_tiles");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// cmu_head_probs
// ---------------------------------------------------------------------------------------------------------------------------------
template <class TR, int KT>      // KT = compiled class count, as in head_predict_kernel
__global__ void __launch_bounds__(256, 3)
head_probs_kernel(const unsigned char* __restrict__ x, int64_t ldx, const float* __restrict__ scale, const float* __restrict__ shift,
                  const float* __restrict__ w, const float* __restrict__ bias, const uint8_t* __restrict__ codes, float* __restrict__ probs,
                  int TH, int TW, int C, int K, int64_t npix) {
    constexpr int EPC = TR::EPC;
    constexpr int ES = (int)sizeof(typename TR::elem_t);
    constexpr int U = 4;         // consecutive OUTPUT pixels per lane group and trip: four 16-byte loads in flight
    const int nchunk = C / EPC;  // power of two <= 64 (checked on the host)
    const int ch = threadIdx.x % nchunk;
    const int g = threadIdx.x / nchunk;
    const int ppb = blockDim.x / nchunk;
    const int KP = K > 1 ? K : 1;
    const int plane = TH * TW;   // < 2^31 (host check)
    const int cmask = TH == TW ? 7 : 3;      // memory safety: a transposed coordinate lies inside a square tile only
    float sc[EPC], sh[EPC], wk[KT][EPC], bk[KT];
    head_lane_operands<TR, KT>(scale, shift, w, bias, C, K, ch, sc, sh, wk, bk);
    const float lo = scale ? 0.f : -__builtin_inff();
    for (int64_t p0 = (int64_t)blockIdx.x * ppb * U; p0 < npix; p0 += (int64_t)gridDim.x * ppb * U) {
        const int64_t pbase = p0 + (int64_t)g * U;      // output pixel (tile, y, x), linear; a multiple of four
        // (tile, y, x) of the group's first pixel: one 32-bit division by the plane and one by the row whenever the pixel count allows
        // (the 64-bit form costs as many instructions as a whole pixel of a two-class head)
        int64_t tile0;
        int rem0;
        if (npix <= 0x7fffffff) {      // pbase < npix + 1024 < 2^32
            const uint32_t pb = (uint32_t)pbase, t = pb / (uint32_t)plane;
            tile0 = t;
            rem0 = (int)(pb - t * (uint32_t)plane);
        } else {
            tile0 = pbase / plane;
            rem0 = (int)(pbase - tile0 * plane);
        }
        const int y0 = rem0 / TW, x0 = rem0 - y0 * TW;
        const bool one_row = x0 + U <= TW;      // the four pixels lie in one row of one tile (always, when TW % 4 == 0)
        const int code0 = (codes != nullptr && pbase < npix) ? codes[tile0] & cmask : 0;
        u32x4 q[U];
        int64_t dst[U];          // where pixel u's class-0 probability goes (-1: past the end)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t tile = tile0;
            int rem = rem0 + u, y = y0, xo = x0 + u, code = code0;
            const bool in = pbase + u < npix;
            if (!one_row) {
                while (rem >= plane) {      // (a plane smaller than four pixels wraps more than once)
                    rem -= plane;
                    ++tile;
                }
                y = rem / TW;
                xo = rem - y * TW;
                code = (codes != nullptr && in) ? codes[tile] & cmask : 0;
            }
            int r, c;
            window_to_view(code, TH, TW, y, xo, r, c);
            const int64_t spix = tile * plane + (int64_t)r * TW + c;      // < npix: (r, c) lies inside the tile (TH == TW under bit 2)
            q[u] = in ? ld_global16(x + (spix * ldx + ch * EPC) * ES) : u32x4{0u, 0u, 0u, 0u};
            dst[u] = in ? tile * KP * plane + rem : -1;
        }
        float kl[KT], km = 0.f;
        int64_t kd = -1;
#pragma unroll
        for (int k = 0; k < KT; ++k) kl[k] = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float l[KT];
            head_pixel_logits<TR, KT>(q[u], sc, sh, wk, bk, lo, nchunk, K, l);
            float m = l[0];
#pragma unroll
            for (int k = 1; k < KT; ++k)
                if (k < K && l[k] > m) m = l[k];
            if (nchunk >= U) {      // lane u of the group keeps pixel u: one softmax per lane and trip
#pragma unroll
                for (int k = 0; k < KT; ++k) kl[k] = (ch == u) ? l[k] : kl[k];
                km = (ch == u) ? m : km;
                kd = (ch == u) ? dst[u] : kd;
            } else if (ch == 0 && dst[u] >= 0) {
                float p[KT];
                head_prob_all<KT>(l, m, K, p);
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < KP) probs[dst[u] + (int64_t)k * plane] = p[k];
            }
        }
        if (nchunk >= U) {
            float p[KT];
            head_prob_all<KT>(kl, km, K, p);
            if (ch < U && kd >= 0) {
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < KP) probs[kd + (int64_t)k * plane] = p[k];
            }
        }
    }
}

template <class TR>
static int head_probs_t(const void* x, int64_t ldx, const float* scale, const float* shift, const float* w, const float* bias,
                        const uint8_t* codes, float* probs, int n, int TH, int TW, int C, int K, hipStream_t st) {
    const int nchunk = C / TR::EPC;
    const int64_t npix = (int64_t)n * TH * TW;
    const int ppb = 256 / nchunk;
    const int64_t nb = cmu_div_up64(npix, ppb * 4);
    const int grid = (int)(nb < TILED_CAP ? nb : TILED_CAP);
    if (K <= 2)
        hipLaunchKernelGGL((head_probs_kernel<TR, 2>), dim3(grid), dim3(256), 0, st, (const unsigned char*)x, ldx, scale, shift, w, bias,
                           codes, probs, TH, TW, C, K, npix);
    else
        hipLaunchKernelGGL((head_probs_kernel<TR, PRED_MAX_K>), dim3(grid), dim3(256), 0, st, (const unsigned char*)x, ldx, scale, shift, w,
                           bias, codes, probs, TH, TW, C, K, npix);
    CMU_CHECK_LAUNCH("cmu_head_probs");
    return CMU_OK;
}

static bool tiled_is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

extern "C" int cmu_head_probs(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, const float* w, const float* bias,
                              const uint8_t* codes, int allow_transpose, float* probs, int n, int TH, int TW, int C, int K, int dt,
                              void* stream) {
    const int es = cmu_dtype_size(dt);
    CMU_CHECK_ARG(es > 0 && x && w && bias && probs && n > 0 && TH > 0 && TW > 0, "cmu_head_probs: bad args");
    const int epc = 16 / es;
    CMU_CHECK_ARG(K >= 1 && K <= PRED_MAX_K, "cmu_head_probs: K=%d must be in 1..%d", K, PRED_MAX_K);
    CMU_CHECK_ARG(C % epc == 0 && tiled_is_pow2(C / epc) && C / epc <= 64, "cmu_head_probs: C=%d: C/%d must be a power of two <= 64", C, epc);
    CMU_CHECK_ARG(cmu_aligned16(x) && ldx % epc == 0 && ldx >= C, "cmu_head_probs: x alignment / stride");
    CMU_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "cmu_head_probs: scale/shift must both be set");
    CMU_CHECK_ARG((reinterpret_cast<uintptr_t>(probs) & 3) == 0, "cmu_head_probs: probs must be 4-byte aligned");
    CMU_CHECK_ARG((int64_t)TH * TW < ((int64_t)1 << 30), "cmu_head_probs: tile %d x %d too large", TH, TW);
    // the codes live on the device: the caller states whether any of them transposes, and a transposing set needs a square tile
    CMU_CHECK_ARG(allow_transpose == 0 || allow_transpose == 1, "cmu_head_probs: allow_transpose must be 0 or 1");
    CMU_CHECK_ARG(!(allow_transpose && codes == nullptr), "cmu_head_probs: allow_transpose without a code array");
    CMU_CHECK_ARG(!allow_transpose || TH == TW, "cmu_head_probs: transposing codes need a square tile, got %d x %d", TH, TW);
    CMU_DISPATCH_DT(dt, head_probs_t, x, ldx, in_scale, in_shift, w, bias, codes, probs, n, TH, TW, C, K, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// cmu_blend_tiles
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
blend_tiles_kernel(const float* __restrict__ probs, const int* __restrict__ ystarts, const int* __restrict__ xstarts,
                   const float* __restrict__ wy, const float* __restrict__ wx, float thr, const uint8_t* __restrict__ lut,
                   uint8_t* __restrict__ labels, float* __restrict__ prob, int pc, int H, int W, int ny, int nx, int A, int TH, int TW,
                   int K, int64_t npix) {
    const int KP = K > 1 ? K : 1;
    const int64_t plane = (int64_t)TH * TW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int64_t t = i / W;
        const int y = (int)(t % H);
        const int64_t img = t / H;
        float num[PRED_MAX_K], den = 0.f;
#pragma unroll
        for (int k = 0; k < PRED_MAX_K; ++k) num[k] = 0.f;
        for (int iy = 0; iy < ny; ++iy) {
            const int dy = y - ystarts[iy];
            if (dy < 0 || dy >= TH) continue;
            const float fy = wy[dy];
            for (int ix = 0; ix < nx; ++ix) {
                const int dx = x - xstarts[ix];
                if (dx < 0 || dx >= TW) continue;
                const float wgt = fy * wx[dx];
                const int64_t tile = ((img * ny + iy) * nx + ix) * A;
                const float* p = probs + tile * KP * plane + (int64_t)dy * TW + dx;
                for (int a = 0; a < A; ++a, p += KP * plane) {
#pragma unroll
                    for (int k = 0; k < PRED_MAX_K; ++k)
                        if (k < KP) num[k] = fmaf(wgt, p[k * plane], num[k]);
                    den += wgt;
                }
            }
        }
        int best = 0;
        if (K == 1) {
            best = (num[0] / den > thr) ? 1 : 0;      // a probability threshold on the blended probability (fp32 division)
        } else {
            float m = num[0];
#pragma unroll
            for (int k = 1; k < PRED_MAX_K; ++k)
                if (k < K && num[k] > m) {            // strict: the smallest index among equal maxima
                    m = num[k];
                    best = k;
                }
        }
        labels[i] = lut ? lut[best] : (uint8_t)best;
        if (prob != nullptr) {
            float v = num[0];
#pragma unroll
            for (int k = 1; k < PRED_MAX_K; ++k) v = (k == pc) ? num[k] : v;
            prob[i] = v / den;
        }
    }
}

extern "C" int cmu_blend_tiles(const float* probs, int N, int H, int W, const int* ystarts, int ny, const int* xstarts, int nx, int A, int TH,
                               int TW, int K, const float* wy, const float* wx, float threshold, const uint8_t* lut, uint8_t* labels,
                               float* prob, int prob_class, void* stream) {
    CMU_CHECK_ARG(probs && ystarts && xstarts && wy && wx && labels, "cmu_blend_tiles: null pointer");
    CMU_CHECK_ARG(N > 0 && H > 0 && W > 0 && ny > 0 && nx > 0 && A > 0 && TH > 0 && TW > 0, "cmu_blend_tiles: sizes must be positive");
    CMU_CHECK_ARG(K >= 1 && K <= PRED_MAX_K, "cmu_blend_tiles: K=%d must be in 1..%d", K, PRED_MAX_K);
    CMU_CHECK_ARG((reinterpret_cast<uintptr_t>(probs) & 3) == 0 && (reinterpret_cast<uintptr_t>(wy) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(wx) & 3) == 0, "cmu_blend_tiles: probs / windows must be 4-byte aligned");
    CMU_CHECK_ARG((int64_t)TH * TW < ((int64_t)1 << 30), "cmu_blend_tiles: tile %d x %d too large", TH, TW);
    CMU_CHECK_ARG((int64_t)N * ny * nx * A < ((int64_t)1 << 31), "cmu_blend_tiles: too many tiles");
    if (prob != nullptr) {
        CMU_CHECK_ARG((reinterpret_cast<uintptr_t>(prob) & 3) == 0, "cmu_blend_tiles: prob must be 4-byte aligned");
        CMU_CHECK_ARG(prob_class >= 0 && prob_class < (K > 1 ? K : 1), "cmu_blend_tiles: prob_class=%d outside 0..%d", prob_class, (K > 1 ? K : 1) - 1);
    }
    const int64_t npix = (int64_t)N * H * W;
    const int64_t nb = cmu_div_up64(npix, 256);
    const int grid = (int)(nb < TILED_CAP ? nb : TILED_CAP);
    hipLaunchKernelGGL(blend_tiles_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, probs, ystarts, xstarts, wy, wx, threshold, lut, labels,
                       prob, prob_class, H, W, ny, nx, A, TH, TW, K, npix);
    CMU_CHECK_LAUNCH("cmu_blend_tiles");
    return CMU_OK;
}
