// moco_views.hip -- MoCo-v2's two augmented views (Pretraining/MoCo/.../moco_data_module.py:119-132, tau_g: RandomApply(RandomRotation(180)),
// RandomResizedCrop(224, scale (0.2, 1)), RandomApply(GaussianBlur((5, 9), (0.1, 2))), RandomHorizontalFlip, RandomVerticalFlip,
// RandomApply(GaussNoise)) for a whole batch of device-resident S x S float32 images.  Every random decision of one (image, view) sits in
// one record (CmuMocoViewRec, include/cmunet_hip.h); DESIGN.md 4.14 restates the rules (torchvision 0.14.0's tensor path).
//
//   cmu_mocoviews_sample     the (B, 2) records, Philox4x32-10 keyed by (seed, offset), one thread per record; the rejection loop of
//                            RandomResizedCrop.get_params (10 attempts, then the centred fallback) runs in the kernel
//   cmu_mocoviews_geometry   rotation -> crop -> resize -> blur -> flips in one pass: a workgroup owns a 32 x 32 tile of one view's output.
//                            It stages the resized tile plus the blur's halo (reflected at the output's border) in LDS -- each staged pixel
//                            the bilinear (or antialiased) combination of pixels of the rotated image, each of those one nearest-neighbour
//                            read of the raw image through the inverse rotation --, blurs separably from LDS, stores with the flips folded
//                            into the address and merges the tile's maximum into the view's word (atomic max on the order-preserving bits)
//   cmu_mocoviews_noise      out += (max / 10) * z for the views whose record asks for it; z from Philox by (seed, offset, view, pixel) or
//                            from an explicit tensor
//
// Built with -ffp-contract=off (Makefile): the nearest-neighbour index and the resize's source coordinates are torch's float32 arithmetic,
// operation by operation.
#include "philox_stream.h"
#include <math.h>
#include <stddef.h>
#pragma clang fp contract(off)

static_assert(sizeof(CmuMocoViewRec) == 40, "CmuMocoViewRec layout");
enum { MV_ROT = 1, MV_BLUR = 2, MV_HFLIP = 4, MV_VFLIP = 8, MV_NOISE = 16 };
enum { MVS_RECORD = 0, MVS_NOISE = 1 };
constexpr int MV_NPARAMS = 12;
constexpr int MV_MAX_K = 9;                          // largest blur kernel on either axis (the LDS halo is (MV_MAX_K - 1) / 2)
constexpr int MV_HALO = (MV_MAX_K - 1) / 2;
constexpr int MV_TILE = 32;
constexpr int MV_IN = MV_TILE + 2 * MV_HALO;
constexpr int MV_TAPS = 6;                           // widest resize window (antialias: 2 * max(in / out, 1) + 2 with in <= 2 * out)
constexpr int MV_ATTEMPTS = 10;

extern "C" int cmu_mocoviews_max_ksize() { return MV_MAX_K; }
extern "C" int cmu_mocoviews_rec_layout(int64_t* out, int n) {
    const int64_t v[] = {(int64_t)sizeof(CmuMocoViewRec), (int64_t)offsetof(CmuMocoViewRec, ops), (int64_t)offsetof(CmuMocoViewRec, top),
                         (int64_t)offsetof(CmuMocoViewRec, left), (int64_t)offsetof(CmuMocoViewRec, height),
                         (int64_t)offsetof(CmuMocoViewRec, width), (int64_t)offsetof(CmuMocoViewRec, angle),
                         (int64_t)offsetof(CmuMocoViewRec, sigma)};
    return cmu_export_layout(v, out, n);
}

// randomness.  Record stream (PhiloxStream, philox_stream.h): c1 = purpose << 28 | record, (c2, c3) = offset, key = seed.  Pixel noise:
// c0 = group of four pixels of the view, c1 = purpose << 28 | record; two Box-Muller pairs on 24-bit uniforms in (0, 1).

// ---------------------------------------------------------------------------------------------
// sampler: every draw is made whether or not its transform fires (all ten crop attempts included), so each parameter sits at a fixed
// position of the record's stream
// ---------------------------------------------------------------------------------------------
struct MvParams {
    double p[MV_NPARAMS];
};
__global__ __launch_bounds__(64) void mocoviews_sample_kernel(CmuMocoViewRec* __restrict__ recs, int n, int H, int W, MvParams P, uint64_t seed,
                                                             uint64_t offset) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* p = P.p;
    PhiloxStream s(seed, offset, philox_id(MVS_RECORD, i));
    CmuMocoViewRec r;
    r.ops = 0;
    r.pad = 0;
    if (s.uniform() < p[0]) r.ops |= MV_ROT;                                    // RandomApply([RandomRotation(degrees)], p)
    r.angle = s.uniform(-p[1], p[1]);
    // RandomResizedCrop.get_params: area * U(scale), exp(U(log ratio)), w = round(sqrt(area * ratio)), h = round(sqrt(area / ratio))
    // (round half to even); the first attempt that fits wins, then top ~ randint(0, H - h + 1), left ~ randint(0, W - w + 1)
    const double area = (double)H * (double)W, llo = log(p[4]), lhi = log(p[5]);
    int ch = 0, cw = 0;
    for (int a = 0; a < MV_ATTEMPTS; ++a) {
        const double target = __dmul_rn(area, s.uniform(p[2], p[3]));
        const double ratio = exp(s.uniform(llo, lhi));
        const int w = (int)rint(sqrt(__dmul_rn(target, ratio))), h = (int)rint(sqrt(__ddiv_rn(target, ratio)));
        if (ch == 0 && 0 < w && w <= W && 0 < h && h <= H) {
            ch = h;
            cw = w;
        }
    }
    const double ut = s.uniform(), ul = s.uniform();
    if (ch > 0) {
        r.top = min((int)(ut * (double)(H - ch + 1)), H - ch);
        r.left = min((int)(ul * (double)(W - cw + 1)), W - cw);
    } else {                                                                    // the centred fallback
        const double in_ratio = (double)W / (double)H;
        if (in_ratio < p[4]) {
            cw = W;
            ch = (int)rint((double)W / p[4]);
        } else if (in_ratio > p[5]) {
            ch = H;
            cw = (int)rint((double)H * p[5]);
        } else {
            cw = W;
            ch = H;
        }
        ch = min(max(ch, 1), H);
        cw = min(max(cw, 1), W);
        r.top = (H - ch) / 2;
        r.left = (W - cw) / 2;
    }
    r.height = ch;
    r.width = cw;
    if (s.uniform() < p[6]) r.ops |= MV_BLUR;                                   // RandomApply([GaussianBlur(kernel, sigma)], p)
    r.sigma = s.uniform(p[7], p[8]);
    if (s.uniform() < p[9]) r.ops |= MV_HFLIP;
    if (s.uniform() < p[10]) r.ops |= MV_VFLIP;
    if (s.uniform() < p[11]) r.ops |= MV_NOISE;                                 // RandomApply([GaussNoise()], p)
    recs[i] = r;
}
extern "C" int cmu_mocoviews_sample(void* recs, int B, int H, int W, const double* params, int nparams, uint64_t seed, uint64_t offset,
                                    void* stream) {
    CMU_CHECK_ARG(recs && params && nparams == MV_NPARAMS && B > 0 && B < (1 << 26) && H > 0 && W > 0 && H <= 32768 && W <= 32768,
                  "cmu_mocoviews_sample: bad args (B %d, %dx%d, %d params)", B, H, W, nparams);
    MvParams P;
    for (int i = 0; i < MV_NPARAMS; ++i) P.p[i] = params[i];
    CMU_CHECK_ARG(P.p[2] > 0.0 && P.p[2] <= P.p[3] && P.p[4] > 0.0 && P.p[4] <= P.p[5] && P.p[7] > 0.0 && P.p[7] <= P.p[8],
                  "cmu_mocoviews_sample: scale, ratio and sigma need 0 < low <= high");
    const int n = 2 * B;
    hipLaunchKernelGGL(mocoviews_sample_kernel, dim3(cmu_div_up(n, 64)), dim3(64), 0, (hipStream_t)stream, (CmuMocoViewRec*)recs, n, H, W, P,
                       seed, offset);
    CMU_CHECK_LAUNCH("cmu_mocoviews_sample");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// geometry + blur + flips
// ---------------------------------------------------------------------------------------------
// order-preserving bits of a float: a < b  <=>  mv_ord(a) < mv_ord(b) as unsigned (0 is below every float: the word's initial value)
__device__ static inline uint32_t mv_ord(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ static inline float mv_unord(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
// one output index of the resize crop-side n -> O: the first source index, the tap count and the weights
struct MvTaps {
    int start, count;
    float w[MV_TAPS];
};
__device__ static inline void mv_taps(MvTaps& t, int o, int n, int O, int antialias) {
    const float scale = __fdiv_rn((float)n, (float)O);                          // area_pixel_compute_scale<float>
    for (int j = 0; j < MV_TAPS; ++j) t.w[j] = 0.f;
    if (!antialias) {
        // upsample_bilinear2d: src = scale * (o + 0.5) - 0.5, clamped at 0; i0 = floor, i1 = i0 + (i0 < n - 1); weights (1 - l, l)
        // (one rounding: ATen's CPU kernels are compiled with fused multiply-add)
        float src = __fmaf_rn(scale, __fadd_rn((float)o, 0.5f), -0.5f);
        if (src < 0.f) src = 0.f;
        const int i0 = min((int)floorf(src), n - 1);
        const float l = fminf(fmaxf(__fadd_rn(src, -(float)i0), 0.f), 1.f);
        t.start = i0;
        t.count = 2;
        t.w[0] = __fadd_rn(1.f, -l);
        t.w[1] = l;
    } else {
        // _upsample_bilinear2d_aa: triangle filter of support max(scale, 1), window [int(c - s + .5), int(c + s + .5)), normalised
        const float support = scale >= 1.f ? scale : 1.f;
        const float invscale = scale >= 1.f ? __fdiv_rn(1.f, scale) : 1.f;
        const float center = __fmul_rn(scale, __fadd_rn((float)o, 0.5f));
        const int xmin = max((int)__fadd_rn(__fadd_rn(center, -support), 0.5f), 0);
        const int xmax = min((int)__fadd_rn(__fadd_rn(center, support), 0.5f), n);
        const int cnt = min(max(xmax - xmin, 0), MV_TAPS);
        float total = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float x = fabsf(__fmul_rn(__fadd_rn(__fadd_rn((float)(j + xmin), -center), 0.5f), invscale));
            const float w = x < 1.f ? __fadd_rn(1.f, -x) : 0.f;
            t.w[j] = w;
            total = __fadd_rn(total, w);
        }
        if (total != 0.f)
            for (int j = 0; j < cnt; ++j) t.w[j] = __fdiv_rn(t.w[j], total);
        t.start = min(xmin, n - 1);
        t.count = cnt;
    }
}
struct MvRot {
    int on;
    float t00, t01, t10, t11, x0, y0;
};
// the rotated image's pixel (Y, X): F.rotate's affine grid (base grid X - W/2 + 0.5, theta^T / (W/2, H/2)), grid_sample's unnormalised
// coordinate ((g + 1) * size - 1) / 2, nearest (round half to even), zero outside
__device__ static inline float mv_read(const float* __restrict__ img, int H, int W, const MvRot& R, int Y, int X) {
    if (!R.on) return img[(int64_t)Y * W + X];
    const float xb = __fadd_rn((float)X, R.x0), yb = __fadd_rn((float)Y, R.y0);
    const float gx = __fadd_rn(__fmul_rn(xb, R.t00), __fmul_rn(yb, R.t01));
    const float gy = __fadd_rn(__fmul_rn(xb, R.t10), __fmul_rn(yb, R.t11));
    const float ix = rintf(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(gx, 1.f), (float)W), -1.f), 0.5f));
    const float iy = rintf(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(gy, 1.f), (float)H), -1.f), 0.5f));
    if (!(ix >= 0.f && ix < (float)W && iy >= 0.f && iy < (float)H)) return 0.f;
    return img[(int64_t)(int)iy * W + (int)ix];
}

__global__ __launch_bounds__(256) void mocoviews_geometry_kernel(const float* __restrict__ src, int B, int H, int W,
                                                                const CmuMocoViewRec* __restrict__ recs, int kx, int ky, int antialias,
                                                                float* __restrict__ out, int O, uint32_t* __restrict__ vmax) {
    __shared__ float tin[MV_IN][MV_IN + 1];
    __shared__ float tmid[MV_IN][MV_TILE + 1];
    __shared__ MvTaps trow[MV_IN], tcol[MV_IN];
    __shared__ float wx[MV_MAX_K], wy[MV_MAX_K];
    __shared__ float wmax[4];
    const int b = blockIdx.z >> 1, v = blockIdx.z & 1, ty0 = blockIdx.y * MV_TILE, tx0 = blockIdx.x * MV_TILE;
    const CmuMocoViewRec rec = recs[b * 2 + v];
    // the record made safe for indexing (records may come from the host)
    const int ch = min(max(rec.height, 1), H), cw = min(max(rec.width, 1), W);
    const int top = min(max(rec.top, 0), H - ch), left = min(max(rec.left, 0), W - cw);
    const bool blur = (rec.ops & MV_BLUR) && rec.sigma > 0.0;
    const int hx = blur ? (kx - 1) / 2 : 0, hy = blur ? (ky - 1) / 2 : 0;
    const int th = min(MV_TILE, O - ty0), tw = min(MV_TILE, O - tx0);
    const int nr = th + 2 * hy, nc = tw + 2 * hx;
    MvRot R;
    R.on = rec.ops & MV_ROT;
    {
        // theta = [[cos r, sin r, 0], [-sin r, cos r, 0]], r = radians(-angle), in double; float32 from there on
        const double r = __dmul_rn(-rec.angle, 3.141592653589793 / 180.0);
        const float c = (float)cos(r), s = (float)sin(r);
        const float hw = __fmul_rn(0.5f, (float)W), hh = __fmul_rn(0.5f, (float)H);
        R.t00 = __fdiv_rn(c, hw);
        R.t01 = __fdiv_rn(s, hw);
        R.t10 = __fdiv_rn(-s, hh);
        R.t11 = __fdiv_rn(c, hh);
        R.x0 = __fadd_rn(__fmul_rn(-(float)W, 0.5f), 0.5f);
        R.y0 = __fadd_rn(__fmul_rn(-(float)H, 0.5f), 0.5f);
    }
    const int tid = threadIdx.x;
    if (tid < nr) mv_taps(trow[tid], reflect101(ty0 - hy + tid, O), ch, O, antialias);
    if (tid >= 64 && tid - 64 < nc) mv_taps(tcol[tid - 64], reflect101(tx0 - hx + tid - 64, O), cw, O, antialias);
    if (blur && tid >= 128 && tid < 130) {
        // _get_gaussian_kernel1d: exp(-0.5 (x / sigma)^2) over linspace(-(k-1)/2, (k-1)/2, k), divided by its sum (float32)
        const int k = tid == 128 ? kx : ky;
        float* w = tid == 128 ? wx : wy;
        const float sg = (float)rec.sigma, half = __fmul_rn((float)(k - 1), 0.5f);
        float sum = 0.f;
        for (int i = 0; i < k; ++i) {
            const float q = __fdiv_rn(__fadd_rn((float)i, -half), sg);
            w[i] = (float)exp((double)__fmul_rn(-0.5f, __fmul_rn(q, q)));
            sum = __fadd_rn(sum, w[i]);
        }
        for (int i = 0; i < k; ++i) w[i] = __fdiv_rn(w[i], sum);
    }
    __syncthreads();
    const float* img = src + (int64_t)b * H * W;
    for (int i = tid; i < nr * nc; i += 256) {
        const int r = i / nc, c = i - r * nc;
        const MvTaps& ry = trow[r];
        const MvTaps& cx = tcol[c];
        float acc = 0.f;
        for (int a = 0; a < ry.count; ++a) {
            const int Y = top + min(ry.start + a, ch - 1);
            float hsum = 0.f;
            for (int e = 0; e < cx.count; ++e) {
                const float p = __fmul_rn(mv_read(img, H, W, R, Y, left + min(cx.start + e, cw - 1)), cx.w[e]);
                hsum = e ? __fadd_rn(hsum, p) : p;
            }
            const float q = __fmul_rn(hsum, ry.w[a]);
            acc = a ? __fadd_rn(acc, q) : q;
        }
        tin[r][c] = acc;
    }
    __syncthreads();
    if (blur) {
        for (int i = tid; i < nr * tw; i += 256) {
            const int r = i / tw, c = i - r * tw;
            float acc = 0.f;
            for (int t = 0; t < kx; ++t) acc = __fadd_rn(acc, __fmul_rn(wx[t], tin[r][c + t]));
            tmid[r][c] = acc;
        }
        __syncthreads();
    }
    // the store runs over the output's rows and columns (full lines); the flips pick the tile's mirrored pixel
    const bool hf = rec.ops & MV_HFLIP, vf = rec.ops & MV_VFLIP;
    const int oy0 = vf ? O - ty0 - th : ty0, ox0 = hf ? O - tx0 - tw : tx0;
    float* dst = out + ((int64_t)v * B + b) * O * O;
    float m = -INFINITY;
    for (int i = tid; i < th * tw; i += 256) {
        const int r = i / tw, c = i - r * tw;
        const int sr = vf ? th - 1 - r : r, sc = hf ? tw - 1 - c : c;
        float a;
        if (blur) {
            a = 0.f;
            for (int t = 0; t < ky; ++t) a = __fadd_rn(a, __fmul_rn(wy[t], tmid[sr + t][sc]));
        } else {
            a = tin[sr][sc];
        }
        dst[(int64_t)(oy0 + r) * O + ox0 + c] = a;
        m = fmaxf(m, a);
    }
    m = wave_max(m);
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        atomicMax(vmax + b * 2 + v, mv_ord(m));
    }
}
extern "C" int cmu_mocoviews_geometry(const float* src, int B, int H, int W, const void* recs, int kx, int ky, int antialias, float* out, int O,
                                      void* vmax, void* stream) {
    CMU_CHECK_ARG(src && recs && out && vmax, "cmu_mocoviews_geometry: null pointer");
    CMU_CHECK_ARG(B > 0 && B < (1 << 15) && H > 0 && W > 0 && O > 0 && H <= 32768 && W <= 32768 && O <= 32768,
                  "cmu_mocoviews_geometry: bad shape (B %d, %dx%d -> %d)", B, H, W, O);
    CMU_CHECK_ARG(kx >= 1 && ky >= 1 && (kx & 1) && (ky & 1) && kx <= MV_MAX_K && ky <= MV_MAX_K,
                  "cmu_mocoviews_geometry: kernel size (%d, %d) must be odd, 1 .. %d", kx, ky, MV_MAX_K);
    CMU_CHECK_ARG(O > (kx - 1) / 2 && O > (ky - 1) / 2, "cmu_mocoviews_geometry: output %d is smaller than the blur's reflection", O);
    CMU_CHECK_ARG(!antialias || (H <= 2 * O && W <= 2 * O), "cmu_mocoviews_geometry: antialias takes crops of at most 2 x the output side (%dx%d -> %d)",
                  H, W, O);
    if (hipError_t e = hipMemsetAsync(vmax, 0, (size_t)2 * B * sizeof(uint32_t), (hipStream_t)stream); e != hipSuccess) {
        cmu_set_error("cmu_mocoviews_geometry: memset failed: %s", hipGetErrorString(e));
        return CMU_ERR_LAUNCH;
    }
    const dim3 grid(cmu_div_up(O, MV_TILE), cmu_div_up(O, MV_TILE), 2 * B);
    hipLaunchKernelGGL(mocoviews_geometry_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, B, H, W, (const CmuMocoViewRec*)recs, kx, ky,
                       antialias, out, O, (uint32_t*)vmax);
    CMU_CHECK_LAUNCH("cmu_mocoviews_geometry");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// the per-view maxima as floats, and GaussNoise: out = image + (max(image) / 10) * randn (float32, operation by operation)
// ---------------------------------------------------------------------------------------------
__global__ void mocoviews_max_kernel(const uint32_t* __restrict__ vmax, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mv_unord(vmax[i]);
}
extern "C" int cmu_mocoviews_max(const void* vmax, float* out, int B, void* stream) {
    CMU_CHECK_ARG(vmax && out && B > 0 && B < (1 << 26), "cmu_mocoviews_max: bad args");
    hipLaunchKernelGGL(mocoviews_max_kernel, dim3(cmu_div_up(2 * B, 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)vmax, out, 2 * B);
    CMU_CHECK_LAUNCH("cmu_mocoviews_max");
    return CMU_OK;
}
__global__ __launch_bounds__(256) void mocoviews_noise_kernel(float* __restrict__ out, int B, int O, const CmuMocoViewRec* __restrict__ recs,
                                                             const uint32_t* __restrict__ vmax, const float* __restrict__ noise, uint64_t seed,
                                                             uint64_t offset) {
    const int b = blockIdx.y >> 1, v = blockIdx.y & 1, ri = b * 2 + v;
    if (!(recs[ri].ops & MV_NOISE)) return;                                      // uniform per workgroup
    const float sigma = __fdiv_rn(mv_unord(vmax[ri]), 10.f);
    const int total = O * O, g = blockIdx.x * 256 + threadIdx.x, p0 = g * 4;
    if (p0 >= total) return;
    const int64_t base = ((int64_t)v * B + b) * total;
    float z[4];
    const int cnt = min(4, total - p0);
    if (noise) {
        for (int j = 0; j < cnt; ++j) z[j] = noise[base + p0 + j];
    } else {
        uint32_t r[4];
        philox4x32_10((uint32_t)g, philox_id(MVS_NOISE, ri), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
        for (int j = 0; j < 2; ++j) {
            const float u1 = ((float)(r[2 * j] >> 8) + 0.5f) * (1.f / 16777216.f), u2 = ((float)(r[2 * j + 1] >> 8) + 0.5f) * (1.f / 16777216.f);
            const float rad = sqrtf(-2.f * logf(u1));
            float sn, cs;
            sincosf(6.2831853071795865f * u2, &sn, &cs);
            z[2 * j] = rad * cs;
            z[2 * j + 1] = rad * sn;
        }
    }
    for (int j = 0; j < cnt; ++j) out[base + p0 + j] = __fadd_rn(out[base + p0 + j], __fmul_rn(sigma, z[j]));
}
extern "C" int cmu_mocoviews_noise(float* out, int B, int O, const void* recs, const void* vmax, const float* noise, uint64_t seed,
                                   uint64_t offset, void* stream) {
    CMU_CHECK_ARG(out && recs && vmax, "cmu_mocoviews_noise: null pointer");
    CMU_CHECK_ARG(B > 0 && B < (1 << 15) && O > 0 && O <= 32768, "cmu_mocoviews_noise: bad shape (B %d, out %d)", B, O);
    const dim3 grid(cmu_div_up(cmu_div_up(O * O, 4), 256), 2 * B);
    hipLaunchKernelGGL(mocoviews_noise_kernel, grid, dim3(256), 0, (hipStream_t)stream, out, B, O, (const CmuMocoViewRec*)recs,
                       (const uint32_t*)vmax, noise, seed, offset);
    CMU_CHECK_LAUNCH("cmu_mocoviews_noise");
    return CMU_OK;
}
