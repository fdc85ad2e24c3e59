// ft_augment.hip -- the finetuning training augmentation (Finetuning/dataset.py:134-165, get_training_augmentation: RandomCrop(475),
// GaussNoise, GaussianBlur, RandomBrightnessContrast, Downscale, OneOf(HorizontalFlip, VerticalFlip, RandomRotate90, GaussNoise)) and the
// SegmentationDataset tail after it (Pillow bicubic resize of the image, NEAREST resize + one-hot of the mask) for a whole batch.
// Every random decision of an image sits in one record (CmuFtAugRec, include/cmunet_hip.h); DESIGN.md 4.13 restates the rules.
//
//   cmu_ftaug_sample          the B records, Philox4x32-10 keyed by (seed, offset), one thread per image
//   cmu_ftaug_photometric     P = brightness(blur(noise(crop(src)))), one workgroup per (64 x 64 tile, image): the tile plus the blur
//                             halo (reflect-101 at the crop's border) in LDS, the separable blur in two LDS passes
//   cmu_ftaug_resize_onehot   (three launches: the resize tables, then two passes) A = OneOf(Downscale(P)) is an index map plus, for OneOf's GaussNoise, a pointwise op: it is composed into
//                             the source read of the Pillow bicubic horizontal pass; the vertical pass gathers the mask through the
//                             same geometry and Pillow's NEAREST table, and writes the one-hot
//   cmu_ftaug_apply           A and the augmented mask themselves (pre-resize: tests and the per-sample albumentations protocol)
//
// Pixel noise is keyed by (seed, offset, image, stage, pixel of the 475 x 475 crop), so a halo pixel two tiles load gets the same draw in
// both, and the horizontal pass that reads an A pixel several times draws the same value each time.  An explicit float64 noise input
// (2, B, S, S) -- plane 0 for GaussNoise, plane 1 for OneOf's GaussNoise -- replaces the generator for parity tests.
// Built with -ffp-contract=off (Makefile): the restated double and float arithmetic rounds after every operation.
#include "philox_stream.h"
#include "pillow_resample.h"
#include <math.h>
#include <stddef.h>
#pragma clang fp contract(off)

static_assert(sizeof(CmuFtAugRec) == 72, "CmuFtAugRec layout");
enum { FA_NOISE = 1, FA_BLUR = 2, FA_BC = 4, FA_DOWN = 8, FA_ONEOF = 16 };
enum { FO_HFLIP = 0, FO_VFLIP = 1, FO_ROT90 = 2, FO_NOISE = 3 };
enum { FS_RECORD = 0, FS_NOISE = 1, FS_ONEOF_NOISE = 2 };
constexpr int FTA_NPARAMS = 19;
constexpr int FTA_MAX_K = 15;                       // largest blur kernel (the halo of a tile is (FTA_MAX_K - 1) / 2)
constexpr int FTA_HALO = (FTA_MAX_K - 1) / 2;
constexpr int FTA_TILE = 64;
constexpr int FTA_IN = FTA_TILE + 2 * FTA_HALO;
constexpr int FTA_MAX_CLASSES = 16;

extern "C" int cmu_ftaug_max_ksize() { return FTA_MAX_K; }
extern "C" int cmu_ftaug_rec_layout(int64_t* out, int n) {
    const int64_t v[] = {(int64_t)sizeof(CmuFtAugRec), (int64_t)offsetof(CmuFtAugRec, ops), (int64_t)offsetof(CmuFtAugRec, y0),
                         (int64_t)offsetof(CmuFtAugRec, x0), (int64_t)offsetof(CmuFtAugRec, ksize), (int64_t)offsetof(CmuFtAugRec, var_noise),
                         (int64_t)offsetof(CmuFtAugRec, var_oneof), (int64_t)offsetof(CmuFtAugRec, sigma), (int64_t)offsetof(CmuFtAugRec, alpha),
                         (int64_t)offsetof(CmuFtAugRec, beta), (int64_t)offsetof(CmuFtAugRec, scale), (int64_t)offsetof(CmuFtAugRec, oneof),
                         (int64_t)offsetof(CmuFtAugRec, rot_k)};
    return cmu_export_layout(v, out, n);
}

// ---------------------------------------------------------------------------------------------
// randomness.  Record stream (PhiloxStream, philox_stream.h): c1 = purpose << 28 | image, (c2, c3) = offset, key = seed.  Pixel noise:
// c0 = pixel of the crop (y * S + x), c1 = stage << 28 | image; Box-Muller on 53-bit uniforms in (0, 1).
// ---------------------------------------------------------------------------------------------
__device__ static inline double fta_normal(uint64_t seed, uint64_t offset, int stage, int b, int64_t pix) {
    uint32_t r[4];
    philox4x32_10((uint32_t)pix, philox_id(stage, b), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return sqrt(-2.0 * log(philox_u53_open(r[0], r[1]))) * cos(6.283185307179586 * philox_u53_open(r[2], r[3]));
}
// x + sigma * z in float64, optionally clipped to [0, 1] (albumentations' maximum for float32), stored as float32
__device__ static inline float fta_add_noise(float x, double sigma, double z, int clip) {
    double d = __dadd_rn((double)x, __dmul_rn(sigma, z));
    if (clip) d = fmin(fmax(d, 0.0), 1.0);
    return (float)d;
}

// ---------------------------------------------------------------------------------------------
// sampler: every draw is made whether or not its transform fires, so each parameter sits at a fixed position of the image's stream
// ---------------------------------------------------------------------------------------------
struct FtaParams {
    double p[FTA_NPARAMS];
};
__global__ __launch_bounds__(64) void ftaug_sample_kernel(CmuFtAugRec* __restrict__ recs, int B, int H, int W, int crop, FtaParams P,
                                                         uint64_t seed, uint64_t offset) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* p = P.p;
    PhiloxStream s(seed, offset, philox_id(FS_RECORD, b));
    CmuFtAugRec r;
    r.ops = 0;
    r.y0 = min((int)((double)(H - crop + 1) * s.uniform()), H - crop);       // RandomCrop: int((H - h + 1) * u)
    r.x0 = min((int)((double)(W - crop + 1) * s.uniform()), W - crop);
    if (s.uniform() < p[0]) r.ops |= FA_NOISE;                                 // GaussNoise(var_limit)
    r.var_noise = s.uniform(p[1], p[2]);
    if (s.uniform() < p[3]) r.ops |= FA_BLUR;                                  // GaussianBlur(blur_limit, sigma_limit)
    const int klo = (int)p[4], khi = (int)p[5];
    int k = klo + (int)s.below((uint32_t)(khi - klo + 1));                     // random.randrange(lo, hi + 1)
    if (k % 2 != 1) k = (k + 1) % (khi + 1);                                   // (the host refuses an even upper limit: never 0)
    r.ksize = k;
    r.sigma = s.uniform(p[6], p[7]);
    if (s.uniform() < p[8]) r.ops |= FA_BC;                                    // RandomBrightnessContrast
    r.alpha = __dadd_rn(1.0, s.uniform(p[11], p[12]));
    r.beta = s.uniform(p[9], p[10]);
    if (s.uniform() < p[13]) r.ops |= FA_DOWN;                                 // Downscale(scale_min, scale_max)
    r.scale = s.uniform(p[14], p[15]);
    if (s.uniform() < p[16]) r.ops |= FA_ONEOF;                                // OneOf([...], p)
    r.oneof = (int)s.below(4);
    r.rot_k = (int)s.below(4);
    r.var_oneof = s.uniform(p[17], p[18]);
    // vector stores of the whole record (plain C++ copy, 72 bytes)
    recs[b] = r;
}
extern "C" int cmu_ftaug_sample(void* recs, int B, int H, int W, int crop, const double* params, int nparams, uint64_t seed, uint64_t offset,
                                void* stream) {
    CMU_CHECK_ARG(recs && params && nparams == FTA_NPARAMS && B > 0 && crop > 0 && H >= crop && W >= crop,
                  "cmu_ftaug_sample: bad args (B %d, %dx%d, crop %d, %d params)", B, H, W, crop, nparams);
    FtaParams P;
    for (int i = 0; i < FTA_NPARAMS; ++i) P.p[i] = params[i];
    const int klo = (int)P.p[4], khi = (int)P.p[5];
    CMU_CHECK_ARG(klo >= 1 && klo <= khi && khi <= FTA_MAX_K && (khi & 1), "cmu_ftaug_sample: blur_limit (%d, %d) must be odd-topped, 1 <= lo <= hi <= %d",
                  klo, khi, FTA_MAX_K);
    hipLaunchKernelGGL(ftaug_sample_kernel, dim3(cmu_div_up(B, 64)), dim3(64), 0, (hipStream_t)stream, (CmuFtAugRec*)recs, B, H, W, crop, P,
                       seed, offset);
    CMU_CHECK_LAUNCH("cmu_ftaug_sample");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// record fields made safe for indexing (records may come from the host)
// ---------------------------------------------------------------------------------------------
struct FtaView {
    int ops, y0, x0, k, oneof, rot_k, small;    // small: the Downscale intermediate's side, cvRound(S * scale)
    double ifx_down, ifx_up;
};
__device__ static inline FtaView fta_view(const CmuFtAugRec& r, int H, int W, int S) {
    FtaView v;
    v.ops = r.ops;
    v.y0 = min(max(r.y0, 0), H - S);
    v.x0 = min(max(r.x0, 0), W - S);
    v.k = r.ksize;
    if (v.k < 1 || v.k > FTA_MAX_K || !(v.k & 1)) v.k = 1;
    v.oneof = r.oneof & 3;
    v.rot_k = r.rot_k & 3;
    // Downscale: cv2.resize(img, None, fx=s, fy=s, INTER_NEAREST) then cv2.resize(small, (S, S), INTER_NEAREST).  OpenCV: the small size
    // is saturate_cast<int>(S * s) (round half to even), resizeNN reads source index min(cvFloor(i * (1 / fx)), n_src - 1) with
    // fx = s going down and fx = S / small (double) going up
    const double s = r.scale > 0.0 ? r.scale : 1.0;
    v.small = (int)rint(__dmul_rn((double)S, s));
    v.small = max(1, v.small);
    v.ifx_down = __ddiv_rn(1.0, s);
    v.ifx_up = __ddiv_rn(1.0, __ddiv_rn((double)S, (double)v.small));
    return v;
}
// OneOf's geometry: the pixel of its input that output (y, x) shows (flips; np.rot90(m, k) on a square)
__device__ static inline void fta_geo(const FtaView& v, int S, int y, int x, int& sy, int& sx) {
    sy = y;
    sx = x;
    if (!(v.ops & FA_ONEOF)) return;
    if (v.oneof == FO_HFLIP) {
        sx = S - 1 - x;
    } else if (v.oneof == FO_VFLIP) {
        sy = S - 1 - y;
    } else if (v.oneof == FO_ROT90) {
        if (v.rot_k == 1) { sy = x; sx = S - 1 - y; }
        else if (v.rot_k == 2) { sy = S - 1 - y; sx = S - 1 - x; }
        else if (v.rot_k == 3) { sy = S - 1 - x; sx = y; }
    }
}
__device__ static inline int fta_down(const FtaView& v, int S, int i) {
    const int u = min((int)floor(__dmul_rn((double)i, v.ifx_up)), v.small - 1);      // the up-pass source index (small image)
    return min((int)floor(__dmul_rn((double)u, v.ifx_down)), S - 1);                  // the down-pass source index (P)
}
// A(y, x): the augmented image (before the resize) read from the photometric output P
__device__ static inline float fta_read(const float* __restrict__ P, const FtaView& v, int S, int b, int y, int x, double sigma1,
                                        const double* __restrict__ noise, int64_t plane, uint64_t seed, uint64_t offset, int clip) {
    int sy, sx;
    fta_geo(v, S, y, x, sy, sx);
    if (v.ops & FA_DOWN) {
        sy = fta_down(v, S, sy);
        sx = fta_down(v, S, sx);
    }
    float a = P[((int64_t)b * S + sy) * S + sx];
    if ((v.ops & FA_ONEOF) && v.oneof == FO_NOISE) {
        const int64_t pix = (int64_t)y * S + x;
        const double z = noise ? noise[plane + (int64_t)b * S * S + pix] : fta_normal(seed, offset, FS_ONEOF_NOISE, b, pix);
        a = fta_add_noise(a, sigma1, z, clip);
    }
    return a;
}
__device__ static inline uint8_t fta_mask(const uint8_t* __restrict__ masks, const FtaView& v, int H, int W, int S, int b, int y, int x) {
    int sy, sx;
    fta_geo(v, S, y, x, sy, sx);
    return masks[((int64_t)b * H + v.y0 + sy) * W + v.x0 + sx];
}

// ---------------------------------------------------------------------------------------------
// photometric pass: crop -> GaussNoise -> GaussianBlur (separable, float64 taps in order, float32 after each pass) -> brightness / contrast
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ftaug_photometric_kernel(const float* __restrict__ src, int H, int W, const CmuFtAugRec* __restrict__ recs,
                                                               const double* __restrict__ noise, uint64_t seed, uint64_t offset, int clip,
                                                               float* __restrict__ out, int S) {
    __shared__ float tin[FTA_IN][FTA_IN + 1];
    __shared__ float tmid[FTA_IN][FTA_TILE + 1];
    __shared__ double wts[FTA_MAX_K];
    const int b = blockIdx.z, ty0 = blockIdx.y * FTA_TILE, tx0 = blockIdx.x * FTA_TILE;
    const CmuFtAugRec rec = recs[b];
    const FtaView v = fta_view(rec, H, W, S);
    const bool blur = v.ops & FA_BLUR;
    const int k = blur ? v.k : 1, h = (k - 1) / 2;
    const int th = min(FTA_TILE, S - ty0), tw = min(FTA_TILE, S - tx0);
    const int nr = th + 2 * h, nc = tw + 2 * h;
    if (blur && threadIdx.x == 0) {
        // OpenCV getGaussianKernel: t_i = exp(-0.5 / sigma^2 * x_i^2), x_i = i - (k - 1) / 2, w_i = t_i * (1 / sum t)
        const double scale2 = __ddiv_rn(-0.5, __dmul_rn(rec.sigma, rec.sigma));
        double sum = 0.0;
        for (int i = 0; i < k; ++i) {
            const double x = __dadd_rn((double)i, -__dmul_rn((double)(k - 1), 0.5));
            wts[i] = exp(__dmul_rn(__dmul_rn(scale2, x), x));
            sum = __dadd_rn(sum, wts[i]);
        }
        const double inv = __ddiv_rn(1.0, sum);
        for (int i = 0; i < k; ++i) wts[i] = __dmul_rn(wts[i], inv);
    }
    const float* img = src + ((int64_t)b * H + v.y0) * W + v.x0;
    const double sd = (v.ops & FA_NOISE) ? sqrt(rec.var_noise) : 0.0;
    for (int i = threadIdx.x; i < nr * nc; i += 256) {
        const int r = i / nc, c = i % nc;
        const int y = reflect101(ty0 - h + r, S), x = reflect101(tx0 - h + c, S);
        float a = img[(int64_t)y * W + x];
        if (v.ops & FA_NOISE) {
            const int64_t pix = (int64_t)y * S + x;
            a = fta_add_noise(a, sd, noise ? noise[(int64_t)b * S * S + pix] : fta_normal(seed, offset, FS_NOISE, b, pix), clip);
        }
        tin[r][c] = a;
    }
    __syncthreads();
    if (blur) {
        for (int i = threadIdx.x; i < nr * tw; i += 256) {
            const int r = i / tw, c = i % tw;
            double acc = 0.0;
            for (int t = 0; t < k; ++t) acc = __dadd_rn(acc, __dmul_rn(wts[t], (double)tin[r][c + t]));
            tmid[r][c] = (float)acc;
        }
        __syncthreads();
    }
    const float alpha = (float)rec.alpha, beta = (float)rec.beta;
    for (int i = threadIdx.x; i < th * tw; i += 256) {
        const int r = i / tw, c = i % tw;
        float a;
        if (blur) {
            double acc = 0.0;
            for (int t = 0; t < k; ++t) acc = __dadd_rn(acc, __dmul_rn(wts[t], (double)tmid[r + t][c]));
            a = (float)acc;
        } else {
            a = tin[r][c];
        }
        if (v.ops & FA_BC) {
            a = __fadd_rn(__fmul_rn(a, alpha), beta);            // img * alpha + beta * max_value, float32
            if (clip) a = fminf(fmaxf(a, 0.f), 1.f);
        }
        out[((int64_t)b * S + ty0 + r) * S + tx0 + c] = a;
    }
}
static int fta_check(const char* name, int B, int H, int W, int S) {
    CMU_CHECK_ARG(B > 0 && S > 0 && H >= S && W >= S && (int64_t)S * S < (1ll << 31), "%s: bad shape (B %d, %dx%d, crop %d)", name, B, H, W, S);
    return CMU_OK;
}
extern "C" int cmu_ftaug_photometric(const float* src, int B, int H, int W, const void* recs, const double* noise, uint64_t seed, uint64_t offset,
                                     int clip, float* out, int S, void* stream) {
    CMU_CHECK_ARG(src && recs && out, "cmu_ftaug_photometric: null pointer");
    if (int e = fta_check("cmu_ftaug_photometric", B, H, W, S)) return e;
    const dim3 grid(cmu_div_up(S, FTA_TILE), cmu_div_up(S, FTA_TILE), B);
    hipLaunchKernelGGL(ftaug_photometric_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, H, W, (const CmuFtAugRec*)recs, noise, seed,
                       offset, clip, out, S);
    CMU_CHECK_LAUNCH("cmu_ftaug_photometric");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// A and the augmented mask, materialised (B, S, S)
// ---------------------------------------------------------------------------------------------
__global__ void ftaug_apply_kernel(const float* __restrict__ P, const uint8_t* __restrict__ masks, int H, int W, const CmuFtAugRec* __restrict__ recs,
                                   const double* __restrict__ noise, uint64_t seed, uint64_t offset, int clip, float* __restrict__ img_out,
                                   uint8_t* __restrict__ mask_out, int S, int64_t total) {
    const int64_t plane = total;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % S), y = (int)((i / S) % S), b = (int)(i / ((int64_t)S * S));
        const CmuFtAugRec& rec = recs[b];
        const FtaView v = fta_view(rec, H, W, S);
        img_out[i] = fta_read(P, v, S, b, y, x, sqrt(rec.var_oneof), noise, plane, seed, offset, clip);
        mask_out[i] = fta_mask(masks, v, H, W, S, b, y, x);
    }
}
extern "C" int cmu_ftaug_apply(const float* aug, const uint8_t* masks, int B, int H, int W, const void* recs, const double* noise, uint64_t seed,
                               uint64_t offset, int clip, float* img_out, uint8_t* mask_out, int S, void* stream) {
    CMU_CHECK_ARG(aug && masks && recs && img_out && mask_out, "cmu_ftaug_apply: null pointer");
    if (int e = fta_check("cmu_ftaug_apply", B, H, W, S)) return e;
    const int64_t t = (int64_t)B * S * S;
    const int g = (int)(cmu_div_up64(t, 256) < 16384 ? cmu_div_up64(t, 256) : 16384);
    hipLaunchKernelGGL(ftaug_apply_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, aug, masks, H, W, (const CmuFtAugRec*)recs, noise, seed,
                       offset, clip, img_out, mask_out, S, t);
    CMU_CHECK_LAUNCH("cmu_ftaug_apply");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// the resize tail: Pillow bicubic (augment.hip's arithmetic, pillow_resample.h) with A composed into the horizontal pass's reads; the
// vertical pass also writes the one-hot of the NEAREST-resized augmented mask.  Both axes have the same sizes, so one table serves
// both passes: per output index the window start, its length and the normalised coefficients (the values aug_coeff returns, computed
// once instead of per output pixel), plus Pillow's NEAREST source indices.  ws = tables, then tmp (B, S, size) f32.
// ---------------------------------------------------------------------------------------------
constexpr int FTA_MAX_TAPS = 32;
struct FtaCoef {
    int xmin, count;
    double c[FTA_MAX_TAPS];
};
struct FtaClasses {
    int n;
    int v[FTA_MAX_CLASSES];
};
static inline int64_t fta_tables_bytes(int size) { return (int64_t)size * (int64_t)sizeof(FtaCoef) + 2 * (int64_t)size * (int64_t)sizeof(int); }
__global__ __launch_bounds__(256) void ftaug_tables_kernel(FtaCoef* __restrict__ coef, int* __restrict__ near, int S, int size) {
    for (int i = threadIdx.x; i < size; i += 256) {
        const AugWin win = aug_window(i, S, size);
        FtaCoef& cf = coef[i];
        cf.xmin = win.xmin;
        cf.count = min(win.count, FTA_MAX_TAPS);      // (the host checks that the window fits)
        for (int x = 0; x < cf.count; ++x) cf.c[x] = aug_coeff(win, x);
    }
    if (threadIdx.x == 0) {
        // Pillow's NEAREST source index: int(x) of the running double x = scale / 2, += scale
        const double scale = __ddiv_rn((double)S, (double)size);
        double xo = __dmul_rn(scale, 0.5);
        for (int x = 0; x < size; ++x) {
            const int q = xo < 0.0 ? -1 : (int)xo;
            near[x] = min(max(q, 0), S - 1);
            xo = __dadd_rn(xo, scale);
        }
    }
}
__global__ void ftaug_resize_h_kernel(const float* __restrict__ P, int H, int W, const CmuFtAugRec* __restrict__ recs, const double* __restrict__ noise,
                                      uint64_t seed, uint64_t offset, int clip, const FtaCoef* __restrict__ coef, float* __restrict__ tmp, int S,
                                      int size, int64_t total) {
    const int64_t plane = total / size * S;      // B * S * S: where the OneOf noise plane of an explicit noise input starts
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % size), y = (int)((i / size) % S), b = (int)(i / ((int64_t)size * S));
        const CmuFtAugRec& rec = recs[b];
        const FtaView v = fta_view(rec, H, W, S);
        const double s1 = sqrt(rec.var_oneof);
        float r;
        if (S == size) {
            r = fta_read(P, v, S, b, y, xx, s1, noise, plane, seed, offset, clip);
        } else {
            const FtaCoef& cf = coef[xx];
            double ss = 0.0;
            for (int x = 0; x < cf.count; ++x)
                ss = __dadd_rn(ss, __dmul_rn((double)fta_read(P, v, S, b, y, cf.xmin + x, s1, noise, plane, seed, offset, clip), cf.c[x]));
            r = (float)ss;
        }
        tmp[i] = r;
    }
}
__global__ void ftaug_resize_v_kernel(const float* __restrict__ tmp, const FtaCoef* __restrict__ coef, const int* __restrict__ near,
                                      const uint8_t* __restrict__ masks, int H, int W, const CmuFtAugRec* __restrict__ recs, FtaClasses cls,
                                      float* __restrict__ img_out, double* __restrict__ onehot, int S, int size, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % size), yy = (int)((i / size) % size), b = (int)(i / ((int64_t)size * size));
        const float* col = tmp + (int64_t)b * S * size + xx;
        float r;
        if (S == size) {
            r = col[(int64_t)yy * size];
        } else {
            const FtaCoef& cf = coef[yy];
            double ss = 0.0;
            for (int y = 0; y < cf.count; ++y) ss = __dadd_rn(ss, __dmul_rn((double)col[(int64_t)(cf.xmin + y) * size], cf.c[y]));
            r = (float)ss;
        }
        img_out[i] = r;
        const FtaView v = fta_view(recs[b], H, W, S);
        const int lab = fta_mask(masks, v, H, W, S, b, near[yy], near[xx]);
        double* oh = onehot + (int64_t)b * cls.n * size * size + (int64_t)yy * size + xx;
        for (int c = 0; c < cls.n; ++c) oh[(int64_t)c * size * size] = lab == cls.v[c] ? 1.0 : 0.0;
    }
}
extern "C" int64_t cmu_ftaug_resize_ws_bytes(int B, int S, int size) {
    return fta_tables_bytes(size) + (int64_t)B * S * size * (int64_t)sizeof(float);
}
extern "C" int cmu_ftaug_resize_onehot(const float* aug, const uint8_t* masks, int B, int H, int W, const void* recs, const double* noise,
                                       uint64_t seed, uint64_t offset, int clip, const int* class_values, int ncls, float* img_out,
                                       double* onehot, int S, int size, void* ws, void* stream) {
    CMU_CHECK_ARG(aug && masks && recs && img_out && onehot && ws && class_values && size > 0, "cmu_ftaug_resize_onehot: bad args");
    if (int e = fta_check("cmu_ftaug_resize_onehot", B, H, W, S)) return e;
    CMU_CHECK_ARG(ncls >= 1 && ncls <= FTA_MAX_CLASSES, "cmu_ftaug_resize_onehot: %d classes (1 .. %d)", ncls, FTA_MAX_CLASSES);
    // a Pillow window spans at most 2 * support + 2 source indices, support = 2 * max(S / size, 1)
    const double support = 2.0 * (S > size ? (double)S / size : 1.0);
    CMU_CHECK_ARG(2.0 * support + 2.0 <= FTA_MAX_TAPS, "cmu_ftaug_resize_onehot: %d -> %d needs more than %d taps", S, size, FTA_MAX_TAPS);
    FtaClasses cls;
    cls.n = ncls;
    for (int c = 0; c < FTA_MAX_CLASSES; ++c) cls.v[c] = c < ncls ? class_values[c] : -1;
    FtaCoef* coef = (FtaCoef*)ws;
    int* near = (int*)((char*)ws + (int64_t)size * (int64_t)sizeof(FtaCoef));
    float* tmp = (float*)((char*)ws + fta_tables_bytes(size));
    const int64_t t1 = (int64_t)B * S * size, t2 = (int64_t)B * size * size;
    const int g1 = (int)(cmu_div_up64(t1, 256) < 16384 ? cmu_div_up64(t1, 256) : 16384);
    const int g2 = (int)(cmu_div_up64(t2, 256) < 16384 ? cmu_div_up64(t2, 256) : 16384);
    hipLaunchKernelGGL(ftaug_tables_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, coef, near, S, size);
    CMU_CHECK_LAUNCH("cmu_ftaug_resize_onehot(tables)");
    hipLaunchKernelGGL(ftaug_resize_h_kernel, dim3(g1), dim3(256), 0, (hipStream_t)stream, aug, H, W, (const CmuFtAugRec*)recs, noise, seed, offset,
                       clip, (const FtaCoef*)coef, tmp, S, size, t1);
    CMU_CHECK_LAUNCH("cmu_ftaug_resize_onehot(horizontal)");
    hipLaunchKernelGGL(ftaug_resize_v_kernel, dim3(g2), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, (const FtaCoef*)coef, (const int*)near,
                       masks, H, W, (const CmuFtAugRec*)recs, cls, img_out, onehot, S, size, t2);
    CMU_CHECK_LAUNCH("cmu_ftaug_resize_onehot(vertical)");
    return CMU_OK;
}
