// prob_hist.hip -- choosing the operating point of a segmentation head on the device (no reference counterpart:
// the reference fixes the threshold at 0.5):
//   cmu_prob_hist       one streaming pass: per (image or pool, class) the histogram of the predicted probability, split by ground truth,
//                       plus the fixed-point sum of the probabilities of every bin -- integers only, the same bits on every call;
//   cmu_hist_curves     from the histogram: the confusion counts at every threshold j / NB (a suffix scan), the reference's scores there,
//                       AUROC, average precision, ECE / MCE and the best threshold (csrc/hist_curves.h);
//   cmu_threshold_mask  p > t ? v_pos : v_neg, element-wise.
// The probability of logits is the bits of seg_softmax (seg_softmax.h, the one cmu_seg_stats_fwd thresholds) for K >= 2 and head_prob's
// sigmoid (head_math.h) for K = 1, so the suffix sums at j ARE the integers cmu_seg_stats_fwd counts at threshold j / NB.
#include <type_traits>

#include "common.h"
#include "head_math.h"
#include "hist_curves.h"
#include "plane_stream.h"
#include "seg_softmax.h"

constexpr int PH_MAX_K = 8;
constexpr int PH_THREADS = 1024;      // lanes of a workgroup
constexpr int PH_MAX_BLOCKS = 256;    // workgroups of a launch (one per CU): every one flushes its non-zero bins with global atomics
// LDS budget of a workgroup: 16 bytes per (class, bin) -- 2 x 4 (the uint32 counts of the two ground-truth values) + 8 (the uint64 sum of
// floor(p * 2^32)) -- plus 8 invalid-value counters.  K' = 8 at NB = 1024 would be 131 KB (one workgroup per CU, and past the 64 KB a
// launch may ask for without an attribute); the classes are therefore taken in groups of G = min(K', 65472 / (16 (NB + 1))) per pass
// over the pixels: all 8 up to NB = 256 (32.9 KB), 7 at NB = 512, 3 at NB = 1024.
constexpr int PH_LDS_BYTES = 65536;
constexpr int PH_LDS_TAIL = 64;
// Diagnostic builds only (tools/build_variant.sh ... "-DPH_AGGREGATE=0"): one LDS atomic pair per pixel instead of one per run of equal keys,
// the baseline the run aggregation was measured against.
#ifndef PH_AGGREGATE
#define PH_AGGREGATE 1
#endif

// TY: float / double one-hot planes of src's shape (positive iff y > 0.5) or uint8_t, a (B,H,W) label map (class c positive for row c only;
// a one-plane src: label != 0).  A lane takes V consecutive pixels of every plane; grid.y = 1 pools all B images into row 0, else grid.y = B
// and a workgroup stays inside image blockIdx.y.  Contention: a lane keeps, per class, the run of equal consecutive (target, bin) keys in
// registers and touches the LDS histogram only when the key changes -- on vessel images, where > 90 % of a class's pixels share a bin,
// that is one LDS atomic per ~10 pixels instead of 64 lanes serialised on one address for every pixel.
template <int KT, int V, typename TY>
__global__ __launch_bounds__(PH_THREADS) void prob_hist_kernel(const float* __restrict__ src, const TY* __restrict__ tgt, int from_logits,
                                                              unsigned long long* __restrict__ counts, unsigned long long* __restrict__ conf,
                                                              int* __restrict__ invalid, int K, int NB, int G, int64_t HW, int64_t ngroups) {
    extern __shared__ unsigned long long ph_lds[];
    constexpr bool LABELS = std::is_same<TY, uint8_t>::value;
    const int NB1 = NB + 1;
    unsigned long long* sconf = ph_lds;                                          // [G][NB1]
    unsigned* scnt = reinterpret_cast<unsigned*>(ph_lds + (size_t)G * NB1);      // [G][2][NB1]
    unsigned* sinv = scnt + (size_t)G * 2 * NB1;                                 // [PH_MAX_K]
    const bool pooled = gridDim.y == 1;
    const int64_t b0 = pooled ? 0 : blockIdx.y;
    const int64_t gpi = HW / V;
    const bool small = ngroups < (int64_t(1) << 31);
    const float fnb = (float)NB;

    for (int c0 = 0; c0 < K; c0 += G) {
        const int Gc = K - c0 < G ? K - c0 : G;
        for (int i = threadIdx.x; i < Gc * NB1; i += blockDim.x) sconf[i] = 0ull;
        for (int i = threadIdx.x; i < Gc * 2 * NB1; i += blockDim.x) scnt[i] = 0u;
        if (threadIdx.x < PH_MAX_K) sinv[threadIdx.x] = 0u;
        __syncthreads();

        int rk[KT];                    // the pending run of class c: key = target * NB1 + bin, length, sum of floor(p * 2^32)
        unsigned rn[KT], ninv[KT];
        unsigned long long rq[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            rk[c] = -1;
            rn[c] = ninv[c] = 0u;
            rq[c] = 0ull;
        }
        for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
            // plane_group_base's split, written out: the image index takes b0 before the multiply, and the label map needs (b, r) too
            int64_t b, r;
            if (small) {
                const unsigned gu = (unsigned)g, bu = gu / (unsigned)gpi;
                b = bu;
                r = gu - bu * (unsigned)gpi;
            } else {
                b = g / gpi;
                r = g - b * gpi;
            }
            b += b0;
            const int64_t base = b * K * HW + r * V;
            PlaneVec<float, V> lv[KT];
            PlaneVec<TY, V> yv[LABELS ? 1 : KT];
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < K) {
                    lv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(src + base + c * HW);
                    if (!LABELS) yv[LABELS ? 0 : c] = *reinterpret_cast<const PlaneVec<TY, V>*>(tgt + base + c * HW);
                }
            if (LABELS) yv[0] = *reinterpret_cast<const PlaneVec<TY, V>*>(tgt + b * HW + r * V);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float l[KT], p[KT], lse;
#pragma unroll
                for (int c = 0; c < KT; ++c) l[c] = c < K ? lv[c].v[v] : 0.f;
                if (!from_logits) {
#pragma unroll
                    for (int c = 0; c < KT; ++c) p[c] = l[c];
                } else if (K == 1) {
                    p[0] = head_prob<KT>(l, l[0], 1, 0);
                } else {
                    seg_softmax<KT>(l, K, p, lse);
                }
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (c < K && c >= c0 && c < c0 + G) {
                        float pc = p[c];
                        if (!(pc >= 0.f && pc <= 1.f)) {      // NaN, negative: 0; above 1, +inf: 1 -- counted as invalid (-0.0 is 0)
                            pc = pc > 1.f ? 1.f : 0.f;
                            ++ninv[c];
                        }
                        const int bin = (int)ceilf(pc * fnb);      // exact product: bin b holds (b - 1) / NB < p <= b / NB, bin 0 holds p == 0
                        const unsigned long long q = (unsigned long long)(pc * 4294967296.f);
                        bool positive;
                        if (LABELS)
                            positive = K == 1 ? yv[0].v[v] != 0 : (int)yv[0].v[v] == c;
                        else
                            positive = yv[LABELS ? 0 : c].v[v] > (TY)0.5;
                        const int key = positive ? bin + NB1 : bin;
                        if (PH_AGGREGATE && key == rk[c]) {
                            ++rn[c];
                            rq[c] += q;
                        } else {
                            if (rn[c]) {
                                atomicAdd(&scnt[(c - c0) * 2 * NB1 + rk[c]], rn[c]);
                                atomicAdd(&sconf[(c - c0) * NB1 + (rk[c] >= NB1 ? rk[c] - NB1 : rk[c])], rq[c]);
                            }
                            rk[c] = key;
                            rn[c] = 1u;
                            rq[c] = q;
                        }
                    }
            }
        }
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K && c >= c0 && c < c0 + G) {
                if (rn[c]) {
                    atomicAdd(&scnt[(c - c0) * 2 * NB1 + rk[c]], rn[c]);
                    atomicAdd(&sconf[(c - c0) * NB1 + (rk[c] >= NB1 ? rk[c] - NB1 : rk[c])], rq[c]);
                }
                if (ninv[c]) atomicAdd(&sinv[c], ninv[c]);
            }
        __syncthreads();
        // one 64-bit integer atomic per non-zero bin of the workgroup: integer sums do not depend on the arrival order
        const int64_t row0 = (int64_t)blockIdx.y * K + c0;
        for (int i = threadIdx.x; i < Gc * 2 * NB1; i += blockDim.x) {
            const unsigned n = scnt[i];
            if (n) atomicAdd(&counts[row0 * 2 * NB1 + i], (unsigned long long)n);
        }
        for (int i = threadIdx.x; i < Gc * NB1; i += blockDim.x) {
            const unsigned long long s = sconf[i];
            if (s) atomicAdd(&conf[row0 * NB1 + i], s);
        }
        if ((int)threadIdx.x < Gc && sinv[c0 + threadIdx.x]) atomicAdd(&invalid[row0 + threadIdx.x], (int)sinv[c0 + threadIdx.x]);
        __syncthreads();
    }
}

template <int KT, int V, typename TY>
static void prob_hist_launch(const float* src, const void* tgt, int from_logits, void* counts, void* conf, int* invalid, int K, int NB, int G,
                             int64_t HW, int64_t ngroups, dim3 grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((prob_hist_kernel<KT, V, TY>), grid, dim3(PH_THREADS), lds, st, src, (const TY*)tgt, from_logits,
                       (unsigned long long*)counts, (unsigned long long*)conf, invalid, K, NB, G, HW, ngroups);
}
// an INNER of PLANE_DISPATCH: the launch for the runtime target kind (0 fp32 planes, 1 fp64 planes, 2 uint8 labels)
#define PH_DISPATCH_TY(KT, V, kind, ...)                                          \
    do {                                                                          \
        if ((kind) == 0) prob_hist_launch<KT, V, float>(__VA_ARGS__);             \
        else if ((kind) == 1) prob_hist_launch<KT, V, double>(__VA_ARGS__);       \
        else prob_hist_launch<KT, V, uint8_t>(__VA_ARGS__);                       \
    } while (0)

static inline bool ph_pow2_bins(int NB) { return NB >= 2 && NB <= HC_MAX_BINS && (NB & (NB - 1)) == 0; }

extern "C" int cmu_prob_hist(const float* src, int from_logits, const void* target, int target_kind, int64_t* counts, uint64_t* conf,
                             int32_t* invalid, int B, int K, int H, int W, int NB, int pooled, int accumulate, void* stream) {
    CMU_CHECK_ARG(src && target && counts && conf && invalid && B > 0 && H > 0 && W > 0, "cmu_prob_hist: bad args");
    CMU_CHECK_ARG(K >= 1 && K <= PH_MAX_K, "cmu_prob_hist: 1 <= K <= %d planes (got %d)", PH_MAX_K, K);
    CMU_CHECK_ARG(ph_pow2_bins(NB), "cmu_prob_hist: NB must be a power of two in 2..%d (got %d)", HC_MAX_BINS, NB);
    CMU_CHECK_ARG(target_kind >= 0 && target_kind <= 2 && (from_logits == 0 || from_logits == 1) && (pooled == 0 || pooled == 1) &&
                      (accumulate == 0 || accumulate == 1),
                  "cmu_prob_hist: target_kind is 0 (fp32 planes), 1 (fp64 planes) or 2 (uint8 labels); the flags are 0 or 1");
    CMU_CHECK_ARG(pooled || B <= 65535, "cmu_prob_hist: at most 65535 images with per-image rows (got %d)", B);
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    // plane_width's rule, but a uint8 label map is aligned to its own V bytes, not 16
    const int VV = K > 4 ? 2 : 4;
    const size_t talign = target_kind == 2 ? (size_t)VV : 16;
    const bool vec = HW % VV == 0 && cmu_aligned16(src) && reinterpret_cast<uintptr_t>(target) % talign == 0;
    const int V = vec ? VV : 1;
    const int Bout = pooled ? 1 : B;
    const int64_t ngroups = (pooled ? (int64_t)B : 1) * (HW / V);
    int64_t gx = cmu_div_up64(ngroups, PH_THREADS);
    const int64_t cap = PH_MAX_BLOCKS / Bout > 0 ? PH_MAX_BLOCKS / Bout : 1;
    gx = gx < cap ? gx : cap;
    // a bin of a workgroup's LDS histogram is a uint32: the pixels one workgroup takes must stay below 2^32
    CMU_CHECK_ARG((ngroups / gx + PH_THREADS) * V < (int64_t(1) << 32), "cmu_prob_hist: %lld pixels per workgroup overflow a 32-bit bin",
                  (long long)((ngroups / gx + PH_THREADS) * V));
    const int NB1 = NB + 1;
    const int fit = (PH_LDS_BYTES - PH_LDS_TAIL) / (16 * NB1);
    const int G = K < fit ? K : fit;
    const size_t lds = (size_t)G * NB1 * 16 + PH_MAX_K * sizeof(unsigned);
    if (!accumulate) {
        const size_t rows = (size_t)Bout * K;
        if (hipMemsetAsync(counts, 0, rows * 2 * NB1 * sizeof(int64_t), st) != hipSuccess ||
            hipMemsetAsync(conf, 0, rows * NB1 * sizeof(uint64_t), st) != hipSuccess ||
            hipMemsetAsync(invalid, 0, rows * sizeof(int32_t), st) != hipSuccess) {
            (void)hipGetLastError();
            cmu_set_error("cmu_prob_hist: zeroing the outputs failed");
            return CMU_ERR_LAUNCH;
        }
    }
    const dim3 grid((unsigned)gx, (unsigned)Bout);
    PLANE_DISPATCH(PH_DISPATCH_TY, K, vec, target_kind, src, target, from_logits, counts, conf, invalid, K, NB, G, HW, ngroups, grid, lds, st);
    CMU_CHECK_LAUNCH("cmu_prob_hist");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// cmu_hist_curves: one workgroup per histogram row.  LDS: pos, neg, conf (3 n) + cum (4 n) 64-bit words + 2 x 256 chunk sums: 61.5 KB at
// NB = 1024.  The scan is integer (chunk sums, then every lane scans its own chunk from the sum of the chunks above it: no order to
// respect); the scores are one lane per threshold; the summaries are ONE lane's sums in ascending bin order (hist_curves.h).
// ---------------------------------------------------------------------------------------------
constexpr int HCK_THREADS = 256;
__global__ __launch_bounds__(HCK_THREADS) void hist_curves_kernel(const int64_t* __restrict__ counts, const uint64_t* __restrict__ conf, int NB,
                                                                 double eps, double beta, int select, int64_t* __restrict__ cum,
                                                                 double* __restrict__ scores, double* __restrict__ summary) {
    extern __shared__ unsigned long long hc_lds[];
    const int n = NB + 1, t = threadIdx.x;
    int64_t* pos = reinterpret_cast<int64_t*>(hc_lds);
    int64_t* neg = pos + n;
    uint64_t* cf = reinterpret_cast<uint64_t*>(neg + n);
    int64_t* cm = reinterpret_cast<int64_t*>(cf + n);
    int64_t* cs_pos = cm + 4 * n;
    int64_t* cs_neg = cs_pos + HCK_THREADS;
    const int64_t row = blockIdx.x;
    for (int i = t; i < n; i += HCK_THREADS) {
        neg[i] = counts[row * 2 * n + i];
        pos[i] = counts[row * 2 * n + n + i];
        cf[i] = conf ? conf[row * n + i] : 0ull;
    }
    __syncthreads();
    int lo, hi;
    hc_chunk_bounds(t, HCK_THREADS, n, &lo, &hi);
    int64_t sp = 0, sn = 0;
    for (int i = lo; i < hi; ++i) {
        sp += pos[i];
        sn += neg[i];
    }
    cs_pos[t] = sp;
    cs_neg[t] = sn;
    __syncthreads();
    int64_t P = 0, N = 0, tail_p = 0, tail_n = 0;
    for (int u = 0; u < HCK_THREADS; ++u) {
        P += cs_pos[u];
        N += cs_neg[u];
        if (u > t) {
            tail_p += cs_pos[u];
            tail_n += cs_neg[u];
        }
    }
    hc_scan_chunk(pos, neg, lo, hi, tail_p, tail_n, P, N, n, cm);
    __syncthreads();
    for (int j = t; j < n; j += HCK_THREADS) {
        double s[HC_SCORES];
        hc_scores(cm[j], cm[n + j], cm[2 * n + j], cm[3 * n + j], eps, beta, s);
#pragma unroll
        for (int q = 0; q < 4; ++q) cum[(row * 4 + q) * n + j] = cm[q * n + j];
#pragma unroll
        for (int q = 0; q < HC_SCORES; ++q) scores[(row * HC_SCORES + q) * n + j] = s[q];
    }
    if (t == 0) hc_summary(pos, neg, conf ? cf : nullptr, cm, NB, eps, beta, select, summary + row * HC_SUMMARY);
}

extern "C" int cmu_hist_curves(const int64_t* counts, const uint64_t* conf, int rows, int NB, double eps, double beta, int select,
                               int64_t* cum, double* scores, double* summary, void* stream) {
    CMU_CHECK_ARG(counts && cum && scores && summary && rows > 0, "cmu_hist_curves: bad args");
    CMU_CHECK_ARG(ph_pow2_bins(NB), "cmu_hist_curves: NB must be a power of two in 2..%d (got %d)", HC_MAX_BINS, NB);
    CMU_CHECK_ARG(select >= 0 && select <= 2 && eps >= 0.0 && beta > 0.0,
                  "cmu_hist_curves: select is 0 (F-beta), 1 (IoU) or 2 (Youden); eps >= 0 and beta > 0");
    const size_t lds = ((size_t)7 * (NB + 1) + 2 * HCK_THREADS) * sizeof(int64_t);
    hipLaunchKernelGGL(hist_curves_kernel, dim3(rows), dim3(HCK_THREADS), lds, (hipStream_t)stream, counts, conf, NB, eps, beta, select, cum,
                       scores, summary);
    CMU_CHECK_LAUNCH("cmu_hist_curves");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// cmu_threshold_mask: out = p > t ? v_pos : v_neg (NaN: v_neg).  16 probabilities per lane (four 16-byte loads, one 16-byte store) when the
// element count is a multiple of 16 and both pointers are 16-byte aligned, one per lane otherwise -- decided for the whole tensor.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void threshold_mask16_kernel(const float4* __restrict__ p, float t, unsigned vp, unsigned vn,
                                                              uint4* __restrict__ out, int64_t n16) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 f = p[i * 4 + k];
            w[k] = (f.x > t ? vp : vn) | (f.y > t ? vp : vn) << 8 | (f.z > t ? vp : vn) << 16 | (f.w > t ? vp : vn) << 24;
        }
        out[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}
__global__ __launch_bounds__(256) void threshold_mask1_kernel(const float* __restrict__ p, float t, unsigned vp, unsigned vn,
                                                             uint8_t* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (uint8_t)(p[i] > t ? vp : vn);
}
extern "C" int cmu_threshold_mask(const float* prob, float threshold, int v_pos, int v_neg, uint8_t* out, int64_t n, void* stream) {
    CMU_CHECK_ARG(prob && out && n > 0, "cmu_threshold_mask: bad args");
    CMU_CHECK_ARG(v_pos >= 0 && v_pos <= 255 && v_neg >= 0 && v_neg <= 255, "cmu_threshold_mask: v_pos and v_neg are bytes (got %d, %d)", v_pos, v_neg);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n % 16 == 0 && cmu_aligned16(prob) && cmu_aligned16(out);
    const int64_t items = vec ? n / 16 : n, blocks = cmu_div_up64(items, 256);
    const int grid = (int)(blocks < 4096 ? blocks : 4096);
    if (vec)
        hipLaunchKernelGGL(threshold_mask16_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4*>(prob), threshold, (unsigned)v_pos,
                           (unsigned)v_neg, reinterpret_cast<uint4*>(out), items);
    else
        hipLaunchKernelGGL(threshold_mask1_kernel, dim3(grid), dim3(256), 0, st, prob, threshold, (unsigned)v_pos, (unsigned)v_neg, out, items);
    CMU_CHECK_LAUNCH("cmu_threshold_mask");
    return CMU_OK;
}
