// map_loss.hip -- losses for thin, rare foregrounds on (B,K,H,W) fp32 logits, 2 <= K <= 8 (no reference
// counterpart): the focal cross entropy (Lin et al.), the map-weighted softmax sums behind the boundary loss (Kervadec et al.) and the
// Hausdorff distance-transform loss (Karimi & Salcudean, as MONAI's HausdorffDTLoss states it), and the distance fields those two take
// from the integer squared distances of cmu_edt_rows (edt.hip).
// Streaming passes under the contract of plane_stream.h; p is seg_softmax<>() (seg_softmax.h: the probability bits of the counters and
// the histogram).
#include "common.h"
#include "plane_stream.h"
#include "seg_softmax.h"
#include "map_loss_math.h"

constexpr int ML_MAX_K = 8;
// The unnormalised exponentials behind seg_softmax's p, e_c = e^(l_c - max) -- its statements again, so the compiler merges the two --,
// the first maximum am (e_am is exactly 1) and the sum of the OTHER e_c, in fp32 class order (rest32: what ice_log_softmax of
// pointwise_loss.hip feeds log1p) and in fp64 (rest64: exact to 2^-53); sum_c e_c = rest64 + 1.
template <int KT>
__device__ static inline void ml_exps(const float (&l)[KT], int K, float (&e)[KT], int& am, float& m, float& rest32, double& rest64) {
    m = l[0];
#pragma unroll
    for (int c = 1; c < KT; ++c)
        if (c < K) m = fmaxf(m, l[c]);
    am = -1;
#pragma unroll
    for (int c = 0; c < KT; ++c)
        if (c < K && am < 0 && l[c] == m) am = c;
    rest32 = 0.f;
    rest64 = 0.0;
#pragma unroll
    for (int c = 0; c < KT; ++c)
        if (c < K) {
            const float x = l[c] - m;
            const float d = (float)(((double)l[c] - (double)m) - (double)x);
            const float ex = expf(x);
            e[c] = fmaf(ex, d, ex);
            if (c != am) {
                rest32 += e[c];
                rest64 += (double)e[c];
            }
        }
}
// sum of e_j over j != c without cancellation: the maximum's own complement is rest64; any other class's complement holds the
// maximum's 1, so (rest64 + 1) - e_c >= 1 keeps every bit that matters
__device__ static inline double ml_others(int c, int am, float ec, double rest64) { return c == am ? rest64 : (rest64 + 1.0) - (double)ec; }
// 1 / s in fp64 for 2^-100 <= s <= 2^100: the fp32 reciprocal instruction (1 ulp) and one Newton step, relative error below 2^-44 --
// two fp64 operations where a division is a dozen at the fp64 rate, which these passes would otherwise wait for
__device__ static inline double ml_rcp(double s) {
    const double r = (double)__builtin_amdgcn_rcpf((float)s);
    return r * (2.0 - s * r);
}

static inline int ml_check_shape(const char* who, int B, int K, int H, int W) {
    CMU_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad args", who);
    CMU_CHECK_ARG(K >= 2 && K <= ML_MAX_K, "%s: 2 <= K <= %d classes (got %d)", who, ML_MAX_K, K);
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// (a) focal cross entropy.  With t the pixel's label, e_c = e^(l_c - max) (the rounding of the fp32 difference given back, as
// seg_softmax has it) and q = 1 - p_t:
//   -log p_t = (max - l_t) + log1p(sum of the e_c other than the maximum's own 1): the form of ice_log_softmax (pointwise_loss.hip), the
//              same bits, so with gamma = 0 the sums are those of cmu_index_ce_fwd;
//   q        = (sum of e_c, c != t) / (sum of e_c), both sums in fp64 and the quotient through ml_rcp: never 1 - p_t, which would leave
//              a confident pixel without a single bit;
//   q^gamma  : cmu_ml_pow_gamma (map_loss_math.h).
// term = alpha_t q^gamma (-log p_t).  With n = -log p_t and C = gamma p_t n q^gamma the gradient
//   dl_j = g alpha_t (d_jt - p_j) (gamma p_t q^(gamma-1) log p_t - q^gamma)
// is evaluated as  j == t: -g alpha_t (C + q q^gamma)   [d_tt - p_t = q]
//                  j != t:  g alpha_t ((e_j / sum_{c != t} e_c) C + p_j q^gamma)   [p_j q^(gamma-1) = (e_j / sum) q^gamma; 0 / 0 := 0]
// so nothing is inf * 0 at q = 0 with gamma < 1, and both addends of every element have one sign: no cancellation.
// The target kinds are those of cmu_index_ce_fwd (CMU_ICE_*); the arg-max of one-hot planes runs over all K channels (ALL_KEPT).  A label
// outside [0, K) that is not ignore_index is never used as an index: NaN into table[0], a zero gradient.
// ---------------------------------------------------------------------------------------------
// one pixel with label t in [0, K): p = seg_softmax, e = the unnormalised exponentials (the statements of seg_softmax again: the
// compiler merges them), pt = p_t, nlp = -log p_t, so = sum of e_c over c != t, q = so / sum of e_c
template <int KT>
__device__ static inline void ml_focal_pixel(const float (&l)[KT], int K, int t, float (&p)[KT], float (&e)[KT], float& pt, double& nlp,
                                             double& so, double& q) {
    float lse, m, rest32, lt = 0.f, et = 0.f;
    double rest64;
    int am;
    seg_softmax<KT>(l, K, p, lse);
    ml_exps<KT>(l, K, e, am, m, rest32, rest64);
    pt = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c)
        if (c == t) {
            lt = l[c];
            pt = p[c];
            et = e[c];
        }
    nlp = ((double)m - (double)lt) + (double)log1pf(rest32);
    so = ml_others(t, am, et, rest64);
    q = so * ml_rcp(rest64 + 1.0);
}

template <int KT, int V, int TK>
__global__ __launch_bounds__(256) void ml_focal_fwd_kernel(const float* __restrict__ x, const typename PlaneTarget<TK>::T* __restrict__ tgt,
                                                          const float* __restrict__ class_w, double* __restrict__ partials, int K,
                                                          int64_t HW, int64_t ngroups, double gamma, int64_t ignore_index) {
    __shared__ double red[4];
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, wc[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) wc[c] = c < K ? (class_w ? (double)class_w[c] : 1.0) : 0.0;
    const int64_t gpi = HW / V;
    const bool small = ngroups < (int64_t(1) << 31);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = plane_group_base(g, gpi, small, K, HW, V);
        PlaneVec<float, V> xv[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) xv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(x + base + c * HW);
        int64_t lab[V];
        plane_labels<KT, V, TK, true>(tgt, g, base, K, HW, 0u, lab);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int64_t t = lab[v];
            if (t == ignore_index) continue;
            t2 += 1.0;
            if (t < 0 || t >= K) {
                t0 += __builtin_nan("");
                continue;
            }
            float l[KT], p[KT], e[KT], pt;
            double nlp, so, q, wt = 0.0;
#pragma unroll
            for (int c = 0; c < KT; ++c) {
                l[c] = c < K ? xv[c].v[v] : 0.f;
                if (c == (int)t) wt = wc[c];
            }
            ml_focal_pixel<KT>(l, K, (int)t, p, e, pt, nlp, so, q);
            t0 += (wt * cmu_ml_pow_gamma(q, gamma)) * nlp;
            t1 += wt;
        }
    }
    t0 = block_sum_d(t0, red);
    t1 = block_sum_d(t1, red);
    t2 = block_sum_d(t2, red);
    if (threadIdx.x == 0) {
        partials[0 * CE_MAX_BLOCKS + blockIdx.x] = t0;
        partials[1 * CE_MAX_BLOCKS + blockIdx.x] = t1;
        partials[2 * CE_MAX_BLOCKS + blockIdx.x] = t2;
    }
}
template <int KT, int V, int TK>
__global__ __launch_bounds__(256) void ml_focal_bwd_kernel(const float* __restrict__ x, const typename PlaneTarget<TK>::T* __restrict__ tgt,
                                                          const float* __restrict__ class_w, const double* __restrict__ g_up,
                                                          float* __restrict__ dx, int K, int64_t HW, int64_t ngroups, double gamma,
                                                          int64_t ignore_index) {
    const double g0 = g_up ? g_up[0] : 0.0;
    double wc[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) wc[c] = c < K ? (class_w ? (double)class_w[c] : 1.0) : 0.0;
    const int64_t gpi = HW / V;
    const bool small = ngroups < (int64_t(1) << 31);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = plane_group_base(g, gpi, small, K, HW, V);
        PlaneVec<float, V> xv[KT], dv[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) xv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(x + base + c * HW);
        int64_t lab[V];
        plane_labels<KT, V, TK, true>(tgt, g, base, K, HW, 0u, lab);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int64_t t = lab[v];
            if (t == ignore_index || t < 0 || t >= K) {
#pragma unroll
                for (int c = 0; c < KT; ++c) dv[c].v[v] = 0.f;
                continue;
            }
            float l[KT], p[KT], e[KT], pt;
            double nlp, so, q, wt = 0.0;
#pragma unroll
            for (int c = 0; c < KT; ++c) {
                l[c] = c < K ? xv[c].v[v] : 0.f;
                if (c == (int)t) wt = wc[c];
            }
            ml_focal_pixel<KT>(l, K, (int)t, p, e, pt, nlp, so, q);
            const double gw = g0 * wt, qg = cmu_ml_pow_gamma(q, gamma);
            const double C = gamma * (double)pt * nlp * qg;
            const double ratio = so >= 0x1p-100 ? C * ml_rcp(so) : (so > 0.0 ? C / so : 0.0);
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < K) dv[c].v[v] = c == (int)t ? (float)(-gw * (C + q * qg)) : (float)(gw * ((double)e[c] * ratio + (double)p[c] * qg));
        }
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) *reinterpret_cast<PlaneVec<float, V>*>(dx + base + c * HW) = dv[c];
    }
}

template <int KT, int V, int TK>
static void ml_focal_fwd_launch(const float* x, const void* tgt, const float* class_w, double* partials, int K, int64_t HW, int64_t npix,
                                double gamma, int64_t ignore_index, int grid, hipStream_t st) {
    hipLaunchKernelGGL((ml_focal_fwd_kernel<KT, V, TK>), dim3(grid), dim3(256), 0, st, x, (const typename PlaneTarget<TK>::T*)tgt, class_w,
                       partials, K, HW, npix / V, gamma, ignore_index);
}
template <int KT, int V, int TK>
static void ml_focal_bwd_launch(const float* x, const void* tgt, const float* class_w, const double* g, float* dx, int K, int64_t HW,
                                int64_t npix, double gamma, int64_t ignore_index, int grid, hipStream_t st) {
    hipLaunchKernelGGL((ml_focal_bwd_kernel<KT, V, TK>), dim3(grid), dim3(256), 0, st, x, (const typename PlaneTarget<TK>::T*)tgt, class_w, g, dx,
                       K, HW, npix / V, gamma, ignore_index);
}
static int ml_focal_check(const char* who, const void* x, const void* tgt, int target_kind, double gamma, int B, int K, int H, int W) {
    if (int rc = ml_check_shape(who, B, K, H, W)) return rc;
    CMU_CHECK_ARG(x && tgt, "%s: bad args", who);
    CMU_CHECK_ARG(target_kind >= CMU_ICE_LABEL_I64 && target_kind <= CMU_ICE_ONEHOT_F64, "%s: unknown target kind %d", who, target_kind);
    CMU_CHECK_ARG(gamma >= 0.0 && gamma <= 1e6, "%s: gamma must be a number in [0, 1e6] (got %g)", who, gamma);
    return CMU_OK;
}
extern "C" int cmu_focal_fwd(const float* x, const void* target, int target_kind, const float* class_w, double gamma, int64_t ignore_index,
                             double* table, double* partials, int B, int K, int H, int W, void* stream) {
    if (int rc = ml_focal_check("cmu_focal_fwd", x, target, target_kind, gamma, B, K, H, W)) return rc;
    CMU_CHECK_ARG(table && partials, "cmu_focal_fwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const PlaneStream ps = plane_stream(B, K, H, W, x, target, nullptr, nullptr);
    PLANE_DISPATCH(PLANE_DISPATCH_TK, K, ps.V > 1, ml_focal_fwd_launch, target_kind, x, target, class_w, partials, K, ps.HW, ps.npix, gamma,
                   ignore_index, ps.grid, st);
    CMU_CHECK_LAUNCH("cmu_focal_fwd");
    hipLaunchKernelGGL(plane_final_kernel<false>, dim3(3), dim3(64), 0, st, (const double*)partials, ps.grid, 7ull, 1.0, table);
    CMU_CHECK_LAUNCH("cmu_focal_fwd(final)");
    return CMU_OK;
}
extern "C" int cmu_focal_bwd(const float* x, const void* target, int target_kind, const float* class_w, double gamma, int64_t ignore_index,
                             const double* g, float* dx, int B, int K, int H, int W, void* stream) {
    if (int rc = ml_focal_check("cmu_focal_bwd", x, target, target_kind, gamma, B, K, H, W)) return rc;
    CMU_CHECK_ARG(dx, "cmu_focal_bwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const PlaneStream ps = plane_stream(B, K, H, W, x, target, dx, nullptr);
    PLANE_DISPATCH(PLANE_DISPATCH_TK, K, ps.V > 1, ml_focal_bwd_launch, target_kind, x, target, class_w, g, dx, K, ps.HW, ps.npix, gamma,
                   ignore_index, ps.grid, st);
    CMU_CHECK_LAUNCH("cmu_focal_bwd");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// (b) map-weighted softmax sums over the classes of keep_mask (the planes of the others are not read; their table entries are 0):
//   kind 0 (linear)   T_c = sum Wm_c p_c                 G_c = g_c Wm_c                   the boundary loss: Wm = the signed distance
//   kind 1 (squared)  T_c = sum Wm_c (p_c - y_c)^2       G_c = 2 g_c Wm_c (p_c - y_c)     the Hausdorff-DT loss: Wm = the two fields
// with Wm (B,K,H,W) fp32 (NULL: ones), y fp32 / fp64 (kind 1 only), the difference and the square in fp64, and
//   dlogits_j = p_j (G_j - sum_c p_c G_c)
// combined in fp64 from p on, as seg_stats_bwd_kernel does.  HBM-bound: 4K + 4K (+ 4K or 8K) bytes in per pixel, 4K more out backward.
// The difference of kind 1 is not (double)p_c - y_c -- against a one-hot target a confident pixel would keep none of its bits, the
// focal loss's 1 - p_t again -- but, in fp64,
//   p_c - y_c = ((1 - y_c) e_c - y_c sum_{j != c} e_j) * (1 / sum_j e_j),
// which for y_c in {0, 1} is one of the two products: as precise as the exponentials themselves.
// ---------------------------------------------------------------------------------------------
__device__ static inline double ml_diff(int c, int am, float ec, double rest64, double inv_se, double y) {
    return ((1.0 - y) * (double)ec - y * ml_others(c, am, ec, rest64)) * inv_se;
}
template <int KT, int V, int KIND, typename TY>
__global__ __launch_bounds__(256) void ml_map_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ wmap,
                                                        const TY* __restrict__ y, double* __restrict__ partials, int K, int64_t HW,
                                                        int64_t ngroups, unsigned keep_mask) {
    __shared__ double red[4];
    double acc[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) acc[c] = 0.0;
    const int64_t gpi = HW / V;
    const bool small = ngroups < (int64_t(1) << 31);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = plane_group_base(g, gpi, small, K, HW, V);
        PlaneVec<float, V> lv[KT], wv[KT];
        PlaneVec<TY, V> yv[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) {
                lv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(logits + base + c * HW);
                if ((keep_mask >> c) & 1u) {
                    if (wmap) wv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(wmap + base + c * HW);
                    if (KIND == 1) yv[c] = *reinterpret_cast<const PlaneVec<TY, V>*>(y + base + c * HW);
                }
            }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float l[KT], p[KT], lse;
#pragma unroll
            for (int c = 0; c < KT; ++c) l[c] = c < K ? lv[c].v[v] : 0.f;
            seg_softmax<KT>(l, K, p, lse);
            float e[KT], m, rest32;
            double rest64 = 0.0;
            int am = 0;
            if (KIND == 1) ml_exps<KT>(l, K, e, am, m, rest32, rest64);
            const double inv_se = KIND == 1 ? ml_rcp(rest64 + 1.0) : 1.0;
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < K && ((keep_mask >> c) & 1u)) {
                    const double w = wmap ? (double)wv[c].v[v] : 1.0;
                    if (KIND == 1) {
                        const double d = ml_diff(c, am, e[c], rest64, inv_se, (double)yv[c].v[v]);
                        acc[c] += w * (d * d);
                    } else {
                        acc[c] += w * (double)p[c];
                    }
                }
        }
    }
#pragma unroll
    for (int c = 0; c < KT; ++c)
        if (c < K && ((keep_mask >> c) & 1u)) {          // (uniform over the block: every thread takes the same barriers)
            const double a = block_sum_d(acc[c], red);
            if (threadIdx.x == 0) partials[(int64_t)c * CE_MAX_BLOCKS + blockIdx.x] = a;
        }
}
template <int KT, int V, int KIND, typename TY>
__global__ __launch_bounds__(256) void ml_map_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ wmap,
                                                        const TY* __restrict__ y, const double* __restrict__ g_up,
                                                        float* __restrict__ dlogits, int K, int64_t HW, int64_t ngroups,
                                                        unsigned keep_mask) {
    double gc[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) gc[c] = (g_up && c < K && ((keep_mask >> c) & 1u)) ? g_up[c] : 0.0;
    const int64_t gpi = HW / V;
    const bool small = ngroups < (int64_t(1) << 31);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = plane_group_base(g, gpi, small, K, HW, V);
        PlaneVec<float, V> lv[KT], wv[KT], dv[KT];
        PlaneVec<TY, V> yv[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) {
                lv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(logits + base + c * HW);
                if ((keep_mask >> c) & 1u) {
                    if (wmap) wv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(wmap + base + c * HW);
                    if (KIND == 1) yv[c] = *reinterpret_cast<const PlaneVec<TY, V>*>(y + base + c * HW);
                }
            }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float l[KT], p[KT], lse;
#pragma unroll
            for (int c = 0; c < KT; ++c) l[c] = c < K ? lv[c].v[v] : 0.f;
            seg_softmax<KT>(l, K, p, lse);
            float e[KT], m, rest32;
            double rest64 = 0.0;
            int am = 0;
            if (KIND == 1) ml_exps<KT>(l, K, e, am, m, rest32, rest64);
            const double inv_se = KIND == 1 ? ml_rcp(rest64 + 1.0) : 1.0;
            double G[KT], spg = 0.0;
#pragma unroll
            for (int c = 0; c < KT; ++c) {
                G[c] = 0.0;
                if (c < K && ((keep_mask >> c) & 1u)) {
                    const double w = wmap ? (double)wv[c].v[v] : 1.0;
                    G[c] = KIND == 1 ? 2.0 * gc[c] * w * ml_diff(c, am, e[c], rest64, inv_se, (double)yv[c].v[v]) : gc[c] * w;
                    spg += (double)p[c] * G[c];
                }
            }
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < K) dv[c].v[v] = (float)((double)p[c] * (G[c] - spg));
        }
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) *reinterpret_cast<PlaneVec<float, V>*>(dlogits + base + c * HW) = dv[c];
    }
}

template <int KT, int V, int KIND, typename TY>
static void ml_map_fwd_launch(const float* logits, const float* wmap, const void* y, double* partials, int K, int64_t HW, int64_t npix,
                              unsigned keep_mask, int grid, hipStream_t st) {
    hipLaunchKernelGGL((ml_map_fwd_kernel<KT, V, KIND, TY>), dim3(grid), dim3(256), 0, st, logits, wmap, (const TY*)y, partials, K, HW, npix / V,
                       keep_mask);
}
template <int KT, int V, int KIND, typename TY>
static void ml_map_bwd_launch(const float* logits, const float* wmap, const void* y, const double* g, float* dlogits, int K, int64_t HW,
                              int64_t npix, unsigned keep_mask, int grid, hipStream_t st) {
    hipLaunchKernelGGL((ml_map_bwd_kernel<KT, V, KIND, TY>), dim3(grid), dim3(256), 0, st, logits, wmap, (const TY*)y, g, dlogits, K, HW,
                       npix / V, keep_mask);
}
// an INNER of PLANE_DISPATCH: FN<KT, V, KIND, TY>(args...) for the runtime kind and target type (kind 0 reads no target)
#define ML_DISPATCH_KY(KT, V, FN, kind, f64, ...)                                      \
    do {                                                                               \
        if ((kind) == 0) FN<KT, V, 0, float>(__VA_ARGS__);                             \
        else if (f64) FN<KT, V, 1, double>(__VA_ARGS__);                               \
        else FN<KT, V, 1, float>(__VA_ARGS__);                                         \
    } while (0)

static int ml_map_check(const char* who, const void* logits, const void* y, int keep_mask, int kind, int B, int K, int H, int W) {
    if (int rc = ml_check_shape(who, B, K, H, W)) return rc;
    CMU_CHECK_ARG(kind == 0 || kind == 1, "%s: unknown kind %d", who, kind);
    CMU_CHECK_ARG(logits && (kind == 0 || y), "%s: bad args", who);
    CMU_CHECK_ARG(keep_mask > 0 && keep_mask < (1 << K), "%s: keep_mask 0x%x names no channel, or one past K = %d", who, keep_mask, K);
    return CMU_OK;
}
extern "C" int cmu_softmax_map_fwd(const float* logits, const float* wmap, const void* y, int y_is_f64, int keep_mask, int kind,
                                   double* table, double* partials, int B, int K, int H, int W, void* stream) {
    if (int rc = ml_map_check("cmu_softmax_map_fwd", logits, y, keep_mask, kind, B, K, H, W)) return rc;
    CMU_CHECK_ARG(table && partials, "cmu_softmax_map_fwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const PlaneStream ps = plane_stream(B, K, H, W, logits, wmap, kind == 1 ? y : nullptr, nullptr);
    PLANE_DISPATCH(ML_DISPATCH_KY, K, ps.V > 1, ml_map_fwd_launch, kind, y_is_f64 != 0, logits, wmap, y, partials, K, ps.HW, ps.npix,
                   (unsigned)keep_mask, ps.grid, st);
    CMU_CHECK_LAUNCH("cmu_softmax_map_fwd");
    hipLaunchKernelGGL(plane_final_kernel<false>, dim3(K), dim3(64), 0, st, (const double*)partials, ps.grid, (unsigned long long)keep_mask,
                       1.0, table);
    CMU_CHECK_LAUNCH("cmu_softmax_map_fwd(final)");
    return CMU_OK;
}
extern "C" int cmu_softmax_map_bwd(const float* logits, const float* wmap, const void* y, int y_is_f64, int keep_mask, int kind,
                                   const double* g, float* dlogits, int B, int K, int H, int W, void* stream) {
    if (int rc = ml_map_check("cmu_softmax_map_bwd", logits, y, keep_mask, kind, B, K, H, W)) return rc;
    CMU_CHECK_ARG(dlogits, "cmu_softmax_map_bwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const PlaneStream ps = plane_stream(B, K, H, W, logits, wmap, kind == 1 ? y : nullptr, dlogits);
    PLANE_DISPATCH(ML_DISPATCH_KY, K, ps.V > 1, ml_map_bwd_launch, kind, y_is_f64 != 0, logits, wmap, y, g, dlogits, K, ps.HW, ps.npix,
                   (unsigned)keep_mask, ps.grid, st);
    CMU_CHECK_LAUNCH("cmu_softmax_map_bwd");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// (c) distance fields from the int32 squared distances of cmu_edt_rows: one fp32 plane per call, written at field + b K HW + plane HW so
// that a (B,K,H,W) map fills class by class without a copy.  mode 0: cmu_ml_signed_field of the pair (d2_to, d2_from); mode 1:
// cmu_ml_unsigned_field of that pair plus, when given, that of a second pair (one fp32 add).  4 pixels per lane when H*W % 4 == 0 and
// every pointer is 16-byte aligned, else 1, for the whole call.
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void ml_field_kernel(const int32_t* __restrict__ to_a, const int32_t* __restrict__ from_a,
                                                      const int32_t* __restrict__ to_b, const int32_t* __restrict__ from_b, int mode,
                                                      double alpha, float* __restrict__ field, int plane, int K, int64_t HW,
                                                      int64_t ngroups) {
    const int64_t gpi = HW / V;
    const bool small = ngroups < (int64_t(1) << 31);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t out = plane_group_base(g, gpi, small, K, HW, V) + plane * HW;
        const PlaneVec<int32_t, V> ta = *reinterpret_cast<const PlaneVec<int32_t, V>*>(to_a + g * V);
        const PlaneVec<int32_t, V> fa = *reinterpret_cast<const PlaneVec<int32_t, V>*>(from_a + g * V);
        PlaneVec<float, V> f;
        if (mode == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v) f.v[v] = cmu_ml_signed_field(ta.v[v], fa.v[v]);
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) f.v[v] = cmu_ml_unsigned_field(ta.v[v], fa.v[v], alpha);
            if (to_b) {
                const PlaneVec<int32_t, V> tb = *reinterpret_cast<const PlaneVec<int32_t, V>*>(to_b + g * V);
                const PlaneVec<int32_t, V> fb = *reinterpret_cast<const PlaneVec<int32_t, V>*>(from_b + g * V);
#pragma unroll
                for (int v = 0; v < V; ++v) f.v[v] = f.v[v] + cmu_ml_unsigned_field(tb.v[v], fb.v[v], alpha);
            }
        }
        *reinterpret_cast<PlaneVec<float, V>*>(field + out) = f;
    }
}
extern "C" int cmu_distance_field(const int32_t* d2_to, const int32_t* d2_from, const int32_t* d2_to_b, const int32_t* d2_from_b, int mode,
                                  double alpha, float* field, int plane, int B, int K, int H, int W, void* stream) {
    CMU_CHECK_ARG(d2_to && d2_from && field && B > 0 && H > 0 && W > 0, "cmu_distance_field: bad args");
    CMU_CHECK_ARG(K >= 1 && plane >= 0 && plane < K, "cmu_distance_field: plane %d of K = %d", plane, K);
    CMU_CHECK_ARG(mode == 0 || mode == 1, "cmu_distance_field: unknown mode %d", mode);
    CMU_CHECK_ARG((d2_to_b == nullptr) == (d2_from_b == nullptr) && (mode == 1 || d2_to_b == nullptr),
                  "cmu_distance_field: the second pair comes whole, in mode 1 only");
    CMU_CHECK_ARG(mode == 0 || (alpha > 0.0 && alpha <= 16.0), "cmu_distance_field: 0 < alpha <= 16 (got %g)", alpha);
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, npix = (int64_t)B * HW;
    const bool vec = HW % 4 == 0 && cmu_aligned16(d2_to) && cmu_aligned16(d2_from) && cmu_aligned16(d2_to_b) && cmu_aligned16(d2_from_b) &&
                     cmu_aligned16(field);
    const int grid = plane_grid(npix / (vec ? 4 : 1));
    if (vec)
        hipLaunchKernelGGL(ml_field_kernel<4>, dim3(grid), dim3(256), 0, st, d2_to, d2_from, d2_to_b, d2_from_b, mode, alpha, field, plane, K, HW,
                           npix / 4);
    else
        hipLaunchKernelGGL(ml_field_kernel<1>, dim3(grid), dim3(256), 0, st, d2_to, d2_from, d2_to_b, d2_from_b, mode, alpha, field, plane, K, HW,
                           npix);
    CMU_CHECK_LAUNCH("cmu_distance_field");
    return CMU_OK;
}
