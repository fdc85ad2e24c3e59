// pointwise_loss.hip -- the element-wise losses (L1 / MSE / BCE / BCE-with-logits) and the class-index cross entropy of
// Finetuning/metrics.py:495-551 (bare subclasses of the torch.nn losses) as streaming passes under the contract of plane_stream.h:
// fp32 predictions, targets read in their own dtype.  The element-wise family walks a flat (outer, C, inner) tensor and takes the
// contract's grid cap, partials and finalisation; its width rule is its own (below).
#include "common.h"
#include "plane_stream.h"

constexpr int PWL_MAX_C = 8;             // channels of the per-channel weight vectors; classes of the index CE
static_assert(PWL_MAX_C == CMU_PWL_MAX_C, "header constant");

// ---------------------------------------------------------------------------------------------
// (a) element-wise family.  The tensor is (outer, C, inner); the optional per-channel fp32 vectors chan_w / chan_pw are indexed by
// (i / inner) % C.  A lane takes 4 consecutive elements (16-byte x / dx accesses, 16- or 2 x 16-byte target loads) when inner % 4 == 0
// and the pointers are 16-byte aligned -- so the 4 share a channel -- and one element otherwise.  HBM-bound: 4 + 4 (fp32 targets) or
// 4 + 8 (fp64) bytes in per element, 4 more out backward.
// The transcendental of a term is taken in fp32 on the fp32 prediction (logf, log1pf, expf: relative error of a few ulp also where
// the result is tiny, which log(1 - x) and 1 + e^-|x| formed in fp32 would not give); everything that combines it with the target,
// the weights and the upstream gradient runs in fp64, in forms without cancellation:
//   BCE               -[y max(log x, -100) + (1 - y) max(log1p(-x), -100)]; the clamp keeps a NaN (x outside [0, 1])
//   BCE with logits   c = 1 + (pw - 1) y,  l = log1p(e^-|x|),  s = e^-|x| / (1 + e^-|x|) = sigma(-|x|)
//                     term  = c l + (x >= 0 ? (1 - y) x : pw y |x|)          [= (1 - y) x + c (l + max(-x, 0))]
//                     dterm = x >= 0 ? (1 - y) - c s : c s - pw y            [= (1 - y) - c sigma(-x)]
//                     (past |x| = 80 e^-|x| leaves the fp32 normal range: l = s = e^-|x| in fp64 there, exact to 1e-35 relative)
// ---------------------------------------------------------------------------------------------
__device__ static inline float pw_log_clamped(float v) { return v < -100.f ? -100.f : v; }   // (not fmaxf: that would drop a NaN)
__device__ static inline double pw_pos_weight_c(double y, double pw) { return 1.0 + (pw - 1.0) * y; }

template <int KIND>
__device__ static inline double pw_term(float x, double y, double pw) {
    const double xd = (double)x;
    if (KIND == CMU_PWL_L1) return fabs(xd - y);
    if (KIND == CMU_PWL_MSE) {
        const double d = xd - y;
        return d * d;
    }
    if (KIND == CMU_PWL_BCE) {
        const float lx = pw_log_clamped(logf(x)), l1x = pw_log_clamped(log1pf(-x));
        return -(y * (double)lx + (1.0 - y) * (double)l1x);
    }
    const float ax = fabsf(x);
    const double l = ax > 80.f ? exp(-(double)ax) : (double)log1pf(expf(-ax));
    return pw_pos_weight_c(y, pw) * l + (x >= 0.f ? (1.0 - y) * xd : -(pw * y) * xd);
}
template <int KIND>
__device__ static inline double pw_dterm(float x, double y, double pw) {
    const double xd = (double)x;
    if (KIND == CMU_PWL_L1) {
        const double d = xd - y;
        return d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0;
    }
    if (KIND == CMU_PWL_MSE) return 2.0 * (xd - y);
    if (KIND == CMU_PWL_BCE) return (xd - y) / fmax(xd * (1.0 - xd), (double)1e-12f);   // (torch's EPSILON is a float constant)
    const float ax = fabsf(x);
    double s;
    if (ax > 80.f) {
        s = exp(-(double)ax);
    } else {
        const float e = expf(-ax);
        s = (double)(e / (1.f + e));
    }
    const double c = pw_pos_weight_c(y, pw);
    return x >= 0.f ? (1.0 - y) - c * s : c * s - pw * y;
}
// channel of element i of (outer, C, inner); ``small``: fewer than 2^31 elements (a 64-bit division is ~10x the instructions)
__device__ static inline int pw_channel(int64_t i, int64_t inner, int C, bool small) {
    if (C == 1) return 0;
    if (small) return (int)(((unsigned)i / (unsigned)inner) % (unsigned)C);
    return (int)((i / inner) % C);
}

template <int KIND, int V, typename TY>
__global__ __launch_bounds__(256) void pw_fwd_kernel(const float* __restrict__ x, const TY* __restrict__ y, const float* __restrict__ chan_w,
                                                    const float* __restrict__ chan_pw, double* __restrict__ ws, int C, int64_t inner,
                                                    int64_t ngroups) {
    __shared__ double red[4];
    double acc = 0.0;
    const bool small = ngroups * V < (int64_t(1) << 31);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = g * V;
        const int c = pw_channel(i0, inner, C, small);
        const double w = chan_w ? (double)chan_w[c] : 1.0, pw = chan_pw ? (double)chan_pw[c] : 1.0;
        const PlaneVec<float, V> xv = *reinterpret_cast<const PlaneVec<float, V>*>(x + i0);
        const PlaneVec<TY, V> yv = *reinterpret_cast<const PlaneVec<TY, V>*>(y + i0);
        double t = 0.0;
#pragma unroll
        for (int v = 0; v < V; ++v) t += pw_term<KIND>(xv.v[v], (double)yv.v[v], pw);
        acc += w * t;
    }
    acc = block_sum_d(acc, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}
template <int KIND, int V, typename TY>
__global__ __launch_bounds__(256) void pw_bwd_kernel(const float* __restrict__ x, const TY* __restrict__ y, const float* __restrict__ chan_w,
                                                    const float* __restrict__ chan_pw, const double* __restrict__ g_up,
                                                    float* __restrict__ dx, int C, int64_t inner, int64_t ngroups) {
    const double g0 = g_up ? g_up[0] : 0.0;
    const bool small = ngroups * V < (int64_t(1) << 31);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = g * V;
        const int c = pw_channel(i0, inner, C, small);
        const double gw = g0 * (chan_w ? (double)chan_w[c] : 1.0), pw = chan_pw ? (double)chan_pw[c] : 1.0;
        const PlaneVec<float, V> xv = *reinterpret_cast<const PlaneVec<float, V>*>(x + i0);
        const PlaneVec<TY, V> yv = *reinterpret_cast<const PlaneVec<TY, V>*>(y + i0);
        PlaneVec<float, V> dv;
#pragma unroll
        for (int v = 0; v < V; ++v) dv.v[v] = (float)(gw * pw_dterm<KIND>(xv.v[v], (double)yv.v[v], pw));
        *reinterpret_cast<PlaneVec<float, V>*>(dx + i0) = dv;
    }
}

template <int KIND, int V, typename TY>
static void pw_fwd_launch(const float* x, const void* y, const float* chan_w, const float* chan_pw, double* ws, int C, int64_t inner,
                          int64_t n, int grid, hipStream_t st) {
    hipLaunchKernelGGL((pw_fwd_kernel<KIND, V, TY>), dim3(grid), dim3(256), 0, st, x, (const TY*)y, chan_w, chan_pw, ws, C, inner, n / V);
}
template <int KIND, int V, typename TY>
static void pw_bwd_launch(const float* x, const void* y, const float* chan_w, const float* chan_pw, const double* g, float* dx, int C,
                          int64_t inner, int64_t n, int grid, hipStream_t st) {
    hipLaunchKernelGGL((pw_bwd_kernel<KIND, V, TY>), dim3(grid), dim3(256), 0, st, x, (const TY*)y, chan_w, chan_pw, g, dx, C, inner, n / V);
}
// FN<KIND, V, TY>(args...) for the runtime kind, vector width and target type
#define PW_DISPATCH_VT(FN, KIND, vec, f64, ...)                                                          \
    do {                                                                                                 \
        if (vec) { if (f64) FN<KIND, 4, double>(__VA_ARGS__); else FN<KIND, 4, float>(__VA_ARGS__); }    \
        else     { if (f64) FN<KIND, 1, double>(__VA_ARGS__); else FN<KIND, 1, float>(__VA_ARGS__); }    \
    } while (0)
#define PW_DISPATCH(FN, kind, vec, f64, ...)                                               \
    do {                                                                                   \
        switch (kind) {                                                                    \
            case CMU_PWL_L1: PW_DISPATCH_VT(FN, CMU_PWL_L1, vec, f64, __VA_ARGS__); break;   \
            case CMU_PWL_MSE: PW_DISPATCH_VT(FN, CMU_PWL_MSE, vec, f64, __VA_ARGS__); break; \
            case CMU_PWL_BCE: PW_DISPATCH_VT(FN, CMU_PWL_BCE, vec, f64, __VA_ARGS__); break; \
            default: PW_DISPATCH_VT(FN, CMU_PWL_BCE_WITH_LOGITS, vec, f64, __VA_ARGS__);     \
        }                                                                                  \
    } while (0)

static int pw_check(const char* who, int kind, const void* x, const void* y, const float* chan_pw, int64_t outer, int C, int64_t inner) {
    CMU_CHECK_ARG(x && y && outer > 0 && inner > 0, "%s: bad args", who);
    CMU_CHECK_ARG(kind >= CMU_PWL_L1 && kind <= CMU_PWL_BCE_WITH_LOGITS, "%s: unknown kind %d", who, kind);
    CMU_CHECK_ARG(C >= 1 && C <= PWL_MAX_C, "%s: 1 <= C <= %d channels (got %d)", who, PWL_MAX_C, C);
    CMU_CHECK_ARG(chan_pw == nullptr || kind == CMU_PWL_BCE_WITH_LOGITS, "%s: chan_pw belongs to BCE_WITH_LOGITS only", who);
    return CMU_OK;
}
extern "C" int64_t cmu_pointwise_loss_ws_bytes(void) { return (int64_t)CE_MAX_BLOCKS * (int64_t)sizeof(double); }
extern "C" int cmu_pointwise_loss_fwd(int kind, const float* x, const void* y, int y_is_f64, const float* chan_w, const float* chan_pw,
                                      double* out, int64_t outer, int C, int64_t inner, void* ws, void* stream) {
    if (int rc = pw_check("cmu_pointwise_loss_fwd", kind, x, y, chan_pw, outer, C, inner)) return rc;
    CMU_CHECK_ARG(out && ws, "cmu_pointwise_loss_fwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = outer * C * inner;
    const bool vec = inner % 4 == 0 && cmu_aligned16(x) && cmu_aligned16(y);
    const int grid = plane_grid(n / (vec ? 4 : 1));
    PW_DISPATCH(pw_fwd_launch, kind, vec, y_is_f64 != 0, x, y, chan_w, chan_pw, (double*)ws, C, inner, n, grid, st);
    CMU_CHECK_LAUNCH("cmu_pointwise_loss_fwd");
    hipLaunchKernelGGL(plane_final_kernel<false>, dim3(1), dim3(64), 0, st, (const double*)ws, grid, PLANE_ALL_COLUMNS, 1.0, out);
    CMU_CHECK_LAUNCH("cmu_pointwise_loss_fwd(final)");
    return CMU_OK;
}
extern "C" int cmu_pointwise_loss_bwd(int kind, const float* x, const void* y, int y_is_f64, const float* chan_w, const float* chan_pw,
                                      const double* g, float* dx, int64_t outer, int C, int64_t inner, void* stream) {
    if (int rc = pw_check("cmu_pointwise_loss_bwd", kind, x, y, chan_pw, outer, C, inner)) return rc;
    CMU_CHECK_ARG(dx, "cmu_pointwise_loss_bwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = outer * C * inner;
    const bool vec = inner % 4 == 0 && cmu_aligned16(x) && cmu_aligned16(y) && cmu_aligned16(dx);
    const int grid = plane_grid(n / (vec ? 4 : 1));
    PW_DISPATCH(pw_bwd_launch, kind, vec, y_is_f64 != 0, x, y, chan_w, chan_pw, g, dx, C, inner, n, grid, st);
    CMU_CHECK_LAUNCH("cmu_pointwise_loss_bwd");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// (b) class-index cross entropy of (B,K,H,W) fp32 input, 2 <= K <= 8 (KT and V: PLANE_DISPATCH).  The target is a label plane (B,H,W) in its own
// dtype, truncated to an integer as .long() does, or K one-hot planes whose arg-max over the channels of keep_mask is taken
// (plane_labels: the first maximum wins).  The input holds logits -- the log-softmax over all K
// channels is taken here -- or log-probabilities used as they are (log_input).
// -log p_c = (max - l_c) + log1p(sum of the other e^(l - max)): the difference is exact in fp64 and the sum leaves out the maximum's
// own 1, so a confident pixel's tiny loss keeps its relative precision (max + log(sum) - l_c in fp32 would leave it with an absolute
// error of ulp(|l|)); e^(l - max) has the rounding of its fp32 argument given back, as seg_softmax (seg_softmax.h) has it.
// A label outside [0, K) that is not ignore_index is never used as an index (the class is picked by comparison, not by address):
// that pixel adds NaN to table[0] and gets a zero gradient.
// ---------------------------------------------------------------------------------------------
// p = softmax(l) in fp32, nlp[c] = -log p_c (see above)
template <int KT>
__device__ static inline void ice_log_softmax(const float (&l)[KT], int K, float (&p)[KT], double (&nlp)[KT]) {
    float m = l[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < KT; ++c)
        if (c < K && l[c] > m) {
            m = l[c];
            am = c;
        }
    float rest = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c)
        if (c < K) {
            const float x = l[c] - m;
            const float d = (float)(((double)l[c] - (double)m) - (double)x);
            const float e = expf(x);
            p[c] = fmaf(e, d, e);                  // (exactly 1 at c == am)
            if (c != am) rest += p[c];
        }
    const float se = 1.f + rest;
    const double lg = (double)log1pf(rest);
#pragma unroll
    for (int c = 0; c < KT; ++c)
        if (c < K) {
            p[c] = p[c] / se;
            nlp[c] = ((double)m - (double)l[c]) + lg;
        }
}
template <int KT, int V, int TK>
__global__ __launch_bounds__(256) void ice_fwd_kernel(const float* __restrict__ x, const typename PlaneTarget<TK>::T* __restrict__ tgt,
                                                     const float* __restrict__ class_w, double* __restrict__ ws, int K, int64_t HW,
                                                     int64_t ngroups, int log_input, unsigned keep_mask, int64_t ignore_index) {
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
        plane_labels<KT, V, TK, false>(tgt, g, base, K, HW, keep_mask, lab);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int64_t t = lab[v];
            if (t == ignore_index) continue;
            if (t < 0 || t >= K) {
                t0 += __builtin_nan("");
                continue;
            }
            float l[KT], p[KT];
            double nlp[KT];
#pragma unroll
            for (int c = 0; c < KT; ++c) l[c] = c < K ? xv[c].v[v] : 0.f;
            if (log_input) {
#pragma unroll
                for (int c = 0; c < KT; ++c) nlp[c] = -(double)l[c];
            } else {
                ice_log_softmax<KT>(l, K, p, nlp);
            }
            double wt = 0.0, nt = 0.0, s2 = 0.0;
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < K) {
                    if (c == (int)t) {
                        wt = wc[c];
                        nt = nlp[c];
                    }
                    if ((keep_mask >> c) & 1u) s2 += wc[c] * nlp[c];
                }
            t0 += wt * nt;
            t1 += wt;
            t2 += s2;
        }
    }
    t0 = block_sum_d(t0, red);
    t1 = block_sum_d(t1, red);
    t2 = block_sum_d(t2, red);
    if (threadIdx.x == 0) {
        ws[0 * CE_MAX_BLOCKS + blockIdx.x] = t0;
        ws[1 * CE_MAX_BLOCKS + blockIdx.x] = t1;
        ws[2 * CE_MAX_BLOCKS + blockIdx.x] = t2;
    }
}
template <int KT, int V, int TK>
__global__ __launch_bounds__(256) void ice_bwd_kernel(const float* __restrict__ x, const typename PlaneTarget<TK>::T* __restrict__ tgt,
                                                     const float* __restrict__ class_w, const double* __restrict__ g_up,
                                                     float* __restrict__ dx, int K, int64_t HW, int64_t ngroups, int log_input,
                                                     unsigned keep_mask, int64_t ignore_index) {
    const double g0 = g_up ? g_up[0] : 0.0, g2 = g_up ? g_up[1] : 0.0;
    double wc[KT], wk[KT], swk = 0.0;       // wk: the weight of a kept channel, 0 outside keep_mask
#pragma unroll
    for (int c = 0; c < KT; ++c) {
        wc[c] = c < K ? (class_w ? (double)class_w[c] : 1.0) : 0.0;
        wk[c] = ((keep_mask >> c) & 1u) ? wc[c] : 0.0;
        swk += wk[c];
    }
    const int64_t gpi = HW / V;
    const bool small = ngroups < (int64_t(1) << 31);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = plane_group_base(g, gpi, small, K, HW, V);
        PlaneVec<float, V> xv[KT], dv[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) xv[c] = *reinterpret_cast<const PlaneVec<float, V>*>(x + base + c * HW);
        int64_t lab[V];
        plane_labels<KT, V, TK, false>(tgt, g, base, K, HW, keep_mask, lab);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int64_t t = lab[v];
            if (t == ignore_index || t < 0 || t >= K) {
#pragma unroll
                for (int c = 0; c < KT; ++c) dv[c].v[v] = 0.f;
                continue;
            }
            double wt = 0.0;
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c == (int)t) wt = wc[c];
            const double gwt = g0 * wt;
            if (log_input) {
                // d(-x_t)/dx_j = -[j == t]
#pragma unroll
                for (int c = 0; c < KT; ++c) dv[c].v[v] = (float)(-(c == (int)t ? gwt : 0.0) - g2 * wk[c]);
            } else {
                // d(-log p_c)/dl_j = p_j - [j == c]
                float l[KT], p[KT];
                double nlp[KT];
#pragma unroll
                for (int c = 0; c < KT; ++c) l[c] = c < K ? xv[c].v[v] : 0.f;
                ice_log_softmax<KT>(l, K, p, nlp);
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (c < K) dv[c].v[v] = (float)(gwt * ((double)p[c] - (c == (int)t ? 1.0 : 0.0)) + g2 * ((double)p[c] * swk - wk[c]));
            }
        }
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) *reinterpret_cast<PlaneVec<float, V>*>(dx + base + c * HW) = dv[c];
    }
}

template <int KT, int V, int TK>
static void ice_fwd_launch(const float* x, const void* tgt, const float* class_w, double* ws, int K, int64_t HW, int64_t npix, int log_input,
                           unsigned keep_mask, int64_t ignore_index, int grid, hipStream_t st) {
    hipLaunchKernelGGL((ice_fwd_kernel<KT, V, TK>), dim3(grid), dim3(256), 0, st, x, (const typename PlaneTarget<TK>::T*)tgt, class_w, ws, K, HW,
                       npix / V, log_input, keep_mask, ignore_index);
}
template <int KT, int V, int TK>
static void ice_bwd_launch(const float* x, const void* tgt, const float* class_w, const double* g, float* dx, int K, int64_t HW, int64_t npix,
                           int log_input, unsigned keep_mask, int64_t ignore_index, int grid, hipStream_t st) {
    hipLaunchKernelGGL((ice_bwd_kernel<KT, V, TK>), dim3(grid), dim3(256), 0, st, x, (const typename PlaneTarget<TK>::T*)tgt, class_w, g, dx, K,
                       HW, npix / V, log_input, keep_mask, ignore_index);
}
static int ice_check(const char* who, const void* x, const void* tgt, int target_kind, int keep_mask, int B, int K, int H, int W) {
    CMU_CHECK_ARG(x && tgt && B > 0 && H > 0 && W > 0, "%s: bad args", who);
    CMU_CHECK_ARG(K >= 2 && K <= PWL_MAX_C, "%s: 2 <= K <= %d classes (got %d)", who, PWL_MAX_C, K);
    CMU_CHECK_ARG(target_kind >= CMU_ICE_LABEL_I64 && target_kind <= CMU_ICE_ONEHOT_F64, "%s: unknown target kind %d", who, target_kind);
    CMU_CHECK_ARG(keep_mask > 0 && keep_mask < (1 << K), "%s: keep_mask 0x%x names no channel, or one past K = %d", who, keep_mask, K);
    return CMU_OK;
}
extern "C" int64_t cmu_index_ce_ws_bytes(void) { return (int64_t)CE_MAX_BLOCKS * 3 * (int64_t)sizeof(double); }
extern "C" int cmu_index_ce_fwd(const float* x, const void* target, int target_kind, int log_input, int keep_mask, const float* class_w,
                                int64_t ignore_index, double* table, int B, int K, int H, int W, void* ws, void* stream) {
    if (int rc = ice_check("cmu_index_ce_fwd", x, target, target_kind, keep_mask, B, K, H, W)) return rc;
    CMU_CHECK_ARG(table && ws, "cmu_index_ce_fwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const PlaneStream ps = plane_stream(B, K, H, W, x, target, nullptr, nullptr);
    PLANE_DISPATCH(PLANE_DISPATCH_TK, K, ps.V > 1, ice_fwd_launch, target_kind, x, target, class_w, (double*)ws, K, ps.HW, ps.npix,
                   log_input != 0, (unsigned)keep_mask, ignore_index, ps.grid, st);
    CMU_CHECK_LAUNCH("cmu_index_ce_fwd");
    hipLaunchKernelGGL(plane_final_kernel<false>, dim3(3), dim3(64), 0, st, (const double*)ws, ps.grid, PLANE_ALL_COLUMNS, 1.0, table);
    CMU_CHECK_LAUNCH("cmu_index_ce_fwd(final)");
    return CMU_OK;
}
extern "C" int cmu_index_ce_bwd(const float* x, const void* target, int target_kind, int log_input, int keep_mask, const float* class_w,
                                int64_t ignore_index, const double* g, float* dx, int B, int K, int H, int W, void* stream) {
    if (int rc = ice_check("cmu_index_ce_bwd", x, target, target_kind, keep_mask, B, K, H, W)) return rc;
    CMU_CHECK_ARG(dx, "cmu_index_ce_bwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const PlaneStream ps = plane_stream(B, K, H, W, x, target, dx, nullptr);
    PLANE_DISPATCH(PLANE_DISPATCH_TK, K, ps.V > 1, ice_bwd_launch, target_kind, x, target, class_w, g, dx, K, ps.HW, ps.npix, log_input != 0,
                   (unsigned)keep_mask, ignore_index, ps.grid, st);
    CMU_CHECK_LAUNCH("cmu_index_ce_bwd");
    return CMU_OK;
}
