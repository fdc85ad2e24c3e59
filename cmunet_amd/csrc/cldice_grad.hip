// cldice_grad.hip -- the differentiable soft-clDice (Finetuning/metrics.py:401-492 with threshold=None).
//   cmu_softmax_planes        softmax(dim=1) of the kept channels of (B,K,H,W) logits as (B*Kk,H,W) planes (soft or thresholded)
//                             and the same channels of the target
//   cmu_softmax_planes_bwd    dlogit_k = p_k (G_k - sum_j p_j G_j), the probabilities recomputed by the forward's own code
//   cmu_soft_skeleton_save    cmu_soft_skeleton's bits, keeping every level image, running skeleton and window selection
//   cmu_soft_skeleton_bwd     one reverse sweep over the levels, written as a gather (no atomics: the same bits every call)
// The sub-gradients are PyTorch autograd's: a max-pool window gives its whole gradient to its FIRST maximum in row-major order,
// torch.min(p1, p2) halves the gradient between equal arguments, relu'(0) = 0.
#include "common.h"

namespace {

constexpr int CG_MAX_K = 8;
inline int cg_grid(int64_t n) { return (int)(cmu_div_up64(n, 256) < 4096 ? cmu_div_up64(n, 256) : 4096); }

// softmax over the K logits of one pixel: ONE instruction sequence for the forward planes and for their backward
template <int K>
__device__ inline void cg_softmax(const float* __restrict__ logits, int64_t base, int64_t HW, float* p) {
    float mx = logits[base];
    p[0] = mx;
#pragma unroll
    for (int k = 1; k < K; ++k) {
        p[k] = logits[base + k * HW];
        mx = fmaxf(mx, p[k]);
    }
    p[0] = expf(p[0] - mx);
    float sum = p[0];
#pragma unroll
    for (int k = 1; k < K; ++k) {
        p[k] = expf(p[k] - mx);
        sum += p[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = p[k] / sum;
}

template <int K>
__global__ void cg_planes_kernel(const float* __restrict__ logits, const void* __restrict__ target, int target_f64, unsigned keep,
                                 int use_thr, float thr, float* __restrict__ pp, float* __restrict__ tp, int64_t HW, int64_t total) {
    const int Kk = __popc(keep);
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = o / HW, r = o % HW;
        float p[K];
        cg_softmax<K>(logits, b * K * HW + r, HW, p);
        int i = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (!((keep >> k) & 1u)) continue;
            const int64_t dst = (b * Kk + i) * HW + r, src = (b * K + k) * HW + r;
            pp[dst] = use_thr ? (p[k] > thr ? 1.f : 0.f) : p[k];
            if (tp) tp[dst] = target_f64 ? (float)((const double*)target)[src] : ((const float*)target)[src];
            ++i;
        }
    }
}

template <int K>
__global__ void cg_planes_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ G, unsigned keep,
                                     float* __restrict__ dlogits, int64_t HW, int64_t total) {
    const int Kk = __popc(keep);
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = o / HW, r = o % HW;
        float p[K], g[K];
        cg_softmax<K>(logits, b * K * HW + r, HW, p);
        float s = 0.f;
        int i = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            g[k] = 0.f;
            if (!((keep >> k) & 1u)) continue;
            g[k] = G[(b * Kk + i) * HW + r];
            s = fmaf(p[k], g[k], s);
            ++i;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) dlogits[(b * K + k) * HW + r] = p[k] * (g[k] - s);
    }
}

// ---- forward that keeps its levels: the arithmetic of soft_erode_kernel / soft_skel_update_kernel (heads.hip) ----
// Selection codes, one byte per pixel and level, written by the forward kernels that read the windows anyway:
//   E code of the erode window at p: (first column minimum: 0 top, 1 centre, 2 bottom) | (first row minimum: 0 left, 1 centre,
//   2 right) << 2 | (twice the column window's share of the gradient: 2 if its minimum is the smaller one, 1 if equal, 0) << 4
//   D code of the dilate window at p: 3 (dy + 1) + (dx + 1) of the first maximum in row-major order (padding never wins)
__global__ void cg_erode_kernel(const float* __restrict__ in, float* __restrict__ out, uint8_t* __restrict__ ecode, int H, int W,
                                int64_t total) {
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(o % W), y = (int)((o / W) % H);
        const float c = in[o];
        float m = c, t = INFINITY, b = INFINITY, l = INFINITY, r = INFINITY;
        if (y > 0) { t = in[o - W]; m = fminf(m, t); }
        if (y + 1 < H) { b = in[o + W]; m = fminf(m, b); }
        if (x > 0) { l = in[o - 1]; m = fminf(m, l); }
        if (x + 1 < W) { r = in[o + 1]; m = fminf(m, r); }
        out[o] = m;
        float m1 = t, m2 = l;
        int cs = 0, rs = 0;
        if (c < m1) { m1 = c; cs = 1; }
        if (b < m1) { m1 = b; cs = 2; }
        if (c < m2) { m2 = c; rs = 1; }
        if (r < m2) { m2 = r; rs = 2; }
        ecode[o] = (uint8_t)(cs | (rs << 2) | ((m1 < m2 ? 2 : (m1 == m2 ? 1 : 0)) << 4));
    }
}
__device__ inline float cg_dilate(const float* __restrict__ next, int64_t o, int y, int x, int H, int W, int& sel) {
    float d = next[o], mx = -INFINITY;
    sel = 4;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const float v = next[o + (int64_t)dy * W + dx];
                d = fmaxf(d, v);
                if (v > mx) {
                    mx = v;
                    sel = (dy + 1) * 3 + (dx + 1);
                }
            }
        }
    return d;
}
__global__ void cg_update_kernel(const float* __restrict__ img, const float* __restrict__ next, const float* __restrict__ skel_prev,
                                 float* __restrict__ skel_out, uint8_t* __restrict__ dcode, int H, int W, int64_t total) {
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(o % W), y = (int)((o / W) % H);
        int sel;
        const float delta = fmaxf(img[o] - cg_dilate(next, o, y, x, H, W, sel), 0.f);
        dcode[o] = (uint8_t)sel;
        if (skel_prev) {
            const float s = skel_prev[o];
            skel_out[o] = s + fmaxf(delta - s * delta, 0.f);
        } else {
            skel_out[o] = delta;
        }
    }
}

// ---- backward: every pixel GATHERS from the windows whose kept selection code names it ----
// gradient that the dilate windows around (y, x) hand to it
__device__ inline float cg_dilate_gather(const float* gD, const uint8_t* dc, int y, int x, int H, int W) {
    float acc = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int py = y + dy, px = x + dx;
            if ((unsigned)py >= (unsigned)H || (unsigned)px >= (unsigned)W) continue;
            const int64_t p = (int64_t)py * W + px;
            if (dc[p] == (1 - dy) * 3 + (1 - dx)) acc += gD[p];   // (y, x) sits at (-dy, -dx) of window p
        }
    return acc;
}
// gradient that the five erode windows whose column or row holds (y, x) hand to it
__device__ inline float cg_erode_gather(const float* T, const uint8_t* ec, int y, int x, int H, int W) {
    float acc = 0.f;
    const int64_t q = (int64_t)y * W + x;
    if (y > 0) {           // (y, x) is the bottom of the column window of the pixel above
        const int e = ec[q - W];
        if ((e & 3) == 2) acc += 0.5f * (float)(e >> 4) * T[q - W];
    }
    if (x > 0) {           // the right end of the row window of the pixel to the left
        const int e = ec[q - 1];
        if (((e >> 2) & 3) == 2) acc += (1.f - 0.5f * (float)(e >> 4)) * T[q - 1];
    }
    {
        const int e = ec[q];
        const float wc = 0.5f * (float)(e >> 4);
        if ((e & 3) == 1) acc += wc * T[q];
        if (((e >> 2) & 3) == 1) acc += (1.f - wc) * T[q];
    }
    if (x + 1 < W) {
        const int e = ec[q + 1];
        if (((e >> 2) & 3) == 0) acc += (1.f - 0.5f * (float)(e >> 4)) * T[q + 1];
    }
    if (y + 1 < H) {
        const int e = ec[q + W];
        if ((e & 3) == 0) acc += 0.5f * (float)(e >> 4) * T[q + W];
    }
    return acc;
}

struct CgLevel {
    // P: level j of the recurrence at pixel o -> A_j (direct gradient of img_j), gD_j (gradient of dilate(img_{j+1})), g_skel_{j-1}
    int do_p, top;
    const float *img_j, *img_j1, *skel_prev;
    const uint8_t* dc_j1;   // D codes of the windows over img_{j+1}
    float* gs;
    const float* gskel_top;
    const double* g4;
    const float* y_true;
    float *A_out, *gD_out;
    // Q: T_m, the whole gradient of img_m (m = j + 2), from gD_{m-1}, A_m and T_{m+1}
    int do_q;
    const uint8_t *dc_m, *ec_m;   // D and E codes of the windows over img_m
    const float *gD_in, *A_in, *T_in;
    float* T_out;
};
// (A_out and A_in may be the same buffer: read and written at the same pixel by the same thread)
__global__ void cg_level_kernel(CgLevel a, int H, int W, int64_t total) {
    float g0 = 0.f, g1 = 0.f;
    if (a.do_p && a.top && a.g4) {
        g0 = (float)a.g4[0];
        g1 = (float)a.g4[1];
    }
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(o % W), y = (int)((o / W) % H);
        const int64_t pb = o - ((int64_t)y * W + x);   // first pixel of this plane
        float t = 0.f;
        if (a.do_q) {
            t = cg_dilate_gather(a.gD_in + pb, a.dc_m + pb, y, x, H, W);
            if (a.A_in) t += a.A_in[o];
            if (a.T_in) t += cg_erode_gather(a.T_in + pb, a.ec_m + pb, y, x, H, W);
        }
        if (a.do_p) {
            const int c = a.dc_j1[o];     // the window's maximum is the value at its first maximum
            const float raw = a.img_j[o] - a.img_j1[o + (int64_t)(c / 3 - 1) * W + (c % 3 - 1)];
            const float delta = fmaxf(raw, 0.f);
            float g;
            if (a.top) {
                g = a.gskel_top ? a.gskel_top[o] : 0.f;
                if (a.g4) g += fmaf(g0, a.y_true[o], g1);
            } else {
                g = a.gs[o];
            }
            float gd = g;
            if (a.skel_prev) {
                const float s = a.skel_prev[o];
                if (delta - s * delta > 0.f) {
                    gd = g - g * s;
                    g = g - g * delta;
                } else {
                    gd = 0.f;
                }
                a.gs[o] = g;
            }
            const bool on = raw > 0.f;
            a.A_out[o] = on ? gd : 0.f;
            a.gD_out[o] = on ? -gd : 0.f;
        }
        if (a.do_q) a.T_out[o] = t;
    }
}
// dL/dimg = A_0 + erode-gather of T_1 over img_0 (+ g2 * skel_true: the clDice tail's own term of y_pred)
__global__ void cg_final_kernel(const uint8_t* __restrict__ ec0, const float* __restrict__ A0, const float* __restrict__ T1,
                                const double* __restrict__ g4, const float* __restrict__ skel_true, float* __restrict__ dimg, int H,
                                int W, int64_t total) {
    const float g2 = g4 ? (float)g4[2] : 0.f;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(o % W), y = (int)((o / W) % H);
        const int64_t pb = o - ((int64_t)y * W + x);
        float d = A0[o] + cg_erode_gather(T1 + pb, ec0 + pb, y, x, H, W);
        if (g4) d = fmaf(g2, skel_true[o], d);
        dimg[o] = d;
    }
}

template <int K>
int cg_planes(const float* logits, const void* target, int target_f64, unsigned keep, int use_thr, float thr, float* pp, float* tp,
              int64_t HW, int64_t total, hipStream_t st) {
    hipLaunchKernelGGL((cg_planes_kernel<K>), dim3(cg_grid(total)), dim3(256), 0, st, logits, target, target_f64, keep, use_thr, thr, pp,
                       tp, HW, total);
    CMU_CHECK_LAUNCH("cmu_softmax_planes");
    return CMU_OK;
}
template <int K>
int cg_planes_bwd(const float* logits, const float* G, unsigned keep, float* dlogits, int64_t HW, int64_t total, hipStream_t st) {
    hipLaunchKernelGGL((cg_planes_bwd_kernel<K>), dim3(cg_grid(total)), dim3(256), 0, st, logits, G, keep, dlogits, HW, total);
    CMU_CHECK_LAUNCH("cmu_softmax_planes_bwd");
    return CMU_OK;
}
#define CG_DISPATCH_K(K, FN, ...)                   \
    switch (K) {                                    \
        case 2: return FN<2>(__VA_ARGS__);          \
        case 3: return FN<3>(__VA_ARGS__);          \
        case 4: return FN<4>(__VA_ARGS__);          \
        case 5: return FN<5>(__VA_ARGS__);          \
        case 6: return FN<6>(__VA_ARGS__);          \
        case 7: return FN<7>(__VA_ARGS__);          \
        default: return FN<8>(__VA_ARGS__);         \
    }

inline bool cg_keep_ok(unsigned keep, int K) { return keep != 0u && (keep >> K) == 0u; }

}  // namespace

extern "C" int cmu_softmax_planes(const float* logits, const void* target, int target_is_f64, int keep_mask, int use_threshold,
                                  float threshold, float* p_planes, float* t_planes, int B, int K, int H, int W, void* stream) {
    CMU_CHECK_ARG(logits && p_planes && B > 0 && H > 0 && W > 0 && (target != nullptr) == (t_planes != nullptr), "cmu_softmax_planes: bad args");
    CMU_CHECK_ARG(K >= 2 && K <= CG_MAX_K, "cmu_softmax_planes: 2 <= K <= %d classes (got %d)", CG_MAX_K, K);
    CMU_CHECK_ARG(cg_keep_ok((unsigned)keep_mask, K), "cmu_softmax_planes: keep mask 0x%x names no channel or one beyond %d", keep_mask, K);
    const int64_t HW = (int64_t)H * W;
    CG_DISPATCH_K(K, cg_planes, logits, target, target_is_f64, (unsigned)keep_mask, use_threshold, threshold, p_planes, t_planes, HW, HW * B,
                  (hipStream_t)stream);
}
extern "C" int cmu_softmax_planes_bwd(const float* logits, const float* g_planes, int keep_mask, float* dlogits, int B, int K, int H,
                                      int W, void* stream) {
    CMU_CHECK_ARG(logits && g_planes && dlogits && B > 0 && H > 0 && W > 0, "cmu_softmax_planes_bwd: bad args");
    CMU_CHECK_ARG(K >= 2 && K <= CG_MAX_K, "cmu_softmax_planes_bwd: 2 <= K <= %d classes (got %d)", CG_MAX_K, K);
    CMU_CHECK_ARG(cg_keep_ok((unsigned)keep_mask, K), "cmu_softmax_planes_bwd: keep mask 0x%x names no channel or one beyond %d", keep_mask, K);
    const int64_t HW = (int64_t)H * W;
    CG_DISPATCH_K(K, cg_planes_bwd, logits, g_planes, (unsigned)keep_mask, dlogits, HW, HW * B, (hipStream_t)stream);
}

// kept: img_1 .. img_{N+1} (N + 1 stacks of n floats), then skel_0 .. skel_{N-1} (N stacks; skel_N is the output), then one byte
// per pixel and level: the D codes of the windows over img_1 .. img_{N+1}, the E codes of the windows over img_0 .. img_N
extern "C" int64_t cmu_soft_skeleton_save_ws_bytes(int64_t n, int num_iter) {
    return (n <= 0 || num_iter < 0) ? 0 : (2 * (int64_t)num_iter + 1) * n * (int64_t)sizeof(float) + 2 * ((int64_t)num_iter + 1) * n;
}
extern "C" int cmu_soft_skeleton_save(const float* img, float* skel, int planes, int H, int W, int num_iter, void* kept, void* stream) {
    CMU_CHECK_ARG(img && skel && kept && planes > 0 && H > 0 && W > 0 && num_iter >= 0, "cmu_soft_skeleton_save: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)planes * H * W;
    const int grid = cg_grid(n);
    float* lev = (float*)kept;                           // lev + (i - 1) * n = img_i
    float* sk = lev + ((int64_t)num_iter + 1) * n;       // sk + i * n = skel_i
    uint8_t* dc = (uint8_t*)(sk + (int64_t)num_iter * n);   // dc + j * n = D codes over img_{j+1}
    uint8_t* ec = dc + ((int64_t)num_iter + 1) * n;         // ec + j * n = E codes over img_j
    for (int j = 0; j <= num_iter; ++j) {
        const float* cur = j == 0 ? img : lev + (int64_t)(j - 1) * n;
        float* nxt = lev + (int64_t)j * n;
        hipLaunchKernelGGL(cg_erode_kernel, dim3(grid), dim3(256), 0, st, cur, nxt, ec + (int64_t)j * n, H, W, n);
        CMU_CHECK_LAUNCH("cmu_soft_skeleton_save(erode)");
        hipLaunchKernelGGL(cg_update_kernel, dim3(grid), dim3(256), 0, st, cur, (const float*)nxt,
                           j == 0 ? (const float*)nullptr : (const float*)(sk + (int64_t)(j - 1) * n),
                           j == num_iter ? skel : sk + (int64_t)j * n, dc + (int64_t)j * n, H, W, n);
        CMU_CHECK_LAUNCH("cmu_soft_skeleton_save(update)");
    }
    return CMU_OK;
}

// ws: g_skel, A[2], gD[2], T[2]
extern "C" int64_t cmu_soft_skeleton_bwd_ws_bytes(int64_t n) { return n <= 0 ? 0 : 7 * n * (int64_t)sizeof(float); }
extern "C" int cmu_soft_skeleton_bwd(const float* img, const void* kept, const float* g_skel, const double* g4, const float* y_true,
                                     const float* skel_true, float* dimg, int planes, int H, int W, int num_iter, void* ws, void* stream) {
    CMU_CHECK_ARG(img && kept && dimg && ws && planes > 0 && H > 0 && W > 0 && num_iter >= 0, "cmu_soft_skeleton_bwd: bad args");
    CMU_CHECK_ARG(g_skel || g4, "cmu_soft_skeleton_bwd: neither g_skel nor the clDice tail's g4 given");
    CMU_CHECK_ARG(!g4 || (y_true && skel_true), "cmu_soft_skeleton_bwd: g4 needs y_true and skel_true");
    hipStream_t st = (hipStream_t)stream;
    const int N = num_iter;
    const int64_t n = (int64_t)planes * H * W;
    const int grid = cg_grid(n);
    const float* lev = (const float*)kept;
    const float* sk = lev + ((int64_t)N + 1) * n;
    const uint8_t* dc = (const uint8_t*)(sk + (int64_t)N * n);   // dc + j * n = D codes over img_{j+1}
    const uint8_t* ec = dc + ((int64_t)N + 1) * n;               // ec + j * n = E codes over img_j
    float* gs = (float*)ws;
    float* A[2] = {gs + n, gs + 2 * n};
    float* gD[2] = {gs + 3 * n, gs + 4 * n};
    float* T[2] = {gs + 5 * n, gs + 6 * n};
    auto image = [&](int i) { return i == 0 ? img : lev + (int64_t)(i - 1) * n; };
    for (int j = N; j >= -1; --j) {       // j = -1: only T_1 is left to gather
        CgLevel a = {};
        if (j >= 0) {
            a.do_p = 1;
            a.top = j == N;
            a.img_j = image(j);
            a.img_j1 = image(j + 1);
            a.dc_j1 = dc + (int64_t)j * n;
            a.skel_prev = j > 0 ? sk + (int64_t)(j - 1) * n : nullptr;
            a.gs = gs;
            a.gskel_top = g_skel;
            a.g4 = g4;
            a.y_true = y_true;
            a.A_out = A[j & 1];
            a.gD_out = gD[j & 1];
        }
        const int m = j + 2;              // T_m from gD_{m-1}, A_m, T_{m+1}
        if (m <= N + 1) {
            a.do_q = 1;
            a.dc_m = dc + (int64_t)(m - 1) * n;
            a.ec_m = m <= N ? ec + (int64_t)m * n : nullptr;
            a.gD_in = gD[(m - 1) & 1];
            a.A_in = m <= N ? A[m & 1] : nullptr;
            a.T_in = m <= N ? T[(m + 1) & 1] : nullptr;
            a.T_out = T[m & 1];
        }
        hipLaunchKernelGGL(cg_level_kernel, dim3(grid), dim3(256), 0, st, a, H, W, n);
        CMU_CHECK_LAUNCH("cmu_soft_skeleton_bwd(level)");
    }
    hipLaunchKernelGGL(cg_final_kernel, dim3(grid), dim3(256), 0, st, ec, (const float*)A[0], (const float*)T[1], g4, skel_true, dimg,
                       H, W, n);
    CMU_CHECK_LAUNCH("cmu_soft_skeleton_bwd(final)");
    return CMU_OK;
}
