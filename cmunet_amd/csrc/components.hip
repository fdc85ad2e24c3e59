// components.hip -- connected components of uint8 label maps on the device, and the clean-up passes built on them (remove small
// objects, keep the n largest, fill holes).  DESIGN.md section 4.20.
//
// cmu_label_components: block-based union-find (Komura 2015; Playne & Hawick 2018), a FIXED sequence of launches whatever the content:
//   1. cc_tile_kernel   one workgroup per 32 x 32 tile: union-find in LDS over the tile's pixels, then every pixel's parent in the
//                       global parent array (workspace) is set to the tile-local root, as an index of the image;
//   2. cc_seam_kernel   one thread per pixel next to a tile seam: unions across the seam in the global parent array.  Workgroups on
//                       different XCDs touch the same entries here: EVERY access to the parent array in this kernel is an
//                       agent-scope atomic (load, min), which is served by the device-coherent level, never by a CU's L1;
//   3. cc_flatten_kernel  after the kernel boundary: every pixel walks to its root, writes label = root + 1 (0 on background), stores
//                       the root as its parent (path compression for the walkers behind it: any value stored is an ancestor, so a
//                       racing reader still arrives at the same root) and roots are counted, one add per wave;
//   4. cc_counts_kernel counts[b] = number of roots, or -1 if any walk of image b overran its trip bound.
// The union keeps the smaller root, so the root of a component is its smallest row-major index (components_uf.h has the argument
// and the termination proof): the labels do not depend on launch order, tile shape or timing.
#include "common.h"
#include "components_uf.h"

namespace {

constexpr int T = CMU_CC_TILE;
constexpr int CC_THREADS = 256;

inline int64_t cc_align256(int64_t n) { return (n + 255) / 256 * 256; }

// parent array in LDS, shared by one workgroup
struct LdsParents {
    int* p;
    __device__ int load(int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ int fetch_min(int i, int v) { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
// parent array of one image in global memory, shared by workgroups on any XCD: agent-scope atomics only
struct AgentParents {
    int* p;
    __device__ int load(int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ int fetch_min(int i, int v) { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// grid (tiles_x, tiles_y, B)
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const uint8_t* __restrict__ src, int cls, int conn, int* __restrict__ parent,
                                                             int* __restrict__ over, int H, int W) {
    __shared__ int lp[T * T];
    __shared__ uint8_t fg[T * T];
    const int b = blockIdx.z, x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int tw = min(T, W - x0), th = min(T, H - y0);
    const int64_t base = (int64_t)b * H * W;
    for (int i = threadIdx.x; i < T * T; i += CC_THREADS) {
        const int lx = i % T, ly = i / T;
        const bool f = lx < tw && ly < th && cmu_uf_foreground(src[base + (int64_t)(y0 + ly) * W + x0 + lx], cls);
        fg[i] = f;
        lp[i] = f ? i : -1;
    }
    __syncthreads();
    LdsParents a{lp};
    int ov = 0;
    for (int i = threadIdx.x; i < T * T; i += CC_THREADS) cmu_uf_tile_link(a, fg, i % T, i / T, tw, conn, &ov);
    __syncthreads();
    for (int i = threadIdx.x; i < T * T; i += CC_THREADS) {
        const int lx = i % T, ly = i / T;
        if (lx < tw && ly < th) {
            int g = -1;
            if (fg[i]) {
                const int r = cmu_uf_find(a, i, T * T, &ov);
                g = (y0 + r / T) * W + x0 + r % T;
            }
            parent[base + (int64_t)(y0 + ly) * W + x0 + lx] = g;
        }
    }
    if (ov) atomicMax(over + b, 1);
}

// grid (ceil(H*W / 256), B)
__global__ __launch_bounds__(CC_THREADS) void cc_seam_kernel(const uint8_t* __restrict__ src, int cls, int conn, int* parent, int* __restrict__ over,
                                                             int H, int W) {
    const int b = blockIdx.y, HW = H * W;
    const int64_t base = (int64_t)b * HW;
    AgentParents a{parent + base};
    int ov = 0;
    for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * CC_THREADS)
        cmu_uf_seam_link(a, src + base, cls, (int)(i % W), (int)(i / W), W, H, conn, &ov);
    if (ov) atomicMax(over + b, 1);
}

// grid (ceil(H*W / 256), B): one pixel per thread, no thread leaves before the ballot
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* parent, int* __restrict__ labels, int* __restrict__ nroots,
                                                                int* __restrict__ over, int H, int W) {
    const int b = blockIdx.y, HW = H * W;
    const int64_t base = (int64_t)b * HW;
    AgentParents a{parent + base};
    const int64_t i64 = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    int ov = 0;
    bool root = false;
    if (i64 < HW) {
        const int i = (int)i64;
        int lab = 0;
        if (a.load(i) >= 0) {
            const int r = cmu_uf_find(a, i, HW, &ov);
            root = r == i;
            if (!root) __hip_atomic_store(parent + base + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lab = r + 1;
        }
        labels[base + i] = lab;
    }
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(nroots + b, __popcll(m));
    if (ov) atomicMax(over + b, 1);
}

__global__ void cc_counts_kernel(const int* __restrict__ nroots, const int* __restrict__ over, int* __restrict__ counts, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) counts[b] = over[b] ? -1 : nroots[b];
}

// sizes[b, label - 1] += pixels: the lanes of a wave that hold the same label -- adjacent or not -- are counted with a ballot and
// ONE lane adds their number: one atomic add per distinct label of a wave (64 consecutive pixels of a row-major scan) instead of one
// per pixel.  A large ragged component, whose pixels alternate with background along a row, costs one add per wave this way; with one
// add per row-run the adds to its single counter serialised (2.1 ms instead of 0.1 for 32 near-percolation masks of 475 x 475).
// The loop is wave-uniform (``todo`` is a ballot) and runs once per distinct label: at most 64 trips.
__global__ __launch_bounds__(CC_THREADS) void cc_sizes_kernel(const int* __restrict__ labels, int* __restrict__ sizes, int HW) {
    const int b = blockIdx.y;
    const int64_t base = (int64_t)b * HW;
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int lab = i < HW ? labels[base + i] : 0;
    if (lab > HW) lab = 0;      // (not a label of an image of this size: never index with it)
    unsigned long long todo = __ballot(lab > 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int cur = __shfl(lab, leader, 64);
        const unsigned long long same = __ballot(lab == cur);
        if (lane == leader) atomicAdd(sizes + base + cur - 1, __popcll(same));
        todo &= ~same;
    }
}

// one workgroup per image; round k picks the largest key below the previous pick (components_uf.h: size first, then the smaller
// index).  Maximum of distinct keys: the result does not depend on the order of the reduction, which is fixed anyway.
constexpr int SEL_THREADS = 1024;
__global__ __launch_bounds__(SEL_THREADS) void cc_select_kernel(const int* __restrict__ sizes, int n, int* __restrict__ keep, int HW) {
    __shared__ uint64_t red[SEL_THREADS];
    const int b = blockIdx.x;
    const int* s = sizes + (int64_t)b * HW;
    uint64_t bound = ~0ull;
    for (int k = 0; k < n; ++k) {
        uint64_t best = 0;
        for (int i = threadIdx.x; i < HW; i += SEL_THREADS) {
            const int v = s[i];
            if (v > 0) {
                const uint64_t key = cmu_uf_rank_key(v, i);
                if (key < bound && key > best) best = key;
            }
        }
        red[threadIdx.x] = best;
        __syncthreads();
        for (int o = SEL_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o && red[threadIdx.x + o] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + o];
            __syncthreads();
        }
        best = red[0];
        __syncthreads();
        if (threadIdx.x == 0) keep[b * n + k] = best ? (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu)) + 1 : -1;
        if (best) bound = best;
        else bound = 0;        // nothing left: every later slot is -1
    }
}

// grid (ceil(2 (H + W) / 256), B): the frame's pixels, corners visited twice (every writer stores the same 1)
__global__ void cc_border_kernel(const int* __restrict__ labels, uint8_t* __restrict__ touches, int H, int W) {
    const int b = blockIdx.y;
    const int64_t base = (int64_t)b * H * W;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    int x, y;
    if (t < W) { x = t; y = 0; }
    else if (t < 2 * W) { x = t - W; y = H - 1; }
    else if (t < 2 * W + H) { x = 0; y = t - 2 * W; }
    else if (t < 2 * W + 2 * H) { x = W - 1; y = t - 2 * W - H; }
    else return;
    const int lab = labels[base + (int64_t)y * W + x];
    if (lab > 0 && lab <= H * W) touches[base + lab - 1] = 1;
}

__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const uint8_t* __restrict__ src, int cls, const int* __restrict__ labels,
                                                               const int* __restrict__ sizes, int min_size, const int* __restrict__ keep, int n_keep,
                                                               int removed, const int* __restrict__ hole_labels, const uint8_t* __restrict__ hole_touches,
                                                               const uint8_t* __restrict__ lut, int n_lut, uint8_t* __restrict__ out, int HW) {
    const int b = blockIdx.y;
    const int64_t base = (int64_t)b * HW;
    for (int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * CC_THREADS) {
        int v = src[base + i];
        const int lab = labels ? labels[base + i] : 0;
        if (lab > 0 && lab <= HW) {
            bool ok = sizes[base + lab - 1] >= min_size;
            if (ok && keep) {
                ok = false;
                for (int k = 0; k < n_keep; ++k) ok = ok || keep[b * n_keep + k] == lab;
            }
            if (!ok) v = removed;
        }
        if (hole_labels) {
            const int hl = hole_labels[base + i];
            if (hl > 0 && hl <= HW && !hole_touches[base + hl - 1]) v = cls;
        }
        out[base + i] = lut && v < n_lut ? lut[v] : (uint8_t)v;      // (a value the table does not cover passes through)
    }
}

inline bool cc_shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31); }
inline unsigned cc_pixel_blocks(int H, int W) { return (unsigned)cmu_div_up64((int64_t)H * W, CC_THREADS); }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t cmu_label_components_ws_bytes(int B, int H, int W) {
    if (!cc_shape_ok(B, H, W)) return 0;
    return cc_align256(2 * (int64_t)B * (int64_t)sizeof(int)) + cc_align256((int64_t)B * H * W * (int64_t)sizeof(int));
}

extern "C" int cmu_label_components(const uint8_t* src, int cls, int connectivity, int32_t* labels, int32_t* counts, int B, int H, int W, void* ws,
                                    void* stream) {
    CMU_CHECK_ARG(src && labels && counts && ws && cc_shape_ok(B, H, W), "cmu_label_components: bad args (1 <= B <= 65535, 1 <= H, W, H * W < 2^31)");
    CMU_CHECK_ARG(connectivity == 4 || connectivity == 8, "cmu_label_components: connectivity must be 4 or 8, got %d", connectivity);
    CMU_CHECK_ARG(cls >= -257 && cls <= 255, "cmu_label_components: cls in 0..255, -1 (non-zero) or -2 - c (not class c), got %d", cls);
    const int tx = cmu_div_up(W, T), ty = cmu_div_up(H, T);
    CMU_CHECK_ARG(ty <= 65535, "cmu_label_components: H <= %d", 65535 * T);
    hipStream_t st = (hipStream_t)stream;
    int* nroots = (int*)ws;
    int* over = nroots + B;
    int* parent = (int*)((char*)ws + cc_align256(2 * (int64_t)B * (int64_t)sizeof(int)));
    if (hipMemsetAsync(ws, 0, 2 * (size_t)B * sizeof(int), st) != hipSuccess) { cmu_set_error("cmu_label_components: memset"); return CMU_ERR_LAUNCH; }
    hipLaunchKernelGGL(cc_tile_kernel, dim3(tx, ty, B), dim3(CC_THREADS), 0, st, src, cls, connectivity, parent, over, H, W);
    CMU_CHECK_LAUNCH("cmu_label_components(tile)");
    const unsigned pb = cc_pixel_blocks(H, W);
    if (tx > 1 || ty > 1) {      // (a host-side property of the shape, not of the content)
        hipLaunchKernelGGL(cc_seam_kernel, dim3(pb, B), dim3(CC_THREADS), 0, st, src, cls, connectivity, parent, over, H, W);
        CMU_CHECK_LAUNCH("cmu_label_components(seam)");
    }
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(pb, B), dim3(CC_THREADS), 0, st, parent, labels, nroots, over, H, W);
    CMU_CHECK_LAUNCH("cmu_label_components(flatten)");
    hipLaunchKernelGGL(cc_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const int*)nroots, (const int*)over, counts, B);
    CMU_CHECK_LAUNCH("cmu_label_components(counts)");
    return CMU_OK;
}

extern "C" int cmu_component_sizes(const int32_t* labels, int32_t* sizes, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(labels && sizes && cc_shape_ok(B, H, W), "cmu_component_sizes: bad args");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sizes, 0, (size_t)B * H * W * sizeof(int), st) != hipSuccess) { cmu_set_error("cmu_component_sizes: memset"); return CMU_ERR_LAUNCH; }
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(cc_pixel_blocks(H, W), B), dim3(CC_THREADS), 0, st, labels, sizes, H * W);
    CMU_CHECK_LAUNCH("cmu_component_sizes");
    return CMU_OK;
}

extern "C" int cmu_select_largest(const int32_t* sizes, int n, int32_t* keep_roots, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(sizes && keep_roots && cc_shape_ok(B, H, W), "cmu_select_largest: bad args");
    CMU_CHECK_ARG(n >= 1 && n <= 8, "cmu_select_largest: n in 1..8, got %d", n);
    hipLaunchKernelGGL(cc_select_kernel, dim3(B), dim3(SEL_THREADS), 0, (hipStream_t)stream, sizes, n, keep_roots, H * W);
    CMU_CHECK_LAUNCH("cmu_select_largest");
    return CMU_OK;
}

extern "C" int cmu_border_components(const int32_t* labels, uint8_t* touches, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(labels && touches && cc_shape_ok(B, H, W) && (int64_t)H + W < (1 << 30), "cmu_border_components: bad args");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(touches, 0, (size_t)B * H * W, st) != hipSuccess) { cmu_set_error("cmu_border_components: memset"); return CMU_ERR_LAUNCH; }
    hipLaunchKernelGGL(cc_border_kernel, dim3((2 * (H + W) + 255) / 256, B), dim3(256), 0, st, labels, touches, H, W);
    CMU_CHECK_LAUNCH("cmu_border_components");
    return CMU_OK;
}

extern "C" int cmu_filter_components(const uint8_t* src, int cls, const int32_t* labels, const int32_t* sizes, int min_size, const int32_t* keep_roots,
                                     int n_keep, int removed_value, const int32_t* hole_labels, const uint8_t* hole_touches,
                                     const uint8_t* class_values, int n_values, uint8_t* out, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(src && out && cc_shape_ok(B, H, W), "cmu_filter_components: bad args");
    CMU_CHECK_ARG(cls >= 0 && cls <= 255 && removed_value >= 0 && removed_value <= 255 && min_size >= 0, "cmu_filter_components: cls, removed_value in 0..255, min_size >= 0");
    CMU_CHECK_ARG(!labels == !sizes, "cmu_filter_components: labels and sizes come together");
    CMU_CHECK_ARG(!keep_roots || (labels && n_keep >= 1 && n_keep <= 8), "cmu_filter_components: keep_roots needs labels and n_keep in 1..8");
    CMU_CHECK_ARG(!class_values || (n_values >= 1 && n_values <= 256), "cmu_filter_components: class_values holds 1..256 bytes");
    CMU_CHECK_ARG(!hole_labels == !hole_touches, "cmu_filter_components: hole_labels and hole_touches come together");
    const unsigned pb = cc_pixel_blocks(H, W);
    hipLaunchKernelGGL(cc_filter_kernel, dim3(pb < 1024 ? pb : 1024, B), dim3(CC_THREADS), 0, (hipStream_t)stream, src, cls, labels, sizes, min_size,
                       keep_roots, n_keep, removed_value, hole_labels, hole_touches, class_values, n_values, out, H * W);
    CMU_CHECK_LAUNCH("cmu_filter_components");
    return CMU_OK;
}
