// genesis.hip -- Models Genesis / MAE baseline pretraining inputs on the device (Pretraining/Transformation_based/utils.py:69-253,
// Genesis_Chest_CT.py:65-181).  The reference draws every batch with single-threaded numpy inside the training loop; here a batch is
//
//   cmu_genesis_sample          one PER-IMAGE RECORD (GenesisRec) per image: dataset index, flip parities, branch flags, Bezier draws,
//                               paint mode + rectangles, and (local shuffle) 10,000 blocks + one uniform permutation per block --
//                               Philox4x32-10 keyed by (seed, offset).  The host replay (genesis.py) fills the SAME records from
//                               Python's random + a numpy RandomState in the reference's order instead.
//   cmu_genesis_gather_shuffle  y = flip(src[idx]); x = local pixel shuffle of y (owner map in LDS: the LAST block covering a pixel
//                               wins, atomicMax of the block number); per-(image, row segment) min / max of x
//   cmu_genesis_bezier          the two sampled cubics (100,000 points, fp64), sorted without a general sort: a cubic's samples form
//                               a few monotone runs (3 in exact arithmetic); runs are found on the device and merged by rank
//                               (more than GEN_MAX_RUNS runs -- a near-constant image -- fall back to a general sort)
//   cmu_genesis_intensity_paint np.interp through the table (fp64) and in- / out-painting
//   cmu_genesis_mae             y = src[idx], x = y * (1 - mask)
//   cmu_mse_fwd_bwd             nn.MSELoss()(logits[:, 0], y) + its gradient, fixed-order reduction
//
// Built with -ffp-contract=off (Makefile): every multiply and add of the fp32 control points and of np.interp rounds on its own.
#include "philox_stream.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------
// the per-image record (layout mirrored by genesis.REC_DTYPE; cmu_genesis_rec_bytes() lets the host check it)
// ---------------------------------------------------------------------------------------------
struct GenesisRec {
    int32_t src;            // dataset index
    int32_t flags;          // GF_* bits
    int32_t paint;          // 0 none, 1 in-painting, 2 out-painting
    int32_t nrect;          // rectangles used (in: <= 5, out: 1 + <= 4)
    int16_t rect[5][4];     // x0 (row), y0 (col), sx, sy
    int32_t nblocks;        // local-shuffle blocks (0 or 10,000)
    int32_t slot;           // bytes per block in the permutation pool ((H / 25) * (W / 25))
    int64_t block_off;      // first block of this image in the block table (int16 x0, y0, bx, by per block)
    int64_t perm_off;       // first byte of this image in the permutation pool
    double bez[4];          // the four random.random() of the Bezier control points, in the reference's order
};
static_assert(sizeof(GenesisRec) == 112, "GenesisRec layout");
enum { GF_FLIP0 = 1, GF_FLIP1 = 2, GF_LOCAL = 4, GF_NONLIN = 8, GF_SORTY = 16 };
constexpr int GEN_NBLOCKS = 10000;
constexpr int GEN_NT = 100000;          // Bezier samples
constexpr int GEN_MAX_RUNS = 16;        // monotone runs the rank merge handles; more go to gen_sort_general
constexpr int GEN_OWNER_WORDS = 32768;  // LDS owner map (128 KB)
constexpr int GEN_MAX_SLOT = 256;       // permutation indices are bytes
constexpr int GEN_MAX_B = 1024;
constexpr int GEN_SLICES = 8;          // workgroups per image of the sampler

extern "C" int cmu_genesis_rec_bytes() { return (int)sizeof(GenesisRec); }
static inline int gen_seg_rows(int H, int W) { return H < GEN_OWNER_WORDS / W ? H : GEN_OWNER_WORDS / W; }
extern "C" int cmu_genesis_segments(int H, int W) { return W > 0 && W <= GEN_OWNER_WORDS ? cmu_div_up(H, gen_seg_rows(H, W)) : 0; }

// ---------------------------------------------------------------------------------------------
// Philox streams (PhiloxStream, philox_stream.h).  Stream id (c1) = purpose << 28 | image << 14 | block; (c2, c3) = offset.
// ---------------------------------------------------------------------------------------------
enum { GS_SELECT = 0, GS_RECORD = 1, GS_BLOCK = 2, GS_NOISE = 3 };
__device__ static inline uint32_t gen_id(int purpose, int img, int blk) { return ((uint32_t)purpose << 28) | ((uint32_t)img << 14) | (uint32_t)blk; }
// paint noise of pixel p of image b: float32(np.random.rand()) law
__device__ static inline float gen_noise(uint64_t seed, uint64_t offset, int b, int64_t p) {
    uint32_t r[4];
    philox4x32_10((uint32_t)p, gen_id(GS_NOISE, b, 0) | (uint32_t)(p >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    return (float)philox_u53(r[0], r[1]);
}

// data_augmentation's flip loop (`while random.random() < prob and cnt > 0`: the draw comes before the count test) and
// local_pixel_shuffling's branch -> GF_FLIP0 / GF_FLIP1 / GF_LOCAL bits
__device__ static inline int gen_flips_local(PhiloxStream& s, double flip_rate, double local_rate) {
    int flags = 0, cnt = 3;
    while (s.uniform() < flip_rate && cnt > 0) {
        flags ^= s.below(2) ? GF_FLIP1 : GF_FLIP0;
        --cnt;
    }
    if (!(s.uniform() >= local_rate)) flags |= GF_LOCAL;
    return flags;
}

// ---------------------------------------------------------------------------------------------
// device sampler: GEN_SLICES workgroups per image.  Thread 0 of the first draws the record with the reference's laws (generate_pair /
// data_augmentation / local_pixel_shuffling / nonlinear_transformation / image_in_painting / image_out_painting); the block table and
// the Fisher-Yates permutations are split over the slices, one block per thread at a time.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void genesis_sample_kernel(GenesisRec* __restrict__ recs, int16_t* __restrict__ blocks,
                                                            uint8_t* __restrict__ perms, int N, int H, int W, int mae, double flip_rate,
                                                            double local_rate, double nonlinear_rate, double paint_rate,
                                                            double inpaint_rate, uint64_t seed, uint64_t offset) {
    __shared__ int chosen[GEN_MAX_B];
    __shared__ int local;
    __shared__ uint8_t scratch[256][GEN_MAX_SLOT];
    const int b = blockIdx.x;
    const int slot = (H / 25) * (W / 25);
    if (threadIdx.x == 0 && blockIdx.y != 0) {
        // the other slices of the image only need the local-shuffle decision: replay the record stream up to it
        PhiloxStream s(seed, offset, gen_id(GS_RECORD, b, 0));
        local = mae ? 0 : gen_flips_local(s, flip_rate, local_rate) & GF_LOCAL;
    }
    if (threadIdx.x == 0 && blockIdx.y == 0) {
        GenesisRec r = {};
        // batch selection: random.shuffle(index)[:B] is a uniformly random ordered sample without replacement -- sequential
        // rejection sampling has the same law (every image's workgroup replays the draws up to its own position)
        PhiloxStream sel(seed, offset, gen_id(GS_SELECT, 0, 0));
        for (int i = 0; i <= b; ++i) {
            int j;
            bool dup;
            do {
                j = (int)sel.below((uint32_t)N);
                dup = false;
                for (int q = 0; q < i; ++q) dup |= chosen[q] == j;
            } while (dup);
            chosen[i] = j;
        }
        r.src = chosen[b];
        r.slot = slot;
        r.block_off = (int64_t)b * GEN_NBLOCKS;
        r.perm_off = (int64_t)b * GEN_NBLOCKS * slot;
        if (!mae) {
            PhiloxStream s(seed, offset, gen_id(GS_RECORD, b, 0));
            r.flags = gen_flips_local(s, flip_rate, local_rate);
            if (r.flags & GF_LOCAL) r.nblocks = GEN_NBLOCKS;
            int cnt;
            if (!(s.uniform() >= nonlinear_rate)) {
                r.flags |= GF_NONLIN;
                for (int k = 0; k < 4; ++k) r.bez[k] = s.uniform();
                if (!(s.uniform() < 0.5)) r.flags |= GF_SORTY;
            }
            if (s.uniform() < paint_rate) {
                if (s.uniform() < inpaint_rate) {
                    r.paint = 1;
                    cnt = 5;
                    while (cnt > 0 && s.uniform() < 0.95) {       // (count tested first: no draw once it is 0)
                        const int sx = s.randint(H / 6, H / 3), sy = s.randint(W / 6, W / 3);
                        const int x0 = s.randint(3, H - sx - 3), y0 = s.randint(3, W - sy - 3);
                        int16_t* q = r.rect[r.nrect++];
                        q[0] = (int16_t)x0; q[1] = (int16_t)y0; q[2] = (int16_t)sx; q[3] = (int16_t)sy;
                        --cnt;
                    }
                } else {
                    r.paint = 2;
                    int sx = H - s.randint(2 * H / 7, 4 * H / 7), sy = W - s.randint(2 * W / 7, 4 * W / 7);
                    int x0 = s.randint(3, H - sx - 3), y0 = s.randint(3, W - sy - 3);
                    int16_t* q = r.rect[r.nrect++];
                    q[0] = (int16_t)x0; q[1] = (int16_t)y0; q[2] = (int16_t)sx; q[3] = (int16_t)sy;
                    cnt = 4;
                    while (cnt > 0 && s.uniform() < 0.95) {
                        sx = H - s.randint(3 * H / 7, 4 * H / 7);
                        sy = W - s.randint(3 * W / 7, 4 * W / 7);
                        x0 = s.randint(3, H - sx - 3);
                        y0 = s.randint(3, W - sy - 3);
                        q = r.rect[r.nrect++];
                        q[0] = (int16_t)x0; q[1] = (int16_t)y0; q[2] = (int16_t)sx; q[3] = (int16_t)sy;
                        --cnt;
                    }
                }
            }
        }
        local = r.nblocks;
        recs[b] = r;
    }
    __syncthreads();
    if (local == 0) return;
    uint8_t* sc = scratch[threadIdx.x];
    const int per = (GEN_NBLOCKS + gridDim.y - 1) / gridDim.y, k1 = min(GEN_NBLOCKS, (int)(blockIdx.y + 1) * per);
    for (int k = blockIdx.y * per + threadIdx.x; k < k1; k += 256) {
        PhiloxStream s(seed, offset, gen_id(GS_BLOCK, b, k));
        const int bx = s.randint(1, H / 25), by = s.randint(1, W / 25);
        const int x0 = s.randint(0, H - bx), y0 = s.randint(0, W - by);
        int16_t* q = blocks + ((int64_t)b * GEN_NBLOCKS + k) * 4;
        q[0] = (int16_t)x0; q[1] = (int16_t)y0; q[2] = (int16_t)bx; q[3] = (int16_t)by;
        const int n = bx * by;
        for (int i = 0; i < n; ++i) sc[i] = (uint8_t)i;
        for (int i = n - 1; i > 0; --i) {                       // Fisher-Yates: uniform over the n! orders
            const int j = (int)s.below((uint32_t)(i + 1));
            const uint8_t t = sc[i];
            sc[i] = sc[j];
            sc[j] = t;
        }
        uint8_t* dst = perms + ((int64_t)b * GEN_NBLOCKS + k) * slot;
        for (int i = 0; i < n; ++i) dst[i] = sc[i];
    }
}
extern "C" int cmu_genesis_sample(void* recs, int16_t* blocks, uint8_t* perms, int N, int B, int H, int W, int mae, double flip_rate,
                                  double local_rate, double nonlinear_rate, double paint_rate, double inpaint_rate, uint64_t seed,
                                  uint64_t offset, void* stream) {
    CMU_CHECK_ARG(recs && N > 0 && B > 0 && B <= GEN_MAX_B && B <= N && H >= 25 && W >= 25 && H <= 4096 && W <= 4096,
                  "cmu_genesis_sample: bad args (N %d, B %d, %dx%d)", N, B, H, W);
    CMU_CHECK_ARG(mae || (blocks && perms && (H / 25) * (W / 25) <= GEN_MAX_SLOT && H >= 42 && W >= 42),
                  "cmu_genesis_sample: %dx%d needs 42 <= side and (H/25)*(W/25) <= %d", H, W, GEN_MAX_SLOT);
    hipLaunchKernelGGL(genesis_sample_kernel, dim3(B, mae ? 1 : GEN_SLICES), dim3(256), 0, (hipStream_t)stream, (GenesisRec*)recs, blocks, perms, N, H, W, mae,
                       flip_rate, local_rate, nonlinear_rate, paint_rate, inpaint_rate, seed, offset);
    CMU_CHECK_LAUNCH("cmu_genesis_sample");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// gather + flip + local pixel shuffle.  Grid (segments, B): a segment is a band of rows whose owner map fits in LDS.  Every block
// reads the UNMODIFIED (flipped) image and the last block covering a pixel wins, so x[i][j] = orig[block origin + perm_b(p)] with b the
// largest block number covering (i, j) -- found with atomicMax of b + 1 (0 = not covered).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void genesis_gather_kernel(const float* __restrict__ src, const GenesisRec* __restrict__ recs,
                                                             const int16_t* __restrict__ blocks, const uint8_t* __restrict__ perms,
                                                             float* __restrict__ x, float* __restrict__ y, float* __restrict__ minmax,
                                                             int H, int W, int R) {
    __shared__ uint32_t owner[GEN_OWNER_WORDS];
    __shared__ float red[2][16];
    const int seg = blockIdx.x, b = blockIdx.y, nseg = gridDim.x;
    const int r0 = seg * R, r1 = min(H, r0 + R);
    const GenesisRec& rec = recs[b];
    const int flags = rec.flags, nb = rec.nblocks, slot = rec.slot;
    const float* img = src + (int64_t)rec.src * H * W;
    const int n = (r1 - r0) * W;
    for (int i = threadIdx.x; i < n; i += 1024) owner[i] = 0u;
    __syncthreads();
    const int16_t* bt = blocks + rec.block_off * 4;
    for (int k = threadIdx.x; k < nb; k += 1024) {
        const int x0 = bt[4 * k], y0 = bt[4 * k + 1], bx = bt[4 * k + 2], by = bt[4 * k + 3];
        const int a = max(x0, r0), e = min(x0 + bx, r1);
        for (int i = a; i < e; ++i)
            for (int j = y0; j < y0 + by; ++j) atomicMax(&owner[(i - r0) * W + j], (uint32_t)(k + 1));
    }
    __syncthreads();
    const bool f0 = flags & GF_FLIP0, f1 = flags & GF_FLIP1;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int p = threadIdx.x; p < n; p += 1024) {
        const int i = r0 + p / W, j = p % W;
        int si = i, sj = j;
        const uint32_t o = owner[p];
        if (o != 0u) {
            const int k = (int)o - 1;
            const int x0 = bt[4 * k], y0 = bt[4 * k + 1], by = bt[4 * k + 3];
            const int q = perms[rec.perm_off + (int64_t)k * slot + (i - x0) * by + (j - y0)];
            si = x0 + q / by;
            sj = y0 + q % by;
        }
        const float v = img[(int64_t)(f0 ? H - 1 - si : si) * W + (f1 ? W - 1 - sj : sj)];
        const int64_t o_ = ((int64_t)b * H + i) * W + j;
        x[o_] = v;
        y[o_] = img[(int64_t)(f0 ? H - 1 - i : i) * W + (f1 ? W - 1 - j : j)];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = mn;
        red[1][threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            mn = fminf(mn, red[0][w]);
            mx = fmaxf(mx, red[1][w]);
        }
        minmax[2 * ((int64_t)b * nseg + seg)] = mn;
        minmax[2 * ((int64_t)b * nseg + seg) + 1] = mx;
    }
}
extern "C" int cmu_genesis_gather_shuffle(const float* src, const void* recs, const int16_t* blocks, const uint8_t* perms, float* x, float* y,
                                          float* minmax, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(src && recs && x && y && minmax && B > 0 && H > 0 && W > 0 && W <= GEN_OWNER_WORDS,
                  "cmu_genesis_gather_shuffle: bad args");
    const int R = gen_seg_rows(H, W);
    hipLaunchKernelGGL(genesis_gather_kernel, dim3(cmu_div_up(H, R), B), dim3(1024), 0, (hipStream_t)stream, src, (const GenesisRec*)recs,
                       blocks, perms, x, y, minmax, H, W, R);
    CMU_CHECK_LAUNCH("cmu_genesis_gather_shuffle");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// Bezier tables.  nonlinear_transformation: control points (min,min), (c1,c2), (c3,c4), (max,max) with c = r * (max - min) + min in
// float32 (numpy >= 2: a Python float times a float32 scalar stays float32), bezier_curve's Bernstein form in reversed t order
// (t**(n-i) * (1-t)**i: t = 0 is the (max, max) end), t = np.linspace(0, 1, 100000).
// ws per image: [raw x][raw y][sorted x][sorted y], GEN_NT doubles each.
// ---------------------------------------------------------------------------------------------
__device__ static inline void gen_controls(const GenesisRec& r, const float* __restrict__ minmax, int b, int nseg, double* cx, double* cy) {
    float mn = minmax[2 * (int64_t)b * nseg], mx = minmax[2 * (int64_t)b * nseg + 1];
    for (int s = 1; s < nseg; ++s) {
        mn = fminf(mn, minmax[2 * ((int64_t)b * nseg + s)]);
        mx = fmaxf(mx, minmax[2 * ((int64_t)b * nseg + s) + 1]);
    }
    const float d = __fsub_rn(mx, mn);
    float c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = __fadd_rn(__fmul_rn((float)r.bez[k], d), mn);
    cx[0] = mn; cx[1] = c[0]; cx[2] = c[2]; cx[3] = mx;
    cy[0] = mn; cy[1] = c[1]; cy[2] = c[3]; cy[3] = mx;
}
__device__ static inline double gen_bezier(const double* P, int k) {
    const double step = 1.0 / (double)(GEN_NT - 1);
    const double t = k == GEN_NT - 1 ? 1.0 : (double)k * step;
    const double u = 1.0 - t;
    const double b0 = pow(t, 3.0), b1 = (3.0 * (t * t)) * u, b2 = (3.0 * t) * (u * u), b3 = pow(u, 3.0);
    return ((P[0] * b0 + P[1] * b1) + P[2] * b2) + P[3] * b3;
}
// does a run's element `val` sit below v?  (ties: strict for runs after the element's own, non-strict for runs before it)
__device__ static inline bool gen_below(double val, double v, bool strict) { return strict ? val < v : val <= v; }

// More than GEN_MAX_RUNS runs (a near-constant image: the samples are rounding noise around one value): a general sort of the table by
// the one workgroup, in place in `sorted` (no scratch).  A bitonic network over the next power of two in its all-ascending form -- the
// first step of a merge compares mirrored partners, the later ones partners at a fixed distance -- so every comparator leaves the
// smaller value at the lower index: the padding above GEN_NT, +inf in thought, never moves, and a comparator that touches it is skipped.
// The comparators of one step are disjoint: each thread loads GEN_SORT_U pairs before it stores any.
constexpr int GEN_SORT_N = 131072;
constexpr int GEN_SORT_U = 8;
static_assert(GEN_SORT_N >= GEN_NT && GEN_SORT_N / 2 < GEN_NT && (GEN_SORT_N / 2) % (1024 * GEN_SORT_U) == 0, "bitonic padding");
__device__ static void gen_sort_general(const double* __restrict__ raw, double* __restrict__ sorted, int tid) {
    for (int k = tid; k < GEN_NT; k += 1024) sorted[k] = raw[k];
    __syncthreads();
    for (int k = 2; k <= GEN_SORT_N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const bool mirrored = j == (k >> 1);
            for (int t0 = tid; t0 < GEN_SORT_N / 2; t0 += 1024 * GEN_SORT_U) {
                int lo[GEN_SORT_U], hi[GEN_SORT_U];
                double a[GEN_SORT_U], b[GEN_SORT_U];
#pragma unroll
                for (int q = 0; q < GEN_SORT_U; ++q) {
                    const int t = t0 + 1024 * q;
                    lo[q] = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    hi[q] = mirrored ? lo[q] ^ (k - 1) : lo[q] + j;
                    if (hi[q] < GEN_NT) {
                        a[q] = sorted[lo[q]];
                        b[q] = sorted[hi[q]];
                    }
                }
#pragma unroll
                for (int q = 0; q < GEN_SORT_U; ++q)
                    if (hi[q] < GEN_NT && a[q] > b[q]) {
                        sorted[lo[q]] = b[q];
                        sorted[hi[q]] = a[q];
                    }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(1024) void genesis_bezier_kernel(const GenesisRec* __restrict__ recs, const float* __restrict__ minmax,
                                                             int nseg, double* __restrict__ ws, int* __restrict__ err) {
    __shared__ int nbnd;
    __shared__ int bnd[GEN_MAX_RUNS + 1];
    __shared__ int rs[GEN_MAX_RUNS + 1];
    __shared__ int asc[GEN_MAX_RUNS];
    __shared__ int carry[1024];
    const int arr = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const GenesisRec& rec = recs[b];
    if (!(rec.flags & GF_NONLIN)) return;
    double cx[4], cy[4];
    gen_controls(rec, minmax, b, nseg, cx, cy);
    const double* P = arr == 0 ? cx : cy;
    double* raw = ws + ((int64_t)b * 4 + arr) * GEN_NT;
    double* sorted = ws + ((int64_t)b * 4 + 2 + arr) * GEN_NT;
    for (int k = tid; k < GEN_NT; k += 1024) raw[k] = gen_bezier(P, k);
    if (arr == 1 && !(rec.flags & GF_SORTY)) return;           // the flipped branch sorts x only: y stays in t order
    if (tid == 0) nbnd = 0;
    __syncthreads();
    // 1. monotone runs: a run ends where the sign of the next non-zero difference changes.  Each thread scans a contiguous chunk;
    //    the last non-zero sign of the chunks before it comes from a scan over the threads.
    constexpr int CH = (GEN_NT + 1023) / 1024;
    const int c0 = tid * CH, c1 = min(GEN_NT, c0 + CH);
    int first = 0, kf = -1, cur = 0;
    for (int k = c0; k < c1 && k < GEN_NT - 1; ++k) {
        const double d = raw[k + 1] - raw[k];
        const int s = d > 0.0 ? 1 : (d < 0.0 ? -1 : 0);
        if (s == 0) continue;
        if (cur == 0) {
            first = s;
            kf = k;
        } else if (s != cur) {
            const int q = atomicAdd(&nbnd, 1);
            if (q < GEN_MAX_RUNS) bnd[q] = k + 1;
        }
        cur = s;
    }
    carry[tid] = cur;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                        // inclusive scan: last non-zero sign up to each thread
        const int v = tid >= o ? carry[tid - o] : 0;
        __syncthreads();
        if (carry[tid] == 0) carry[tid] = v;
        __syncthreads();
    }
    const int before = tid > 0 ? carry[tid - 1] : 0;
    if (first != 0 && before != 0 && first != before) {
        const int q = atomicAdd(&nbnd, 1);
        if (q < GEN_MAX_RUNS) bnd[q] = kf + 1;
    }
    __syncthreads();
    const int nb = nbnd;
    if (nb + 1 > GEN_MAX_RUNS) {                                // (uniform: every thread reads the same count)
        gen_sort_general(raw, sorted, tid);
        return;
    }
    if (tid == 0) {
        for (int i = 1; i < nb; ++i)
            for (int j = i; j > 0 && bnd[j - 1] > bnd[j]; --j) {
                const int t = bnd[j];
                bnd[j] = bnd[j - 1];
                bnd[j - 1] = t;
            }
        rs[0] = 0;
        for (int i = 0; i < nb; ++i) rs[i + 1] = bnd[i];
        rs[nb + 1] = GEN_NT;
        for (int r = 0; r <= nb; ++r) asc[r] = raw[rs[r + 1] - 1] >= raw[rs[r]] ? 1 : 0;
    }
    __syncthreads();
    const int nr = nb + 1;
    // 2. merge by rank: total order (value, run, index along the run's direction); the element's position is its rank in its own
    //    run plus, per other run, how many of that run's elements sit below it -- a boundary that moves monotonically along a chunk
    //    (found once by bisection, then walked).
    int r = 0;
    while (r + 1 < nr && rs[r + 1] <= c0) ++r;
    int pb[GEN_MAX_RUNS];
    int k = c0;
    while (k < c1) {
        while (rs[r + 1] <= k) ++r;
        const int e = min(c1, rs[r + 1]);
        const double v0 = raw[k];
        for (int s = 0; s < nr; ++s) {
            if (s == r) continue;
            const bool strict = s > r;
            int lo = rs[s], hi = rs[s + 1];                     // bisection for the boundary
            if (asc[s]) {
                while (lo < hi) {
                    const int m = (lo + hi) >> 1;
                    if (gen_below(raw[m], v0, strict)) lo = m + 1; else hi = m;
                }
            } else {
                while (lo < hi) {
                    const int m = (lo + hi) >> 1;
                    if (gen_below(raw[m], v0, strict)) hi = m; else lo = m + 1;
                }
            }
            pb[s] = lo;
        }
        for (; k < e; ++k) {
            const double v = raw[k];
            int pos = asc[r] ? k - rs[r] : rs[r + 1] - 1 - k;
            for (int s = 0; s < nr; ++s) {
                if (s == r) continue;
                const bool strict = s > r;
                const int a = rs[s], z = rs[s + 1];
                int p = pb[s];
                if (asc[s]) {                                   // below = [a, p)
                    while (p < z && gen_below(raw[p], v, strict)) ++p;
                    while (p > a && !gen_below(raw[p - 1], v, strict)) --p;
                    pos += p - a;
                } else {                                        // below = [p, z)
                    while (p > a && gen_below(raw[p - 1], v, strict)) --p;
                    while (p < z && !gen_below(raw[p], v, strict)) ++p;
                    pos += z - p;
                }
                pb[s] = p;
            }
            if (pos >= 0 && pos < GEN_NT) sorted[pos] = v;   // (a rank outside the table would mean broken runs: flagged, never written)
            else atomicOr(err, 2);
        }
    }
}
extern "C" int64_t cmu_genesis_bezier_ws_bytes(int B) { return (int64_t)B * 4 * GEN_NT * (int64_t)sizeof(double); }
extern "C" int cmu_genesis_bezier(const void* recs, const float* minmax, int B, int H, int W, void* ws, int* err, void* stream) {
    CMU_CHECK_ARG(recs && minmax && ws && err && B > 0 && H > 0 && W > 0 && W <= GEN_OWNER_WORDS, "cmu_genesis_bezier: bad args");
    hipLaunchKernelGGL(genesis_bezier_kernel, dim3(2, B), dim3(1024), 0, (hipStream_t)stream, (const GenesisRec*)recs, minmax,
                       cmu_genesis_segments(H, W), (double*)ws, err);
    CMU_CHECK_LAUNCH("cmu_genesis_bezier");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// np.interp(x, xs, ys) as numpy's arr_interp evaluates it (j = last index with xs[j] <= x; x == xs[j] -> ys[j]; slope * (x - xs[j]) +
// ys[j]), then painting.  Grid (tiles, B); a coarse copy of xs (every 128th sample) in LDS narrows the bisection to 7 global steps.
// noise (nullable): the host replay's np.random.rand values, (B, H, W) float32; NULL: Philox per pixel.
// ---------------------------------------------------------------------------------------------
constexpr int GEN_COARSE = 128;
constexpr int GEN_NCOARSE = (GEN_NT + GEN_COARSE - 1) / GEN_COARSE;
__global__ __launch_bounds__(256) void genesis_paint_kernel(const GenesisRec* __restrict__ recs, const double* __restrict__ ws,
                                                           const float* __restrict__ noise, uint64_t seed, uint64_t offset,
                                                           float* __restrict__ x, int H, int W) {
    __shared__ double coarse[GEN_NCOARSE];
    const int b = blockIdx.y;
    const GenesisRec& rec = recs[b];
    const int flags = rec.flags, paint = rec.paint;
    const bool nonlin = flags & GF_NONLIN;
    if (!nonlin && paint == 0) return;
    const double* xs = ws + ((int64_t)b * 4 + 2) * GEN_NT;
    const double* ys = ws + ((int64_t)b * 4 + ((flags & GF_SORTY) ? 3 : 1)) * GEN_NT;
    if (nonlin) {
        for (int i = threadIdx.x; i < GEN_NCOARSE; i += 256) coarse[i] = xs[i * GEN_COARSE];
        __syncthreads();
    }
    const int HW = H * W;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        const int64_t o = (int64_t)b * HW + p;
        float v = x[o];
        if (nonlin) {
            const double xv = (double)v;
            double res;
            if (xv < xs[0]) {
                res = ys[0];
            } else if (xv > xs[GEN_NT - 1]) {
                res = ys[GEN_NT - 1];
            } else {
                int lo = 0, hi = GEN_NCOARSE;                   // first coarse entry > xv
                while (lo < hi) {
                    const int m = (lo + hi) >> 1;
                    if (xv >= coarse[m]) lo = m + 1; else hi = m;
                }
                // upper bound of xv in xs lies in ((lo-1)*C, lo*C]
                int a = (lo - 1) * GEN_COARSE + 1, z = min(GEN_NT, lo * GEN_COARSE);
                while (a < z) {
                    const int m = (a + z) >> 1;
                    if (xv >= xs[m]) a = m + 1; else z = m;
                }
                const int j = a - 1;
                if (j == GEN_NT - 1 || xs[j] == xv) {
                    res = ys[j];
                } else {
                    const double slope = (ys[j + 1] - ys[j]) / (xs[j + 1] - xs[j]);
                    res = slope * (xv - xs[j]) + ys[j];
                    if (isnan(res)) {
                        res = slope * (xv - xs[j + 1]) + ys[j + 1];
                        if (isnan(res) && ys[j] == ys[j + 1]) res = ys[j];
                    }
                }
            }
            v = (float)res;
        }
        if (paint != 0) {
            const int i = p / W, j = p % W;
            bool inside = false;
            for (int q = 0; q < rec.nrect; ++q) {
                const int x0 = rec.rect[q][0], y0 = rec.rect[q][1], sx = rec.rect[q][2], sy = rec.rect[q][3];
                inside |= i >= x0 && i < x0 + sx && j >= y0 && j < y0 + sy;
            }
            // in-painting: noise inside the rectangles; out-painting: noise outside the kept windows
            if (inside == (paint == 1)) v = noise ? noise[o] : gen_noise(seed, offset, b, p);
        }
        x[o] = v;
    }
}
extern "C" int cmu_genesis_intensity_paint(const void* recs, const void* ws, const float* noise, uint64_t seed, uint64_t offset, float* x,
                                           int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(recs && ws && x && B > 0 && H > 0 && W > 0, "cmu_genesis_intensity_paint: bad args");
    const int tiles = cmu_div_up(H * W, 4096);
    hipLaunchKernelGGL(genesis_paint_kernel, dim3(tiles, B), dim3(256), 0, (hipStream_t)stream, (const GenesisRec*)recs, (const double*)ws,
                       noise, seed, offset, x, H, W);
    CMU_CHECK_LAUNCH("cmu_genesis_intensity_paint");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// MAE pair (generate_pair_mae): y = src[idx], x = y * (1 - mask[0]) as numpy evaluates it (float32 times 0 or 1: -0.0 and NaN kept)
// ---------------------------------------------------------------------------------------------
__global__ void genesis_mae_kernel(const float* __restrict__ src, const GenesisRec* __restrict__ recs, const uint8_t* __restrict__ mask,
                                   float* __restrict__ x, float* __restrict__ y, int HW, int64_t total) {
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(o / HW), p = (int)(o % HW);
        const float v = src[(int64_t)recs[b].src * HW + p];
        y[o] = v;
        x[o] = __fmul_rn(v, (float)(1 - (int)mask[p]));
    }
}
extern "C" int cmu_genesis_mae(const float* src, const void* recs, const uint8_t* mask, float* x, float* y, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(src && recs && mask && x && y && B > 0 && H > 0 && W > 0, "cmu_genesis_mae: bad args");
    const int64_t total = (int64_t)B * H * W;
    const int g = (int)(cmu_div_up64(total, 256) < 8192 ? cmu_div_up64(total, 256) : 8192);
    hipLaunchKernelGGL(genesis_mae_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, src, (const GenesisRec*)recs, mask, x, y, H * W, total);
    CMU_CHECK_LAUNCH("cmu_genesis_mae");
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------
// nn.MSELoss()(logits[:, 0], y): loss = mean((l - y)^2) over B*H*W.  One pass writes per-workgroup fp64 partial sums and (dlogits
// non-NULL) the gradient 2 (l - y) / n * loss_scale [* amp scale]; a second one-workgroup pass adds the partials in a fixed order.
// ---------------------------------------------------------------------------------------------
constexpr int MSE_MAX_BLOCKS = 1024;
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ logits, int K, const float* __restrict__ y,
                                                         float* __restrict__ dlogits, float loss_scale, const CmuAmpState* __restrict__ amp,
                                                         double* __restrict__ part, int HW, int64_t n) {
    __shared__ double red[4];
    if (amp != nullptr) loss_scale *= amp->scale;
    const float k = __fdiv_rn(2.f * loss_scale, (float)n);
    double acc = 0.0;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / HW, p = o % HW;
        const int64_t li = b * K * HW + p;
        const float d = __fsub_rn(logits[li], y[o]);
        acc += (double)d * (double)d;
        if (dlogits) {
            dlogits[li] = __fmul_rn(k, d);
            for (int c = 1; c < K; ++c) dlogits[li + (int64_t)c * HW] = 0.f;
        }
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void mse_final_kernel(const double* __restrict__ part, int nparts, int64_t n, float* __restrict__ loss) {
    __shared__ double red[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) a += part[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)n);
}
extern "C" int64_t cmu_mse_ws_bytes() { return (int64_t)MSE_MAX_BLOCKS * (int64_t)sizeof(double); }
extern "C" int cmu_mse_fwd_bwd(const float* logits, int K, const float* y, float* loss, float* dlogits, float loss_scale, const void* amp_state,
                               int B, int H, int W, void* ws, void* stream) {
    CMU_CHECK_ARG(logits && y && loss && ws && K > 0 && B > 0 && H > 0 && W > 0, "cmu_mse_fwd_bwd: bad args");
    const int64_t n = (int64_t)B * H * W;
    const int g = (int)(cmu_div_up64(n, 256 * 16) < MSE_MAX_BLOCKS ? cmu_div_up64(n, 256 * 16) : MSE_MAX_BLOCKS);
    hipLaunchKernelGGL(mse_partial_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, logits, K, y, dlogits, loss_scale,
                       (const CmuAmpState*)amp_state, (double*)ws, H * W, n);
    CMU_CHECK_LAUNCH("cmu_mse_fwd_bwd(partial)");
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, g, n, loss);
    CMU_CHECK_LAUNCH("cmu_mse_fwd_bwd(final)");
    return CMU_OK;
}
