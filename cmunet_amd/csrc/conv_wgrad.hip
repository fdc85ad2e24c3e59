// conv_wgrad.hip -- weight gradients of Conv2d 3x3 and ConvTranspose2d 2x2 on MFMA (gfx950).
//
//   MODE_W3:  dW[n][c][kh][kw] = sum_p dY[p][n] * act(X)[p + (kh-1,kw-1)][c]        (autograd of model.py:17,20)
//   MODE_WT:  dW[c][n][i][j]   = sum_p dOut[2p+(i,j)][n] * act(X)[p][c]              (autograd of model.py:60)
//
// GEMM view: M = output channels n (rows, operand A = dY^T), N = input channels c (cols, operand B = X),
// K = pixels.  Both operands are pixel-major NHWC in HBM, i.e. K is the SLOW axis of both -- the opposite of
// what an MFMA fragment wants (8 consecutive k per lane).  CDNA4 answer: keep the natural [pixel][channel]
// image in LDS and read fragments with ds_read_b64_tr_b16 (hardware 4x16 transpose), two reads per
// fragment; for fp32 the 32x32x2 MFMA takes one k per lane-half, so plain ds_read_b32 is already right.
//
//   * workgroup = 512 threads = 8 wave64, one per CU; block tile = 128-byte channel rows on both sides
//     (64x64 channels for f16/bf16, 32x32 for f32) x all 9 taps: each wave keeps 9 accumulator tiles
//     (144 VGPRs) for its (32n x 32c) block and half (1/8 for f32) of the tile's pixel rows; the A
//     fragment of a pixel row is loaded once and reused by the 9 taps.
//   * K loop = 16x16 spatial tiles (split-K over workgroups); per tile the dY tile and the 18x18 X halo are
//     staged ONCE (global -> regs -> LDS, BatchNorm+ReLU of the producer applied to X on the way) and the
//     9 taps read the halo at shifted pixel addresses.
//   * LDS image: 128-byte pixel rows, 64-byte halves XOR-swizzled by bit 1 of the pixel index: the four
//     pixels a transposed read touches land on the four 64-byte quarters of the 256-byte bank row.
//   * accumulators of the k-parts are combined through LDS, partial slabs [split][tap][n][c] go to a
//     workspace and a second kernel sums them in split order (deterministic) into the reference layout.
// (Its eight waves multiply, then stage, in lockstep.  Running waves 4-7 one stage phase ahead -- the two-phase ping-pong of
// conv_wgrad2.inc -- on THIS loop measured 11.9 against 10.2 ms of weight-gradient time per bench step: alone on its SIMD a
// wave waits for every transposed fragment read, which two waves multiplying side by side hide for each other; the
// ping-pong needs the register double buffer of fragments that conv_wgrad2.inc has and the 144 accumulator registers
// here leave no room for.  The Cout = 64 layers that still run here are 64 x 64 blocks: 7.2 MFMAs per staged chunk
// whatever the schedule, against 10.3 for the 128 x 64 blocks of conv_wgrad2.inc.)
#include "common.h"
#include <stdlib.h>

enum { MODE_W3 = 0, MODE_WT = 1 };

struct WGParams {
    const void* a;  // dY (MODE_W3) / dOut (MODE_WT)
    int64_t lda;
    const void* b;  // X
    int64_t ldb;
    const float* b_scale;
    const float* b_shift;
    int relu_from;
    float* ws;
    int B, H, W;  // pixel grid of the contraction (MODE_WT: the low-res grid)
    int CA, CB;   // channels of A (output channels) and B (input channels)
    int CApad, CBpad;
    int nAB, nBB, splitk, ntiles, tilesX, tilesY;
    // sparse (SparK) form of the first kernel: the K loop runs over the 16 x 16 pixel tiles tile_list[0 .. *tile_count) only
    // (device arrays from cmu_sparse_tile_list; elsewhere dY is zero by construction, so the sum is unchanged)
    const int* tile_list;
    const int* tile_count;
};

template <class TR, int MODE>
struct WGCfg {
    typedef typename TR::elem_t elem_t;
    static constexpr int ES = (int)sizeof(elem_t);
    static constexpr int CW = 128 / ES;
    static constexpr int NB32 = CW / 32;
    static constexpr int NT = NB32 * NB32;
    static constexpr int KPARTS = 8 / NT;
    static constexpr int RPP = 16 / KPARTS;  // pixel rows per k-part
    static constexpr int TAPS = (MODE == MODE_W3) ? 9 : 1;
    static constexpr int HALO = (MODE == MODE_W3) ? 1 : 0;
    static constexpr int LW = 16 + 2 * HALO;
    static constexpr int LWP = (MODE == MODE_W3) ? 20 : 16;  // LDS row pitch in pixels: a multiple of 4, so that the
                                                             // swizzle bit of a fragment read is a per-lane constant
    static constexpr int NPIXB = LW * LW;
    static constexpr int A_BYTES = 256 * 128;
    static constexpr int B_BYTES = LW * LWP * 128;
    static constexpr int A_ITERS = (256 * 8) / 512;
    static constexpr int B_ITERS = (NPIXB * 8 + 511) / 512;
    static constexpr int RED_BYTES = NT * TAPS * 4096;
    static constexpr int BUF_BYTES = A_BYTES + B_BYTES;   // one stage: dY tile + X halo
    static constexpr int MAIN_BYTES = 2 * BUF_BYTES;      // double-buffered: stage t+1 is written while t is read
    static constexpr int LDS_BYTES = MAIN_BYTES > RED_BYTES ? MAIN_BYTES : RED_BYTES;
};

__device__ static inline int swz(int pix, int cbyte) { return pix * 128 + (cbyte ^ (((pix >> 1) & 1) << 6)); }

__device__ static inline u32x2 lds_tr16(const unsigned char* smem, int off) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(smem + off));
    return __builtin_bit_cast(u32x2, v);
}

#ifdef CMU_IG_STAMPS
__device__ unsigned long long g_wg_stamps[64 * 16 * 8];
extern "C" int cmu_debug_wg_stamps(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wg_stamps), sizeof(g_wg_stamps));
}
#define WG_STAMP(k_)                                                                          \
    do {                                                                                       \
        if (stamp_slot >= 0 && stamp_i < 16 && tid == 0)                                       \
            g_wg_stamps[(stamp_slot * 16 + stamp_i) * 8 + (k_)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define WG_STAMP(k_) do {} while (0)
#endif

template <class TR, int MODE>
__global__ __launch_bounds__(512, 2) void conv_wgrad_kernel(const WGParams p) {
    typedef WGCfg<TR, MODE> C;
    constexpr int EPC = TR::EPC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* smA = smem;                 // buffer being read (swapped every tile)
    unsigned char* smB = smem + C::A_BYTES;
    unsigned char* stA = smem;                 // buffer being written by store_tile
    unsigned char* stB = smem + C::A_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 31;
    const int h = lane >> 5;

    int bid = blockIdx.x;
    const int ab = bid % p.nAB;
    bid /= p.nAB;
    const int bb = bid % p.nBB;
    bid /= p.nBB;
    int ij = 0;
    if (MODE == MODE_WT) { ij = bid & 3; bid >>= 2; }
    const int split = bid;

    const int tile_id = wave % C::NT;
    const int kpart = wave / C::NT;
    const int nb32 = tile_id % C::NB32, cb32 = tile_id / C::NB32;

    const int Ha = (MODE == MODE_WT) ? 2 * p.H : p.H;
    const int Wa = (MODE == MODE_WT) ? 2 * p.W : p.W;
    const unsigned char* ga = reinterpret_cast<const unsigned char*>(p.a);
    const unsigned char* gb = reinterpret_cast<const unsigned char*>(p.b);

    // staging role: 16-byte chunk cgi of the 128-byte channel row, constant per thread
    const int cgi = tid & 7;
    const int a_c0 = ab * C::CW + cgi * EPC;
    const int b_c0 = bb * C::CW + cgi * EPC;
    const bool a_cok = a_c0 < p.CA;
    const bool b_cok = b_c0 < p.CB;
    const bool has_tf = (p.b_scale != nullptr);
    float sc[EPC], sh[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        sc[e] = (has_tf && b_cok) ? p.b_scale[b_c0 + e] : 1.f;
        sh[e] = (has_tf && b_cok) ? p.b_shift[b_c0 + e] : 0.f;
    }
    const bool relu = has_tf && cmu_relu_on(b_c0, p.relu_from);

    f32x16 acc[C::TAPS];
#pragma unroll
    for (int t = 0; t < C::TAPS; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    u32x4 areg[C::A_ITERS];
    u32x4 breg[C::B_ITERS];
    unsigned b_ok = 0;  // bit it: B chunk is inside the image (so the transform applies)

    const int ntiles = (MODE == MODE_W3 && p.tile_list != nullptr) ? __builtin_amdgcn_readfirstlane(*p.tile_count) : p.ntiles;
    auto load_tile = [&](int tile) {
        if (MODE == MODE_W3 && p.tile_list != nullptr) tile = __builtin_amdgcn_readfirstlane(p.tile_list[tile]);
        const int tx = tile % p.tilesX, ty = (tile / p.tilesX) % p.tilesY, b = tile / (p.tilesX * p.tilesY);
        const int ty0 = ty * 16, tx0 = tx * 16;
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) {
            const int pix = (it * 512 + tid) >> 3;
            const int py = pix >> 4, px = pix & 15;
            int gy = ty0 + py, gx = tx0 + px;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (a_cok && gy < p.H && gx < p.W) {
                if (MODE == MODE_WT) { gy = 2 * gy + (ij >> 1); gx = 2 * gx + (ij & 1); }
                v = ld_global16(ga + ((((int64_t)b * Ha + gy) * Wa + gx) * p.lda + a_c0) * C::ES);
            }
            areg[it] = v;
        }
        b_ok = 0;
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it) {
            const int idx = it * 512 + tid;
            const int pix = idx >> 3;
            const int py = pix / C::LW, px = pix % C::LW;
            const int gy = ty0 - C::HALO + py, gx = tx0 - C::HALO + px;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (idx < C::NPIXB * 8 && b_cok && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
                v = ld_global16(gb + ((((int64_t)b * p.H + gy) * p.W + gx) * p.ldb + b_c0) * C::ES);
                b_ok |= 1u << it;
            }
            breg[it] = v;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) {
            const int pix = (it * 512 + tid) >> 3;
            *reinterpret_cast<u32x4*>(stA + swz(pix, cgi * 16)) = areg[it];
        }
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it) {
            const int idx = it * 512 + tid;
            if (idx < C::NPIXB * 8) {
                u32x4 v = breg[it];
                if (has_tf && ((b_ok >> it) & 1u)) {
                    float f[EPC];
                    TR::unpack(v, f);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        const float t = fmaf(f[e], sc[e], sh[e]);
                        f[e] = relu ? fmaxf(t, 0.f) : t;
                    }
                    v = TR::pack(f);
                }
                const int pix = idx >> 3;
                *reinterpret_cast<u32x4*>(stB + swz((pix / C::LW) * C::LWP + pix % C::LW, cgi * 16)) = v;
            }
        }
    };

    // fragment addressing.  16-bit path: 16-lane group g = lane>>4 covers channels 16*(g&1).. of the wave's
    // 32-block and pixels 8*(g>>1) + 4*t + q of the row; lane li = lane&15: q = li>>2, quad = li&3.
    // Row pitches (16 / 20 pixels) are multiples of 4, so bit 1 of the pixel index -- the swizzle bit -- depends
    // only on (kw + q): every read is base(py,kh) + per-lane constant + immediate.
    const int li = lane & 15, g = lane >> 4;
    const int q4 = li >> 2, quad = li & 3;
    const int a_cbyte16 = (nb32 * 32 + 16 * (g & 1) + 4 * quad) * 2;
    const int b_cbyte16 = (cb32 * 32 + 16 * (g & 1) + 4 * quad) * 2;
    const int a_off16 = (8 * h + q4) * 128 + (a_cbyte16 ^ (((q4 >> 1) & 1) << 6));
    int b_off16[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) b_off16[kw] = (kw + 8 * h + q4) * 128 + (b_cbyte16 ^ ((((kw + q4) >> 1) & 1) << 6));
    // f32 path: lane-half h holds pixel 2s+h of the k-pair; swizzle bit = ((kw + h) >> 1 + s) & 1
    const int a_off32 = h * 128 + (nb32 * 32 + r) * 4;
    int b_off32[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) b_off32[kw] = (kw + h) * 128 + (((cb32 * 32 + r) * 4) ^ ((((kw + h) >> 1) & 1) << 6));

    // software pipeline over this split's tiles: LDS holds tile t (being read) and tile t+1 (being written by
    // store_tile from registers loaded one iteration earlier); registers are then refilled with tile t+2.
    // One barrier per tile; a wave's LDS writes overlap the other waves' MFMAs.
    int tile = split;
    if (tile < ntiles) {
        load_tile(tile);
        store_tile();
        if (tile + p.splitk < ntiles) load_tile(tile + p.splitk);
    }
    __syncthreads();
#ifdef CMU_IG_STAMPS
    const int stamp_slot = (blockIdx.x % 7 == 0 && blockIdx.x / 7 < 64) ? (int)(blockIdx.x / 7) : -1;
    int stamp_i = -1;
#endif
    for (; tile < ntiles; tile += p.splitk) {
#ifdef CMU_IG_STAMPS
        ++stamp_i;
#endif
        WG_STAMP(0);
        stA = (smA == smem) ? smem + C::BUF_BYTES : smem;
        stB = stA + C::A_BYTES;
#pragma unroll 1
        for (int rr = 0; rr < C::RPP; ++rr) {
            const int py = kpart * C::RPP + rr;
            if constexpr (EPC == 8) {
                // A fragment: 8 consecutive pixels (k = 8h + j) of row py for channel row r
                const unsigned char* pa = smA + py * (16 * 128) + a_off16;
                const u32x2 a_lo = lds_tr16(pa, 0);
                const u32x2 a_hi = lds_tr16(pa, 512);
                const u32x4 afrag = {a_lo[0], a_lo[1], a_hi[0], a_hi[1]};
                const unsigned char* pbrow = smB + py * (C::LWP * 128);
#pragma unroll
                for (int t = 0; t < C::TAPS; ++t) {
                    const int kh = (C::TAPS == 9) ? t / 3 : 0, kw = (C::TAPS == 9) ? t % 3 : 0;
                    const unsigned char* pb = pbrow + kh * (C::LWP * 128) + b_off16[kw];
                    const u32x2 b_lo = lds_tr16(pb, 0);
                    const u32x2 b_hi = lds_tr16(pb, 512);
                    const u32x4 bfrag = {b_lo[0], b_lo[1], b_hi[0], b_hi[1]};
                    TR::mma16(afrag, bfrag, acc[t]);
                }
            } else {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const float av = *reinterpret_cast<const float*>(smA + (py * 16 + 2 * s) * 128 + (a_off32 ^ ((s & 1) << 6)));
#pragma unroll
                    for (int t = 0; t < C::TAPS; ++t) {
                        const int kh = (C::TAPS == 9) ? t / 3 : 0, kw = (C::TAPS == 9) ? t % 3 : 0;
                        const float bv = *reinterpret_cast<const float*>(smB + ((py + kh) * C::LWP + 2 * s) * 128 + (b_off32[kw] ^ ((s & 1) << 6)));
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
                    }
                }
            }
        }
        WG_STAMP(1);
        if (tile + p.splitk < ntiles) store_tile();                       // tile t+1: registers -> the other buffer
        WG_STAMP(2);
        __syncthreads();
        WG_STAMP(3);
        if (tile + 2 * p.splitk < ntiles) load_tile(tile + 2 * p.splitk);  // tile t+2: in flight during the next compute
        WG_STAMP(4);
        smA = stA;
        smB = stB;
    }
    // ---- combine the k-parts through LDS (fixed order), then write the partial slab ----------------------
    float* red = reinterpret_cast<float*>(smem) + (int64_t)tile_id * (C::TAPS * 1024);
    for (int kp = 1; kp < C::KPARTS; ++kp) {
        __syncthreads();
        if (kpart == kp) {
#pragma unroll
            for (int t = 0; t < C::TAPS; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) red[(t * 16 + e) * 64 + lane] = acc[t][e];
        }
        __syncthreads();
        if (kpart == 0) {
#pragma unroll
            for (int t = 0; t < C::TAPS; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][e] += red[(t * 16 + e) * 64 + lane];
        }
    }
    if (kpart == 0) {
        const int T = (MODE == MODE_W3) ? 9 : 4;
#pragma unroll
        for (int t = 0; t < C::TAPS; ++t) {
            const int tt = (MODE == MODE_W3) ? t : ij;
            float* base = p.ws + (((int64_t)split * T + tt) * p.CApad + ab * C::CW + nb32 * 32) * p.CBpad + bb * C::CW + cb32 * 32 + r;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = (e & 3) + 8 * (e >> 2) + 4 * h;
                base[(int64_t)n * p.CBpad] = acc[t][e];
            }
        }
    }
}

#include "conv_wgrad2.inc"
#include "conv_wgrad2s.inc"
#include "conv_wgrad2f.inc"

// partial slabs -> parameter-gradient layout, summed in split order
#ifndef CMU_WGR_CAP
#define CMU_WGR_CAP 8192
#endif
// sum over the split slabs k = part, part + 4, ... (fixed order), eight loads in flight per trip
__device__ static inline float sum_split(const float* __restrict__ p, int64_t stride, int part, int splitk) {
    constexpr int U = 8;
    float s = 0.f;
    int k = part;
    for (; k + 4 * (U - 1) < splitk; k += 4 * U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = p[(int64_t)(k + 4 * u) * stride];
#pragma unroll
        for (int u = 0; u < U; ++u) s += v[u];
    }
    for (; k < splitk; k += 4) s += p[(int64_t)k * stride];
    return s;
}
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, int splitk, int T, int CApad, int CBpad, int CA,
                                                          int CB, float* __restrict__ dW, int mode) {
    // 64 outputs x 4 split-parts per block; the parts are combined through LDS in a fixed order
    __shared__ float red[4][64];
    const int64_t total = (int64_t)T * CA * CB;
    const int ol = threadIdx.x & 63, part = threadIdx.x >> 6;
    for (int64_t o0 = (int64_t)blockIdx.x * 64; o0 < total; o0 += (int64_t)gridDim.x * 64) {
        const int64_t o = o0 + ol;
        int c = (int)(o % CB);
        int n = (int)((o / CB) % CA);
        const int t = (int)(o / ((int64_t)CB * CA));
        float s = 0.f;
        if (mode == 2) {   // wide ConvTranspose kernel: slabs are [split][ij][c][n], n fastest
            n = (int)(o % CA);
            c = (int)((o / CA) % CB);
            if (o < total) s = sum_split(ws + ((int64_t)t * CB + c) * CA + n, (int64_t)T * CB * CA, part, splitk);
        } else if (o < total)
            s = sum_split(ws + ((int64_t)t * CApad + n) * CBpad + c, (int64_t)T * CApad * CBpad, part, splitk);
        __syncthreads();
        red[part][ol] = s;
        __syncthreads();
        if (part == 0 && o < total) {
            s = (red[0][ol] + red[1][ol]) + (red[2][ol] + red[3][ol]);
            if (mode == MODE_W3) dW[((int64_t)n * CB + c) * 9 + t] = s;      // (Cout,Cin,3,3)
            else dW[((int64_t)c * CA + n) * 4 + t] = s;                      // (Cin,Cout,2,2)
        }
    }
}

// the same reduction four channels per lane (16-byte loads: four times the bytes in flight; every output element still sums its
// slabs in the scalar kernel's order, so the two kernels agree bit for bit).  Needs the fast slab axis in whole 4-element groups.
__device__ static inline f32x4 sum_split4(const float* __restrict__ p, int64_t stride, int part, int splitk) {
    constexpr int U = 8;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int k = part;
    for (; k + 4 * (U - 1) < splitk; k += 4 * U) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const f32x4*>(p + (int64_t)(k + 4 * u) * stride);
#pragma unroll
        for (int u = 0; u < U; ++u) s += v[u];
    }
    for (; k < splitk; k += 4) s += *reinterpret_cast<const f32x4*>(p + (int64_t)k * stride);
    return s;
}
__global__ __launch_bounds__(256) void wgrad_reduce4_kernel(const float* __restrict__ ws, int splitk, int T, int CApad, int CBpad, int CA,
                                                           int CB, float* __restrict__ dW, int mode) {
    __shared__ f32x4 red[4][64];
    const int F = (mode == 2 ? CA : CB) / 4;                       // 4-element groups along the slab's fast axis
    const int S = mode == 2 ? CB : CA;                             // the slower channel axis
    const int64_t total = (int64_t)T * S * F;
    const int ol = threadIdx.x & 63, part = threadIdx.x >> 6;
    for (int64_t o0 = (int64_t)blockIdx.x * 64; o0 < total; o0 += (int64_t)gridDim.x * 64) {
        const int64_t o = o0 + ol;
        const int f4 = (int)(o % F), sl = (int)((o / F) % S), t = (int)(o / ((int64_t)F * S));
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (o < total) {
            if (mode == 2) s = sum_split4(ws + ((int64_t)t * CB + sl) * CA + 4 * f4, (int64_t)T * CB * CA, part, splitk);
            else s = sum_split4(ws + ((int64_t)t * CApad + sl) * CBpad + 4 * f4, (int64_t)T * CApad * CBpad, part, splitk);
        }
        __syncthreads();
        red[part][ol] = s;
        __syncthreads();
        if (part == 0 && o < total) {
            s = (red[0][ol] + red[1][ol]) + (red[2][ol] + red[3][ol]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (mode == 2) dW[((int64_t)sl * CA + 4 * f4 + j) * 4 + t] = s[j];             // slab [ij][c][n]: sl = c, fast = n
                else if (mode == MODE_W3) dW[((int64_t)sl * CB + 4 * f4 + j) * 9 + t] = s[j];  // (Cout,Cin,3,3): sl = n, fast = c
                else dW[((int64_t)(4 * f4 + j) * CA + sl) * 4 + t] = s[j];                     // (Cin,Cout,2,2): sl = n, fast = c
            }
        }
    }
}
// CMU_WGR_VEC=0 keeps the scalar reduction (A/B switch)
static void launch_wgrad_reduce(const float* ws, int splitk, int T, int CApad, int CBpad, int CA, int CB, float* dW, int mode, hipStream_t st) {
    const bool vec = cmu_knob(CMU_KNOB_WGR_VEC) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && (mode == 2 ? CA % 4 == 0 : (CB % 4 == 0 && CBpad % 4 == 0));
    const int64_t total = (int64_t)T * CA * CB / (vec ? 4 : 1);
    const int grid = (int)(cmu_div_up64(total, 64) < CMU_WGR_CAP ? cmu_div_up64(total, 64) : CMU_WGR_CAP);
    if (vec) hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3(grid), dim3(256), 0, st, ws, splitk, T, CApad, CBpad, CA, CB, dW, mode);
    else hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid), dim3(256), 0, st, ws, splitk, T, CApad, CBpad, CA, CB, dW, mode);
}

// per-channel sum over all pixels (ConvTranspose2d bias gradient)
template <class TR>
__global__ __launch_bounds__(256) void channel_sum_kernel(const unsigned char* __restrict__ x, int64_t ldx, float* __restrict__ ws,
                                                         int64_t npix, int C, int cpb, int ppb) {
    constexpr int EPC = TR::EPC;
    constexpr int ES = (int)sizeof(typename TR::elem_t);
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const int nchunk = C / EPC;
    const int ch = blockIdx.y * cpb + tid % cpb;
    const int prow = tid / cpb;
    const bool active = prow < ppb && ch < nchunk;
    float s[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) s[e] = 0.f;
    if (active)
        for (int64_t pp = (int64_t)blockIdx.x * ppb + prow; pp < npix; pp += (int64_t)gridDim.x * ppb) {
            float f[EPC];
            TR::unpack(ld_global16(x + (pp * ldx + ch * EPC) * ES), f);
#pragma unroll
            for (int e = 0; e < EPC; ++e) s[e] += f[e];
        }
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        __syncthreads();
        red[tid] = s[e];
        __syncthreads();
        if (tid < cpb && blockIdx.y * cpb + tid < nchunk) {
            float a = 0.f;
            for (int k = 0; k < ppb; ++k) a += red[k * cpb + tid];
            ws[(int64_t)blockIdx.x * C + (blockIdx.y * cpb + tid) * EPC + e] = a;
        }
    }
}
// 16 channels x 16 row parts per 256-thread block, eight rows in flight per thread, fixed-order combine (one thread per channel
// walking up to 256 rows was a chain of dependent round trips: 23 us per launch)
__global__ __launch_bounds__(256) void channel_sum_final_kernel(const float* __restrict__ ws, int nblocks, int C, float* out) {
    __shared__ double red[16][16];
    const int cl = threadIdx.x & 15, part = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    double s = 0.0;
    if (c < C) {
        constexpr int U = 8;
        int b = part;
        for (; b + 16 * (U - 1) < nblocks; b += 16 * U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = ws[(int64_t)(b + 16 * u) * C + c];
#pragma unroll
            for (int u = 0; u < U; ++u) s += (double)v[u];
        }
        for (; b < nblocks; b += 16) s += (double)ws[(int64_t)b * C + c];
    }
    red[part][cl] = s;
    __syncthreads();
    if (part == 0 && c < C) {
        s = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += red[q][cl];
        out[c] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
static int wg_splitk(int nbase, int ntiles, int mult, int target) {
    // aim at ~target workgroups; every split gets at least one tile
    int s = target / (nbase * mult);
    if (s < 1) s = 1;
    if (s > ntiles) s = ntiles;
    return s;
}
constexpr int CSUM_BLOCKS = 256;
constexpr int64_t WG_BUF_RANGE = 0x7fff0000ll;   // bytes of one image that a buffer descriptor of the wide kernels can address

// splitk decomposed into (tile column, tile row, image) steps for the kernels that walk their K tiles by increments
static WG2Params wg2_params(const WGParams& p) {
    WG2Params pp;
    pp.g = p;
    pp.dtx = p.splitk % p.tilesX;
    pp.dty = (p.splitk / p.tilesX) % p.tilesY;
    pp.dtb = p.splitk / (p.tilesX * p.tilesY);
    return pp;
}

// One launch function per kernel: the dynamic-LDS launch and the kernel tag (nothing else differs between the forms' launches)
typedef int (*WGLaunch)(const WGParams& p, hipStream_t st, const char* name);
template <class TR, int MODE>
static int wg_launch_first(const WGParams& p, hipStream_t st, const char* name) {
    const int grid = p.nAB * p.nBB * p.splitk * (MODE == MODE_WT ? 4 : 1);
    if (int rc = cmu_launch_lds<&conv_wgrad_kernel<TR, MODE>>(dim3(grid), dim3(512), WGCfg<TR, MODE>::LDS_BYTES, st, name, p)) return rc;
    cmu_set_kernel_tag("conv_wgrad_kernel");
    return CMU_OK;
}
template <class TR, bool SWAP>
static int wg_launch_wide(const WGParams& p, hipStream_t st, const char* name) {
    if (int rc = cmu_launch_lds<&conv_wgrad2_kernel<TR, SWAP>>(dim3(p.nAB * p.nBB * p.splitk), dim3(512), WG2Cfg<TR>::LDS_BYTES, st, name, wg2_params(p))) return rc;
    cmu_set_kernel_tag("conv_wgrad2_kernel");
    return CMU_OK;
}
template <class TR>
static int wg_launch_square(const WGParams& p, hipStream_t st, const char* name) {
    if (int rc = cmu_launch_lds<&conv_wgrad2s_kernel<TR>>(dim3(p.nAB * p.nBB * p.splitk), dim3(512), WG2SCfg<TR>::LDS_BYTES, st, name, wg2_params(p))) return rc;
    cmu_set_kernel_tag("conv_wgrad2s_kernel");
    return CMU_OK;
}
template <int NAI>
static int wg_launch_wide_f32(const WGParams& p, hipStream_t st, const char* name) {
    if (int rc = cmu_launch_lds<&conv_wgrad2f_kernel<NAI>>(dim3(p.nAB * p.nBB * p.splitk), dim3(512), WG2FCfg<NAI>::LDS_BYTES, st, name, wg2_params(p))) return rc;
    cmu_set_kernel_tag("conv_wgrad2f_kernel");
    return CMU_OK;
}
template <class TR, int NXI>
static int wg_launchT_wide(const WGParams& p, hipStream_t st, const char* name) {
    if (int rc = cmu_launch_lds<&conv_wgradT2_kernel<TR, NXI>>(dim3(p.nAB * p.nBB * p.splitk), dim3(512), WGT2Cfg<TR, NXI>::LDS_BYTES, st, name, wg2_params(p))) return rc;
    cmu_set_kernel_tag("conv_wgradT2_kernel");
    return CMU_OK;
}
static int wg_launchT_wide_f32(const WGParams& p, hipStream_t st, const char* name) {
    if (int rc = cmu_launch_lds<&conv_wgradT2f_kernel>(dim3(p.nAB * p.nBB * p.splitk), dim3(512), WGT2FCfg::LDS_BYTES, st, name, wg2_params(p))) return rc;
    cmu_set_kernel_tag("conv_wgradT2f_kernel");
    return CMU_OK;
}

// ---- the forms: which kernel serves a shape, with what split-K geometry, and what it writes to the workspace.  One row each; every entry
// point below -- both size queries, the tile-height query and the three launches -- reads this table through wg_plan / wg_ws_bytes.
enum WGRange {
    WG_ANY,      // the first kernel: 64-bit addresses, every shape
    WG_HALO_B,   // buffer descriptors per image: dY plain, X with its halo row (W + 1 pixels past the image)
    WG_HALO_A,   // the swapped roles: the halo is on dY, the plain images are X
    WG_PLAIN     // ConvTranspose: dOut (four pixels per pixel of X) and X without halo
};
enum WGBias {
    WG_BIAS_NONE,
    WG_BIAS_SUMS,     // the channel-sum kernels run behind the reduction: CSUM_BLOCKS rows of partial sums behind the slabs
    WG_BIAS_SPLITS    // the kernel wrote one row of partial sums per split behind the slabs: only the final sum runs
};
struct WGForm {
    const char* name;        // of the launch in error messages
    int family;              // MODE_W3 / MODE_WT
    int tile_h;              // rows of a K tile (16 pixels wide)
    int a_blk, b_blk;        // channels of Cout / Cin per workgroup; 0: 128 bytes' worth, and the slab pads the channel count to whole blocks
    bool swap;               // nAB counts the blocks of Cin and nBB those of Cout
    int slabs;               // slabs per split (the wave halves of a 64 x 64 block write separate slabs, summed in slab order)
    int wgs;                 // workgroups per block pair and split (the first ConvTranspose kernel: one per sub-pixel)
    int aim;                 // knob that holds the number of workgroups the split count aims at; -1: 512 (two rounds over 256 CUs)
    bool (*shape)(int CA, int CB, int dt);
    bool (*knobs)(int CA, int CB);
    bool size_any_knobs;     // the size query counts the form whatever its knobs say
    WGRange range;
    int tf_align;            // mask the addresses of a pending transform's scale / shift must clear
    bool lists8;             // walks 8 x 16 tile lists (cmu_conv3x3_wgrad_tiles)
    int reduce_mode;         // of launch_wgrad_reduce: MODE_W3, MODE_WT, 2 (slabs [split][ij][c][n])
    WGBias bias;
    WGLaunch launch[3];      // by dtype
};
static bool wg_on(int, int) { return true; }
static bool wg_wide_on(int, int) { return cmu_knob(CMU_KNOB_WGRAD_WIDE); }   // CMU_WGRAD_WIDE=0 keeps every layer on the first kernel (A/B switch for the benches)
static bool wg_wide_f32_on(int, int) { return cmu_knob(CMU_KNOB_WGRAD_WIDE) && cmu_knob(CMU_KNOB_WGRAD_WIDE_F32); }
static bool wg_nx256(int CB) { return cmu_knob(CMU_KNOB_WGT2_NX256) && CB % 256 == 0; }
// The wide kernels hold one workgroup per CU (LDS): 256 workgroups (CMU_WGRAD_BLOCKS) are exactly one round over the chip, and every
// workgroup writes its whole accumulator tile to the split-K slab -- half the workgroups is half the slab traffic of the reduction
// (1.1 ms per bench step at 512).  The rows of a family stand in the order in which they are tried.
static const WGForm WG_FORMS[] = {
    // each row:  name, family, tile_h, a_blk, b_blk, swap, slabs, wgs, aim,
    //            shape, knobs, size_any_knobs,
    //            range, tf_align, lists8, reduce_mode, bias, launch by dtype
    // wide-tile kernel (conv_wgrad2.inc): 16-bit dtypes, Cout in whole 128-blocks, Cin in whole 64-blocks
    {"cmu_conv3x3_wgrad(wide)", MODE_W3, 8, 128, 64, false, 1, 1, CMU_KNOB_WGRAD_BLOCKS,
     [](int CA, int CB, int dt) { return cmu_dtype_size(dt) == 2 && CA % 128 == 0 && CB % 64 == 0; }, wg_wide_on, false,
     WG_HALO_B, 3, true, MODE_W3, WG_BIAS_NONE, {nullptr, wg_launch_wide<F16Traits, false>, wg_launch_wide<BF16Traits, false>}},
    // swapped roles (conv_wgrad2.inc, SWAP): Cout = 64 with Cin in whole 128-blocks.  CMU_WGRAD_SWAP=0 keeps those layers off it (A/B switch).
    // (the slab is [split][tap][Cout][Cin] in both forms)
    {"cmu_conv3x3_wgrad(wide)", MODE_W3, 8, 64, 128, true, 1, 1, CMU_KNOB_WGRAD_BLOCKS,
     [](int CA, int CB, int dt) { return cmu_dtype_size(dt) == 2 && CA == 64 && CB % 128 == 0; },
     [](int, int) { return cmu_knob(CMU_KNOB_WGRAD_SWAP) && cmu_knob(CMU_KNOB_WGRAD_WIDE); }, false,
     WG_HALO_A, 15, false, MODE_W3, WG_BIAS_NONE, {nullptr, wg_launch_wide<F16Traits, true>, wg_launch_wide<BF16Traits, true>}},
    // 64 n x 64 c form for the 16-bit dtypes (conv_wgrad2s.inc): whole 64-blocks on both sides where neither form above claims the shape
    // (the 64 -> 64 layers).  CMU_WGRAD_SQUARE=0 keeps them on the first kernel (A/B switch).
    {"cmu_conv3x3_wgrad(64 x 64)", MODE_W3, 8, 64, 64, false, 2, 1, CMU_KNOB_WGRAD_BLOCKS,
     [](int CA, int CB, int dt) { return cmu_dtype_size(dt) == 2 && CA % 64 == 0 && CB % 64 == 0; },
     [](int, int) { return cmu_knob(CMU_KNOB_WGRAD_WIDE) && cmu_knob(CMU_KNOB_WGRAD_SQUARE); }, true,
     WG_HALO_B, 3, true, MODE_W3, WG_BIAS_NONE, {nullptr, wg_launch_square<F16Traits>, wg_launch_square<BF16Traits>}},
    // fp32 wide kernel (conv_wgrad2f.inc): Cout and Cin in whole 64-blocks -- 128 n x 64 c blocks (NAI = 4) when Cout allows, else 64 x 64
    // with two k-parts (NAI = 2).  CMU_WGRAD_WIDE_F32=0 keeps fp32 on the first kernel (A/B switch).
    {"cmu_conv3x3_wgrad(wide, fp32)", MODE_W3, 4, 128, 64, false, 1, 1, CMU_KNOB_WGRAD_BLOCKS,
     [](int CA, int CB, int dt) { return dt == CMU_F32 && CA % 128 == 0 && CB % 64 == 0; }, wg_wide_f32_on, true,
     WG_HALO_B, 3, false, MODE_W3, WG_BIAS_NONE, {wg_launch_wide_f32<4>, nullptr, nullptr}},
    {"cmu_conv3x3_wgrad(wide, fp32)", MODE_W3, 4, 64, 64, false, 2, 1, CMU_KNOB_WGRAD_BLOCKS,
     [](int CA, int CB, int dt) { return dt == CMU_F32 && CA % 64 == 0 && CA % 128 != 0 && CB % 64 == 0; }, wg_wide_f32_on, true,
     WG_HALO_B, 3, false, MODE_W3, WG_BIAS_NONE, {wg_launch_wide_f32<2>, nullptr, nullptr}},
    // the first kernel: every shape and dtype, 16 x 16 tiles and tile lists; its split count aims at CMU_WGRAD_BLOCKS1 workgroups
    {"cmu_conv3x3_wgrad", MODE_W3, 16, 0, 0, false, 1, 1, CMU_KNOB_WGRAD_BLOCKS1,
     [](int, int, int) { return true; }, wg_on, false,
     WG_ANY, 0, false, MODE_W3, WG_BIAS_NONE, {wg_launch_first<F32Traits, MODE_W3>, wg_launch_first<F16Traits, MODE_W3>, wg_launch_first<BF16Traits, MODE_W3>}},

    // wide ConvTranspose kernel (conv_wgrad2.inc): 16-bit dtypes, Cout in whole 64-blocks; 256 X channels per workgroup (NXI = 4) where Cin
    // allows -- the deeper decoder levels (CMU_WGT2_NX256=0: A/B) -- else 128 (NXI = 2)
    {"cmu_convT2x2_wgrad(wide)", MODE_WT, 4, 64, 256, false, 1, 1, CMU_KNOB_WGRAD_BLOCKS,
     [](int CA, int CB, int dt) { return cmu_dtype_size(dt) == 2 && CA % 64 == 0 && CB % 256 == 0; },
     [](int, int CB) { return cmu_knob(CMU_KNOB_WGRAD_WIDE) && wg_nx256(CB); }, false,
     WG_PLAIN, 0, false, 2, WG_BIAS_SPLITS, {nullptr, wg_launchT_wide<F16Traits, 4>, wg_launchT_wide<BF16Traits, 4>}},
    {"cmu_convT2x2_wgrad(wide)", MODE_WT, 4, 64, 128, false, 1, 1, CMU_KNOB_WGRAD_BLOCKS,
     [](int CA, int CB, int dt) { return cmu_dtype_size(dt) == 2 && CA % 64 == 0 && CB % 128 == 0; },
     [](int, int CB) { return cmu_knob(CMU_KNOB_WGRAD_WIDE) && !wg_nx256(CB); }, false,
     WG_PLAIN, 0, false, 2, WG_BIAS_SPLITS, {nullptr, wg_launchT_wide<F16Traits, 2>, wg_launchT_wide<BF16Traits, 2>}},
    // fp32 wide ConvTranspose kernel (conv_wgrad2f.inc): 128 c x 64 n blocks.  Follows CMU_WGRAD_WIDE_F32.
    {"cmu_convT2x2_wgrad(wide, fp32)", MODE_WT, 2, 64, 128, false, 1, 1, CMU_KNOB_WGRAD_BLOCKS,
     [](int CA, int CB, int dt) { return dt == CMU_F32 && CA % 64 == 0 && CB % 128 == 0; }, wg_wide_f32_on, true,
     WG_PLAIN, 3, false, 2, WG_BIAS_SUMS, {wg_launchT_wide_f32, nullptr, nullptr}},
    {"cmu_convT2x2_wgrad", MODE_WT, 16, 0, 0, false, 1, 4, -1,
     [](int, int, int) { return true; }, wg_on, false,
     WG_ANY, 0, false, MODE_WT, WG_BIAS_SUMS, {wg_launch_first<F32Traits, MODE_WT>, wg_launch_first<F16Traits, MODE_WT>, wg_launch_first<BF16Traits, MODE_WT>}},
};

// Tiles, blocks, pads and the split count of form f for the dims in p; returns the bytes the form writes to the workspace
static int64_t wg_geometry(const WGForm& f, int dt, WGParams& p) {
    const int cw = 128 / cmu_dtype_size(dt);
    const int a_blk = f.a_blk ? f.a_blk : cw, b_blk = f.b_blk ? f.b_blk : cw;
    const int na = cmu_div_up(p.CA, a_blk), nb = cmu_div_up(p.CB, b_blk);
    p.tilesX = cmu_div_up(p.W, 16);
    p.tilesY = cmu_div_up(p.H, f.tile_h);
    p.ntiles = p.B * p.tilesX * p.tilesY;
    p.nAB = f.swap ? nb : na;
    p.nBB = f.swap ? na : nb;
    p.CApad = na * a_blk;
    p.CBpad = nb * b_blk;
    p.splitk = wg_splitk(na * nb, p.ntiles, f.wgs, f.aim < 0 ? 512 : cmu_knob(f.aim));
    const int taps = f.family == MODE_W3 ? 9 : 4;
    const int64_t bias_rows = f.bias == WG_BIAS_SUMS ? CSUM_BLOCKS : f.bias == WG_BIAS_SPLITS ? p.splitk : 0;
    return ((int64_t)p.splitk * f.slabs * taps * p.CApad * p.CBpad + bias_rows * p.CA) * (int64_t)sizeof(float);
}
// both operands of one image within the range of a buffer descriptor
static bool wg_in_range(const WGForm& f, const WGParams& p, int dt) {
    if (f.range == WG_ANY) return true;
    const int64_t px = (int64_t)p.H * p.W, halo = p.W + 1, es = cmu_dtype_size(dt);
    const int64_t a_px = (f.family == MODE_WT ? 4 * px : px) + (f.range == WG_HALO_A ? halo : 0), b_px = px + (f.range == WG_HALO_B ? halo : 0);
    return (a_px * p.lda + p.CA) * es < WG_BUF_RANGE && (b_px * p.ldb + p.CB) * es < WG_BUF_RANGE;
}
static bool wg_tf_aligned(const WGForm& f, const WGParams& p) {
    return p.b_scale == nullptr || ((reinterpret_cast<uintptr_t>(p.b_scale) | reinterpret_cast<uintptr_t>(p.b_shift)) & f.tf_align) == 0;
}
// The form that serves the launch described by p (operands, transform, dims), its geometry filled into p.  The first row of the family whose
// shape and knobs hold claims the shape; where its tensors are out of range or misaligned, the first kernel runs -- no later wide row.
// tile_h: 0 for a dense launch, else the height of the tile list's tiles (16: the first kernel; 8: nullptr unless the form walks such lists).
// (The bytes the planned form writes are wg_geometry's return value: the size queries take their maximum over the candidate rows.)
static const WGForm* wg_plan(int family, int dt, int tile_h, WGParams& p) {
    bool claimed = false;
    for (const WGForm& f : WG_FORMS) {
        if (f.family != family) continue;
        if (f.range != WG_ANY) {
            if (claimed || tile_h == 16 || !f.shape(p.CA, p.CB, dt) || !f.knobs(p.CA, p.CB)) continue;
            claimed = true;
            if (!wg_in_range(f, p, dt) || !wg_tf_aligned(f, p)) continue;
        }
        if (tile_h == 8 && !f.lists8) return nullptr;
        wg_geometry(f, dt, p);
        return &f;
    }
    return nullptr;
}
// The size queries: the largest workspace of the forms that may serve the shape, whatever the strides, the transform and (for the forms
// marked so) the knobs turn out to be
static int64_t wg_ws_bytes(int family, int B, int H, int W, int Cin, int Cout, int dt) {
    if (cmu_dtype_size(dt) == 0 || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1;
    int64_t need = 0;
    for (const WGForm& f : WG_FORMS) {
        if (f.family != family || !f.shape(Cout, Cin, dt) || !(f.size_any_knobs || f.knobs(Cout, Cin))) continue;
        WGParams q = {};
        q.B = B; q.H = H; q.W = W; q.CA = Cout; q.CB = Cin;
        const int64_t w = wg_geometry(f, dt, q);
        if (w > need) need = w;
    }
    return need;
}

// bias gradient of the ConvTranspose: sum of dOut over all (B,2H,2W) pixels, CSUM_BLOCKS rows of partial sums in ws_sum
template <class TR>
static int wg_bias_sums_t(const WGParams& p, float* ws_sum, float* dbias, hipStream_t st) {
    const int nchunk = p.CA / TR::EPC;
    const int cpb = nchunk < 256 ? nchunk : 256, ppb = 256 / cpb, gy = cmu_div_up(nchunk, cpb);
    const int64_t npix = (int64_t)p.B * 4 * p.H * p.W;
    int gx = (int)(cmu_div_up64(npix, ppb * 4) < CSUM_BLOCKS ? cmu_div_up64(npix, ppb * 4) : CSUM_BLOCKS);
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL((channel_sum_kernel<TR>), dim3(gx, gy), dim3(256), 0, st, (const unsigned char*)p.a, p.lda, ws_sum, npix, p.CA, cpb, ppb);
    CMU_CHECK_LAUNCH("cmu_convT2x2_wgrad(bias)");
    hipLaunchKernelGGL(channel_sum_final_kernel, dim3(cmu_div_up(p.CA, 16)), dim3(256), 0, st, (const float*)ws_sum, gx, p.CA, dbias);
    CMU_CHECK_LAUNCH("cmu_convT2x2_wgrad(bias final)");
    return CMU_OK;
}
static int wg_bias_sums(const WGParams& p, int dt, float* ws_sum, float* dbias, hipStream_t st) { CMU_DISPATCH_DT(dt, wg_bias_sums_t, p, ws_sum, dbias, st); }

// the planned form's kernel, the reduction of its slabs in slab order, and the bias gradient where the form has one
static int wg_run(const WGForm& f, const WGParams& p, int dt, float* dW, float* dbias, hipStream_t st) {
    const bool wt = f.family == MODE_WT;
    if (int rc = f.launch[dt](p, st, f.name)) return rc;
    CMU_CHECK_LAUNCH(f.name);
    launch_wgrad_reduce((const float*)p.ws, p.splitk * f.slabs, wt ? 4 : 9, p.CApad, p.CBpad, p.CA, p.CB, dW, f.reduce_mode, st);
    CMU_CHECK_LAUNCH(wt ? "cmu_convT2x2_wgrad(reduce)" : "cmu_conv3x3_wgrad(reduce)");
    float* ws_sum = p.ws + (int64_t)p.splitk * f.slabs * 4 * p.CApad * p.CBpad;
    if (f.bias == WG_BIAS_SUMS) return wg_bias_sums(p, dt, ws_sum, dbias, st);
    if (f.bias == WG_BIAS_SPLITS) {
        hipLaunchKernelGGL(channel_sum_final_kernel, dim3(cmu_div_up(p.CA, 16)), dim3(256), 0, st, (const float*)ws_sum, p.splitk, p.CA, dbias);
        CMU_CHECK_LAUNCH("cmu_convT2x2_wgrad(bias final)");
    }
    return CMU_OK;
}

// the argument checks and the WGParams fill that the three launch entries share (a: the output gradient, b: the layer's input)
static int wg_args(const char* name, WGParams& p, const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from, const void* dA,
                   int64_t lda, bool ptrs_ok, void* ws, int B, int H, int W, int Cin, int Cout, int dt) {
    CMU_CHECK_ARG(ptrs_ok && ws && B > 0 && H > 0 && W > 0, "%s: null argument / bad dims", name);
    CMU_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "%s: scale/shift must both be set", name);
    CMU_CHECK_ARG(relu_from % (16 / cmu_dtype_size(dt)) == 0, "%s: relu_from=%d must be a multiple of the 16-byte chunk", name, relu_from);
    p.a = dA; p.lda = lda; p.b = x; p.ldb = ldx; p.b_scale = in_scale; p.b_shift = in_shift; p.relu_from = relu_from;
    p.ws = (float*)ws; p.B = B; p.H = H; p.W = W; p.CA = Cout; p.CB = Cin;
    return CMU_OK;
}

extern "C" int64_t cmu_conv3x3_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout, int dt) { return wg_ws_bytes(MODE_W3, B, H, W, Cin, Cout, dt); }
extern "C" int cmu_conv3x3_wgrad(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from, const void* dY,
                                 int64_t ldd, float* dW, int B, int H, int W, int Cin, int Cout, int dt, void* ws, void* stream) {
    int rc;
    if ((rc = cmu_check_act("cmu_conv3x3_wgrad(x)", x, ldx, Cin, dt))) return rc;
    if ((rc = cmu_check_act("cmu_conv3x3_wgrad(dY)", dY, ldd, Cout, dt))) return rc;
    WGParams p = {};
    if ((rc = wg_args("cmu_conv3x3_wgrad", p, x, ldx, in_scale, in_shift, relu_from, dY, ldd, dW != nullptr, ws, B, H, W, Cin, Cout, dt))) return rc;
    return wg_run(*wg_plan(MODE_W3, dt, 0, p), p, dt, dW, nullptr, (hipStream_t)stream);
}

// Sparse (SparK) weight gradient over a device-side tile list (cmu_sparse_tile_list).  The list's tile height says which kernel
// walks it: 16 (16 x 16 pixel tiles) = the first kernel, any shape; 8 (8 x 16 tiles, the wide kernel's K tile) = the wide kernel or the
// 64 x 64 form, for the shapes cmu_conv3x3_wgrad_tile_h names.  ws: cmu_conv3x3_wgrad_ws_bytes.
extern "C" int cmu_conv3x3_wgrad_tile_h(int B, int H, int W, int Cin, int Cout, int dt) {
    if (cmu_dtype_size(dt) == 0 || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1;
    WGParams p = {};
    p.B = B; p.H = H; p.W = W; p.CA = Cout; p.CB = Cin; p.lda = Cout; p.ldb = Cin;   // (dense NHWC tensors: ld = C)
    return wg_plan(MODE_W3, dt, 0, p)->lists8 ? 8 : 16;
}
extern "C" int cmu_conv3x3_wgrad_tiles(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from,
                                       const void* dY, int64_t ldd, float* dW, const int* tile_list, const int* tile_count, int tile_h,
                                       int B, int H, int W, int Cin, int Cout, int dt, void* ws, void* stream) {
    int rc;
    if ((rc = cmu_check_act("cmu_conv3x3_wgrad_tiles(x)", x, ldx, Cin, dt))) return rc;
    if ((rc = cmu_check_act("cmu_conv3x3_wgrad_tiles(dY)", dY, ldd, Cout, dt))) return rc;
    WGParams p = {};
    if ((rc = wg_args("cmu_conv3x3_wgrad_tiles", p, x, ldx, in_scale, in_shift, relu_from, dY, ldd, dW && tile_list && tile_count, ws, B, H, W, Cin, Cout, dt)))
        return rc;
    CMU_CHECK_ARG(tile_h == 16 || tile_h == 8, "cmu_conv3x3_wgrad_tiles: tile_h=%d (16: 16 x 16 tiles, 8: 8 x 16 tiles)", tile_h);
    p.tile_list = tile_list; p.tile_count = tile_count;
    const WGForm* f = wg_plan(MODE_W3, dt, tile_h, p);
    CMU_CHECK_ARG(f != nullptr,
                  "cmu_conv3x3_wgrad_tiles: an 8 x 16 tile list needs a shape of the wide kernel (16-bit, Cout %% 128 == 0, Cin %% 64 == 0; "
                  "cmu_conv3x3_wgrad_tile_h), got %d -> %d", Cin, Cout);
    return wg_run(*f, p, dt, dW, nullptr, (hipStream_t)stream);
}

extern "C" int64_t cmu_convT2x2_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout, int dt) { return wg_ws_bytes(MODE_WT, B, H, W, Cin, Cout, dt); }
extern "C" int cmu_convT2x2_wgrad(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from, const void* dOut,
                                  int64_t ldd, float* dW, float* dbias, int B, int H, int W, int Cin, int Cout, int dt, void* ws,
                                  void* stream) {
    int rc;
    if ((rc = cmu_check_act("cmu_convT2x2_wgrad(x)", x, ldx, Cin, dt))) return rc;
    if ((rc = cmu_check_act("cmu_convT2x2_wgrad(dOut)", dOut, ldd, Cout, dt))) return rc;
    WGParams p = {};
    if ((rc = wg_args("cmu_convT2x2_wgrad", p, x, ldx, in_scale, in_shift, relu_from, dOut, ldd, dW && dbias, ws, B, H, W, Cin, Cout, dt))) return rc;
    return wg_run(*wg_plan(MODE_WT, dt, 0, p), p, dt, dW, dbias, (hipStream_t)stream);
}
