// conv_igemm3.inc -- wide-tile 3x3 implicit-GEMM kernel (included by conv_igemm.hip).
//
// Why: an s_memtime timeline of the first kernel (tools/igemm_stamps.py, 256->256 @128x128) shows a wave spending
// ~4,300 cycles per K stage staging operands (issuing 14 x 1 KiB global loads through the CU's 64 B/clk vector-memory
// path: 1,760 cycles; BatchNorm+ReLU transform + LDS writes: 2,530) against 2,304 cycles of MFMA issue -- with two
// waves per SIMD the matrix pipe cannot be more than ~55 % busy.  The cure is arithmetic intensity per staged byte
// and a schedule that puts every MFMA phase beside a staging phase:
//   * workgroup = 512 threads (8 wave64, two per SIMD, one workgroup per CU); output tile = 16 x 32 pixels
//     (M = 512) x NB channels, NB = 128 (waves 4 x 2, wave tile 128 px x 64 ch = 4x2 MFMA 32x32 accumulators, 0.75 LDS
//     fragment reads per MFMA) or NB = 64 (waves 8 x 1, wave tile 64 px x 64 ch).
//   * K advances in 32-BYTE channel slices (the packed weights' native slice) and one step is ALL NINE taps of a slice:
//     the 18 x 34 pixel halo of the slice is staged once (transformed on the way: x*scale[c]+shift[c], ReLU, zero padding
//     kept zero; the (scale, shift) table sits in LDS) and re-read at the 9 tap offsets, next to the 9 x NB weight rows;
//     both simply double-buffered by slice parity (132 KB at NB = 128).  72 (NB = 128) / 36 (NB = 64) MFMAs per wave
//     and step against 3 halo chunks + 5 / 3 weight chunks staged per thread.
//   * TWO-PHASE PING-PONG: every wave runs the same straight-line body [MFMAs of slice k | barrier | stage slice k+1,
//     issue the loads of slice k+2 | barrier]; waves 4-7 (the SIMD partners of waves 0-3) run one stage phase + barrier
//     ahead of the loop, so in time a wave's MFMA phase (s_setprio 2) sits beside its partner's staging phase.  (A role
//     `if` inside the loop instead makes hipcc split live ranges and open the MFMA phase with vmcnt(0); so do loads the
//     prologue leaves pending, through the waitcnt scoreboard merge -- they are drained explicitly.)
//   * global loads are raw buffer loads: the per-thread offsets are loop-invariant VGPRs, the slice advance is a scalar
//     offset, out-of-image halo pixels point past num_records and read as zero -- no per-load address arithmetic, no
//     predication, no branches in the main loop.
//   * LDS: halo rows 48 B (32 + 16 pad) with the first kernel's MFMA row -> pixel map (pm_row / pm_col); weight rows 32 B
//     with the two 16-byte chunks swapped in rows whose bit 3 is set -- every ds_read_b128 fragment read is conflict-free.
//     During its MFMA phase a wave has the matrix pipe to itself, so tap t+1's fragments are read while tap t's MFMAs
//     issue (register double buffer, order pinned with sched_group_barrier).
// Epilogue: BatchNorm batch statistics of the raw output from the accumulators into the per-16x16-tile slab (two slab
// rows per workgroup: same slab shape as the first kernel -> same ABI) or, for data gradients, the BatchNorm-backward
// partial sums of the layer the gradient flows into; LDS transpose; 16-byte NHWC stores.
// Used when N % 128 == 0 (or N == 64 with K >= 128), K is a whole number of 64-byte slices, K <= 1024 when a transform
// is pending and one image fits a buffer descriptor; everything else (the 64->64 layers, odd channel counts of the tests,
// ConvTranspose modes) stays on the first kernel.  Earlier forms of this kernel that measured worse are in the round's
// history: 64-byte slices with a 3-part halo schedule and a 3-tap weight ring (-1...-4 %), a second register set with
// loads two stage phases ahead (-3 %), NB = 64 with 24 MFMAs per phase (below the first kernel).
#include <type_traits>

template <class TR, int NB_, int TWB_ = 2, int THB_ = 1>
struct IG3Cfg {
    typedef typename TR::elem_t elem_t;
    static constexpr int ES = (int)sizeof(elem_t);
    static constexpr int EPC = TR::EPC;
    static constexpr int KC = 32 / ES;  // channels per 32-byte slice
    static constexpr int NB = NB_;
    static constexpr int TWB = TWB_;                // tile width in 16-pixel column blocks: 2 (16 x 32 px) or 4 (16 x 64 px)
    static constexpr int THB = THB_;                // tile height in 16-pixel row blocks (2: the persistent kernel's 32 x 32 tile)
    static constexpr int TH = 16 * THB, TW = 16 * TWB;
    static constexpr int LW = TW + 2, LH = TH + 2, NPIX = LW * LH;  // 34 x 18 = 612 (66 x 18 = 1,188) halo pixels
    static constexpr int PS = 48;                   // halo rows: 32 B + 16 B pad (conflict-free 16-byte fragment reads)
    static constexpr int A_BYTES = NPIX * PS;       // 29,376
    static constexpr int PSB = 32;                  // weight rows: 32 B, the two 16-byte chunks swapped in rows with bit 3 set
    static constexpr int B_TAP = NB * PSB;
    static constexpr int B_BYTES = 9 * B_TAP;       // 18,432 / 36,864
    static constexpr int BUF_BYTES = A_BYTES + B_BYTES;
    static constexpr int MAIN_BYTES = 2 * BUF_BYTES;  // 95,616 / 132,480
    static constexpr int WN = NB / 64, WM = 8 / WN;
    static constexpr int RB = WM / TWB;             // row bands of waves; a wave owns (16 / RB) rows x 16 columns x 64 channels
    static constexpr int SW = TH / 2 / RB;          // 2x16-pixel strips per wave (4 or 2)
    static constexpr int A_CHUNKS = NPIX * 2, A_ITERS = (A_CHUNKS + 511) / 512;  // idx = it*512 + tid -> pixel idx/2, chunk idx&1 (3 / 5 iterations)
    static constexpr int B_CHUNKS = 9 * NB * 2, B_ITERS = (B_CHUNKS + 511) / 512;  // 1,152 (3) / 2,304 (5)
    static constexpr int MAX_K = THB == 1 ? 1024 : 128;   // pending-transform table (scale, shift) lives in LDS behind the buffers
    static constexpr int TAB_BYTES = 2 * MAX_K * 4;
    // epilogue: NFP n-fragments (32 channels each) staged per pass so that a pixel row is 128 B + pad for every dtype
    static constexpr int NFP = ES == 2 ? 2 : 1;
    static constexpr int EPI_ROW = NFP * 32 * ES + 16;  // 144
    static constexpr int EPI_WAVE = SW * 32 * EPI_ROW;
    static constexpr int EPI_STAGE = 8 * EPI_WAVE;
    static constexpr int EPI_BYTES = EPI_STAGE + 8 * 64 * 2 * 4;
#ifdef CMU_IG_STAMPS
    static constexpr int STAMP_OFF = MAIN_BYTES + TAB_BYTES;
    static constexpr int LDS_BYTES = (STAMP_OFF + 2048 > EPI_BYTES ? STAMP_OFF + 2048 : EPI_BYTES);
#else
    static constexpr int LDS_BYTES = MAIN_BYTES + TAB_BYTES > EPI_BYTES ? MAIN_BYTES + TAB_BYTES : EPI_BYTES;
#endif
    static constexpr unsigned OOB = 0x7fff0000u;  // offset no buffer reaches: the load returns zero
};

__device__ static inline u32x4 ig3_bload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}

// per-lane BatchNorm statistics of the accumulators: sums and sums of squares of the lane's 16*SW pixels of channels 32j + r,
// kept as two running pairs per channel (packed f32 math: v_pk_add_f32 / v_pk_fma_f32 take two accumulator elements per issue
// slot -- the epilogue is bound by the SIMD's vector issue), folded at the end.  Both wide kernels use it: same order, same bits.
typedef __attribute__((ext_vector_type(2))) float f32x2;
template <int SW, class OK>
__device__ __forceinline__ void ig3_lane_stats(const f32x16 (&acc)[SW][2], OK ok, float (&s1)[2], float (&s2)[2]) {
    f32x2 a[2], q[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) a[j] = q[j] = f32x2{0.f, 0.f};
#pragma unroll
    for (int i = 0; i < SW; ++i)
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
            const bool ok0 = ok(i, e), ok1 = ok(i, e + 1);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x2 v = {ok0 ? acc[i][j][e] : 0.f, ok1 ? acc[i][j][e + 1] : 0.f};
                a[j] += v;
                q[j] = __builtin_elementwise_fma(v, v, q[j]);
            }
        }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        s1[j] = a[j][0] + a[j][1];
        s2[j] = q[j][0] + q[j][1];
    }
}

// ---- BatchNorm+ReLU backward partial sums in the data-gradient epilogues (both wide kernels: same order, same bits) ----
// A lane holds the 16-byte chunk (EPC channels) of one pixel of dX as stored and of the producer layer's raw output x.
// The ReLU gate [scale*x + shift > 0] is taken as clamp(2^60 * (scale*x + shift), 0, 1): the clamp rides on the FMA
// (v_fma_mix_f32 ... clamp straight from the 16-bit x), where compare + select cost two more issue slots per element in an
// epilogue bound by vector issue.  2^60 scales the per-channel constants once (exact: a power of two; |scale*x|, |shift|
// stay below 2^90 for 16-bit x and eps = 1e-5), so the gate is exactly 0 for t <= 0 and exactly 1 from t = 2^-60 up; in
// between (never reached by an FMA of a 16-bit x unless |shift| < 1e-8) it fades instead of stepping.
template <int EPC>
__device__ __forceinline__ void ig3_bst_consts(const float* scale, const float* shift, int n, float (&gs)[EPC], float (&gh)[EPC]) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        gs[e] = scale[n + e] * 0x1p60f;
        gh[e] = shift[n + e] * 0x1p60f;
    }
}
template <class TR>
__device__ __forceinline__ void ig3_bst_accum(const u32x4& g, const u32x4& x, const float (&gs)[TR::EPC], const float (&gh)[TR::EPC],
                                              float (&bs1)[TR::EPC], float (&bs2)[TR::EPC]) {
    float gv[TR::EPC], xv[TR::EPC];
    TR::unpack(g, gv);
    TR::unpack(x, xv);
#pragma unroll
    for (int e = 0; e < TR::EPC; e += 2) {
        const float gate0 = __builtin_amdgcn_fmed3f(fmaf(xv[e], gs[e], gh[e]), 0.f, 1.f);
        const float gate1 = __builtin_amdgcn_fmed3f(fmaf(xv[e + 1], gs[e + 1], gh[e + 1]), 0.f, 1.f);
        const f32x2 dz = f32x2{gate0, gate1} * f32x2{gv[e], gv[e + 1]};
        const f32x2 s1 = f32x2{bs1[e], bs1[e + 1]} + dz;
        const f32x2 s2 = __builtin_elementwise_fma(dz, f32x2{xv[e], xv[e + 1]}, f32x2{bs2[e], bs2[e + 1]});   // sum(dz*x); xhat: in the fold
        bs1[e] = s1[0]; bs1[e + 1] = s1[1];
        bs2[e] = s2[0]; bs2[e + 1] = s2[1];
    }
}
// Fold over the eight pixel rows of the wave (lane bits 3..5; lane & 7 = channel chunk q) and write the wave's partials.
// gfx950's v_permlane32_swap / v_permlane16_swap exchange halves of two registers, so one add folds TWO channels' sums over a
// lane bit and halves the register count: EPC x 2 values -> EPC/4 x 2 in 3/4 * EPC swaps + adds, then row_ror:8 adds for bit 3.
// Afterwards lane (q, bit4, bit5) holds channels q*EPC + (EPC/2)*bit5 + (EPC/4)*bit4 + e, e < EPC/4 (lanes with bit 3 clear
// write).  `mean`, `invstd` and `stat` point at channel 0 of this pass's 32*NFP-channel block.
template <int EPC>
__device__ __forceinline__ void ig3_bst_fold(float (&bs1)[EPC], float (&bs2)[EPC], int lane, const float* mean, const float* invstd, float* stat) {
    constexpr int H1 = EPC / 2, H2 = EPC / 4;
    float a1[H1], a2[H1], b1[H2], b2[H2];
    auto fold32 = [](float d, float s) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(d), __float_as_uint(s), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);   // lanes 0-31: d over bit 5; lanes 32-63: s over bit 5
    };
    auto fold16 = [](float d, float s) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(d), __float_as_uint(s), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);   // even 16-lane rows: d over bit 4; odd rows: s over bit 4
    };
    auto fold8 = [](float v) { return v + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x128 /* row_ror:8 */, 0xf, 0xf, false)); };
#pragma unroll
    for (int e = 0; e < H1; ++e) { a1[e] = fold32(bs1[e], bs1[e + H1]); a2[e] = fold32(bs2[e], bs2[e + H1]); }
#pragma unroll
    for (int e = 0; e < H2; ++e) { b1[e] = fold8(fold16(a1[e], a1[e + H2])); b2[e] = fold8(fold16(a2[e], a2[e + H2])); }
    const int c0 = (lane & 7) * EPC + H1 * (lane >> 5) + H2 * ((lane >> 4) & 1);
    if (!(lane & 8)) {
#pragma unroll
        for (int e = 0; e < H2; ++e) {
            stat[(c0 + e) * 2 + 0] = b1[e];
            stat[(c0 + e) * 2 + 1] = (b2[e] - mean[c0 + e] * b1[e]) * invstd[c0 + e];   // sum(dz*(x-mean)*invstd) over the wave's pixels
        }
    }
}

// ---- shared epilogue of the wide-tile kernels: BatchNorm statistics (forward use) / BatchNorm-backward partial sums
// (data-gradient use) + LDS transpose + 16-byte NHWC stores.  Wave (wm, wn) of the 8 holds a (2*SW rows x 16 columns) x 64
// channel block of the 16 x 32 pixel x NB channel tile in acc[SW][2].
template <class TR, int NB, int TWB>
__device__ __forceinline__ void ig3_epilogue(const IGParams& p, unsigned char* smem, f32x16 (&acc)[IG3Cfg<TR, NB, TWB>::SW][2], int tid, int lane,
                                             int wave, int wn, int wrow, int wcol, int r, int h, int b, int ty, int tx, int ty0, int tx0,
                                             int n0) {
    typedef IG3Cfg<TR, NB, TWB> C;
    typedef typename TR::elem_t elem_t;
    constexpr int EPC = TR::EPC;
    constexpr int SW = C::SW;
    // accumulator element e of (strip i, n-fragment j): pixel m32 = (e&3) + 8*(e>>2) + 4*h of the strip, channel 32*j + r
    float* stat_lds = reinterpret_cast<float*>(smem + C::EPI_STAGE);
    const int row0 = wrow * 2 * SW, col0 = wcol * 16;
    if (p.stats != nullptr) {
        float s1[2], s2[2];
        ig3_lane_stats<SW>(acc, [&](int i, int e) {
            const int m32 = (e & 3) + 8 * (e >> 2) + 4 * h;
            const int row = row0 + 2 * i + pm_row(m32), col = col0 + pm_col(m32);
            return (ty0 + row < p.H) && (tx0 + col < p.W);
        }, s1, s2);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            s1[j] += __shfl_xor(s1[j], 32, 64);
            s2[j] += __shfl_xor(s2[j], 32, 64);
            if (h == 0) {
                stat_lds[(wave * 64 + 32 * j + r) * 2 + 0] = s1[j];
                stat_lds[(wave * 64 + 32 * j + r) * 2 + 1] = s2[j];
            }
        }
    }
    unsigned char* my = smem + wave * C::EPI_WAVE;
    unsigned char* yb = reinterpret_cast<unsigned char*>(p.y);
    constexpr int CPR = C::NFP * 32 / EPC;  // 16-byte chunks per staged pixel row (8)
    // per-wave channel partials in stat_lds -> one slab row per 16x16 half of the tile (the slab keeps the first
    // kernel's 16x16-tile shape)
    auto write_slab = [&](float* dst) {
        if (tid < TWB * NB) {
            const int half = tid / NB, c = tid % NB;                      // 16-column block of the tile
            const int tx16 = TWB * tx + half, tiles16 = (p.W + 15) / 16;
            if (tx16 < tiles16 && n0 + c < p.N) {
                float a = 0.f, q = 0.f;
#pragma unroll
                for (int wr = 0; wr < C::RB; ++wr) {
                    const int wv = (c / 64) * C::WM + wr * TWB + half;
                    a += stat_lds[(wv * 64 + (c & 63)) * 2 + 0];
                    q += stat_lds[(wv * 64 + (c & 63)) * 2 + 1];
                }
                const int64_t t16 = ((int64_t)b * p.tilesY + ty) * tiles16 + tx16;
                dst[(t16 * 2 + 0) * p.N + n0 + c] = a;
                dst[(t16 * 2 + 1) * p.N + n0 + c] = q;
            }
        }
    };
    constexpr int NIT = (SW * 32 * CPR) / 64;  // 16-byte chunks per lane and pass
    // ConvTranspose forward (p.bias set, N = 4*Cq, n = ij*Cq + co): bias add, and the store scatters to pixel (2y+i, 2x+j)
    float badd[2] = {0.f, 0.f};
    // (the wave's 64 channels lie inside ONE sub-pixel position when Cq is a multiple of 64 -- every layer of the reference UNet: the
    // position and the first channel are then wave-uniform and computed once; the per-chunk n / Cq, n % Cq of the general case were
    // two runtime integer divisions per 16-byte chunk, ~1,000 VALU instructions per tile in kernels that issue 32-64 MFMAs per tile)
    const bool cq64 = p.bias != nullptr && (p.Cq & 63) == 0;
    int ij_w = 0, co_w = 0;
    if (p.bias != nullptr) {
        const int nw = n0 + wn * 64;
        ij_w = nw / p.Cq;
        co_w = nw - ij_w * p.Cq;
#pragma unroll
        for (int j = 0; j < 2; ++j) badd[j] = p.bias[cq64 ? co_w + 32 * j + r : (nw + 32 * j + r) % p.Cq];
    }
#pragma unroll
    for (int jp = 0; jp < 2 / C::NFP; ++jp) {
        if (jp > 0) __syncthreads();
        // (BN-backward statistics, dgrad use) this pass's chunks of the producer layer's raw output: all loads in flight
        // before the accumulators go through LDS -- issued one by one inside the store loop each would expose a full HBM
        // round trip with nothing else resident on the CU to cover it
        u32x4 xr[NIT];
        if (p.bstats != nullptr) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int idx = it * 64 + lane;
                const int m = idx / CPR, q = idx % CPR;
                const int row = row0 + 2 * (m >> 5) + pm_row(m & 31), col = col0 + pm_col(m & 31);
                const int gy = ty0 + row < p.H ? ty0 + row : p.H - 1, gx = tx0 + col < p.W ? tx0 + col : p.W - 1;  // clamped
                const int n = n0 + wn * 64 + jp * C::NFP * 32 + q * EPC;
                const int64_t pixel = ((int64_t)b * p.H + gy) * p.W + gx;
                xr[it] = ld_global16(reinterpret_cast<const unsigned char*>(p.bx) + (pixel * p.ldbx + n) * (int64_t)sizeof(elem_t));
            }
        }
#pragma unroll
        for (int i = 0; i < SW; ++i)
#pragma unroll
            for (int jj = 0; jj < C::NFP; ++jj)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                    *reinterpret_cast<elem_t*>(my + m * C::EPI_ROW + (32 * jj + r) * C::ES) =
                        TR::from_float(acc[i][jp * C::NFP + jj][e] + badd[jp * C::NFP + jj]);
                }
        __syncthreads();
        if (jp == 0 && p.stats != nullptr) write_slab(p.stats);
        // BatchNorm+ReLU backward statistics of the layer this gradient flows into: per channel sum(gate*dX) and
        // sum(gate*dX*xhat) over the tile, on dX as stored; x = that layer's raw conv output
        float bsc[EPC], bsh[EPC], bs1[EPC], bs2[EPC];
        const int nq = n0 + wn * 64 + jp * C::NFP * 32 + (lane % CPR) * EPC;
        if (p.bstats != nullptr) {
            ig3_bst_consts<EPC>(p.b_scale, p.b_shift, nq, bsc, bsh);
#pragma unroll
            for (int e = 0; e < EPC; ++e) bs1[e] = bs2[e] = 0.f;
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = it * 64 + lane;
            const int m = idx / CPR, q = idx % CPR;
            const int row = row0 + 2 * (m >> 5) + pm_row(m & 31), col = col0 + pm_col(m & 31);
            const int gy = ty0 + row, gx = tx0 + col;
            const int n = n0 + wn * 64 + jp * C::NFP * 32 + q * EPC;
            if (gy < p.H && gx < p.W) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(my + m * C::EPI_ROW + q * 16);
                const int64_t pixel = ((int64_t)b * p.H + gy) * p.W + gx;
                if (p.bias != nullptr) {
                    const int ij = cq64 ? ij_w : n / p.Cq, co = cq64 ? co_w + (n - (n0 + wn * 64)) : n % p.Cq;
                    const int64_t po = ((int64_t)b * (2 * p.H) + 2 * gy + (ij >> 1)) * (2 * p.W) + 2 * gx + (ij & 1);
                    st_global16_nt(yb + (po * p.ldy + co) * (int64_t)sizeof(elem_t), v);
                } else {
                    st_global16_nt(yb + (pixel * p.ldy + n) * (int64_t)sizeof(elem_t), v);
                }
                if (p.bstats != nullptr) ig3_bst_accum<TR>(v, xr[it], bsc, bsh, bs1, bs2);
            }
        }
        if (p.bstats != nullptr) {
            const int nb0 = n0 + wn * 64 + jp * C::NFP * 32;
            ig3_bst_fold<EPC>(bs1, bs2, lane, p.b_mean + nb0, p.b_invstd + nb0, stat_lds + (wave * 64 + jp * C::NFP * 32) * 2);
        }
    }
    if (p.bstats != nullptr) {
        __syncthreads();
        write_slab(p.bstats);
    }
}

template <class TR, int NB, bool TF, int TWB>
__global__ __launch_bounds__(512) void conv_igemm3_kernel(const IGParams p) {
    typedef IG3Cfg<TR, NB, TWB> C;
    constexpr int EPC = TR::EPC;
    constexpr int SW = C::SW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;
    const int wm = wave % C::WM, wn = wave / C::WM;
    const int wcol = wm % TWB, wrow = wm / TWB;

    int64_t bid = blockIdx.x;
    {
        const int64_t nb = p.total_blocks;
        const int64_t q = nb >> 3, rem = nb & 7;
        const int64_t xcd = bid & 7, local = bid >> 3;
        bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + local;
    }
    const int nbk = (int)(bid % p.nblk);
    const int64_t tile = bid / p.nblk;
    const int tx = (int)(tile % p.tilesX);
    const int ty = (int)((tile / p.tilesX) % p.tilesY);
    const int b = (int)(tile / ((int64_t)p.tilesX * p.tilesY));
    const int ty0 = ty * C::TH, tx0 = tx * C::TW;
    const int n0 = nbk * NB;

    const int64_t img_elems = (int64_t)p.H * p.W * p.ldx;
    const unsigned char* ximg = reinterpret_cast<const unsigned char*>(p.x) + (int64_t)b * img_elems * C::ES;
    const unsigned x_bytes = (unsigned)((((int64_t)p.H * p.W - 1) * p.ldx + p.K) * C::ES);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(ximg), 0, (int)x_bytes, 0x00020000);
    const unsigned w_bytes = (unsigned)((int64_t)p.nslices32 * 9 * p.npad * 32);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)w_bytes, 0x00020000);

    // ---- per-thread staging roles (loop invariant) ------------------------------------------------------------------
    const int cg = tid & 1;  // 16-byte chunk of the 32-byte slice
    unsigned a_voff[C::A_ITERS];
    unsigned a_inb = 0;
#pragma unroll
    for (int it = 0; it < C::A_ITERS; ++it) {
        const int pix = it * 256 + (tid >> 1);
        const int py = pix / C::LW, px = pix % C::LW;
        const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
        const bool ok = pix < C::NPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        a_voff[it] = ok ? (unsigned)((((int64_t)gy * p.W + gx) * p.ldx + cg * EPC) * C::ES) : C::OOB;
        a_inb |= (ok ? 1u : 0u) << it;
    }
    const bool a_last_live = ((C::A_ITERS - 1) * 256 + (tid >> 1)) < C::NPIX;
    const unsigned a_st = (unsigned)((tid >> 1) * C::PS + cg * 16);  // + it * 256 * PS (+ buffer)
    // weights: chunk idx = it*512 + tid -> row = idx >> 1 = tap * NB + n.  Rows are 32 B in LDS; the chunk goes to slot
    // cg ^ bit3(row) (bit 3 of the row = bit 4 of tid: NB and 256 are multiples of 16), which makes the 16 rows a
    // ds_read_b128 lane group touches cover all 16 slots of the 256-byte bank row
    unsigned b_voff[C::B_ITERS];
#pragma unroll
    for (int it = 0; it < C::B_ITERS; ++it) {
        const int row = it * 256 + (tid >> 1);
        const int t = row / NB, n = row % NB;
        b_voff[it] = row < 9 * NB ? (unsigned)(((int64_t)t * p.npad + n0 + n) * 32 + cg * 16) : C::OOB;
    }
    const bool b_last_live = ((C::B_ITERS - 1) * 256 + (tid >> 1)) < 9 * NB;
    const unsigned b_st = (unsigned)(C::A_BYTES + (tid >> 1) * C::PSB + ((cg ^ ((tid >> 4) & 1)) * 16));  // + it * 256 * PSB
    const unsigned w_slice = (unsigned)p.npad * 32u * 9u;                                                  // bytes per slice of the pack

    u32x4 areg[C::A_ITERS], breg[C::B_ITERS];
    const int nsl = p.nslices32;
    // pending BN transform of the input: the whole (scale, shift) table sits in LDS (8 KB for 1024 channels) and is read
    // when a slice is stored -- 17 fewer registers held across the MFMA phase than a per-slice register copy
    float* tab = reinterpret_cast<float*>(smem + C::MAIN_BYTES);
    if (TF)
        for (int c = tid; c < p.K; c += 512) {
            tab[c] = p.in_scale[c];
            tab[C::MAX_K + c] = p.in_shift[c];
        }
    auto issue_loads = [&](int s) {
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) areg[it] = ig3_bload(rs_x, a_voff[it], (unsigned)(s * 32));
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it) breg[it] = ig3_bload(rs_w, b_voff[it], (unsigned)s * w_slice);
    };
    auto store_regs = [&](unsigned buf, int s) {
        float sc[EPC], sh[EPC];
        float lo = 0.f;
        if (TF) {
            const int c0 = s * C::KC + cg * EPC;
#pragma unroll
            for (int e = 0; e < EPC; e += 4) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(tab + c0 + e);
                const f32x4 c = *reinterpret_cast<const f32x4*>(tab + C::MAX_K + c0 + e);
#pragma unroll
                for (int q = 0; q < 4; ++q) { sc[e + q] = a[q]; sh[e + q] = c[q]; }
            }
            lo = cmu_relu_on(c0, p.relu_from) ? 0.f : -__builtin_inff();
        }
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) {
            u32x4 v = areg[it];
            if (TF) {
                float f[EPC];
                TR::unpack(v, f);
#pragma unroll
                for (int e = 0; e < EPC; ++e) f[e] = fmaxf(fmaf(f[e], sc[e], sh[e]), lo);
                v = TR::pack(f);
                if (!((a_inb >> it) & 1u)) v = u32x4{0u, 0u, 0u, 0u};
            }
            if (it < C::A_ITERS - 1 || a_last_live) *reinterpret_cast<u32x4*>(smem + buf + a_st + it * (256 * C::PS)) = v;
        }
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it)
            if (it < C::B_ITERS - 1 || b_last_live) *reinterpret_cast<u32x4*>(smem + buf + b_st + it * (256 * C::PSB)) = breg[it];
    };

    f32x16 acc[SW][2];
#pragma unroll
    for (int i = 0; i < SW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const unsigned a_frag = (unsigned)(((wrow * 2 * SW + pm_row(r)) * C::LW + wcol * 16 + pm_col(r)) * C::PS + h * 16);
    const unsigned b_frag = (unsigned)(C::A_BYTES + (wn * 64 + r) * C::PSB + ((h ^ ((r >> 3) & 1)) * 16));

    // the 9 x (SW x 2) MFMAs of one slice: tap t+1's fragments are read while tap t's MFMAs issue
    auto mfma_step = [&](unsigned buf) {
        u32x4 fa[2][SW], fb[2][2];
        auto rd = [&](int t, int set) {
            const unsigned ao = (unsigned)(((t / 3) * C::LW + (t % 3)) * C::PS);
            fa[set][0] = *reinterpret_cast<const u32x4*>(smem + buf + a_frag + ao);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[set][j] = *reinterpret_cast<const u32x4*>(smem + buf + b_frag + t * C::B_TAP + j * (32 * C::PSB));
#pragma unroll
            for (int i = 1; i < SW; ++i) fa[set][i] = *reinterpret_cast<const u32x4*>(smem + buf + a_frag + ao + i * (2 * C::LW * C::PS));
        };
        rd(0, 0);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t + 1 < 9) rd(t + 1, (t + 1) & 1);
#pragma unroll
            for (int i = 0; i < SW; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) TR::mma16(fa[t & 1][i], fb[t & 1][j], acc[i][j]);
        }
        if (sizeof(typename TR::elem_t) == 2) {
            __builtin_amdgcn_sched_group_barrier(0x100, SW + 2, 0);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
#pragma unroll
                for (int n = 0; n < SW + 2; ++n) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * SW - (SW + 2), 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * SW, 0);
        }
    };

    // ---- prologue: slice 0 staged, slice 1 in flight --------------------------------------------------------------------
    // both slices' loads go out together (the accumulators are not live yet: registers are free), so slice 1 travels
    // while slice 0 is transformed and stored
    issue_loads(0);
    {
        u32x4 a0[C::A_ITERS], b0[C::B_ITERS];
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) a0[it] = areg[it];
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it) b0[it] = breg[it];
        issue_loads(nsl > 1 ? 1 : 0);
        __syncthreads();   // the transform table is complete
        u32x4 a1[C::A_ITERS], b1[C::B_ITERS];
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) { a1[it] = areg[it]; areg[it] = a0[it]; }
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it) { b1[it] = breg[it]; breg[it] = b0[it]; }
        store_regs(0u, 0);
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) areg[it] = a1[it];
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it) breg[it] = b1[it];
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);   // no prologue load may stay pending into the loop (see the header)
    __syncthreads();

    // ---- main loop: [MFMAs of slice k | barrier | stage | barrier]; waves 4-7 run one stage phase ahead ---------------
    const bool second = wave >= 4;
#ifdef CMU_IG_STAMPS
    // diagnostic build: waves 0 and 4 stamp s_memtime into LDS (a global store per stamp would sit in vmcnt and stall the
    // very loads being timed); copied out after the loop
    const int stamp_slot = (blockIdx.x % 61 == 0 && blockIdx.x / 61 < 32) ? (int)(blockIdx.x / 61) : -1;
    unsigned long long* stamp_lds = reinterpret_cast<unsigned long long*>(smem + C::STAMP_OFF);
#define IG3_STAMP(k_)                                                                                   \
    do {                                                                                                 \
        if (stamp_slot >= 0 && k < 15 && (tid & 255) == 0)                                               \
            stamp_lds[((tid >> 8) * 16 + k) * 8 + (k_)] = __builtin_amdgcn_s_memtime();                  \
    } while (0)
#else
#define IG3_STAMP(k_) do {} while (0)
#endif
    auto stage_phase = [&](int j) {
        store_regs((unsigned)((j + 1) & 1) * C::BUF_BYTES, j + 1);   // slice j+1
        issue_loads(j + 2 < nsl ? j + 2 : nsl - 1);                   // slice j+2, clamped
    };
    if (second) {
        if (1 < nsl) stage_phase(0);
        __syncthreads();
    }
#ifdef CMU_IG_STAMPS
    // shader clock under this load: delta s_memtime / delta s_memrealtime (100 MHz) around the loop, slot 15 of wave 0
    if (stamp_slot >= 0 && tid == 0) {
        stamp_lds[15 * 8 + 0] = __builtin_amdgcn_s_memtime();
        stamp_lds[15 * 8 + 1] = __builtin_amdgcn_s_memrealtime();
    }
#endif
#pragma unroll 1
    for (int k = 0; k < nsl; ++k) {
        IG3_STAMP(0);
        __builtin_amdgcn_s_setprio(2);   // the MFMA phase outranks the partner wave's staging instructions at issue
        mfma_step((unsigned)(k & 1) * C::BUF_BYTES);
        __builtin_amdgcn_s_setprio(0);
        IG3_STAMP(1);
        __syncthreads();
        IG3_STAMP(2);
        const int j = k + (second ? 1 : 0);
        if (j + 1 < nsl) stage_phase(j);
        IG3_STAMP(3);
        __syncthreads();
        IG3_STAMP(4);
    }
    if (!second) __syncthreads();
#ifdef CMU_IG_STAMPS
    if (stamp_slot >= 0 && tid == 0) {
        stamp_lds[15 * 8 + 2] = __builtin_amdgcn_s_memtime();
        stamp_lds[15 * 8 + 3] = __builtin_amdgcn_s_memrealtime();
    }
    __syncthreads();
    if (stamp_slot >= 0 && tid < 256) g_ig_stamps[stamp_slot * 256 + tid] = ((tid >> 3) % 16 < nsl || (tid >> 3) == 15) ? stamp_lds[tid] : 0ull;
    __syncthreads();
#endif

    ig3_epilogue<TR, NB, TWB>(p, smem, acc, tid, lane, wave, wn, wrow, wcol, r, h, b, ty, tx, ty0, tx0, n0);
}

template <class TR, int NB, bool TF, int TWB>
static int launch_igemm3_cfg(IGParams p, hipStream_t st) {
    typedef IG3Cfg<TR, NB, TWB> C;
    constexpr const char* name = "cmu_conv3x3_fwd(wide, 32-byte slices)";
    p.tilesX = cmu_div_up(p.W, C::TW);
    p.tilesY = cmu_div_up(p.H, C::TH);
    p.nblk = p.N / NB;
    p.nslices32 = p.K / C::KC;
    p.nslices = p.nslices32;
    p.npad = cmu_conv3x3_npad(p.N);
    p.total_blocks = (int64_t)p.B * p.tilesX * p.tilesY * p.nblk;
    if (int rc = cmu_launch_lds<&conv_igemm3_kernel<TR, NB, TF, TWB>>(dim3((unsigned)p.total_blocks), dim3(512), C::LDS_BYTES, st, name, p)) return rc;
    cmu_set_kernel_tag("conv_igemm3_kernel");
    CMU_CHECK_LAUNCH(name);
    return CMU_OK;
}

static bool cmu_conv_persist_enabled();   // conv_igemm3p.inc
// CMU_CONV_PERSIST_PART=0: shapes with partial tiles stay on the one-tile kernel (A/B switch: environment read once; tests flip it
// through cmu_set_dispatch_override)
static bool igemm3_persist_part_enabled() { return cmu_knob(CMU_KNOB_CONV_PERSIST_PART); }
// CMU_CONV_WIDE=0 keeps every layer on the first kernel (A/B switch for the benches)
static bool cmu_conv_wide_enabled() { return cmu_knob(CMU_KNOB_CONV_WIDE) != 0; }
template <class TR>
static bool igemm3_eligible(const IGParams& p) {
    constexpr int KC = 64 / (int)sizeof(typename TR::elem_t);
    if (!cmu_conv_wide_enabled()) return false;
    // 64-channel layers: NB = 64 measures +6 % over the first kernel with 128 input channels and -5 %
    // with 64 (both ~700-850 TFLOP/s: at 512 x 512 these layers run into the per-CU fetch rate, not the matrix pipe), so
    // it takes K >= 128 by default; CMU_CONV_WIDE=2 sends every 64-channel layer to it (the tests run both)
    const bool nb64 = cmu_knob(CMU_KNOB_CONV_WIDE) == 2;
    // (the persistent form, conv_igemm3p.inc, measures 837 vs 690 TFLOP/s on 64 -> 64 at 512 x 512: with it every
    // whole-tile 64-channel layer goes wide)
    const bool persist = cmu_conv_persist_enabled() && ((p.H % 16 == 0 && p.W % 32 == 0) || igemm3_persist_part_enabled());
    if (p.N == 64 && !nb64 && !persist && p.K < 128) return false;
    if (p.in_scale != nullptr && p.K > 1024) return false;   // the transform table in LDS holds 1024 channels
    if (p.N % 64 != 0 || (p.N > 64 && p.N % 128 != 0) || p.K % KC != 0 || p.K < KC) return false;
    if (((int64_t)p.H * p.W * p.ldx + p.K) * (int64_t)sizeof(typename TR::elem_t) >= 0x7fff0000ll) return false;
    if ((int64_t)(p.K / KC) * 2 * 9 * cmu_conv3x3_npad(p.N) * 32 >= 0x7fff0000ll) return false;
    if ((reinterpret_cast<uintptr_t>(p.in_scale) | reinterpret_cast<uintptr_t>(p.in_shift)) & 15) return false;
    return true;
}
// Small batches / deep levels (finetuning at 256 x 256, bs 6 ... 16: level 4 has 12 ... 32 pixel tiles): with 128-channel blocks the
// launch has fewer items than the chip has CUs, and a workgroup's time is its own K loop whatever the others do -- 64-channel blocks
// double the items at half the MFMAs each (same MFMA order per accumulator: bit-identical outputs; the statistics fold the same
// 16 x 16 tiles in another lane order).  Taken while the doubled item count still fits one round of workgroups.
// CMU_CONV_NARROW=0 keeps the 128-channel blocks (A/B switch).
static int cmu_num_cus();   // conv_igemm3p.inc
static bool igemm3_narrow_blocks(const IGParams& p, int tw = 32) {
    if (!cmu_knob(CMU_KNOB_CONV_NARROW) || p.N % 128 != 0) return false;   // (tests flip it through cmu_set_dispatch_override)
    const int64_t items = (int64_t)p.B * cmu_div_up(p.W, tw) * cmu_div_up(p.H, 16) * (p.N / 128);
    return 2 * items <= cmu_num_cus();
}
// Images whose width in 16-pixel columns is odd leave the right half of their last 16 x 32 tile empty: a 16 x 16 image (level 5 of
// a 256 x 256 input, 14 x 14 of a 224 x 224 one) fills HALF of its only tile.  16 x 16 pixel tiles (TWB = 1: a wave owns 4 rows x
// 16 columns x 64 channels) waste nothing there; they stage the same weight rows for half the MFMAs, which the 16-bit tile cannot
// hide (taken for one-column images only), while the f32 tile (MFMAs 16 x slower per byte staged) takes them up to 7 columns.
// Measured (tools/slim_sweep.sh): 1024 -> 1024 @ 16 x 16, bs 32: f32 2.12 -> 1.10 ms, f16 0.236 -> 0.162 ms; @ 14 x 14 the same ratios.
// Same MFMA order per accumulator -> bit-identical outputs.  CMU_CONV_SLIM=0: off (A/B switch; cmu_set_dispatch_override in tests).
static bool igemm3_slim_tiles(const IGParams& p, int es) {
    if (!cmu_knob(CMU_KNOB_CONV_SLIM)) return false;
    const int c16 = cmu_div_up(p.W, 16);
    if (!(c16 & 1)) return false;
    if (c16 == 1) return true;
    // wider images: only where the 32-pixel tiles already fill the chip (below that the half-empty tiles cost nothing: measured
    // -2 % at bs 16, +11 ... 29 % at bs 32 on 48 / 80 / 112 pixel levels)
    const int64_t items = (int64_t)p.B * cmu_div_up(p.W, 32) * cmu_div_up(p.H, 16) * cmu_div_up(p.N, 128);
    return es == 4 && c16 <= 7 && items >= cmu_num_cus();
}
template <class TR, int TWB>
static int launch_igemm3_tw(const IGParams& p, hipStream_t st) {
    const bool tf = p.in_scale != nullptr;
    if (p.N % 128 == 0 && !igemm3_narrow_blocks(p, 16 * TWB))
        return tf ? launch_igemm3_cfg<TR, 128, true, TWB>(p, st) : launch_igemm3_cfg<TR, 128, false, TWB>(p, st);
    // (64-channel layers on 16 x 64 pixel tiles -- TWB = 4, 72 MFMAs per phase -- measured -2.5 % at K = 64 and +5 % at
    // K = 128: those layers are short of overlap between their memory and MFMA phases across tiles, not of phase length;
    // the variant is not instantiated)
    return tf ? launch_igemm3_cfg<TR, 64, true, TWB>(p, st) : launch_igemm3_cfg<TR, 64, false, TWB>(p, st);
}
template <class TR>
static int launch_igemm3(const IGParams& p, hipStream_t st) {
    if (igemm3_slim_tiles(p, (int)sizeof(typename TR::elem_t))) return launch_igemm3_tw<TR, 1>(p, st);
    return launch_igemm3_tw<TR, 2>(p, st);
}
