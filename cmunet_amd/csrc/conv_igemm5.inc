// conv_igemm5.inc -- persistent 3x3 implicit-GEMM kernel on the 16x16x32 MFMA shape (round 5; included by conv_igemm.hip after
// conv_igemm3p.inc, whose item lists, ping-pong schedule and slab ABI it keeps).
//
// Why: the 32x32x16 kernels run their steady state at the matrix pipe's pace (35 cycles per MFMA) and the chip holds ~1.27-1.34 GHz
// under them: they are bound by POWER, not by issue slots (profiles/r04_igemm3p_timeline.txt, profiles/r02_mfma_clock.txt).  The
// levers the hardware offers (MI355X guide, "DVFS give-back" items 4 and 7) are less energy per MFMA: the 16x16x32 shape (half the
// accumulator traffic per FLOP: 1.12-1.15 x the FLOP/s of 32x32x16 at equal cycles on LDS-fed random data), fewer LDS bytes and
// fewer vector instructions per MFMA.  16x16x32 contracts 32 channels of one tap per instruction = a 64-byte channel slice; with
// the weights of a slice in LDS next to the halo (9 x 128 x 64 B = 74 KB, twice) that does not fit a CU -- DESIGN section 8 item 0.
// So here
//   * only the HALO of a 64-byte slice is staged in LDS (two planes of 32-byte pixel rows, double-buffered by slice parity:
//     2 x 39,296 B), transformed on the way exactly as in conv_igemm3p (pending BatchNorm + ReLU, zero padding);
//   * the WEIGHT fragments go straight from the packed tensor (L2 / L1) into registers, one tap ahead of the MFMAs that use them:
//     the four waves of a half hold the same 64 output channels and run in step, so three of their four requests hit the CU's L1;
//     the pack is the one every other kernel reads ([32-byte slice][tap][row][32 B]) -- a lane's 16 bytes are one 16-byte chunk of
//     one row, a wave's 1 KiB fragment is eight whole 128-byte lines;
//   * MFMA roles are swapped against the older kernels: A = weights (M = 16 output channels), B = pixels (N = 16 pixels of one image
//     row), so a lane of the result holds 4 channels of ONE pixel and, with the rows of the four channel blocks permuted on the load
//     side (row m of block j = channel 32 (j >> 1) + 8 (m >> 2) + 4 (j & 1) + (m & 3)), 2 x 8 contiguous channels of it: the
//     epilogue converts and stores 16 bytes per lane with no LDS transpose (four lanes = 64 contiguous bytes of a pixel), the two
//     halves' epilogues share nothing and nothing of a tile's end is serialised between them;
//   * per tap a wave reads 8 pixel fragments from LDS and 4 weight fragments from L1 for 32 MFMAs: 0.5 LDS fragment reads per
//     32x32x16-equivalent (0.75 before), a third of the staging stores and transform instructions per MFMA.
// LDS bank mapping (ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...: every group mixes
// two 16-byte K chunks over all 16 pixels, so no odd row stride and no XOR swizzle of a 64-byte row is conflict-free at every tap
// offset): rows of 32 bytes = one PLANE per pair of K chunks, MFMA column n -> pixel x offset pi(n) with pi({0-3, 12-15}) = 0..7
// and pi({4-11}) = 8..15: within a group the lanes of one chunk read 8 consecutive 32-byte rows = 64 distinct banks between the
// two chunks, whatever the tap offset.
// Served: 16-bit operands, N % 128 == 0, K % 64 == 0, whole 16 x 32 tiles, dense launches (the tile-list form stays on
// conv_igemm3p); forward with pending transform + statistics, plain, and the data-gradient form with the BatchNorm-backward sums.
// The accumulation order differs from the 32x32x16 kernels (32 channels per MFMA instead of 16): results agree to rounding, not
// bit for bit; CMU_CONV_V5=0 keeps the older kernels (A/B switch).
#ifndef CMU_V5_ST_NT
#define CMU_V5_ST_NT 1
#endif
struct IG5Cfg {
    static constexpr int ES = 2, EPC = 8;
    static constexpr int KC = 32;                       // channels per 64-byte slice
    static constexpr int NB = 128;
    static constexpr int TH = 16, TW = 32, LW = TW + 2, LH = TH + 2, NPIX = LW * LH;   // 34 x 18 = 612 halo pixels
    static constexpr int PLANE = NPIX * 32;             // 19,584
    static constexpr int PSTRIDE = PLANE + 64;          // plane 1 starts 16 banks off plane 0: a staging store's 8-lane group (two pixels x four chunks) is conflict-free
    static constexpr int A_BYTES = 2 * PSTRIDE;         // 39,296
    static constexpr int MAIN_BYTES = 2 * A_BYTES;      // 78,592
    static constexpr int MAX_K = 1024;
    static constexpr int TAB_BYTES = 2 * MAX_K * 4;
    static constexpr int STAT_OFF = MAIN_BYTES + TAB_BYTES;
    static constexpr int STAT_PAR = 8 * 64 * 2 * 4;     // per-wave channel partials of one item
    // data-gradient form: the producer layer's raw output for rows 0-3 of every wave's tile, fetched by LDS-DMA during the item's last MFMA
    // phase (8 x 1 KiB per wave, lane-linear: a lane reads back exactly the 16 bytes it asked for)
    static constexpr int BX_OFF = STAT_OFF + 2 * STAT_PAR;
    static constexpr int BX_WAVE = 8 * 1024, BX_BYTES = 8 * BX_WAVE;
    static constexpr int STAMP_OFF = BX_OFF + BX_BYTES;   // diagnostic build only (-DCMU_IG_STAMPS, tools/v5_stamps.py)
    static constexpr int STAMP_ITERS = 16;
#ifdef CMU_IG_STAMPS
    static constexpr int LDS_BYTES = STAMP_OFF + 2 * STAMP_ITERS * 8 * 8;
    static constexpr int LDS_BYTES_BST = LDS_BYTES;
#else
    static constexpr int LDS_BYTES = STAT_OFF + 2 * STAT_PAR;   // two item parities (K = 64 layers: two positions per item)
    static constexpr int LDS_BYTES_BST = BX_OFF + BX_BYTES;     // 160,512
#endif
    static constexpr int A_ITERS = 5;                   // 2,448 chunks over 512 threads
    static constexpr unsigned OOB = 0x7fff0000u;
};

__device__ __forceinline__ float ig5_row16_sum(float v) {
    // sum over the 16 lanes of a DPP row (the 16 pixels of an MFMA column block); every lane ends with the total
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x128 /* row_ror:8 */, 0xf, 0xf, false));
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x124 /* row_ror:4 */, 0xf, 0xf, false));
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x122 /* row_ror:2 */, 0xf, 0xf, false));
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x121 /* row_ror:1 */, 0xf, 0xf, false));
    return v;
}

// Sums over the 16 lanes of a DPP row for a BATCH of values: four rotate-and-add steps, each over all values before the next step starts.
// Round 5's first form reduced one value at a time with a conditional LDS write behind each: sixteen basic blocks of one dependent chain
// each (v_mov 0 / v_mov_dpp / v_pk_add per step: ~340 cycles per value, 5.4K cycles of a 10K-cycle epilogue by s_memtime stamps).  Here the
// chains interleave: v_add_f32_dpp straight on the rotated operand; a value's next step comes N instructions later (asm volatile keeps the
// order), far beyond the two wait states a DPP read of a freshly written register needs.
template <int N>
__device__ __forceinline__ void ig5_row16_sum_batch(float (&v)[N]) {
    static_assert(N >= 4, "the DPP read-after-write distance relies on the batch size");
    // (two wait states between a VALU write of a register and a DPP read of it: what precedes the batch is the compiler's to schedule)
    asm volatile("s_nop 1");
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf" : "+v"(v[k]));
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf" : "+v"(v[k]));
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("v_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf" : "+v"(v[k]));
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("v_add_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf" : "+v"(v[k]));
}

// One row of the wave's tile (16 pixels x 64 channels) as FULL 128-byte lines.  A lane holds two 16-byte chunks of ITS pixel (channels
// 8 g ..+8 and 32 + 8 g ..+8); stored as they are, an instruction writes 16 pixels x 64 bytes -- and the CU's store path takes 57 cycles per
// such instruction against 17 for eight full lines (tools/store_probe.hip: 15 against 47-54 B/clk/CU; the epilogue's 16 stores per wave were
// 3.9K of its 7.7K cycles by s_memtime stamps).  So lanes L and L + 8 of a 16-lane row trade one chunk through DPP (row_ror:8): the first
// instruction then writes both halves of the pixel of lane L < 8, the second both halves of the pixel of lane L >= 8 -- 8 lanes x 16 B per
// pixel, 8 pixels per instruction, 16 selects + 4 DPP moves per row.
__device__ __forceinline__ void ig5_store_row_lines(unsigned char* rowbase, unsigned offA, unsigned offB, bool lo, const u32x4& c0, const u32x4& c1) {
    u32x4 send, recv;
#pragma unroll
    for (int q = 0; q < 4; ++q) send[q] = lo ? c1[q] : c0[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) recv[q] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send[q], 0x128 /* row_ror:8 */, 0xf, 0xf, false);
    u32x4 a, b;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a[q] = lo ? c0[q] : recv[q];     // instruction 1: the pixel of the pair's lower lane -- its own first half | the partner's copy of its second half
        b[q] = lo ? recv[q] : c1[q];     // instruction 2: the pixel of the pair's upper lane
    }
#if CMU_V5_ST_NT
    st_global16_nt(rowbase + offA, a);
    st_global16_nt(rowbase + offB, b);
#else
    st_global16(rowbase + offA, a);
    st_global16(rowbase + offB, b);
#endif
}

template <int N, int I = 0, class F>
__device__ __forceinline__ void ig5_static_for(F& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        ig5_static_for<N, I + 1>(f);
    }
}

template <class TR, bool TF, bool BST>
__global__ __launch_bounds__(512) void conv_igemm5_kernel(const IGParams p) {
    typedef IG5Cfg C;
    static_assert(sizeof(typename TR::elem_t) == 2, "16-bit operands only");
    constexpr int EPC = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 2, wm = wave & 3;        // waves 0-3: channels [0, 64) of the block, waves 4-7: [64, 128)
    const int wcol = wm & 1, wrow = wm >> 1;        // the wave's 8 rows x 16 columns of the 16 x 32 pixel tile

    // ---- this workgroup's items (as conv_igemm3p: XCD-contiguous static lists) ---------------------------------------------
    const int nx = gridDim.x < 8u ? (int)gridDim.x : 8;
    const int xcd = (int)blockIdx.x % nx, local = (int)blockIdx.x / nx;
    const int nloc = ((int)gridDim.x - xcd + nx - 1) / nx;
    int item0, n_my;
    {
        const int total = (int)p.total_blocks;
        const int q = total / nx, rem = total % nx;
        const int start = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
        const int cnt = q + (xcd < rem ? 1 : 0);
        if (local >= cnt) return;
        item0 = start + local;
        n_my = (cnt - local + nloc - 1) / nloc;
    }
    const int nsl = p.nslices;   // 64-byte slices per item (even)
    const int G = n_my * nsl;
#ifdef CMU_IG_TAILS
    if (tid == 0) g_ig_stamps[3072 + blockIdx.x] = __builtin_amdgcn_s_memrealtime();      // (behind the per-phase stamps' slots)
#endif

    struct Item { int b, ty, tx, n0; };
    auto fdiv = [](unsigned n, const unsigned (&fd)[2]) { return (__umulhi(n, fd[0]) + n) >> fd[1]; };
    auto decode = [&](int i) {
#ifdef CMU_V5_MOCK_WINO
        const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(item0 + i * nloc) % (unsigned)(p.total_blocks / 4);     // every item four times
#else
        const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(item0 + i * nloc);
#endif
        const unsigned tile = fdiv(w, p.fd_nblk), nbk = w - tile * (unsigned)p.nblk;
        const unsigned rest = fdiv(tile, p.fd_tx);
        Item t;
        t.tx = (int)(tile - rest * (unsigned)p.tilesX);
        t.b = (int)fdiv(rest, p.fd_ty);
        t.ty = (int)(rest - (unsigned)t.b * (unsigned)p.tilesY);
        t.n0 = (int)nbk * C::NB;
        return t;
    };
    auto decode_n0 = [&](int i) {
#ifdef CMU_V5_MOCK_WINO
        const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(item0 + i * nloc) % (unsigned)(p.total_blocks / 4);
#else
        const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(item0 + i * nloc);
#endif
        return (int)(w - fdiv(w, p.fd_nblk) * (unsigned)p.nblk) * C::NB;
    };

    const int64_t img_bytes = (int64_t)p.H * p.W * p.ldx * C::ES;
    const unsigned x_bytes = (unsigned)((((int64_t)p.H * p.W - 1) * p.ldx + p.K) * C::ES);
    const unsigned w_bytes = (unsigned)((int64_t)p.nslices32 * 9 * p.npad * 32);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)w_bytes, 0x00020000);

    // ---- halo staging roles: chunk idx = it * 512 + tid -> pixel idx >> 2, 16-byte chunk idx & 3 of the 64-byte slice ----------
    const int kcs = tid & 3;
    unsigned a_voff[C::A_ITERS];
    unsigned a_inb = 0;
    const unsigned char* ximg = reinterpret_cast<const unsigned char*>(p.x);
    auto set_load_tile = [&](int i) {
        const Item t = decode(i);
        const int ty0 = t.ty * C::TH, tx0 = t.tx * C::TW;
        a_inb = 0;
        int tl = tid;
        asm volatile("" : "+v"(tl));   // (rebuilt from an opaque copy: no loop-invariant index registers parked across the MFMA phase)
        const int kcl = tl & 3;
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) {
            const int pix = it * 128 + (tl >> 2);
            const int py = pix / C::LW, px = pix % C::LW;
            const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
            const bool ok = pix < C::NPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
            a_voff[it] = ok ? (((unsigned)gy * (unsigned)p.W + (unsigned)gx) * (unsigned)p.ldx + (unsigned)(kcl * EPC)) * (unsigned)C::ES : C::OOB;
            a_inb |= (ok ? 1u : 0u) << it;
        }
        ximg = reinterpret_cast<const unsigned char*>(p.x) + (int64_t)t.b * img_bytes;
    };
    const bool a_last_live = ((C::A_ITERS - 1) * 128 + (tid >> 2)) < C::NPIX;
    const unsigned a_st = (unsigned)((kcs >> 1) * C::PSTRIDE + (tid >> 2) * 32 + (kcs & 1) * 16);

    u32x4 areg[C::A_ITERS];
    float* tab = reinterpret_cast<float*>(smem + C::MAIN_BYTES);
    if (TF)
        for (int c = tid; c < p.K; c += 512) {
            tab[c] = p.in_scale[c];
            tab[C::MAX_K + c] = p.in_shift[c];
        }

    int pos_ld = 0, i_ld = 0, s_ld = 0;
    auto issue_loads = [&]() {
        const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(ximg), 0, (int)x_bytes, 0x00020000);
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) areg[it] = ig3_bload(rs_x, a_voff[it], (unsigned)(s_ld * 64));
    };
    // the stream's form: inline asm like the weight fragments (conv_igemm5's vmcnt discipline, below) -- with compiler-tracked halo loads
    // hipcc put vmcnt(0) in front of every staging part (it cannot see the weight loads in flight behind them): a round trip of the
    // next position's first weights per position
    auto issue_loads_stream = [&]() {
        typedef __attribute__((ext_vector_type(4))) int i32x4_t;
        const uint64_t xa = reinterpret_cast<uint64_t>(ximg);
        const i32x4_t xd = {__builtin_amdgcn_readfirstlane((int)(uint32_t)xa), __builtin_amdgcn_readfirstlane((int)((xa >> 32) & 0xffffu)),
                            __builtin_amdgcn_readfirstlane((int)x_bytes), 0x00020000};
        const unsigned so = (unsigned)__builtin_amdgcn_readfirstlane(s_ld * 64);
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it)
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=&v"(areg[it]) : "v"(a_voff[it]), "s"(xd), "s"(so) : "memory");
    };
    auto advance = [&]() {
        if (pos_ld + 1 < G) {
            ++pos_ld;
            if (++s_ld == nsl) {
                s_ld = 0;
                set_load_tile(++i_ld);
            }
        }
    };
    int s_regs = 0;
    unsigned inb_regs = 0;
    auto store_regs = [&]() {
        const unsigned buf = (unsigned)(s_regs & 1) * C::A_BYTES;   // nsl is even: stream parity == slice parity
        float sc[EPC], sh[EPC];
        float lo = 0.f;
        if (TF) {
            const int c0 = s_regs * C::KC + kcs * EPC;
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
                if (!((inb_regs >> it) & 1u)) v = u32x4{0u, 0u, 0u, 0u};
            }
            if (it < C::A_ITERS - 1 || a_last_live) *reinterpret_cast<u32x4*>(smem + buf + a_st + it * (128 * 32)) = v;
        }
    };
    auto stage_phase = [&]() {
        store_regs();
        advance();
        issue_loads_stream();
        s_regs = s_ld;
        inb_regs = a_inb;
    };

    f32x4 acc[8][4];   // [pixel row i of the wave's 8][channel block j]: pixel pi(lane & 15), channels 32 (j >> 1) + 8 (lane >> 4) + 4 (j & 1) + e
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    zero_acc();

    // ---- fragment addresses ---------------------------------------------------------------------------------------------
    const int n16 = lane & 15, kq = lane >> 4;
    const int pi = n16 < 4 ? n16 : (n16 < 12 ? n16 + 4 : n16 - 8);
    const unsigned p_frag = (unsigned)((kq >> 1) * C::PSTRIDE + ((8 * wrow) * C::LW + 16 * wcol + pi) * 32 + (kq & 1) * 16);
    const unsigned w_voff = (unsigned)((((kq >> 1) * 9 * p.npad) + 2 * (n16 & ~3) + (n16 & 3)) * 32 + (kq & 1) * 16);
    const unsigned w_tap = (unsigned)p.npad * 32u;          // one tap of one 32-byte slice
    const unsigned w_s64 = w_tap * 18u;                     // one 64-byte slice = two 32-byte slices x nine taps
    constexpr unsigned JOFF[4] = {0u, 128u, 1024u, 1152u};  // channel blocks: rows 0-3 / 4-7 (+ 8 per lane group), rows 32-35 / 36-39

    // Weight fragments and halo chunks: inline-asm buffer loads + hand-placed s_waitcnt.  With compiler-tracked loads the waitcnt pass made the
    // first MFMAs of EVERY position wait for the halo chunks issued behind the weights (vmcnt(3..0) where 8 younger loads were in flight) and
    // drained everything in front of every staging part.  vmcnt retires in issue order, so what a wait costs is decided by what was issued
    // BEFORE the awaited load.  A wave's order per position:
    //     tap t (t = 0..8): issue W(t + 1) [tap 8: the next position's tap 0] | wait for W(t) | 32 MFMAs
    //     staging part:     wait for the halo chunks in the registers (behind them only the weight set in flight: vmcnt(4)) | registers ->
    //                       LDS | slab stores | halo chunks of a later position | epilogue (stores; data-gradient form: loads + stores)
    // so the first tap of a position never waits for the halo chunks or the epilogue's stores, the second one does (they were issued a
    // staging part + a tap earlier).  (A distance of TWO taps -- three live weight sets, 16 registers more -- measured the same on every
    // layer, same box: dropped; the registers are what the data-gradient epilogue needs.)
    // hipcc's own waits for the loads it knows (prologue, data-gradient epilogue) count fewer operations in flight than there are: too strict,
    // never too loose.
    typedef __attribute__((ext_vector_type(4))) int i32x4;
    const uint64_t w_addr = reinterpret_cast<uint64_t>(p.w);
    const i32x4 w_desc = {__builtin_amdgcn_readfirstlane((int)(uint32_t)w_addr), __builtin_amdgcn_readfirstlane((int)((w_addr >> 32) & 0xffffu)),
                          __builtin_amdgcn_readfirstlane((int)w_bytes), 0x00020000};
    u32x4 w0[4];   // weight fragments of the next position's first tap (carried across the staging part)
    auto load_w = [&](u32x4 (&w)[4], unsigned soff) {
        const unsigned so = (unsigned)__builtin_amdgcn_readfirstlane((int)soff);
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=&v"(w[0]) : "v"(w_voff), "s"(w_desc), "s"(so) : "memory");
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:128" : "=&v"(w[1]) : "v"(w_voff), "s"(w_desc), "s"(so) : "memory");
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:1024" : "=&v"(w[2]) : "v"(w_voff), "s"(w_desc), "s"(so) : "memory");
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:1152" : "=&v"(w[3]) : "v"(w_voff), "s"(w_desc), "s"(so) : "memory");
    };
#define IG5_WAIT_VM(n_) do { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(n_) : "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

    // one position: nine taps x (4 weight fragments from L1, 8 pixel fragments from LDS, 32 MFMAs); the weight fragments run one
    // tap ahead (three register sets in rotation: 9 % 3 == 0, so the set that leaves the step is the set that enters the next).
    // `last` (forward / plain forms): the item's last tap runs ROW BY ROW and retires row r - 1 (statistics terms, conversion, two
    // 16-byte stores) beside the four MFMAs of row r.  Measured before this (timing-only builds, 128 -> 128 @ 256 x 256): the epilogue
    // behind the last MFMA cost 18 % of the kernel (stores 12 %, statistics 5 %) -- with one barrier per position the first half's
    // epilogue runs while the second half waits at the barrier, i.e. beside NO MFMA; inside the MFMA phase the partner's MFMAs fill
    // the matrix pipe while this wave converts and stores.
#ifdef CMU_IG_STAMPS
    // diagnostic build: waves 0 and 4 of a few workgroups stamp s_memtime through LDS around the phases of 16 positions from the
    // second item boundary on (tools/v5_stamps.py)
    const int stamp_slot = (blockIdx.x % 61 == 0 && blockIdx.x / 61 < 4) ? (int)(blockIdx.x / 61) : -1;
    unsigned long long* stamp_lds = reinterpret_cast<unsigned long long*>(smem + C::STAMP_OFF);
    const int stamp_g0 = 2 * nsl - 3;
    int stamp_g = 0;
#define IG5_STAMP(k_)                                                                                                     \
    do {                                                                                                                   \
        if (stamp_slot >= 0 && stamp_g >= stamp_g0 && stamp_g < stamp_g0 + C::STAMP_ITERS && (tid & 255) == 0)              \
            stamp_lds[((tid >> 8) * C::STAMP_ITERS + (stamp_g - stamp_g0)) * 8 + (k_)] = __builtin_amdgcn_s_memtime();      \
    } while (0)
#else
#define IG5_STAMP(k_) do {} while (0)
#endif
#ifdef CMU_V5_MOCK_WINO
    // TIMING MOCK of a Winograd F(2x2, 3x3) tile (review item 4 of round 5; wrong results by construction, diagnostic builds only -- tools/
    // build_variant.sh ... -DCMU_V5_MOCK_WINO, profiles/r06_winograd.txt): a "position" is ONE 64-byte channel slice of the 16 transformed-input
    // planes -- 32 MFMAs per wave (two of the sixteen element-wise GEMMs x 4 x 4 blocks of 16 tiles x 16 channels) on 8 pixel-side fragments from
    // LDS and 8 weight-side fragments from L1 -- behind a staging part of its own (a direct conv stages once per nine taps); an item is a quarter
    // of this kernel's (64 tiles = 16 x 16 output pixels x 64 channels: sixteen accumulator planes fill the registers), so the launcher walks every
    // item four times and the epilogue stores a quarter of its rows behind a round trip of all accumulators through LDS (the output transform
    // needs the sixteen planes of a tile, which live in eight waves).
    constexpr int NHS = 2;
#else
    constexpr int NHS = 18;
#endif
    auto mfma_step = [&](unsigned buf, unsigned soff_cur, unsigned soff_next, int epi_ops, bool dma) {
        u32x4 w1[4], w2[4];
        u32x4 pf[2][4];
        auto rd = [&](int hs, int set) {   // half step hs = 2 * tap + half: pixel rows 4 * half .. + 4 of the wave's 8
            const int t = hs >> 1, hf = hs & 1;
            const unsigned ao = (unsigned)((((t / 3) + 4 * hf) * C::LW + (t % 3)) * 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) pf[set][i] = *reinterpret_cast<const u32x4*>(smem + buf + p_frag + ao + i * (C::LW * 32));
        };
        rd(0, 0);
        // one scheduling region per half step: [next tap's weights | next half step's pixel fragments | 16 MFMAs]; the memory clobber
        // keeps the compiler from merging the LDS reads of overlapping halo rows across taps (it would hold them in registers for three
        // taps: spills); inside the region the LDS reads are issued one per MFMA from the region's start (left to itself the scheduler
        // issues them behind 8-12 of the 16 MFMAs)
        auto half_step = [&](auto hs_c) {
            constexpr int hs = decltype(hs_c)::value, t = hs >> 1, hf = hs & 1;
            u32x4(&wc)[4] = (t % 3 == 0) ? w0 : (t % 3 == 1 ? w1 : w2);
            u32x4(&wnx)[4] = (t % 3 == 0) ? w1 : (t % 3 == 1 ? w2 : w0);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#ifndef CMU_IG_STAMPS_EPI
            if constexpr (hs == 2) IG5_STAMP(1);
            if constexpr (hs == 4) IG5_STAMP(2);
#endif
            if constexpr (hf == 0) {
#ifdef CMU_V5_MOCK_WINO
                load_w(w1, soff_next);                       // the next slice's eight weight-side fragments
                load_w(w2, soff_next + w_tap);
                if (epi_ops == 0) IG5_WAIT_VM(8 + C::A_ITERS);
                else IG5_WAIT_VM(8 + C::A_ITERS + 4);
#else
                load_w(wnx, t < 8 ? soff_cur + (unsigned)(t + 1) * w_tap : soff_next);
                if constexpr (t == 0) {
                    // behind this tap's weights: the halo chunks, the epilogue's operations if one ran (data-gradient form, last position of
                    // an item: the eight DMA loads issued in front of the phase), the four loads just issued
                    if (BST && dma) IG5_WAIT_VM(4 + C::A_ITERS + 8);
                    else if (epi_ops == 0) IG5_WAIT_VM(4 + C::A_ITERS);
                    else if (epi_ops == 16) IG5_WAIT_VM(4 + C::A_ITERS + 16);
                    else IG5_WAIT_VM(4 + C::A_ITERS + 24);
                } else {
                    IG5_WAIT_VM(4);
                }
#endif
            }
            if constexpr (hs + 1 < NHS) rd(hs + 1, (hs + 1) & 1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) TR::mma32(wc[j], pf[hs & 1][i], acc[4 * hf + i][j]);
            if constexpr (hs + 1 < NHS) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
            }
        };
        ig5_static_for<NHS>(half_step);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#ifdef CMU_V5_MOCK_WINO
        // the carried set of the next slice (in front of it only the just-issued eight loads: waited for at that slice's first MFMA)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) w0[j][q] = w1[j][q] ^ (w2[j][q] & 1u);
#endif
    };

    // ---- epilogue of one item: statistics (or BatchNorm-backward sums), conversion, 16-byte stores straight from the accumulators ---
    auto epilogue = [&](const Item t, int par) {
        int ln = tid & 63;
        asm volatile("" : "+v"(ln));
        const int n16 = ln & 15, g = ln >> 4;
        const int pi = n16 < 4 ? n16 : (n16 < 12 ? n16 + 4 : n16 - 8);
        float* stat_lds = reinterpret_cast<float*>(smem + C::STAT_OFF + par * C::STAT_PAR) + wave * 128;
        const int nw = t.n0 + wn * 64;
        const int64_t pix0 = ((int64_t)t.b * p.H + t.ty * C::TH + 8 * wrow) * p.W + t.tx * C::TW + 16 * wcol;
        unsigned char* ybase = reinterpret_cast<unsigned char*>(p.y) + (pix0 * p.ldy + nw) * (int64_t)C::ES;
        const unsigned yoff = (unsigned)((pi * (int)p.ldy + 8 * g) * C::ES);
        const int64_t yrow = (int64_t)p.W * p.ldy * C::ES;
        // full-line stores (ig5_store_row_lines): lanes n16 and n16 ^ 8 form a pair; pixel of the pair's lower / upper lane
        const bool lo = n16 < 8;
        const int nA = n16 & 7, nB = nA + 8;
        const int piA = nA < 4 ? nA : nA + 4, piB = nB < 12 ? nB + 4 : nB - 8;
        const unsigned offA = (unsigned)((piA * (int)p.ldy + 8 * g) * C::ES) + (lo ? 0u : 64u);
        const unsigned offB = (unsigned)((piB * (int)p.ldy + 8 * g) * C::ES) + (lo ? 0u : 64u);
        if (!BST) {
#ifdef CMU_V5_MOCK_WINO
            constexpr int EROWS = 2;      // a quarter of the rows leave the item (see the mock's note at mfma_step)
            {
                // sixteen accumulator planes of a tile live in eight waves: all 128 registers through LDS and back (a 64 KiB window of the halo
                // buffers, written and read by this thread alone: a mock), then the output transform's adds (24 per 16 values)
                unsigned char* win = smem + (tid & 511) * 16;
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(win + ((i * 4 + j) & 7) * 8192) = acc[i][j];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 r = *reinterpret_cast<const f32x4*>(win + ((i * 4 + j + 3) & 7) * 8192);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][j][e] = (acc[i][j][e] + r[e]) - acc[(i + 1) & 7][j][e] * 0.5f;
                    }
            }
#else
            constexpr int EROWS = 8;
#endif
            if (p.stats != nullptr) {
                // channel (j, e) of this lane group: sums over the 8 rows in the registers (32 independent chains), then over the row's 16
                // pixels (batched DPP steps), then one predicated block of eight 16-byte LDS writes
                float sv[32];    // [2 * (4 j + e) + {0: sum, 1: sum of squares}]
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float s1 = 0.f, s2 = 0.f;
#pragma unroll
                        for (int i = 0; i < EROWS; ++i) {
                            const float v = acc[i][j][e];
                            s1 += v;
                            s2 = fmaf(v, v, s2);
                        }
                        sv[2 * (4 * j + e)] = s1;
                        sv[2 * (4 * j + e) + 1] = s2;
                    }
                ig5_row16_sum_batch(sv);
                if (n16 == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // channels 32 (j >> 1) + 8 g + 4 (j & 1) + e, e = 0..3: eight consecutive floats (sum, sum of squares interleaved)
                        float* d = stat_lds + (32 * (j >> 1) + 8 * g + 4 * (j & 1)) * 2;
                        *reinterpret_cast<f32x4*>(d) = f32x4{sv[8 * j], sv[8 * j + 1], sv[8 * j + 2], sv[8 * j + 3]};
                        *reinterpret_cast<f32x4*>(d + 4) = f32x4{sv[8 * j + 4], sv[8 * j + 5], sv[8 * j + 6], sv[8 * j + 7]};
                    }
                }
            }
#ifdef CMU_IG_STAMPS_EPI
            IG5_STAMP(1);
#endif
#pragma unroll
            for (int i = 0; i < EROWS; ++i) {
                u32x4 v[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    v[s][0] = TR::pack2(acc[i][2 * s][0], acc[i][2 * s][1]);
                    v[s][1] = TR::pack2(acc[i][2 * s][2], acc[i][2 * s][3]);
                    v[s][2] = TR::pack2(acc[i][2 * s + 1][0], acc[i][2 * s + 1][1]);
                    v[s][3] = TR::pack2(acc[i][2 * s + 1][2], acc[i][2 * s + 1][3]);
                }
                ig5_store_row_lines(ybase + i * yrow, offA, offB, lo, v[0], v[1]);
            }
#ifdef CMU_IG_STAMPS_EPI
            IG5_STAMP(2);
#endif
        } else {
            const unsigned char* xbase = reinterpret_cast<const unsigned char*>(p.bx) + (pix0 * p.ldbx + nw) * (int64_t)C::ES;
            const unsigned xoff = (unsigned)((pi * (int)p.ldbx + 8 * g) * C::ES);
            const int64_t xrow = (int64_t)p.W * p.ldbx * C::ES;
            float bsc[2][EPC], bsh[2][EPC], bs1[2][EPC], bs2[2][EPC];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                ig3_bst_consts<EPC>(p.b_scale, p.b_shift, nw + 32 * s + 8 * g, bsc[s], bsh[s]);
#pragma unroll
                for (int e = 0; e < EPC; ++e) bs1[s][e] = bs2[s][e] = 0.f;
            }
            // The producer layer's raw output.  Rows 0-3 were fetched by LDS-DMA during the item's last MFMA phase (issue_bx_dma: no registers,
            // an HBM round trip that ended long ago); rows 4-7 by loads that go out now and one row ahead afterwards -- their round trips run
            // under the work on rows 0-3.  (Before: every row's loads went out one row ahead of their use: eight exposed round trips per
            // item, ~12K cycles of a ~15K-cycle epilogue.)
#ifdef CMU_IG_STAMPS_EPI
            IG5_STAMP(1);
#endif
            const unsigned char* bxl = smem + C::BX_OFF + wave * C::BX_WAVE + (ln & 63) * 16;
            u32x4 xr[2][2];
#pragma unroll
            for (int s = 0; s < 2; ++s) xr[0][s] = ld_global16(xbase + 4 * xrow + s * 64 + xoff);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < 4) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) xr[1][s] = *reinterpret_cast<const u32x4*>(bxl + (i * 2 + s) * 1024);
                } else if (i + 1 < 8) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) xr[(i + 1) & 1][s] = ld_global16(xbase + (i + 1) * xrow + s * 64 + xoff);
                }
                u32x4 v[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    v[s][0] = TR::pack2(acc[i][2 * s][0], acc[i][2 * s][1]);
                    v[s][1] = TR::pack2(acc[i][2 * s][2], acc[i][2 * s][3]);
                    v[s][2] = TR::pack2(acc[i][2 * s + 1][0], acc[i][2 * s + 1][1]);
                    v[s][3] = TR::pack2(acc[i][2 * s + 1][2], acc[i][2 * s + 1][3]);
                    ig3_bst_accum<TR>(v[s], xr[i < 4 ? 1 : (i & 1)][s], bsc[s], bsh[s], bs1[s], bs2[s]);
                }
                ig5_store_row_lines(ybase + i * yrow, offA, offB, lo, v[0], v[1]);
            }
#ifdef CMU_IG_STAMPS_EPI
            IG5_STAMP(2);
#endif
            // folds over the row's 16 pixels in one batch; the partials go to LDS as they are -- (sum dz, sum dz x): the slab writer turns the
            // second into sum dz xhat with the channel's mean / invstd (linear in the partials).  Round 5's first form loaded mean / invstd
            // from global memory inside sixteen predicated blocks: sixteen serial round trips, 9K cycles by the stamps.
            float sv[32];      // [2 * (8 s + e) + {0, 1}]
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    sv[2 * (8 * s + e)] = bs1[s][e];
                    sv[2 * (8 * s + e) + 1] = bs2[s][e];
                }
            ig5_row16_sum_batch(sv);
            if (n16 == 0) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float* d = stat_lds + (32 * s + 8 * g) * 2;        // channels 32 s + 8 g + e, e = 0..7
#pragma unroll
                    for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(d + 4 * q) = f32x4{sv[16 * s + 4 * q], sv[16 * s + 4 * q + 1], sv[16 * s + 4 * q + 2], sv[16 * s + 4 * q + 3]};
                }
            }
        }
    };
    // per-wave channel partials -> one slab row per 16 x 16 half of the tile (the slab keeps the first kernel's shape)
    auto write_slab = [&](const Item t, int par) {
        float* dst = BST ? p.bstats : p.stats;
        int tl = threadIdx.x;
        asm volatile("" : "+v"(tl));
        if (dst != nullptr && tl < 2 * C::NB) {
            const float* stat_lds = reinterpret_cast<const float*>(smem + C::STAT_OFF + par * C::STAT_PAR);
            const int half = tl / C::NB, c = tl % C::NB;
            const int tx16 = 2 * t.tx + half, tiles16 = p.W / 16;
            float a = 0.f, q2 = 0.f;
#pragma unroll
            for (int wr = 0; wr < 2; ++wr) {
                const int wv = (c / 64) * 4 + wr * 2 + half;
                a += stat_lds[(wv * 64 + (c & 63)) * 2 + 0];
                q2 += stat_lds[(wv * 64 + (c & 63)) * 2 + 1];
            }
            if (BST) q2 = (q2 - p.b_mean[t.n0 + c] * a) * p.b_invstd[t.n0 + c];     // sum dz x -> sum dz (x - mean) invstd over the 16 x 16 block
            const int64_t t16 = ((int64_t)t.b * p.tilesY + t.ty) * tiles16 + tx16;
            dst[(t16 * 2 + 0) * p.N + t.n0 + c] = a;
            dst[(t16 * 2 + 1) * p.N + t.n0 + c] = q2;
        }
    };

    // ---- prologue: position 0 staged, position 1 in the registers, the first tap's weights on their way ----------------------
    set_load_tile(0);
    int n0_mma = decode_n0(0);
    issue_loads();
    {
        u32x4 a0[C::A_ITERS];
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) a0[it] = areg[it];
        advance();          // nsl >= 2: still item 0
        issue_loads();
        __syncthreads();    // the transform table is complete
        u32x4 a1[C::A_ITERS];
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) { a1[it] = areg[it]; areg[it] = a0[it]; }
        s_regs = 0;
        inb_regs = a_inb;
        store_regs();
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) areg[it] = a1[it];
        s_regs = s_ld;
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);   // no prologue load may stay pending into the loop (conv_igemm3.inc header)
    __syncthreads();
    load_w(w0, (unsigned)(n0_mma + wn * 64) * 32u);

    // (every wave enters the loop with [first tap's weights | a position's halo chunks] in flight, in that order -- the order of a
    // loop iteration: hipcc's waitcnt pass merges the entry state with the back edge's, and a halo load OLDER than the weights on one
    // path makes the first MFMA of every position wait for all of them)
    const int second = wave >= 4 ? 1 : 0;   // waves 4-7 run one stage phase ahead (conv_igemm3p.inc: one barrier per position)
    if (second && 1 < G) stage_phase();
    else issue_loads_stream();               // position 1's chunks once more (the same bytes into the same registers)
    int s_mma = 0, i_mma = 0, epi_ops = 0;
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
        const unsigned soff_cur = (unsigned)s_mma * w_s64 + (unsigned)(n0_mma + wn * 64) * 32u;
        int n0_next = n0_mma;
        unsigned soff_next;
        if (s_mma + 1 < nsl) soff_next = soff_cur + w_s64;
        else {
            if (i_mma + 1 < n_my) n0_next = decode_n0(i_mma + 1);
            soff_next = (unsigned)(n0_next + wn * 64) * 32u;
        }
        const bool last = s_mma == nsl - 1;
#ifdef CMU_IG_STAMPS
        stamp_g = g;
#endif
        IG5_STAMP(0);
        // (data-gradient form, the item's last position) rows 0-3 of the producer layer's raw output -> LDS, straight from the buffer load
        auto issue_bx_dma = [&]() {
            if constexpr (BST) {
                const Item t = decode(i_mma);
                const int64_t pix0 = ((int64_t)t.b * p.H + t.ty * C::TH + 8 * wrow) * p.W + t.tx * C::TW + 16 * wcol;
                const uint64_t xa = reinterpret_cast<uint64_t>(p.bx) + (uint64_t)((pix0 * p.ldbx + t.n0 + wn * 64) * (int64_t)C::ES);
                typedef __attribute__((ext_vector_type(4))) int i32x4_t;
                const i32x4_t xd = {__builtin_amdgcn_readfirstlane((int)(uint32_t)xa), __builtin_amdgcn_readfirstlane((int)((xa >> 32) & 0xffffu)), -1, 0x00020000};
                int ln = tid & 63;
                asm volatile("" : "+v"(ln));
                const int n16l = ln & 15, gl = ln >> 4;
                const int pil = n16l < 4 ? n16l : (n16l < 12 ? n16l + 4 : n16l - 8);
                const unsigned xoffl = (unsigned)((pil * (int)p.ldbx + 8 * gl) * C::ES);
                const unsigned xrowl = (unsigned)((int64_t)p.W * p.ldbx * C::ES);
                const unsigned lds0 = (unsigned)(C::BX_OFF + wave * C::BX_WAVE);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const unsigned m0v = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + (i * 2 + s) * 1024));
                        const unsigned so = (unsigned)__builtin_amdgcn_readfirstlane((int)(i * xrowl + s * 64));
                        // (one wait state between an SALU write of M0 and the LDS-DMA instruction that reads it: hipcc inserts nothing inside an asm block)
                        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(m0v), "v"(xoffl), "s"(xd), "s"(so) : "memory", "m0");
                    }
            }
        };
        // (in front of the phase: behind the carried weight sets and the halo chunks in vmcnt order, so the first two taps do not wait for
        // it; the third does -- as it does for the halo chunks)
        if (BST && last) issue_bx_dma();
        __builtin_amdgcn_s_setprio(2);
        mfma_step((unsigned)(g & 1) * C::A_BYTES, soff_cur, soff_next, epi_ops, BST && last);
        __builtin_amdgcn_s_setprio(0);
        IG5_STAMP(3);
        if (second) __syncthreads();
        IG5_STAMP(4);
        const bool staging = g + second + 1 < G;
        IG5_WAIT_VM(4);              // the halo chunks in the registers: behind them only the next position's first weight set
        if (staging) store_regs();
        if (s_mma == 1 && i_mma > 0) write_slab(decode(i_mma - 1), (i_mma - 1) & 1);
        // the next halo chunks go out as early as the registers are free (in front of the epilogue): they are older than every weight
        // load of the next position but its first tap's, whose second tap therefore waits for them
        // (forward forms: in front of the epilogue, as early as the registers are free.  Data-gradient form: behind it -- its epilogue needs the 20
        // registers: with the chunks in flight across it the allocator SPILLED them right behind the asm loads, i.e. before the data had
        // arrived: scratch must stay at zero in these kernels, tests/test_cpu_abi.py checks the code object)
        if (staging) advance();
        if (!BST) issue_loads_stream();
        IG5_STAMP(5);
        epi_ops = 0;
        if (last) {
            epilogue(decode(i_mma), i_mma & 1);
            zero_acc();
#ifdef CMU_V5_MOCK_WINO
            epi_ops = 4;
#else
            epi_ops = BST ? 24 : 16;     // operations issued behind the carried weight sets: 16 stores (+ 8 loads of rows 4-7)
#endif
        }
        if (BST) issue_loads_stream();
        s_regs = s_ld;
        inb_regs = a_inb;
        IG5_STAMP(6);
        if (++s_mma == nsl) {
            s_mma = 0;
            ++i_mma;
            n0_mma = n0_next;
        }
        // (timing mock, profiles/r05_conv_v5.txt section 5: both halves skipping this barrier at an item's last position -- the bound of a flag-based
        // hand-over that lets the partner run on during an epilogue -- changes nothing: each half's own instruction stream is the limit, not the waiting)
        if (!second) __syncthreads();
        IG5_STAMP(7);
    }
    __syncthreads();
#ifdef CMU_IG_STAMPS
    if (stamp_slot >= 0 && tid < 2 * C::STAMP_ITERS * 8) g_ig_stamps[stamp_slot * 256 + tid] = stamp_lds[tid];
#endif
    write_slab(decode(n_my - 1), (n_my - 1) & 1);
#ifdef CMU_IG_TAILS
    // diagnostic build (tools/v5_tails.py): when does each workgroup of the persistent launch END (constant-rate clock)?  The static item
    // lists give every workgroup the same number of items -- how long do the first finishers idle before the launch is over?
    if (tid == 0) {
        g_ig_stamps[1024 + blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        g_ig_stamps[2048 + blockIdx.x] = (unsigned long long)n_my;
    }
#endif
}

template <class TR, bool TF, bool BST>
static int launch_igemm5_cfg(IGParams p, hipStream_t st) {
    typedef IG5Cfg C;
    static_assert(C::LDS_BYTES <= 163840 && C::LDS_BYTES_BST <= 163840, "LDS budget");
    constexpr const char* name = "cmu_conv3x3_fwd(16x16x32, persistent)";
    p.tilesX = p.W / C::TW;
    p.tilesY = p.H / C::TH;
    p.nblk = p.N / C::NB;
    p.nslices = p.K / C::KC;
    p.nslices32 = p.K / 16;
    p.npad = cmu_conv3x3_npad(p.N);
    p.total_blocks = (int64_t)p.B * p.tilesX * p.tilesY * p.nblk;
#ifdef CMU_V5_MOCK_WINO
    p.total_blocks *= 4;         // (the kernel's decode wraps: every item four times -- a Winograd item is a quarter of this kernel's)
#endif
    cmu_fastdiv_init((unsigned)p.nblk, p.fd_nblk);
    cmu_fastdiv_init((unsigned)p.tilesX, p.fd_tx);
    cmu_fastdiv_init((unsigned)p.tilesY, p.fd_ty);
    const int forced = cmu_knob(CMU_KNOB_CONV_PERSIST_GRID);
    const int64_t want = forced > 0 ? forced : cmu_num_cus();
    const int64_t grid = p.total_blocks < want ? p.total_blocks : want;
    if (int rc = cmu_launch_lds<&conv_igemm5_kernel<TR, TF, BST>>(dim3((unsigned)grid), dim3(512), BST ? C::LDS_BYTES_BST : C::LDS_BYTES, st, name, p)) return rc;
    cmu_set_kernel_tag("conv_igemm5_kernel");
    CMU_CHECK_LAUNCH(name);
    return CMU_OK;
}

// shapes the 16x16x32 kernel serves (see the header); everything else stays on conv_igemm3p / conv_igemm3 / the first kernel
template <class TR>
static bool igemm5_eligible(const IGParams& p) {
    if constexpr (sizeof(typename TR::elem_t) != 2) return false;
    if (!cmu_knob(CMU_KNOB_CONV_V5)) return false;
    if (p.tile_list != nullptr) return false;
    if (p.in_scale != nullptr && p.bstats != nullptr) return false;
    if (p.N % 128 != 0 || p.K % 64 != 0) return false;
    // measured against conv_igemm3p (tools/v5_check.py, f16, bs 32, same box): K = 64 (two positions per item) loses 5 %; the data-gradient
    // form with its BatchNorm-backward epilogue loses 4-5 % at K = 128 and gains from K = 256 up
    const int min_k = cmu_knob(CMU_KNOB_V5_MIN_K), min_k_bst = cmu_knob(CMU_KNOB_V5_MIN_K_BST);          // (A/B knobs)
    if (p.K < min_k || (p.bstats != nullptr && p.K < min_k_bst)) return false;
    if (p.H % 16 != 0 || p.W % 32 != 0) return false;
    if ((int64_t)p.B * (p.H / 16) * (p.W / 32) * (p.N / 128) >= (1ll << 30)) return false;
    return !igemm3_narrow_blocks(p);
}
template <class TR>
static int launch_igemm5(const IGParams& p, hipStream_t st) {
    if constexpr (sizeof(typename TR::elem_t) == 2) {
        const bool tf = p.in_scale != nullptr, bst = p.bstats != nullptr;
        return tf ? launch_igemm5_cfg<TR, true, false>(p, st) : (bst ? launch_igemm5_cfg<TR, false, true>(p, st) : launch_igemm5_cfg<TR, false, false>(p, st));
    } else {
        return CMU_ERR_ARG;
    }
}
