// conv_igemm6.inc -- the 64-channel-block form of the 16x16x32 3x3 implicit-GEMM kernel (round 6; included by conv_igemm.hip after
// conv_igemm5.inc, whose LDS halo layout, weight-fragment addressing, MFMA step and epilogue it keeps).
//
// Why.  What conv_igemm5 cannot serve well are the items with little MFMA work per epilogue: K = 64 (two positions per item) and the
// 64-output-channel layers at 512 x 512.  Its two halves (waves 0-3 / 4-7) alternate MFMA phase and staging in LOCKSTEP (one barrier per
// position), so a half's epilogue -- longer than an MFMA phase -- is the critical path of every second position at K = 64, and the round-4
// kernel those layers stayed on (conv_igemm3p<64>) is bound by its waves' staging / epilogue instruction streams (matrix pipe busy
// 0.38-0.57, 10-14 % LDS bank conflicts; profiles/r05_pmc_conv.txt).  Here
//   * a workgroup is FOUR waves (256 threads) that own one (16 x 32 pixel tile, 64 output channels) item at a time -- a wave = 8 rows x
//     16 columns x 64 channels, exactly a conv_igemm5 wave -- and TWO such workgroups live on a CU (2 x 81,664 B of LDS, 256 registers
//     per wave).  The two are independent: no barrier couples them, the hardware interleaves the MFMA phase of one with the staging /
//     epilogue of the other on every SIMD (one wave of each), whatever their relative phase -- the hand-made ping-pong of the 512-thread
//     kernels with none of its lockstep;
//   * the halo of a 64-byte channel slice goes HBM / L2 -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds: 1 KiB per wave instruction, ten
//     per wave and position), so a position's staging holds no data registers across the MFMA phase (conv_igemm5: 20) and, in the forms
//     without a pending transform, costs no vector instructions at all; out-of-image pixels are out-of-range buffer offsets: the DMA
//     writes zeros.  With a pending BatchNorm + ReLU (forward forms) each thread transforms IN PLACE the ten 16-byte chunks it asked
//     for (ds_read_b128 / fma + max in fp32 / ds_write_b128) behind the MFMA phase -- beside the other workgroup's phase;
//   * buffer loads retire in order, so the first weight wait behind a position's DMA also waits for the DMA (one HBM round trip per
//     position and wave): that is what the second workgroup is there to cover.
// Same LDS planes as conv_igemm5 (32-byte pixel rows, one plane per pair of 16-byte chunks: conflict-free ds_read_b128 fragments), same
// packed weights straight from L2 / L1 one tap ahead, same accumulation order per output: BIT-IDENTICAL to conv_igemm5 where both
// serve a shape (tests/test_gpu_conv_v6.py), rounding-level agreement with the 32x32x16 kernels.
// Served: 16-bit operands, N % 64 == 0, K in {64, 128} (the (scale, shift) table shares the 80 KiB with the halo), whole 16 x 32 tiles,
// dense launches; forward with pending transform + statistics, and plain.  The BatchNorm-backward data-gradient form stays where it was.
struct IG6Cfg {
    static constexpr int ES = 2, EPC = 8;
    static constexpr int KC = 32;
    static constexpr int NB = 64;
    static constexpr int TH = 16, TW = 32, LW = TW + 2, LH = TH + 2, NPIX = LW * LH;   // 612 halo pixels
    static constexpr int PLANE = NPIX * 32;             // 19,584
    static constexpr int PSTRIDE = PLANE + 64;
    static constexpr int A_BYTES = 2 * PSTRIDE;         // 39,296
    static constexpr int MAIN_BYTES = 2 * A_BYTES;      // 78,592
    static constexpr int MAX_K = 128;
    static constexpr int TAB_BYTES = 2 * MAX_K * 4;     // 1,024
    static constexpr int STAT_OFF = MAIN_BYTES + TAB_BYTES;
    static constexpr int STAT_BYTES = 4 * 64 * 2 * 4;   // per-wave channel partials of one item
#ifdef CMU_IG_STAMPS
    static constexpr int STAMP_OFF = STAT_OFF + STAT_BYTES;   // diagnostic build (tools/v6_stamps.py): 4 pairs x 8 stamps in the last 256 bytes
    static constexpr int LDS_BYTES = STAMP_OFF + 256;
#else
    static constexpr int LDS_BYTES = STAT_OFF + STAT_BYTES;   // 81,664 <= 81,920: two workgroups per CU
#endif
    static constexpr int DMA_ITERS = 10;                // 20 one-KiB instructions per plane, two waves per plane
    static constexpr unsigned OOB = 0x7fff0000u;
};

template <class TR, bool TF>
__global__ __launch_bounds__(256, 2) void conv_igemm6_kernel(const IGParams p) {
    typedef IG6Cfg C;
    static_assert(sizeof(typename TR::elem_t) == 2, "16-bit operands only");
    constexpr int EPC = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wcol = wave & 1, wrow = wave >> 1;     // the wave's 8 rows x 16 columns of the 16 x 32 pixel tile

    // ---- this workgroup's items (XCD-contiguous static lists, as conv_igemm3p / conv_igemm5) ---------------------------------
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
    const int nsl = p.nslices;   // 64-byte slices per item (1 ... MAX_K / 32)

    struct Item { int b, ty, tx, n0; };
    auto fdiv = [](unsigned n, const unsigned (&fd)[2]) { return (__umulhi(n, fd[0]) + n) >> fd[1]; };
    auto decode = [&](int i) {
        const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(item0 + i * nloc);
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
        const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(item0 + i * nloc);
        return (int)(w - fdiv(w, p.fd_nblk) * (unsigned)p.nblk) * C::NB;
    };

    const int64_t img_bytes = (int64_t)p.H * p.W * p.ldx * C::ES;
    const unsigned x_bytes = (unsigned)((((int64_t)p.H * p.W - 1) * p.ldx + p.K) * C::ES);
    const unsigned w_bytes = (unsigned)((int64_t)p.nslices32 * 9 * p.npad * 32);

    // ---- halo staging roles ------------------------------------------------------------------------------------------------
    // plane q = wave >> 1 (16-byte chunks 2 q, 2 q + 1 of the 64-byte slice); the wave's instruction jj covers the plane's bytes
    // [ii * 1024, + 1024), ii = 10 (wave & 1) + jj: lane L = pixel 32 ii + (L >> 1), chunk 2 q + (L & 1) -- lane-linear, as the DMA writes
    const int q_pl = wave >> 1;
    const int ii0 = (wave & 1) * C::DMA_ITERS;
    unsigned a_voff[C::DMA_ITERS];
    unsigned a_inb = 0;
    const unsigned char* ximg = reinterpret_cast<const unsigned char*>(p.x);
    auto set_load_tile = [&](int i) {
        const Item t = decode(i);
        const int ty0 = t.ty * C::TH, tx0 = t.tx * C::TW;
        a_inb = 0;
        int ll = lane;
        asm volatile("" : "+v"(ll));   // (rebuilt from an opaque copy: no loop-invariant index registers parked across the MFMA phase)
        const int chunk = 2 * q_pl + (ll & 1);
#pragma unroll
        for (int jj = 0; jj < C::DMA_ITERS; ++jj) {
            const int pix = (ii0 + jj) * 32 + (ll >> 1);
            const int py = pix / C::LW, px = pix % C::LW;
            const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
            const bool ok = pix < C::NPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
            a_voff[jj] = ok ? (((unsigned)gy * (unsigned)p.W + (unsigned)gx) * (unsigned)p.ldx + (unsigned)(chunk * EPC)) * (unsigned)C::ES : C::OOB;
            a_inb |= (ok ? 1u : 0u) << jj;
        }
        ximg = reinterpret_cast<const unsigned char*>(p.x) + (int64_t)t.b * img_bytes;
    };
    // the plane's last instruction (ii = 19) covers pixels 608 ... 639 of 612: lanes 8 ... 63 would write behind the plane
    const bool dma_tail_live = (wave & 1) == 0 || lane < 8;

    float* tab = reinterpret_cast<float*>(smem + C::MAIN_BYTES);
    if (TF)
        for (int c = tid; c < p.K; c += 256) {
            tab[c] = p.in_scale[c];
            tab[C::MAX_K + c] = p.in_shift[c];
        }

    typedef __attribute__((ext_vector_type(4))) int i32x4;
#ifdef CMU_V6_MOCK_REGLOAD
    u32x4 mock_dst = {0u, 0u, 0u, 0u};
#endif
    // one position's halo: ten LDS-DMA instructions per wave (vmcnt counts them like any load)
    auto issue_dma = [&](unsigned buf, int s_ld, int jlo = 0, int jhi = C::DMA_ITERS) {
        const uint64_t xa = reinterpret_cast<uint64_t>(ximg);
        const i32x4 xd = {__builtin_amdgcn_readfirstlane((int)(uint32_t)xa), __builtin_amdgcn_readfirstlane((int)((xa >> 32) & 0xffffu)),
                          __builtin_amdgcn_readfirstlane((int)x_bytes), 0x00020000};
        const unsigned so = (unsigned)__builtin_amdgcn_readfirstlane(s_ld * 64);
        const unsigned lds0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(buf + (unsigned)q_pl * C::PSTRIDE + (unsigned)ii0 * 1024u));
#pragma unroll
        for (int jj = 0; jj < C::DMA_ITERS; ++jj) {
            const unsigned m0v = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + jj * 1024));
            // (one wait state between the SALU write of M0 and the LDS-DMA instruction that reads it)
#ifdef CMU_V6_MOCK_REGLOAD     // (timing mock: the same addresses through the register path, data dropped -- is it the LDS-DMA path that issues slowly?)
            // (ONE destination held for the whole kernel: a register the allocator may reuse while a load is in flight would be overwritten late)
            if (jj >= jlo && jj < jhi && (jj < C::DMA_ITERS - 1 || dma_tail_live))
                asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(mock_dst) : "v"(a_voff[jj]), "s"(xd), "s"(so) : "memory");
            continue;
#endif
            if (jj >= jlo && jj < jhi && (jj < C::DMA_ITERS - 1 || dma_tail_live))
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(m0v), "v"(a_voff[jj]), "s"(xd), "s"(so) : "memory", "m0");
        }
    };
    // pending BatchNorm + ReLU of the producer layer, in place on the chunks this thread asked for (cursor = the position just loaded)
    auto transform = [&](unsigned buf, int s_ld) {
        int ll = lane;
        asm volatile("" : "+v"(ll));
        const int chunk = 2 * q_pl + (ll & 1);
        const int c0 = s_ld * C::KC + chunk * EPC;
        float sc[EPC], sh[EPC];
#pragma unroll
        for (int e = 0; e < EPC; e += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(tab + c0 + e);
            const f32x4 c = *reinterpret_cast<const f32x4*>(tab + C::MAX_K + c0 + e);
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) { sc[e + qq] = a[qq]; sh[e + qq] = c[qq]; }
        }
        const float lo = cmu_relu_on(c0, p.relu_from) ? 0.f : -__builtin_inff();
        unsigned char* base = smem + buf + q_pl * C::PSTRIDE + ii0 * 1024 + ll * 16;
#pragma unroll
        for (int jj = 0; jj < C::DMA_ITERS; ++jj) {
            if (jj < C::DMA_ITERS - 1 || dma_tail_live) {
                u32x4 v = *reinterpret_cast<const u32x4*>(base + jj * 1024);
                float f[EPC];
                TR::unpack(v, f);
#pragma unroll
                for (int e = 0; e < EPC; ++e) f[e] = fmaxf(fmaf(f[e], sc[e], sh[e]), lo);
                v = TR::pack(f);
                if (!((a_inb >> jj) & 1u)) v = u32x4{0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4*>(base + jj * 1024) = v;
            }
        }
    };

    f32x4 acc[8][4];   // [pixel row i of the wave's 8][channel block j]: conv_igemm5's accumulator layout
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    zero_acc();

    // ---- fragment addresses (conv_igemm5) ---------------------------------------------------------------------------------
    const int n16 = lane & 15, kq = lane >> 4;
    const int pi = n16 < 4 ? n16 : (n16 < 12 ? n16 + 4 : n16 - 8);
    const unsigned p_frag = (unsigned)((kq >> 1) * C::PSTRIDE + ((8 * wrow) * C::LW + 16 * wcol + pi) * 32 + (kq & 1) * 16);
    const unsigned w_voff = (unsigned)((((kq >> 1) * 9 * p.npad) + 2 * (n16 & ~3) + (n16 & 3)) * 32 + (kq & 1) * 16);
    const unsigned w_tap = (unsigned)p.npad * 32u;
    const unsigned w_s64 = w_tap * 18u;

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

    // one position: nine taps x (4 weight fragments from L1, 8 pixel fragments from LDS, 32 MFMAs), weights one tap ahead (conv_igemm5's
    // step).  vmcnt at the first tap: behind the carried weight set are the previous epilogue's 16 stores (if one ran; the DMA in front of
    // them has been waited for) and the four loads just issued; at every other tap only the four just issued.
    auto mfma_step = [&](unsigned buf, unsigned soff_cur, unsigned soff_next, bool epi) {
        u32x4 w1[4], w2[4];
        u32x4 pf[2][4];
        auto rd = [&](int hs, int set) {
            const int t = hs >> 1, hf = hs & 1;
            const unsigned ao = (unsigned)((((t / 3) + 4 * hf) * C::LW + (t % 3)) * 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) pf[set][i] = *reinterpret_cast<const u32x4*>(smem + buf + p_frag + ao + i * (C::LW * 32));
        };
        rd(0, 0);
        auto half_step = [&](auto hs_c) {
            constexpr int hs = decltype(hs_c)::value, t = hs >> 1, hf = hs & 1;
            u32x4(&wc)[4] = (t % 3 == 0) ? w0 : (t % 3 == 1 ? w1 : w2);
            u32x4(&wnx)[4] = (t % 3 == 0) ? w1 : (t % 3 == 1 ? w2 : w0);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (hf == 0) {
                load_w(wnx, t < 8 ? soff_cur + (unsigned)(t + 1) * w_tap : soff_next);
                if constexpr (t == 0) {
                    if (!epi) IG5_WAIT_VM(4);
                    else IG5_WAIT_VM(4 + 16);
                } else {
                    IG5_WAIT_VM(4);
                }
            }
            if constexpr (hs + 1 < 18) rd(hs + 1, (hs + 1) & 1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
#ifdef CMU_V6_MOCK_NO_MFMA
                for (int j = 0; j < 4; ++j) { if (i == 0 && hs < 2) TR::mma32(wc[j], pf[hs & 1][i], acc[4 * hf + i][j]); else asm volatile("" :: "v"(wc[j]), "v"(pf[hs & 1][i])); }
#else
                for (int j = 0; j < 4; ++j) TR::mma32(wc[j], pf[hs & 1][i], acc[4 * hf + i][j]);
#endif
#ifndef CMU_V6_MOCK_NO_MFMA
            if constexpr (hs + 1 < 18) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
            }
#endif
        };
        ig5_static_for<18>(half_step);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- epilogue of one item (conv_igemm5's forward form with one 64-channel half) ------------------------------------------
    // `dma_s0` >= 0: the next pair's halo (slices dma_s0, dma_s0 + 1 -> buffers 0, 1) goes out BETWEEN the epilogue's parts, a few instructions
    // at a time: a wave that issues twenty DMA instructions in one burst stands at the issue port for 8-11K cycles (the CU's queue of
    // outstanding vector-memory instructions is full: s_memtime stamps, profiles/r06_conv_v6.txt) with its whole epilogue still to do
    auto epilogue = [&](const Item t, int dma_s0) {
        int ln = tid & 63;
        asm volatile("" : "+v"(ln));
        const int n16 = ln & 15, g = ln >> 4;
        float* stat_lds = reinterpret_cast<float*>(smem + C::STAT_OFF) + wave * 128;
        const int64_t pix0 = ((int64_t)t.b * p.H + t.ty * C::TH + 8 * wrow) * p.W + t.tx * C::TW + 16 * wcol;
        unsigned char* ybase = reinterpret_cast<unsigned char*>(p.y) + (pix0 * p.ldy + t.n0) * (int64_t)C::ES;
        const int64_t yrow = (int64_t)p.W * p.ldy * C::ES;
        const bool lo = n16 < 8;
        const int nA = n16 & 7, nB = nA + 8;
        const int piA = nA < 4 ? nA : nA + 4, piB = nB < 12 ? nB + 4 : nB - 8;
        const unsigned offA = (unsigned)((piA * (int)p.ldy + 8 * g) * C::ES) + (lo ? 0u : 64u);
        const unsigned offB = (unsigned)((piB * (int)p.ldy + 8 * g) * C::ES) + (lo ? 0u : 64u);
        if (dma_s0 >= 0) issue_dma(0u, dma_s0, 0, 5);
        if (p.stats != nullptr) {
            float sv[32];    // [2 * (4 j + e) + {0: sum, 1: sum of squares}]
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
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
                    float* d = stat_lds + (32 * (j >> 1) + 8 * g + 4 * (j & 1)) * 2;
                    *reinterpret_cast<f32x4*>(d) = f32x4{sv[8 * j], sv[8 * j + 1], sv[8 * j + 2], sv[8 * j + 3]};
                    *reinterpret_cast<f32x4*>(d + 4) = f32x4{sv[8 * j + 4], sv[8 * j + 5], sv[8 * j + 6], sv[8 * j + 7]};
                }
            }
        }
        if (dma_s0 >= 0) issue_dma(0u, dma_s0, 5, 10);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // (two DMA instructions of the second buffer in front of rows 0 ... 4: behind the last of them only the stores of rows 4 ... 7)
            if (dma_s0 >= 0 && i < 5) issue_dma((unsigned)C::A_BYTES, dma_s0 + 1, 2 * i, 2 * i + 2);
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
    };
    // per-wave channel partials -> one slab row per 16 x 16 half of the tile (the first kernel's slab shape)
    auto write_slab = [&](const Item t) {
        int tl = threadIdx.x;
        asm volatile("" : "+v"(tl));
        if (p.stats != nullptr && tl < 2 * C::NB) {
            const float* stat_lds = reinterpret_cast<const float*>(smem + C::STAT_OFF);
            const int half = tl / C::NB, c = tl % C::NB;
            const int tx16 = 2 * t.tx + half, tiles16 = p.W / 16;
            float a = 0.f, q2 = 0.f;
#pragma unroll
            for (int wr = 0; wr < 2; ++wr) {
                const int wv = wr * 2 + half;
                a += stat_lds[(wv * 64 + c) * 2 + 0];
                q2 += stat_lds[(wv * 64 + c) * 2 + 1];
            }
            const int64_t t16 = ((int64_t)t.b * p.tilesY + t.ty) * tiles16 + tx16;
            p.stats[(t16 * 2 + 0) * p.N + t.n0 + c] = a;
            p.stats[(t16 * 2 + 1) * p.N + t.n0 + c] = q2;
        }
    };

    // ---- main loop over PAIRS of positions (slices 2 k, 2 k + 1 of an item: buffers 0 and 1) -------------------------------------
    // Buffer loads retire in order, so a DMA issued in front of an MFMA phase is forced by that phase's second weight wait: one HBM round
    // trip of stall per position (first form of this kernel, profiles/r06_conv_v6.txt: 64 -> 64 @ 512 x 512 0.71 ms, 0.47 ms with no DMA at
    // all).  So the halo of a whole pair goes out at ONE point -- behind the pair's second phase (both buffers are free then) and IN FRONT of
    // the item's epilogue, whose conversion / statistics / stores run while it flies -- and is waited for once, before the barrier that
    // opens the next pair.  K = 64: one burst per item, hidden by the epilogue; K = 128: the burst between an item's two pairs is exposed
    // (the CU's second workgroup covers it).  Inside a pair nothing separates the two phases: eighteen taps in one stream.
    const int npairs_item = nsl >> 1;
    const int NP = n_my * npairs_item;
    int i_ld = 0, sp_ld = 0;
    set_load_tile(0);
    int n0_mma = decode_n0(0);
    issue_dma(0u, 0);
    issue_dma((unsigned)C::A_BYTES, 1);
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): the DMA has landed
    __syncthreads();                      // ... and the transform table is complete
    if (TF) {
        transform(0u, 0);
        transform((unsigned)C::A_BYTES, 1);
    }
    __syncthreads();
    load_w(w0, (unsigned)n0_mma * 32u);

    int sp_mma = 0, i_mma = 0;
    bool epi_prev = false;
#ifdef CMU_IG_STAMPS
    // waves 0 of workgroups 0, 256 (most likely the same CU), 61, 317 stamp s_memtime through LDS around the parts of pairs 8 ... 11
    const int stamp_slot = blockIdx.x == 0 ? 0 : (blockIdx.x == 256 ? 1 : (blockIdx.x == 61 ? 2 : (blockIdx.x == 317 ? 3 : -1)));
    unsigned long long* stamp_lds = reinterpret_cast<unsigned long long*>(smem + C::STAMP_OFF);
    int stamp_p = -1;
#define IG6_STAMP(k_) do { if (stamp_slot >= 0 && stamp_p >= 0 && stamp_p < 4 && tid == 0) stamp_lds[stamp_p * 8 + (k_)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define IG6_STAMP(k_) do {} while (0)
#endif
#pragma unroll 1
    for (int P = 0; P < NP; ++P) {
#ifdef CMU_IG_STAMPS
        stamp_p = P - 8;
#endif
        IG6_STAMP(0);
        const unsigned soff_a = (unsigned)(2 * sp_mma) * w_s64 + (unsigned)n0_mma * 32u;
        const unsigned soff_b = soff_a + w_s64;
        const bool last = sp_mma == npairs_item - 1;
        int n0_next = n0_mma;
        unsigned soff_next = soff_b + w_s64;
        if (last) {
            if (i_mma + 1 < n_my) n0_next = decode_n0(i_mma + 1);
            soff_next = (unsigned)n0_next * 32u;
        }
        const bool more = P + 1 < NP;
        __builtin_amdgcn_s_setprio(2);
        mfma_step(0u, soff_a, soff_b, epi_prev);
        IG6_STAMP(1);
        mfma_step((unsigned)C::A_BYTES, soff_b, soff_next, false);
        __builtin_amdgcn_s_setprio(0);
        IG6_STAMP(2);
        __syncthreads();          // every wave has read both buffers
        IG6_STAMP(3);
        if (more) {
            if (++sp_ld == npairs_item) {
                sp_ld = 0;
                set_load_tile(++i_ld);
            }
#ifndef CMU_V6_MOCK_NO_DMA      // (timing mocks -- diagnostic builds through tools/build_variant.sh, wrong results by construction, never shipped)
            if (!last) {
                issue_dma(0u, 2 * sp_ld);
                issue_dma((unsigned)C::A_BYTES, 2 * sp_ld + 1);
            }
#endif
        }
        IG6_STAMP(4);
        epi_prev = false;
        if (last) {
#ifdef CMU_V6_MOCK_NO_EPI
            if (acc[0][0][0] == 123.456f) epilogue(decode(i_mma), -1);    // (keeps the accumulators live)
            if (more) {
                issue_dma(0u, 2 * sp_ld);
                issue_dma((unsigned)C::A_BYTES, 2 * sp_ld + 1);
            }
            zero_acc();
#else
#ifdef CMU_V6_MOCK_NO_DMA
            epilogue(decode(i_mma), -1);
#else
            epilogue(decode(i_mma), more ? 2 * sp_ld : -1);
#endif
            zero_acc();
            epi_prev = true;
#endif
        }
        IG6_STAMP(5);
        if (more) {
            // the pair's halo: behind its last instruction in vmcnt order only the stores of the epilogue's rows 4 ... 7
            if (epi_prev) IG5_WAIT_VM(8);
            else IG5_WAIT_VM(0);
#ifdef CMU_V6_MOCK_REGLOAD
            asm volatile("" : "+v"(mock_dst));
#endif
            IG6_STAMP(6);
            if (TF) {
                transform(0u, 2 * sp_ld);
                transform((unsigned)C::A_BYTES, 2 * sp_ld + 1);
            }
        }
        IG6_STAMP(7);
        __syncthreads();          // the next pair's halo (and this item's statistics partials) are in LDS
        if (last) write_slab(decode(i_mma));
        if (++sp_mma == npairs_item) {
            sp_mma = 0;
            ++i_mma;
            n0_mma = n0_next;
        }
    }
#ifdef CMU_V6_MOCK_REGLOAD
    __builtin_amdgcn_s_waitcnt(0x0f70);
    asm volatile("" : "+v"(mock_dst));
#endif
#ifdef CMU_IG_STAMPS
    __syncthreads();
    if (stamp_slot >= 0 && tid < 32) g_ig_stamps[stamp_slot * 32 + tid] = stamp_lds[tid];
#endif
}

template <class TR, bool TF>
static int launch_igemm6_cfg(IGParams p, hipStream_t st) {
    typedef IG6Cfg C;
    static_assert(C::LDS_BYTES <= 81920, "two workgroups per CU");
    constexpr const char* name = "cmu_conv3x3_fwd(16x16x32, 64-channel items)";
    p.tilesX = p.W / C::TW;
    p.tilesY = p.H / C::TH;
    p.nblk = p.N / C::NB;
    p.nslices = p.K / C::KC;
    p.nslices32 = p.K / 16;
    p.npad = cmu_conv3x3_npad(p.N);
    p.total_blocks = (int64_t)p.B * p.tilesX * p.tilesY * p.nblk;
    cmu_fastdiv_init((unsigned)p.nblk, p.fd_nblk);
    cmu_fastdiv_init((unsigned)p.tilesX, p.fd_tx);
    cmu_fastdiv_init((unsigned)p.tilesY, p.fd_ty);
    const int forced = cmu_knob(CMU_KNOB_CONV_PERSIST_GRID);
    const int64_t want = forced > 0 ? forced : 2 * cmu_num_cus();
    const int64_t grid = p.total_blocks < want ? p.total_blocks : want;
    if (int rc = cmu_launch_lds<&conv_igemm6_kernel<TR, TF>>(dim3((unsigned)grid), dim3(256), C::LDS_BYTES, st, name, p)) return rc;
    cmu_set_kernel_tag("conv_igemm6_kernel");
    CMU_CHECK_LAUNCH(name);
    return CMU_OK;
}

// shapes the 64-channel-item kernel CAN take (see the header).  It is OPT-IN: measured on the bench's layers (profiles/r06_conv_v6.txt, same
// box, alternating) it ends within -8 ... +2 % of the kernels those layers run on -- 64 -> 64 @ 512 x 512 0.667 against 0.653 ms, 128 -> 64 1.203
// against 1.215, 64 -> 128 1.293 against 1.195 -- although its MFMA / epilogue side alone runs them 21-28 % faster (timing mock without the
// halo traffic: 0.508 / 0.874 / 1.007 ms): what it cannot do with two halo buffers per workgroup is keep enough bytes in flight.  So the
// default dispatch leaves every shape where it was; CMU_CONV_V6=1 in the environment (or cmu_set_dispatch_override("CMU_CONV_V6", 1), which
// also lifts the launch-size gate: tests) routes the eligible shapes here.  CMU_V6_MAX_N / CMU_V6_MAX_N_K128: widest layers taken.
template <class TR>
static bool igemm6_eligible(const IGParams& p) {
    if constexpr (sizeof(typename TR::elem_t) != 2) return false;
    if (p.tile_list != nullptr || p.bstats != nullptr) return false;
    if (p.N % 64 != 0 || p.K % 64 != 0 || p.K > IG6Cfg::MAX_K) return false;      // whole pairs of 64-byte slices
    if (p.H % 16 != 0 || p.W % 32 != 0) return false;
    const int64_t items = (int64_t)p.B * (p.H / 16) * (p.W / 32) * (p.N / 64);
    if (items >= (1ll << 30)) return false;
    if (cmu_knob_forced(CMU_KNOB_CONV_V6)) return true;     // tests (cmu_set_dispatch_override(..., 1)): every shape the kernel can serve
    if (!cmu_knob(CMU_KNOB_CONV_V6)) return false;          // opt-in (see above): the knob's default is off
    if (p.N > cmu_knob(CMU_KNOB_V6_MAX_N) || (p.K > 64 && p.N > cmu_knob(CMU_KNOB_V6_MAX_N_K128))) return false;
    return items >= 4 * (int64_t)cmu_num_cus();     // small launches stay on the one-round forms
}
template <class TR>
static int launch_igemm6(const IGParams& p, hipStream_t st) {
    if constexpr (sizeof(typename TR::elem_t) == 2) {
        return p.in_scale != nullptr ? launch_igemm6_cfg<TR, true>(p, st) : launch_igemm6_cfg<TR, false>(p, st);
    } else {
        return CMU_ERR_ARG;
    }
}
