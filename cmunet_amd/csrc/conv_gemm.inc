// conv_gemm.inc -- ConvTranspose2d 2x2 s2 forward and data gradient as plain GEMMs (included by conv_igemm.hip).
//
// Both are 1x1 convolutions on the LOW-RES pixel grid: forward M = pixels, N = 4*Cout (n = ij*Cout + co, scattered to
// pixel (2y+i, 2x+j) by the store), K = Cin; data gradient M = pixels, N = Cin, K = 4*Cout gathered from the four
// sub-pixel positions of dOut.  The first kernel runs them as a 64-channel-block form with 16 MFMAs per wave between two
// barriers and re-reads the activation tile once per 64 output channels (0.30 / 0.38 PFLOP/s).  Without tap reuse a GEMM
// stages ~3x the bytes per MFMA of the 3x3 kernels, so the tile is chosen for staging per MFMA: 256 pixels (16 x 16) x 256
// channels, 128 BYTES of K per step (two 64-byte slices of the pack), 8 waves as 2 (M) x 4 (N) with the wide conv
// kernel's wave tile (128 px x 64 ch, 4x2 MFMA 32x32) -- 32 MFMAs per wave and phase against 4 + 4 staged chunks per
// thread; LDS rows 144 B (128 + 16: conflict-free 16-byte fragment reads), A and B double-buffered (147 KB), the pending
// BatchNorm transform table of the input in LDS behind them.  Same machinery as conv_igemm3.inc otherwise: raw buffer loads
// with loop-invariant per-thread offsets (the sub-pixel position of the data gradient is a scalar offset), two-phase
// ping-pong (waves 4-7 one stage phase ahead), fragment double buffer pinned with sched_group_barrier, s_setprio, and the
// shared epilogue (bias + pixel-shuffle store for the forward, BatchNorm-backward partial sums for the data gradient).
// Used when N % 256 == 0 and K is a whole number of 128-byte steps (K of more than four steps: the shallow layers take the
// two-workgroup form at the end of this file); odd shapes stay on the first kernel.

template <class TR>
struct CGCfg {
    typedef IG3Cfg<TR, 256, 1> E;   // epilogue geometry: 16 x 16 pixel tile, waves 2 (row bands of 8 rows) x 4 (64-channel blocks)
    static constexpr int ES = (int)sizeof(typename TR::elem_t);
    static constexpr int EPC = TR::EPC;
    static constexpr int NB = 256;
    static constexpr int KSC = 128 / ES;            // channels per step
    static constexpr int PS = 144;
    static constexpr int A_BYTES = 256 * PS;        // 36,864
    static constexpr int B_BYTES = NB * PS;         // 36,864
    static constexpr int BUF_BYTES = A_BYTES + B_BYTES;
    static constexpr int MAIN_BYTES = 2 * BUF_BYTES;  // 147,456
    static constexpr int MAX_K = 1024;
    static constexpr int TAB_BYTES = 2 * MAX_K * 4;
    static constexpr int LDS_BYTES = MAIN_BYTES + TAB_BYTES > E::EPI_BYTES ? MAIN_BYTES + TAB_BYTES : E::EPI_BYTES;
    static constexpr int ITERS = 4;                 // 2,048 16-byte chunks per operand and step / 512 threads
    static constexpr unsigned OOB = 0x7fff0000u;
};

template <class TR, bool DG, bool TF>
__global__ __launch_bounds__(512) void conv_gemm_kernel(const IGParams p) {
    typedef CGCfg<TR> C;
    constexpr int EPC = TR::EPC;
    constexpr int SW = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;
    const int wrow = wave & 1, wn = wave >> 1;   // wave = 8 rows x 16 columns x 64 channels

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
    const int ty0 = ty * 16, tx0 = tx * 16;
    const int n0 = nbk * C::NB;

    // ---- buffer descriptors: one image of the activation operand (the full-resolution dOut for the data gradient) --------
    const int Hin = DG ? 2 * p.H : p.H, Win = DG ? 2 * p.W : p.W;
    const int64_t img_elems = (int64_t)Hin * Win * p.ldx;
    const unsigned char* ximg = reinterpret_cast<const unsigned char*>(p.x) + (int64_t)b * img_elems * C::ES;
    const unsigned x_bytes = (unsigned)((((int64_t)Hin * Win - 1) * p.ldx + p.K / (DG ? 4 : 1)) * C::ES);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(ximg), 0, (int)x_bytes, 0x00020000);
    const int nsteps = p.K / C::KSC;
    const unsigned w_bytes = (unsigned)((int64_t)2 * nsteps * p.npad * 64);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)w_bytes, 0x00020000);

    // ---- per-thread staging roles: 16-byte chunk c8 of a 128-byte K step ---------------------------------------------------
    const int c8 = tid & 7;
    unsigned a_voff[C::ITERS];
    unsigned a_inb = 0;
#pragma unroll
    for (int it = 0; it < C::ITERS; ++it) {
        const int pix = it * 64 + (tid >> 3);
        const int gy = ty0 + (pix >> 4), gx = tx0 + (pix & 15);
        const bool ok = gy < p.H && gx < p.W;
        const int64_t po = DG ? ((int64_t)2 * gy * Win + 2 * gx) : ((int64_t)gy * Win + gx);
        a_voff[it] = ok ? (unsigned)((po * p.ldx + c8 * EPC) * C::ES) : C::OOB;
        a_inb |= (ok ? 1u : 0u) << it;
    }
    const unsigned a_st = (unsigned)((tid >> 3) * C::PS + c8 * 16);   // + it * 64 * PS (+ buffer)
    // packed ConvTranspose weights: [64-byte slice][row][64 B]; chunk c8 of row n lives in slice 2*step + (c8 >> 2)
    unsigned b_voff[C::ITERS];
#pragma unroll
    for (int it = 0; it < C::ITERS; ++it) {
        const int row = it * 64 + (tid >> 3);
        b_voff[it] = (unsigned)(((int64_t)(c8 >> 2) * p.npad + n0 + row) * 64 + (c8 & 3) * 16);
    }
    const unsigned b_st = (unsigned)(C::A_BYTES + (tid >> 3) * C::PS + c8 * 16);
    const unsigned w_step = (unsigned)p.npad * 128u;   // two 64-byte slices

    float* tab = reinterpret_cast<float*>(smem + C::MAIN_BYTES);
    if (TF)
        for (int c = tid; c < p.K; c += 512) {
            tab[c] = p.in_scale[c];
            tab[C::MAX_K + c] = p.in_shift[c];
        }

    u32x4 areg[C::ITERS], breg[C::ITERS];
    const int cpi = DG ? (p.K / 4) / C::KSC : 1;   // data gradient: steps per sub-pixel position
    auto issue_loads = [&](int s) {
        unsigned soff;
        if (DG) {
            const int ij = s / cpi, cc = s - ij * cpi;
            soff = (unsigned)((((int64_t)(ij >> 1) * Win + (ij & 1)) * p.ldx + cc * C::KSC) * C::ES);
        } else {
            soff = (unsigned)(s * 128);
        }
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) areg[it] = ig3_bload(rs_x, a_voff[it], soff);
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) breg[it] = ig3_bload(rs_w, b_voff[it], (unsigned)s * w_step);
    };
    auto store_regs = [&](unsigned buf, int s) {
        float sc[EPC], sh[EPC];
        float lo = 0.f;
        if (TF) {
            const int c0 = s * C::KSC + c8 * EPC;
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
        for (int it = 0; it < C::ITERS; ++it) {
            u32x4 v = areg[it];
            if (TF) {
                float f[EPC];
                TR::unpack(v, f);
#pragma unroll
                for (int e = 0; e < EPC; ++e) f[e] = fmaxf(fmaf(f[e], sc[e], sh[e]), lo);
                v = TR::pack(f);
                if (!((a_inb >> it) & 1u)) v = u32x4{0u, 0u, 0u, 0u};
            }
            *reinterpret_cast<u32x4*>(smem + buf + a_st + it * (64 * C::PS)) = v;
        }
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) *reinterpret_cast<u32x4*>(smem + buf + b_st + it * (64 * C::PS)) = breg[it];
    };

    f32x16 acc[SW][2];
#pragma unroll
    for (int i = 0; i < SW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const unsigned a_frag = (unsigned)(((wrow * 8 + pm_row(r)) * 16 + pm_col(r)) * C::PS + h * 16);
    const unsigned b_frag = (unsigned)(C::A_BYTES + (wn * 64 + r) * C::PS + h * 16);

    // the 4 k-steps x 8 MFMAs of one 128-byte K step: k-step q+1's fragments are read while k-step q's MFMAs issue
    auto mfma_step = [&](unsigned buf) {
        u32x4 fa[2][SW], fb[2][2];
        auto rd = [&](int q, int set) {
            fa[set][0] = *reinterpret_cast<const u32x4*>(smem + buf + a_frag + q * 32);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[set][j] = *reinterpret_cast<const u32x4*>(smem + buf + b_frag + j * (32 * C::PS) + q * 32);
#pragma unroll
            for (int i = 1; i < SW; ++i) fa[set][i] = *reinterpret_cast<const u32x4*>(smem + buf + a_frag + i * (2 * 16 * C::PS) + q * 32);
        };
        rd(0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q + 1 < 4) rd(q + 1, (q + 1) & 1);
#pragma unroll
            for (int i = 0; i < SW; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) TR::mma16(fa[q & 1][i], fb[q & 1][j], acc[i][j]);
        }
        if (sizeof(typename TR::elem_t) == 2) {
            __builtin_amdgcn_sched_group_barrier(0x100, SW + 2, 0);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
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

    // both steps' loads go out together (see conv_igemm3.inc)
    issue_loads(0);
    {
        u32x4 a0[C::ITERS], b0[C::ITERS], a1[C::ITERS], b1[C::ITERS];
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) { a0[it] = areg[it]; b0[it] = breg[it]; }
        issue_loads(nsteps > 1 ? 1 : 0);
        __syncthreads();   // the transform table is complete
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) { a1[it] = areg[it]; b1[it] = breg[it]; areg[it] = a0[it]; breg[it] = b0[it]; }
        store_regs(0u, 0);
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) { areg[it] = a1[it]; breg[it] = b1[it]; }
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);   // no prologue load may stay pending into the loop
    __syncthreads();

    const bool second = wave >= 4;
    auto stage_phase = [&](int j) {
        store_regs((unsigned)((j + 1) & 1) * C::BUF_BYTES, j + 1);
        issue_loads(j + 2 < nsteps ? j + 2 : nsteps - 1);
    };
    // ONE barrier per step (round 3: the schedule conv_igemm3p.inc and conv_wgrad2.inc got in round 2, see conv_gather.inc): the first
    // half takes it after its staging part, the second half -- one stage phase ahead -- after its MFMAs.  (CMU_GEMM_2BAR: two-barrier form)
    if (second && 1 < nsteps) stage_phase(0);
#ifdef CMU_GEMM_2BAR
    __syncthreads();
#endif
#pragma unroll 1
    for (int k = 0; k < nsteps; ++k) {
        __builtin_amdgcn_s_setprio(2);
        mfma_step((unsigned)(k & 1) * C::BUF_BYTES);
        __builtin_amdgcn_s_setprio(0);
#ifdef CMU_GEMM_2BAR
        __syncthreads();
#else
        if (second) __syncthreads();
#endif
        const int j = k + (second ? 1 : 0);
        if (j + 1 < nsteps) stage_phase(j);
#ifdef CMU_GEMM_2BAR
        __syncthreads();
#else
        if (!second) __syncthreads();
#endif
    }
    __syncthreads();   // every MFMA read is done: the epilogue reuses the staging buffers

    ig3_epilogue<TR, 256, 1>(p, smem, acc, tid, lane, wave, wn, wrow, 0, r, h, b, ty, tx, ty0, tx0, n0);
}

template <class TR, bool DG, bool TF>
static int launch_conv_gemm(IGParams p, hipStream_t st, const char* name) {
    typedef CGCfg<TR> C;
    p.tilesX = cmu_div_up(p.W, 16);
    p.tilesY = cmu_div_up(p.H, 16);
    p.nblk = p.N / C::NB;
    p.npad = cmu_div_up(p.N, 64) * 64;
    p.total_blocks = (int64_t)p.B * p.tilesX * p.tilesY * p.nblk;
    if (int rc = cmu_launch_lds<&conv_gemm_kernel<TR, DG, TF>>(dim3((unsigned)p.total_blocks), dim3(512), C::LDS_BYTES, st, name, p)) return rc;
    cmu_set_kernel_tag("conv_gemm_kernel");
    CMU_CHECK_LAUNCH(name);
    return CMU_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Shallow-K form (the last decoder levels: K = 128 ... 256 channels, i.e. two to four 128-byte steps).  There a tile of the
// kernel above is all prologue and epilogue -- one HBM round trip for its operands, 32 ... 64 MFMAs per wave, 128 KB of
// stores -- and with one workgroup per CU nothing runs beside them: 128 -> 64 @ 256^2 took 0.60 ms forward against an HBM
// floor of 0.26 ms (tools/convt_sweep.py).  These layers are HBM-bound, so the cure is residency, not MFMA phases: tile
// 256 pixels x 128 channels, ONE staging buffer (54 KB; with the epilogue's transpose area 78 KB per workgroup), wave tile
// 64 px x 64 ch (64 accumulator registers) under __launch_bounds__(512, 4) (four waves per SIMD): two workgroups per CU, one loading / storing
// while the other multiplies.  No ping-pong, no fragment double buffer (four waves per SIMD hide the LDS latency); same
// raw buffer loads, LDS rows, fragment reads and shared epilogue as above.  With N = 256 the two channel blocks of a pixel
// tile are neighbouring workgroups (the second reads the tile from L2).
// ---------------------------------------------------------------------------------------------------------------------
template <class TR>
struct CGSCfg {
    typedef IG3Cfg<TR, 128, 1> E;   // epilogue geometry: 16 x 16 pixel tile, waves 4 (row bands of 4 rows) x 2 (64-channel blocks)
    static constexpr int ES = (int)sizeof(typename TR::elem_t);
    static constexpr int NB = 128;
    static constexpr int KSC = 128 / ES;
    static constexpr int PS = 144;
    static constexpr int A_BYTES = 256 * PS;        // 36,864
    static constexpr int B_BYTES = NB * PS;         // 18,432
    static constexpr int BUF_BYTES = A_BYTES + B_BYTES;
    static constexpr int MAX_K = 1024;
    static constexpr int TAB_BYTES = 2 * MAX_K * 4;
    static constexpr int LDS_BYTES = BUF_BYTES + TAB_BYTES > E::EPI_BYTES ? BUF_BYTES + TAB_BYTES : E::EPI_BYTES;   // 77,824
    static constexpr int A_ITERS = 4, B_ITERS = 2;
    static constexpr unsigned OOB = 0x7fff0000u;
};

template <class TR, bool DG, bool TF>
__global__ __launch_bounds__(512, 4) void conv_gemm_s_kernel(const IGParams p) {
    typedef CGSCfg<TR> C;
    constexpr int EPC = TR::EPC;
    constexpr int SW = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;
    const int wrow = wave & 3, wn = wave >> 2;   // wave = 4 rows x 16 columns x 64 channels

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
    const int ty0 = ty * 16, tx0 = tx * 16;
    const int n0 = nbk * C::NB;

    const int Hin = DG ? 2 * p.H : p.H, Win = DG ? 2 * p.W : p.W;
    const int64_t img_elems = (int64_t)Hin * Win * p.ldx;
    const unsigned char* ximg = reinterpret_cast<const unsigned char*>(p.x) + (int64_t)b * img_elems * C::ES;
    const unsigned x_bytes = (unsigned)((((int64_t)Hin * Win - 1) * p.ldx + p.K / (DG ? 4 : 1)) * C::ES);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(ximg), 0, (int)x_bytes, 0x00020000);
    const int nsteps = p.K / C::KSC;
    const unsigned w_bytes = (unsigned)((int64_t)2 * nsteps * p.npad * 64);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)w_bytes, 0x00020000);

    const int c8 = tid & 7;
    unsigned a_voff[C::A_ITERS];
    unsigned a_inb = 0;
#pragma unroll
    for (int it = 0; it < C::A_ITERS; ++it) {
        const int pix = it * 64 + (tid >> 3);
        const int gy = ty0 + (pix >> 4), gx = tx0 + (pix & 15);
        const bool ok = gy < p.H && gx < p.W;
        const int64_t po = DG ? ((int64_t)2 * gy * Win + 2 * gx) : ((int64_t)gy * Win + gx);
        a_voff[it] = ok ? (unsigned)((po * p.ldx + c8 * EPC) * C::ES) : C::OOB;
        a_inb |= (ok ? 1u : 0u) << it;
    }
    const unsigned a_st = (unsigned)((tid >> 3) * C::PS + c8 * 16);
    const unsigned b_voff0 = (unsigned)(((int64_t)(c8 >> 2) * p.npad + n0 + (tid >> 3)) * 64 + (c8 & 3) * 16);   // + it * 64 rows
    const unsigned b_st = (unsigned)(C::A_BYTES + (tid >> 3) * C::PS + c8 * 16);
    const unsigned w_step = (unsigned)p.npad * 128u;

    float* tab = reinterpret_cast<float*>(smem + C::BUF_BYTES);
    if (TF)
        for (int c = tid; c < p.K; c += 512) {
            tab[c] = p.in_scale[c];
            tab[C::MAX_K + c] = p.in_shift[c];
        }

    u32x4 areg[C::A_ITERS], breg[C::B_ITERS];
    const int cpi = DG ? (p.K / 4) / C::KSC : 1;
    auto issue_loads = [&](int s) {
        unsigned soff;
        if (DG) {
            const int ij = s / cpi, cc = s - ij * cpi;
            soff = (unsigned)((((int64_t)(ij >> 1) * Win + (ij & 1)) * p.ldx + cc * C::KSC) * C::ES);
        } else {
            soff = (unsigned)(s * 128);
        }
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) areg[it] = ig3_bload(rs_x, a_voff[it], soff);
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it) breg[it] = ig3_bload(rs_w, b_voff0, (unsigned)s * w_step + (unsigned)it * (64u * 64u));
    };
    auto store_regs = [&](int s) {
        float sc[EPC], sh[EPC];
        float lo = 0.f;
        if (TF) {
            const int c0 = s * C::KSC + c8 * EPC;
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
            *reinterpret_cast<u32x4*>(smem + a_st + it * (64 * C::PS)) = v;
        }
#pragma unroll
        for (int it = 0; it < C::B_ITERS; ++it) *reinterpret_cast<u32x4*>(smem + b_st + it * (64 * C::PS)) = breg[it];
    };

    f32x16 acc[SW][2];
#pragma unroll
    for (int i = 0; i < SW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const unsigned a_frag = (unsigned)(((wrow * 2 * SW + pm_row(r)) * 16 + pm_col(r)) * C::PS + h * 16);
    const unsigned b_frag = (unsigned)(C::A_BYTES + (wn * 64 + r) * C::PS + h * 16);

    issue_loads(0);
    if (TF) __syncthreads();   // the transform table is complete
#pragma unroll 1
    for (int s = 0; s < nsteps; ++s) {
        if (s > 0) __syncthreads();   // the buffer's readers (MFMAs of step s-1) are done
        store_regs(s);
        if (s + 1 < nsteps) issue_loads(s + 1);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u32x4 fa[SW], fb[2];
#pragma unroll
            for (int i = 0; i < SW; ++i) fa[i] = *reinterpret_cast<const u32x4*>(smem + a_frag + i * (2 * 16 * C::PS) + q * 32);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const u32x4*>(smem + b_frag + j * (32 * C::PS) + q * 32);
#pragma unroll
            for (int i = 0; i < SW; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) TR::mma16(fa[i], fb[j], acc[i][j]);
        }
    }
    __syncthreads();
    ig3_epilogue<TR, 128, 1>(p, smem, acc, tid, lane, wave, wn, wrow, 0, r, h, b, ty, tx, ty0, tx0, n0);
}

template <class TR, bool DG, bool TF>
static int launch_conv_gemm_s(IGParams p, hipStream_t st, const char* name) {
    typedef CGSCfg<TR> C;
    static_assert(2 * C::LDS_BYTES <= 163840, "two workgroups per CU");
    p.tilesX = cmu_div_up(p.W, 16);
    p.tilesY = cmu_div_up(p.H, 16);
    p.nblk = p.N / C::NB;
    p.npad = cmu_div_up(p.N, 64) * 64;
    p.total_blocks = (int64_t)p.B * p.tilesX * p.tilesY * p.nblk;
    if (int rc = cmu_launch_lds<&conv_gemm_s_kernel<TR, DG, TF>>(dim3((unsigned)p.total_blocks), dim3(512), C::LDS_BYTES, st, name, p)) return rc;
    cmu_set_kernel_tag("conv_gemm_s_kernel");
    CMU_CHECK_LAUNCH(name);
    return CMU_OK;
}

// shallow-K form: 16-bit operands, N in whole 128-channel blocks, at most CMU_CONVT_SMALL_STEPS (default 4) 128-byte K steps;
// CMU_CONVT_SMALL=0 switches it off (A/B)
template <class TR>
static bool conv_gemm_s_eligible(const IGParams& p, bool dg) {
    const bool on = cmu_knob(CMU_KNOB_CONVT_SMALL);
    const int max_steps = cmu_knob(CMU_KNOB_CONVT_SMALL_STEPS);
    constexpr int KSC = 128 / (int)sizeof(typename TR::elem_t);
    if (!on || sizeof(typename TR::elem_t) != 2 || p.N % 128 != 0 || p.K % KSC != 0 || p.K / KSC > max_steps) return false;
    if (dg && (p.K / 4) % KSC != 0) return false;
    if (p.in_scale != nullptr && p.K > 1024) return false;
    const int64_t px = (int64_t)(dg ? 4 : 1) * p.H * p.W;
    if ((px * p.ldx + p.K) * (int64_t)sizeof(typename TR::elem_t) >= 0x7fff0000ll) return false;
    if ((int64_t)p.K * 2 * cmu_div_up(p.N, 64) * 64 * (int64_t)sizeof(typename TR::elem_t) >= 0x7fff0000ll) return false;
    return (int64_t)p.B * cmu_div_up(p.W, 16) * cmu_div_up(p.H, 16) * (p.N / 128) < (1ll << 31);
}

// CMU_CONVT_GEMM=0 keeps ConvTranspose forward / data gradient on the first kernel (A/B switch)
template <class TR>
static bool conv_gemm_eligible(const IGParams& p, bool dg) {
    const bool on = cmu_knob(CMU_KNOB_CONVT_GEMM);
    constexpr int KSC = 128 / (int)sizeof(typename TR::elem_t);
    if (!on || p.N % 256 != 0 || p.K % KSC != 0) return false;
    if (dg && (p.K / 4) % KSC != 0) return false;                 // a 128-byte step stays inside one sub-pixel position
    if (p.in_scale != nullptr && p.K > 1024) return false;
    const int64_t px = (int64_t)(dg ? 4 : 1) * p.H * p.W;
    if ((px * p.ldx + p.K) * (int64_t)sizeof(typename TR::elem_t) >= 0x7fff0000ll) return false;
    if ((int64_t)p.K * 2 * cmu_div_up(p.N, 64) * 64 * (int64_t)sizeof(typename TR::elem_t) >= 0x7fff0000ll) return false;
    return true;
}
