// conv_gather.inc -- 3x3 convolution over a LIST OF ACTIVE PIXELS as a gather-GEMM (included by conv_igemm.hip after conv_gemm.inc,
// whose tile configuration, staging and MFMA step it shares).
//
// SparK's sparse convolution (Pretraining/Spark/encoder.py:20-23: dense conv, then `*= active`) only needs the outputs at active
// pixels, and its input is zero at masked ones.  Skipping whole 16 x 32 tiles (cmu_conv3x3_fwd_tiles) works where patches are at
// least as large as tiles; at the deeper levels (patch side 4, 2, 1 px) every dense tile holds an active pixel.  Here the GEMM's M
// dimension is the list itself: 256 rows per workgroup = 256 active pixels wherever they lie (rows[] holds their dense pixel
// indices, patch-major), N = 256 output channels, K = 9 taps x Cin walked tap by tap in 128-byte channel steps.  The A operand
// of a step is gathered: row m reads the channel vector of pixel rows[m] + (dy, dx) of the DENSE NHWC input (zero by buffer-range
// when the neighbour is outside the image; a masked neighbour holds zeros in the tensor), so no neighbour table and no packed
// copy of the activations exist -- the producers and consumers of the dense layout stay as they are -- and the halo is re-read
// per tap from L2 instead of from an LDS tile (9 x the A traffic per output, at >= 256 output channels per staged byte: 16 B/clk
// per CU at the matrix pipe's full rate).  Outputs are scattered to y at rows[m]; the rest of y is left untouched.
// FLOPs = active fraction x dense exactly.  Used for Cout % 128 == 0, Cin a whole number of 128-byte steps (levels 2-5 of the
// reference UNet; 256 channels per workgroup where Cout allows, else 128); the weights are the ordinary conv3x3 packs (forward or flipped for the data gradient).

// NB = 256: waves 2 (M) x 4 (N), wave = 128 rows x 64 channels (32 MFMAs per step); NB = 128 (level 2 of the reference UNet): waves
// 4 x 2, wave = 64 rows x 64 channels (16 MFMAs per step against 4 + 2 staged chunks)
template <class TR, int NB>
__global__ __launch_bounds__(512) void conv_gather_kernel(const IGParams p) {
    typedef CGCfg<TR> C;
    typedef IG3Cfg<TR, NB, 1> E;
    typedef typename TR::elem_t elem_t;
    constexpr int EPC = TR::EPC;
    constexpr int WN = NB / 64, WM = 8 / WN;
    constexpr int SW = 8 / WM;                    // 32-row strips per wave (4 / 2)
    constexpr int B_ITERS = NB / 64;              // weight rows staged per thread and step
    constexpr int B_OFF = C::A_BYTES;             // (the B region keeps the 256-row stride: buffers sized for NB = 256)
    static_assert(E::SW == SW && E::WN == WN, "epilogue geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;
    const int wrow = wave % WM, wn = wave / WM;   // wave = SW*32 rows x 64 channels

    int64_t bid = blockIdx.x;
    {
        const int64_t nb = p.total_blocks;
        const int64_t q = nb >> 3, rem = nb & 7;
        const int64_t xcd = bid & 7, local = bid >> 3;
        bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + local;
    }
    const int nbk = (int)(bid % p.nblk);
    const int rtile = (int)(bid / p.nblk);
    const int nrows = __builtin_amdgcn_readfirstlane(*p.tile_count);
    if (rtile * 256 >= nrows) return;             // (uniform per workgroup, before any barrier)
    const int n0 = nbk * NB;

    // ---- the tile's rows: dense pixel indices (-1: padding past the end of the list) ----------------------------------------------
    int* pixmap = reinterpret_cast<int*>(smem + C::MAIN_BYTES);
    if (tid < 256) {
        const int row = rtile * 256 + tid;
        pixmap[tid] = row < nrows ? p.tile_list[row] : -1;
    }
    __syncthreads();

    const unsigned x_bytes = (unsigned)((((int64_t)p.B * p.H * p.W - 1) * p.ldx + p.K) * C::ES);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)x_bytes, 0x00020000);
    const int cpi = p.K / C::KSC;                 // 128-byte steps per tap
    const int nsteps = 9 * cpi;
    const unsigned w_bytes = (unsigned)((int64_t)p.nslices32 * 9 * p.npad * 32);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)w_bytes, 0x00020000);

    // ---- per-thread staging roles: 16-byte chunk c8 of a 128-byte K step, rows it*64 + tid/8 ----------------------------------------
    const int c8 = tid & 7;
    int a_pix[C::ITERS], a_y[C::ITERS], a_x[C::ITERS];
#pragma unroll
    for (int it = 0; it < C::ITERS; ++it) {
        const int px = pixmap[it * 64 + (tid >> 3)];
        a_pix[it] = px;
        const int rem = px >= 0 ? px % (p.H * p.W) : 0;
        a_y[it] = rem / p.W;
        a_x[it] = rem % p.W;
    }
    unsigned a_voff[C::ITERS];
    auto set_tap = [&](int t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) {
            const int yy = a_y[it] + dy, xx = a_x[it] + dx;
            const bool ok = a_pix[it] >= 0 && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
            a_voff[it] = ok ? (unsigned)(((int64_t)(a_pix[it] + dy * p.W + dx) * p.ldx + c8 * EPC) * C::ES) : C::OOB;
        }
    };
    const unsigned a_st = (unsigned)((tid >> 3) * C::PS + c8 * 16);
    // conv3x3 pack: [32-byte slice][tap][npad][32 B]; chunk c8 of row n of step (tap, cc) lives in slice 4*cc + (c8 >> 1)
    unsigned b_voff[B_ITERS];
#pragma unroll
    for (int it = 0; it < B_ITERS; ++it) {
        const int row = it * 64 + (tid >> 3);
        b_voff[it] = (unsigned)((((int64_t)(c8 >> 1) * 9) * p.npad + n0 + row) * 32 + (c8 & 1) * 16);
    }
    const unsigned b_st = (unsigned)(B_OFF + (tid >> 3) * C::PS + c8 * 16);
    const unsigned w_tap = (unsigned)p.npad * 32u;           // one tap further inside a slice
    const unsigned w_step = w_tap * 36u;                     // four slices further

    u32x4 areg[C::ITERS], breg[B_ITERS];
    auto issue_loads = [&](int s) {
        const int t = s / cpi, cc = s - t * cpi;
        set_tap(t);       // (recomputed every step: ~40 VALU, no branch inside the staging phase)
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) areg[it] = ig3_bload(rs_x, a_voff[it], (unsigned)(cc * 128));
#pragma unroll
        for (int it = 0; it < B_ITERS; ++it) breg[it] = ig3_bload(rs_w, b_voff[it], (unsigned)cc * w_step + (unsigned)t * w_tap);
    };
    auto store_regs = [&](unsigned buf) {
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) *reinterpret_cast<u32x4*>(smem + buf + a_st + it * (64 * C::PS)) = areg[it];
#pragma unroll
        for (int it = 0; it < B_ITERS; ++it) *reinterpret_cast<u32x4*>(smem + buf + b_st + it * (64 * C::PS)) = breg[it];
    };

    f32x16 acc[SW][2];
#pragma unroll
    for (int i = 0; i < SW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const unsigned a_frag = (unsigned)(((wrow * 2 * SW + pm_row(r)) * 16 + pm_col(r)) * C::PS + h * 16);
    const unsigned b_frag = (unsigned)(B_OFF + (wn * 64 + r) * C::PS + h * 16);

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
        if (sizeof(elem_t) == 2) {
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

    // ---- prologue / two-phase ping-pong main loop: conv_gemm.inc --------------------------------------------------------------------
    issue_loads(0);
    {
        u32x4 a0[C::ITERS], b0[B_ITERS], a1[C::ITERS], b1[B_ITERS];
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) a0[it] = areg[it];
#pragma unroll
        for (int it = 0; it < B_ITERS; ++it) b0[it] = breg[it];
        issue_loads(nsteps > 1 ? 1 : 0);
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) { a1[it] = areg[it]; areg[it] = a0[it]; }
#pragma unroll
        for (int it = 0; it < B_ITERS; ++it) { b1[it] = breg[it]; breg[it] = b0[it]; }
        store_regs(0u);
#pragma unroll
        for (int it = 0; it < C::ITERS; ++it) areg[it] = a1[it];
#pragma unroll
        for (int it = 0; it < B_ITERS; ++it) breg[it] = b1[it];
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);
    __syncthreads();

    const bool second = wave >= 4;
    auto stage_phase = [&](int j) {
        store_regs((unsigned)((j + 1) & 1) * C::BUF_BYTES);
        issue_loads(j + 2 < nsteps ? j + 2 : nsteps - 1);
    };
    // ONE barrier per step (round 3; the schedule of conv_igemm3p.inc / conv_wgrad2.inc): between two barriers the first half multiplies
    // step k and then stages its part of step k+1; the second half -- one stage phase ahead -- stages its part of step k+1 and then
    // multiplies step k.  The first half takes the barrier after its staging, the second half after its MFMAs: step k+1's buffer is
    // complete one barrier before anybody reads it, and a buffer is rewritten only behind the barrier that follows its last reader.
    // (CMU_GATHER_2BAR: the two-barrier form, A/B)
    if (second && 1 < nsteps) stage_phase(0);
#ifdef CMU_GATHER_2BAR
    __syncthreads();
#endif
#pragma unroll 1
    for (int k = 0; k < nsteps; ++k) {
        __builtin_amdgcn_s_setprio(2);
        mfma_step((unsigned)(k & 1) * C::BUF_BYTES);
        __builtin_amdgcn_s_setprio(0);
#ifdef CMU_GATHER_2BAR
        __syncthreads();
#else
        if (second) __syncthreads();
#endif
        const int j = k + (second ? 1 : 0);
        if (j + 1 < nsteps) stage_phase(j);
#ifdef CMU_GATHER_2BAR
        __syncthreads();
#else
        if (!second) __syncthreads();
#endif
    }
    __syncthreads();   // every MFMA read is done: the epilogue reuses the staging buffers

    // ---- epilogue: accumulators -> per-wave LDS rows (pixel-major) -> 16-byte stores scattered to y at rows[m] ------------------------
    unsigned char* my = smem + wave * E::EPI_WAVE;
    unsigned char* yb = reinterpret_cast<unsigned char*>(p.y);
    constexpr int CPR = E::NFP * 32 / EPC;
    constexpr int NIT = (SW * 32 * CPR) / 64;
#pragma unroll
    for (int jp = 0; jp < 2 / E::NFP; ++jp) {
        if (jp > 0) __syncthreads();
#pragma unroll
        for (int i = 0; i < SW; ++i)
#pragma unroll
            for (int jj = 0; jj < E::NFP; ++jj)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                    *reinterpret_cast<elem_t*>(my + m * E::EPI_ROW + (32 * jj + r) * C::ES) = TR::from_float(acc[i][jp * E::NFP + jj][e]);
                }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = it * 64 + lane;
            const int m = idx / CPR, q = idx % CPR;
            const int mt = (wrow * 2 * SW + 2 * (m >> 5) + pm_row(m & 31)) * 16 + pm_col(m & 31);   // the row's slot in the tile (A-operand order)
            const int px = pixmap[mt];
            const int n = n0 + wn * 64 + jp * E::NFP * 32 + q * EPC;
            if (px >= 0) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(my + m * E::EPI_ROW + q * 16);
                st_global16(yb + ((int64_t)px * p.ldy + n) * (int64_t)sizeof(elem_t), v);
            }
        }
    }
}

template <class TR, int NB>
static int launch_conv_gather_nb(IGParams p, int64_t max_rows, hipStream_t st) {
    typedef CGCfg<TR> C;
    constexpr int LDS = C::MAIN_BYTES + 1024 > IG3Cfg<TR, NB, 1>::EPI_STAGE + 1024 ? C::MAIN_BYTES + 1024 : IG3Cfg<TR, NB, 1>::EPI_STAGE + 1024;
    static_assert(LDS <= 163840, "LDS budget");
    p.nblk = p.N / NB;
    p.npad = cmu_conv3x3_npad(p.N);
    p.nslices32 = p.K / (32 / C::ES);
    p.total_blocks = cmu_div_up64(max_rows, 256) * p.nblk;
    if (int rc = cmu_launch_lds<&conv_gather_kernel<TR, NB>>(dim3((unsigned)p.total_blocks), dim3(512), LDS, st, "cmu_conv3x3_fwd_rows", p)) return rc;
    cmu_set_kernel_tag("conv_gather_kernel");
    CMU_CHECK_LAUNCH("cmu_conv3x3_fwd_rows");
    return CMU_OK;
}
template <class TR>
static int launch_conv_gather(IGParams p, int64_t max_rows, hipStream_t st) {
    // 256 output channels per workgroup stage the fewest bytes per MFMA, but the deep levels have few rows: level 5 of the bench
    // shape (8,192 active pixels = 32 row tiles) gives 128 workgroups at N = 1,024 and 64 at N = 512 -- half / a quarter of the chip.
    // Where the 256-channel grid does not fill the CUs, 128 channels per workgroup double it (CMU_GATHER_NB=128|256 forces a form: A/B).
    const int forced = cmu_knob(CMU_KNOB_GATHER_NB);
    bool wide = p.N % 256 == 0;
    if (wide && forced == 0) wide = cmu_div_up64(max_rows, 256) * (p.N / 256) >= cmu_num_cus();
    if (forced == 128) wide = false;
    if (forced == 256) wide = p.N % 256 == 0;
    return wide ? launch_conv_gather_nb<TR, 256>(p, max_rows, st) : launch_conv_gather_nb<TR, 128>(p, max_rows, st);
}
