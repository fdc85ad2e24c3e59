// conv_igemm3p.inc -- persistent form of the wide-tile 3x3 implicit-GEMM kernel (included by conv_igemm.hip after
// conv_igemm3.inc, whose tile configuration, LDS layouts and MFMA step it shares).
//
// Why: conv_igemm3_kernel's main loop keeps the matrix pipe ~79 % busy, but a workgroup is one 16 x 32 pixel x NB channel
// tile and the CU holds exactly one workgroup (LDS), so nothing runs beside a tile's fixed costs: dispatch of the next
// workgroup, the (scale, shift) table, the first slices' HBM round trip, the second half's first stage phase, the
// epilogue and the drain of its stores.  Measured through the layer sweep (tools/layer_sweep.sh) that is ~12 us per tile
// whatever K is: 1,431 TFLOP/s at K = 1024 but 995 at K = 128, where a tile's main loop is only 26 us.
// Here one workgroup per CU walks a list of tiles and the K slices of consecutive tiles form ONE stream through the same
// two-phase ping-pong: while the last slices of tile t are multiplied, the staging side is already loading tile t+1, and
// a half's epilogue runs in its staging slot beside the other half's MFMA phase.  What changes against conv_igemm3:
//   * static tile list per workgroup: XCD x (blockIdx & 7) owns a contiguous range of (pixel tile, channel block) items,
//     its CUs take them round-robin, so at any time the CUs of an XCD work on neighbouring items (shared halo / weights
//     in that XCD's L2) exactly as the hardware's in-order dispatch arranged it for the one-tile kernel;
//   * the load cursor (item, slice) runs two positions ahead of the MFMAs; at an item switch the per-thread halo offsets
//     and the image's buffer descriptor are rebuilt (a few dozen VALU/SALU per tile);
//   * the epilogue goes through two private 2.3 KB LDS strips per wave (16 pixels x 64 channels each; four waves run
//     epilogues at once), so the staging buffers stay live: 132,480 (buffers) + 8,192 (table) + 4,096 (statistics) +
//     18,432 = 163,200 B of the 163,840; it handles whole tiles only (the launcher sends shapes with partial tiles to the
//     one-tile kernel), which removes every bounds predicate and turns a pixel's address into scalar base + one of two
//     per-lane offsets; its index arithmetic is rebuilt from an opaque copy of the lane id each time, or LICM parks it in
//     registers across the MFMA phase (spills).  Round 2 (tools/igemm3p_stamps.py, -DCMU_IG_STAMPS_EPI for stamps inside
//     the epilogue; 128 -> 128: the slot went from 5,870 to 4,600 cycles, BatchNorm-backward form 5.8 -> 5.1 ms per step):
//     the slot was bound by LDS operations and latency, not by vector issue -- halving the statistics' instruction count
//     with packed f32 math changed nothing (v_pk_add/fma_f32 issue at half rate), but (a) staging the weight rows of a
//     16-bit tile so that a lane holds ADJACENT channels turns the transpose's 128 two-byte LDS writes per lane into 64
//     dword writes (ds_write2_b32 pairs), (b) the second strip lets unit u+1 be converted and written while unit u's
//     transposed reads are in flight, (c) the ReLU gate of the BatchNorm-backward sums is a clamped FMA straight from the
//     16-bit x (v_fma_mix_f32 ... clamp) and their fold over the wave uses gfx950's permlane swaps (two channels per add)
//     instead of 48 ds_bpermute, (d) the accumulators are cleared by eight 0 x 0 MFMAs instead of 128 v_mov;
//   * the per-16x16-tile statistics slab rows of a tile are written one barrier after both halves' epilogues.
// Results are bit-identical to conv_igemm3_kernel (same MFMA order per accumulator, same statistics folding order).
// Measured (tools/layer_sweep.sh, bs 32): a tile costs a*nsl + c with a = 3.3 us per 32-byte slice in both kernels and
// c = 13.5 us (one-tile) -> 7.7 us (here); what is left of c is the ~1,150-instruction epilogue of each half, of which
// only the part that fits beside the partner's 2,800-cycle MFMA phase is hidden.  Did not pay: starting a tile's
// accumulators from an inline-constant 0 in a second copy of the MFMA step (the duplicated body spills), 64-bit item
// arithmetic (4 x ~130 scalar instructions per decode); running the second half's epilogue before its barrier, beside the
// first half's (tools/igemm3p_stamps.py: alone an epilogue takes 6,060 cycles for ~1,150 instructions, two side by side
// 7,900 and 9,900 -- round 1 read that as vector-issue bound; round 2's stamps inside the epilogue showed LDS operations and
// latency, see above; a normal iteration is 2,500 MFMA + 133 barrier + 1,950 staging + ~1,000 idle); a one-buffer form of
// the 64-channel tile with two workgroups per CU (the cure that halved the shallow ConvTranspose GEMMs, conv_gemm.inc:
// 64 accumulator registers, __launch_bounds__(512, 4)) measured 0.747 / 1.314 ms against 0.729 / 1.232 ms here on 64 -> 64 /
// 128 -> 64 at 512 x 512 and was dropped;
// a DEFERRED epilogue that only retires the accumulators at the last slice (statistics, packed conversion, a dump of the
// registers into the unit's own output bytes) and transposes one 16-pixel unit per later staging slot (read back from L2,
// LDS strip, NHWC store) to use that idle time: correct, but the raw bytes held across the slot's LDS stores cost the
// registers that keep loop invariants out of scratch, scratch reloads share vmcnt with the loads in flight, and each such
// slot grew by ~3,000 cycles instead of ~500 (128 -> 128: 818 TFLOP/s against 1,132);
// (second session of round 2) for the 64-channel tile, whose accumulators are 64 registers with ~100 to spare: accumulators
// RETIRED at the last slice (statistics from the fp32 values, packed 16-bit copy in 32 registers) and the four 16-pixel units
// sent through per-wave LDS strips one per staging slot of the NEXT tile, each beside a whole MFMA phase of the partner --
// bit-identical, 173 / 212 registers, no scratch, and SLOWER: 64 -> 64 @ 512 0.733 -> 0.767 ms, 128 -> 64 @ 512 1.221 -> 1.256.
// The exposed epilogue it removes is idle time, and idle time is not what bounds this kernel: the chip is at its power limit
// (probe.hip: an LDS-fed 32x32x16 MFMA loop with dense N(0,1) operands sustains 1.41 PFLOP/s at 1.44 GHz and nothing more),
// so the clock falls as the bubbles fill, and the spread form executes more instructions (item decode and address set-up per
// slot, no overlap between units) for the same MFMAs.

// WRES (round 3, the 64 -> 64 layers at 16 bits: K = 64 = four slices, one channel block): the WHOLE packed weight tensor
// (4 slices x 9 taps x 64 rows x 32 B = 73,728 B) is loaded into LDS once per workgroup and stays there for every tile of its
// list; only the halo is double-buffered (2 x 29,376 B).  The 16 x 32 x 64 tile is staging-bound (1,630 cycles of staging per
// 1,370 of MFMAs, DESIGN section 5) and the weight rows are half of what a slice stages: 2.4 chunks per thread and slice
// instead of 4.65.  Same MFMA order per accumulator: bit-identical to the streaming form.  Measured (tools/layer_sweep.sh, f16,
// same box): 64 -> 64 @ 512 x 512 0.749 -> 0.705 ms; the default step 40.30 -> 40.03 ms.  Less than the staging share suggests: the
// slice's store_regs slot went from ~1,050 to ~820 cycles (tools/igemm3p_stamps.py) -- most of it is the wait for the halo loads and
// their BatchNorm+ReLU transform, not the weight rows -- and half of a cycle saving comes back as a lower clock (the kernel runs
// 0.58 ms on zeroed operands against 0.72 ms on data: power-bound even at ~50 % matrix-pipe duty, at 3 TB/s of HBM traffic).
// Also measured here and dropped: a DIRECT epilogue for the 16-bit 64-channel tile -- no LDS transpose: with the interleaved
// weight-row order a half wave holds the 128 contiguous bytes of one pixel's 64 channels, so 32 global_store_dword per lane
// replace 32 LDS writes + 8 LDS reads + 8 16-byte stores; bit-identical output, all tests green, and the epilogue slot grew from
// 2,130 to 2,720 cycles (dword stores issue at a quarter of the bytes per instruction): 0.713 -> 0.708 ms on 64 -> 64, 1.265 ->
// 1.276 ms on 128 -> 64, data-gradient launches +0.09 ms per step.
// And (same round) the SPREAD epilogue again, now on top of WRES where the staging slots are shorter than the partner's MFMA phases:
// the last slice's slot only retires the accumulators (statistics from the fp32 values, packed copy in 32 registers, cleared on the
// matrix pipe), slots 0 / 1 of the next tile send two 16-pixel units each through a per-wave strip, slot 3 writes the previous tile's
// slab rows from a statistics strip per tile parity (the table shrunk to K = 64 to make room).  Bit-identical (the persistent-kernel
// identity tests passed), 154 / 207 registers, no scratch -- and 0.706 -> 0.704 ms (0.558 -> 0.541 on zeroed operands), the step
// 40.38 -> 40.44 ms: the serialised epilogues are not what bounds this layer.
// (Round 3 concluded "HBM-bound first" from the 0.54 ms the layer takes on zeroed operands = 2.15 GB at 4 TB/s.  Round 4 withdraws that:
// the same structure's data-gradient instance moves 4.0 GB at 5.15 TB/s, this instance 3.3 TB/s; stamps + PMC
// (profiles/r04_igemm3p_timeline.txt) show a matrix pipe busy 51 % of the time, steady-state positions paced by the pipe AND by each
// wave's own chain alike (2 x 1,350 cycles of MFMA against 1,350 + ~1,500 of barrier / store_regs / issue), and the tile's last two
// positions stretched by the two halves' epilogues running one after the other on the shared LDS strips: 6.6K of a tile's 17.4K
// cycles are covered by no MFMA, and the non-MFMA instruction streams of a SIMD's two waves (12.7K cycles per tile) exceed their MFMA
// phases (10.8K).  The tile is bound by those streams.  A load cursor three positions ahead would not shorten the pipe-paced
// positions.  Two timing-only experiments of round 4 (wrong results by construction, never shipped; layer sweep f16, same box,
// profiles/r04_igemm3p_timeline.txt) priced the ways out before anything was built:
//   * both halves' epilogues SIDE BY SIDE (the second half takes its barrier at the end of a tile's last iteration): 64 -> 64 0.720 ->
//     0.698 ms, 128 -> 64 1.276 -> 1.265, 128 -> 128 @ 256 and every deeper layer +-0: the epilogues are bound by LDS throughput, two
//     at once take as long as one after the other -- private strips + a flag in place of the barrier would buy <= 3 % of one layer;
//   * an epilogue WITHOUT the LDS transpose (what swapped MFMA operands would allow: a lane holds 16 channels of one pixel, two
//     16-byte row-per-lane stores per (strip, fragment) + a cross-lane fold for the statistics): 64 -> 64 0.70 -> 0.83 ms, 128 -> 64
//     1.27 -> 1.40, 128 -> 128 0.55 -> 0.61, 1024 -> 1024 0.46 -> 0.47: partial-line stores cost more than the transpose they save.
// The transposing epilogue through per-wave strips stays.)
template <class TR, int NB, int THB = 1, bool WRES = false>
struct IG3PCfg {
    typedef IG3Cfg<TR, NB, 2, THB> C;
    static constexpr int WRES_SLICES = 4;
    static constexpr int A_STRIDE = WRES ? C::A_BYTES : C::BUF_BYTES;   // distance between the two halo buffers
    static constexpr int B_BASE = WRES ? 2 * C::A_BYTES : C::A_BYTES;   // weight rows: behind both halo buffers / behind each
    static constexpr int MAIN_BYTES = WRES ? 2 * C::A_BYTES + WRES_SLICES * C::B_BYTES : C::MAIN_BYTES;
    static constexpr int STAT_OFF = MAIN_BYTES + C::TAB_BYTES;
    static constexpr int STAT_BYTES = 8 * 64 * 2 * 4;
    static constexpr int EPI_OFF = STAT_OFF + STAT_BYTES;
    static constexpr int EPI_WAVE1 = 16 * C::EPI_ROW;  // one 16-pixel unit x (NFP x 32) channels
#ifdef CMU_IG_STAMPS
    static constexpr int STAMP_OFF = MAIN_BYTES + 1024;   // diagnostic stamps (tools/igemm3p_stamps.py) sit in the unused middle of
    static constexpr int STAMP_ITERS = 12;                   // the (scale, shift) table: layers of at most 256 input channels only
    static constexpr int LDS_BYTES = EPI_OFF + 8 * EPI_WAVE1;
#else
    static constexpr int LDS_BYTES = EPI_OFF + 8 * EPI_WAVE1;   // two strips for each of the four waves in an epilogue
#endif
};

template <class TR, int NB, bool TF, bool BST, int THB = 1, bool WRES = false, bool PART = false>
__global__ __launch_bounds__(512) void conv_igemm3p_kernel(const IGParams p) {
    typedef IG3Cfg<TR, NB, 2, THB> C;
    typedef IG3PCfg<TR, NB, THB, WRES> P;
    typedef typename TR::elem_t elem_t;
    constexpr int EPC = TR::EPC;
    constexpr int SW = C::SW;
    constexpr int TWB = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;
    const int wm = wave % C::WM, wn = wave / C::WM;
    const int wcol = wm % TWB, wrow = wm / TWB;

    // ---- this workgroup's items ---------------------------------------------------------------------------------------
    // workgroup ids go round-robin over the 8 XCDs (fewer groups when the grid is smaller than that)
    const int nx = gridDim.x < 8u ? (int)gridDim.x : 8;
    const int xcd = (int)blockIdx.x % nx, local = (int)blockIdx.x / nx;
    const int nloc = ((int)gridDim.x - xcd + nx - 1) / nx;   // workgroups on this XCD
    int item0, n_my;   // 32-bit item arithmetic: the launcher keeps total_blocks below 2^30
    {
        // (sparse form: the number of listed tiles lives on the device -- no host round trip between the list builder and
        // this launch; the grid was sized for the dense count, surplus workgroups leave at once)
        const int total = p.tile_list != nullptr ? __builtin_amdgcn_readfirstlane(*p.tile_count) * p.nblk : (int)p.total_blocks;
        const int q = total / nx, rem = total % nx;
        const int start = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
        const int cnt = q + (xcd < rem ? 1 : 0);
        if (local >= cnt) return;
        item0 = start + local;
        n_my = (cnt - local + nloc - 1) / nloc;
    }
    const int nsl = p.nslices32;
    const int G = n_my * nsl;   // length of the slice stream

    struct Item { int b, ty, tx, n0; };
    auto fdiv = [](unsigned n, const unsigned (&fd)[2]) { return (__umulhi(n, fd[0]) + n) >> fd[1]; };
    auto decode = [&](int i) {
        const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(item0 + i * nloc);
        const unsigned slot = fdiv(w, p.fd_nblk), nbk = w - slot * (unsigned)p.nblk;
        const unsigned tile = p.tile_list != nullptr ? (unsigned)__builtin_amdgcn_readfirstlane(p.tile_list[slot]) : slot;
        const unsigned rest = fdiv(tile, p.fd_tx);
        Item t;
        t.tx = (int)(tile - rest * (unsigned)p.tilesX);
        t.b = (int)fdiv(rest, p.fd_ty);
        t.ty = (int)(rest - (unsigned)t.b * (unsigned)p.tilesY);
        t.n0 = (int)nbk * NB;
        return t;
    };

    const int64_t img_bytes = (int64_t)p.H * p.W * p.ldx * C::ES;
    const unsigned x_bytes = (unsigned)((((int64_t)p.H * p.W - 1) * p.ldx + p.K) * C::ES);
    const unsigned w_bytes = (unsigned)((int64_t)p.nslices32 * 9 * p.npad * 32);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)w_bytes, 0x00020000);

    // ---- per-thread staging roles ---------------------------------------------------------------------------------------
    const int cg = tid & 1;  // 16-byte chunk of the 32-byte slice
    unsigned a_voff[C::A_ITERS];
    unsigned a_inb = 0;        // in-image flags of the load cursor's tile
    const unsigned char* ximg = reinterpret_cast<const unsigned char*>(p.x);
    unsigned n0off = 0;        // byte offset of the cursor's channel block inside a (slice, tap) of the weight pack
    auto set_load_tile = [&](int i) {
        const Item t = decode(i);
        const int ty0 = t.ty * C::TH, tx0 = t.tx * C::TW;
        a_inb = 0;
        // (the tile-switch and epilogue code runs inside the slice loop: its per-lane index arithmetic is rebuilt from an
        // opaque copy of the thread id, or LICM parks dozens of loop-invariant registers across the MFMA phase -> spills)
        int tl = tid;
        asm volatile("" : "+v"(tl));
        const int cgl = tl & 1;
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) {
            const int pix = it * 256 + (tl >> 1);
            const int py = pix / C::LW, px = pix % C::LW;
            const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
            const bool ok = pix < C::NPIX && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
            // (32-bit: igemm3_eligible keeps one image below 0x7fff0000 bytes)
            a_voff[it] = ok ? (((unsigned)gy * (unsigned)p.W + (unsigned)gx) * (unsigned)p.ldx + (unsigned)(cgl * EPC)) * (unsigned)C::ES : C::OOB;
            a_inb |= (ok ? 1u : 0u) << it;
        }
        ximg = reinterpret_cast<const unsigned char*>(p.x) + (int64_t)t.b * img_bytes;
        n0off = (unsigned)t.n0 * 32u;
    };
    const bool a_last_live = ((C::A_ITERS - 1) * 256 + (tid >> 1)) < C::NPIX;
    const unsigned a_st = (unsigned)((tid >> 1) * C::PS + cg * 16);
    // weights: chunk idx = it*512 + tid -> row = it*256 + (tid >> 1) = tap * NB + n: the iterations are a constant number of
    // taps apart, so one register holds the offset (channel block 0, iteration 0) and iteration, channel block and slice
    // ride in the scalar offset; the last iteration is live for the first rows only
    constexpr int B_TAPS_PER_IT = 256 / NB;
    // 16-bit operands: LDS row m = 32*j + r of a 64-row group holds weight row n = 2r + j, so MFMA column r of n-fragment j is
    // output channel 2r + j: a lane then holds two ADJACENT channels of each of its pixels, and the epilogue's LDS transpose
    // writes them as one dword (the 16-bit ds_write pairs it replaces were the epilogue's bound: 4 waves x 128 sub-dword LDS
    // writes per half tile, against the partner half's fragment reads).  The permutation is on the LOAD side -- thread m
    // fetches row n(m) and stores at LDS row m -- so the stores of a wave stay on consecutive rows (storing row n at its
    // permuted position put lanes 2k and 2k+1 1,024 bytes apart: two-way bank conflicts, SQ_LDS_BANK_CONFLICT 8 -> 19 % of
    // the LDS-active cycles); the fragment reads do not change.
    constexpr bool ILV = (C::ES == 2);
    const int b_m = (tid >> 1) % NB;
    const int b_n = ILV ? ((b_m & ~63) | ((b_m & 31) << 1) | ((b_m >> 5) & 1)) : b_m;
    const unsigned b_voff0 = (unsigned)(((int64_t)((tid >> 1) / NB) * p.npad + b_n) * 32 + cg * 16);
    const bool b_last_live = ((C::B_ITERS - 1) * 256 + (tid >> 1)) < 9 * NB;
    const unsigned b_voff_last = b_last_live ? b_voff0 : C::OOB;
    const unsigned b_it_bytes = (unsigned)(B_TAPS_PER_IT * p.npad * 32);
    const unsigned b_st = (unsigned)(P::B_BASE + (tid >> 1) * C::PSB + ((cg ^ ((tid >> 4) & 1)) * 16));
    const unsigned w_slice = (unsigned)p.npad * 32u * 9u;

    u32x4 areg[C::A_ITERS], breg[C::B_ITERS];
    float* tab = reinterpret_cast<float*>(smem + P::MAIN_BYTES);
    if (TF)
        for (int c = tid; c < p.K; c += 512) {
            tab[c] = p.in_scale[c];
            tab[C::MAX_K + c] = p.in_shift[c];
        }

    // load cursor: stream position pos_ld = item i_ld, slice s_ld; stops on the last position
    int pos_ld = 0, i_ld = 0, s_ld = 0;
    auto issue_loads = [&]() {
        const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(ximg), 0, (int)x_bytes, 0x00020000);
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) areg[it] = ig3_bload(rs_x, a_voff[it], (unsigned)(s_ld * 32));
        if (!WRES) {
#pragma unroll
            for (int it = 0; it < C::B_ITERS; ++it)
                breg[it] = ig3_bload(rs_w, it < C::B_ITERS - 1 ? b_voff0 : b_voff_last, (unsigned)s_ld * w_slice + n0off + it * b_it_bytes);
        }
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
    // what sits in areg / breg: slice index inside its tile and the tile's in-image flags
    int s_regs = 0;
    unsigned inb_regs = 0;
    auto store_regs = [&]() {
        const unsigned buf = (unsigned)(s_regs & 1) * P::A_STRIDE;   // nsl is even: stream parity == slice parity
        float sc[EPC], sh[EPC];
        float lo = 0.f;
        if (TF) {
            const int c0 = s_regs * C::KC + cg * EPC;
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
            if (it < C::A_ITERS - 1 || a_last_live) *reinterpret_cast<u32x4*>(smem + buf + a_st + it * (256 * C::PS)) = v;
        }
        if (!WRES) {
#pragma unroll
            for (int it = 0; it < C::B_ITERS; ++it)
                if (it < C::B_ITERS - 1 || b_last_live) *reinterpret_cast<u32x4*>(smem + buf + b_st + it * (256 * C::PSB)) = breg[it];
        }
    };
    // one stage phase: the slice in the registers goes to LDS, the cursor moves on, its loads go out
    auto stage_phase = [&]() {
        store_regs();
        advance();
        issue_loads();
        s_regs = s_ld;
        inb_regs = a_inb;
    };

    f32x16 acc[SW][2];
    auto zero_acc = [&]() {
        if constexpr (sizeof(elem_t) == 2) {
            // 0 x 0 + 0 on the matrix pipe: one issue slot per 16 registers instead of 16 v_mov in the epilogue's VALU stream
            u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < SW; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    asm volatile("" : "+v"(z));   // (opaque per tile, or the eight results are one MFMA and 112 copies)
                    f32x16 c;
#pragma unroll
                    for (int e = 0; e < 16; ++e) c[e] = 0.f;
                    TR::mma16(z, z, c);
                    acc[i][j] = c;
                }
        } else {
#pragma unroll
            for (int i = 0; i < SW; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        }
    };
    zero_acc();

    const unsigned a_frag = (unsigned)(((wrow * 2 * SW + pm_row(r)) * C::LW + wcol * 16 + pm_col(r)) * C::PS + h * 16);
    const unsigned b_frag = (unsigned)(P::B_BASE + (wn * 64 + r) * C::PSB + ((h ^ ((r >> 3) & 1)) * 16));

    // ``buf``: byte offset of the position's halo buffer; ``bufb``: of its weight rows (the same buffer, or slice s of the resident set)
    auto mfma_step = [&](unsigned buf, unsigned bufb) {
        u32x4 fa[2][SW], fb[2][2];
        auto rd = [&](int t, int set) {
            const unsigned ao = (unsigned)(((t / 3) * C::LW + (t % 3)) * C::PS);
            fa[set][0] = *reinterpret_cast<const u32x4*>(smem + buf + a_frag + ao);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[set][j] = *reinterpret_cast<const u32x4*>(smem + bufb + b_frag + t * C::B_TAP + j * (32 * C::PSB));
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

    // ---- epilogue of one item (this wave's (2*SW rows x 16 columns) x 64 channels), one 32-pixel strip at a time -------
    float* stat_lds = reinterpret_cast<float*>(smem + P::STAT_OFF);
#if defined(CMU_IG_STAMPS) && defined(CMU_IG_STAMPS_EPI)
    // diagnostic: stamps 4 / 5 / 6 of an iteration are taken INSIDE the epilogue (after the statistics, after unit 3, at the end)
    int epi_g = 0;
#define IG3P_STAMP_E(k_)                                                                                                   \
    do {                                                                                                                   \
        if ((blockIdx.x % 61 == 0 && blockIdx.x / 61 < 4) && epi_g >= nsl - 3 && epi_g < nsl - 3 + P::STAMP_ITERS && (tid & 255) == 0) \
            reinterpret_cast<unsigned long long*>(smem + P::STAMP_OFF)[((tid >> 8) * P::STAMP_ITERS + (epi_g - (nsl - 3))) * 8 + (k_)] = \
                __builtin_amdgcn_s_memtime();                                                                              \
    } while (0)
#else
#define IG3P_STAMP_E(k_) do {} while (0)
#endif
    const int row0 = wrow * 2 * SW, col0 = wcol * 16;
    constexpr int CPR = C::NFP * 32 / EPC;   // 16-byte chunks per staged pixel row (8)
    constexpr int NIT = (16 * CPR) / 64;     // chunks per lane and 16-pixel unit (2)
    // FULL (the tile lies inside the image -- every tile of the bench shapes): no bounds predicates, and a pixel's address
    // is a scalar base per (unit, chunk row) plus one of two per-lane offsets, instead of 64-bit VALU arithmetic per store
    auto epilogue_impl = [&](const Item t, auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        const int ty0 = t.ty * C::TH, tx0 = t.tx * C::TW;
        unsigned char* yb = reinterpret_cast<unsigned char*>(p.y);
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const int r = lane & 31, h = lane >> 5;
        unsigned char* my = smem + P::EPI_OFF + (wave & 3) * (2 * P::EPI_WAVE1);
        if (!BST && p.stats != nullptr) {
            float s1[2], s2[2];
            if constexpr (FULL) {
                ig3_lane_stats<SW>(acc, [](int, int) { return true; }, s1, s2);
            } else {
                ig3_lane_stats<SW>(acc, [&](int i, int e) {
                    const int m32 = (e & 3) + 8 * (e >> 2) + 4 * h;
                    return (ty0 + row0 + 2 * i + pm_row(m32) < p.H) && (tx0 + col0 + pm_col(m32) < p.W);
                }, s1, s2);
            }
            IG3P_STAMP_E(7);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                s1[j] += __shfl_xor(s1[j], 32, 64);
                s2[j] += __shfl_xor(s2[j], 32, 64);
                const int ch = ILV ? 2 * r + j : 32 * j + r;   // channel of (fragment j, column r) inside the wave's 64
                if (h == 0) {
                    stat_lds[(wave * 64 + ch) * 2 + 0] = s1[j];
                    stat_lds[(wave * 64 + ch) * 2 + 1] = s2[j];
                }
            }
        }
        IG3P_STAMP_E(4);
        // transposed read: lane -> pixel (lane >> 3) + 8*it of the 16-pixel unit, channel chunk q = lane % CPR
        const int q = lane % CPR;
        // FULL addressing.  Pixel m = 16*hs + 8*it + (lane >> 3) of strip i sits at row 2*i + (h ^ it ^ hs), column
        // 4*(2*hs + it) + ((lane >> 3) & 3) of the wave's block (pm_row / pm_col): scalar part + lane part
        const int64_t pix0 = ((int64_t)t.b * p.H + ty0 + row0) * p.W + tx0 + col0;
        const int cl = (lane >> 3) & 3;
        unsigned yoff[2], xoff[2];   // [row parity of the lane's pixel]
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            yoff[c] = (unsigned)((((h ^ c) * p.W + cl) * p.ldy + q * EPC) * C::ES);
            xoff[c] = BST ? (unsigned)((((h ^ c) * p.W + cl) * p.ldbx + q * EPC) * C::ES) : 0u;
        }
#pragma unroll
        for (int jp = 0; jp < 2 / C::NFP; ++jp) {
            const int n = t.n0 + wn * 64 + jp * C::NFP * 32 + q * EPC;
            const int nw = t.n0 + wn * 64 + jp * C::NFP * 32;   // scalar part of n
            unsigned char* ybase = yb + (pix0 * p.ldy + nw) * (int64_t)C::ES;
            const unsigned char* xbase = reinterpret_cast<const unsigned char*>(p.bx) + (pix0 * p.ldbx + nw) * (int64_t)C::ES;
            float bsc[EPC], bsh[EPC], bs1[EPC], bs2[EPC];
            if (BST) {
                ig3_bst_consts<EPC>(p.b_scale, p.b_shift, n, bsc, bsh);
#pragma unroll
                for (int e = 0; e < EPC; ++e) bs1[e] = bs2[e] = 0.f;
            }
            // units of 16 pixels (half an MFMA strip: accumulator elements 8*hs .. 8*hs+7); the producer layer's raw output
            // for unit u+1 is in flight while unit u goes through LDS
            auto load_x = [&](int u, u32x4* xr) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (FULL) {
                        const int soff = ((2 * (u >> 1)) * p.W + 4 * (2 * (u & 1) + it)) * (int)p.ldbx * C::ES;
                        xr[it] = ld_global16(xbase + soff + xoff[(it ^ u) & 1]);
                    } else {
                        const int m = 16 * (u & 1) + (it * 64 + lane) / CPR;
                        const int row = row0 + 2 * (u >> 1) + pm_row(m), col = col0 + pm_col(m);
                        const int gy = ty0 + row < p.H ? ty0 + row : p.H - 1, gx = tx0 + col < p.W ? tx0 + col : p.W - 1;  // clamped
                        const int64_t pixel = ((int64_t)t.b * p.H + gy) * p.W + gx;
                        xr[it] = ld_global16(reinterpret_cast<const unsigned char*>(p.bx) + (pixel * p.ldbx + n) * (int64_t)sizeof(elem_t));
                    }
                }
            };
            // a unit's accumulators -> the wave's LDS strip (u & 1): packed conversion, pixel-major rows
            auto write_unit = [&](int u) {
                const int i = u >> 1, hs = u & 1;
                unsigned char* st = my + (u & 1) * P::EPI_WAVE1;
                if constexpr (ILV) {
                    static_assert(C::NFP == 2, "both n-fragments of a 16-bit tile are staged in one pass");
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int ml = (e & 3) + 8 * (e >> 2) + 4 * h;   // row of the unit (0..15)
                        // channels 2r (low half) and 2r + 1 (high half) of pixel ml: one packed conversion, one dword
                        *reinterpret_cast<uint32_t*>(st + ml * C::EPI_ROW + r * 4) = TR::pack2(acc[i][0][8 * hs + e], acc[i][1][8 * hs + e]);
                    }
                } else
#pragma unroll
                for (int jj = 0; jj < C::NFP; ++jj)
#pragma unroll
                    for (int e8 = 0; e8 < 8; e8 += 2) {
                        const int ml = (e8 & 3) + 8 * (e8 >> 2) + 4 * h;   // row of the unit (0..15); element e8+1: row ml+1
                        const float va = acc[i][jp * C::NFP + jj][8 * hs + e8], vb = acc[i][jp * C::NFP + jj][8 * hs + e8 + 1];
                        unsigned char* d0 = st + ml * C::EPI_ROW + (32 * jj + r) * C::ES;
                        if constexpr (sizeof(elem_t) == 2) {
                            const uint32_t pk = TR::pack2(va, vb);   // one packed conversion, two 16-bit LDS writes (low / high half)
                            *reinterpret_cast<uint16_t*>(d0) = (uint16_t)pk;
                            *reinterpret_cast<uint16_t*>(d0 + C::EPI_ROW) = (uint16_t)(pk >> 16);
                        } else {
                            *reinterpret_cast<elem_t*>(d0) = TR::from_float(va);
                            *reinterpret_cast<elem_t*>(d0 + C::EPI_ROW) = TR::from_float(vb);
                        }
                    }
            };
            // (PART: tiles may overhang the image -- the addresses below stay valid formulas, a lane whose pixel lies outside skips
            // its store and its BN-backward terms; the statistics above mask the same pixels)
            u32x4 xr[2][NIT];
            if (BST) load_x(0, xr[0]);
            write_unit(0);
            // two strips per wave: unit u+1 is converted and written while unit u's transposed reads are in flight (the LDS
            // runs a wave's operations in order, so the reads only queue behind their own unit's writes) -- the unit-by-unit
            // form exposed write drain + read latency eight times per tile
#pragma unroll
            for (int u = 0; u < 2 * SW; ++u) {
                const int i = u >> 1, hs = u & 1;
                if (BST && u + 1 < 2 * SW) load_x(u + 1, xr[(u + 1) & 1]);
                __builtin_amdgcn_wave_barrier();
                u32x4 v[NIT];
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int ml = (it * 64 + lane) / CPR;
                    v[it] = *reinterpret_cast<const u32x4*>(my + (u & 1) * P::EPI_WAVE1 + ml * C::EPI_ROW + q * 16);
                }
                __builtin_amdgcn_sched_barrier(0);   // (or the scheduler sinks the reads behind the writes, next to their stores)
                if (u + 1 < 2 * SW) write_unit(u + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int soff = ((2 * i) * p.W + 4 * (2 * hs + it)) * (int)p.ldy * C::ES;
                    // streaming store: the output is not read by this kernel, and write-allocating it in L2 evicts halo
                    // and weight lines the neighbouring tiles are about to hit (+1 ... 3 % per layer)
                    bool inimg = true;
                    if constexpr (!FULL)
                        inimg = (ty0 + row0 + 2 * i + (h ^ ((it ^ hs) & 1)) < p.H) && (tx0 + col0 + 4 * (2 * hs + it) + cl < p.W);
                    if (inimg) {
                        st_global16_nt(ybase + soff + yoff[(it ^ hs) & 1], v[it]);
                        if (BST) ig3_bst_accum<TR>(v[it], xr[u & 1][it], bsc, bsh, bs1, bs2);
                    }
                }
                if (u == SW - 1) IG3P_STAMP_E(5);
            }
            IG3P_STAMP_E(6);
            __builtin_amdgcn_wave_barrier();
            if (BST) ig3_bst_fold<EPC>(bs1, bs2, lane, p.b_mean + nw, p.b_invstd + nw, stat_lds + (wave * 64 + jp * C::NFP * 32) * 2);
        }
    };
    // whole-tile shapes (H % 16 == 0, W % 32 == 0: every layer of the bench shapes) run the predicate-free form; PART is the
    // instantiation for every other shape (224 x 224 inputs: 112 / 56 / 28-pixel levels)
    auto epilogue = [&](const Item t) { epilogue_impl(t, std::integral_constant<bool, !PART>{}); };
    // per-wave channel partials in stat_lds -> one slab row per 16x16 half of the tile
    auto write_slab = [&](const Item t) {
        float* dst = BST ? p.bstats : p.stats;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        if (dst != nullptr && tid < TWB * THB * NB) {
            // one slab row per 16x16 block of the tile: (vhalf, half) = its row / column block; the waves of a block are the
            // RB / THB row bands of that vertical half
            const int blk = tid / NB, c = tid % NB;
            const int vhalf = blk / TWB, half = blk % TWB;
            const int tx16 = TWB * t.tx + half, tiles16 = (p.W + 15) / 16;
            if (tx16 < tiles16 && t.n0 + c < p.N) {
                float a = 0.f, q2 = 0.f;
#pragma unroll
                for (int wr = 0; wr < C::RB / THB; ++wr) {
                    const int wv = (c / 64) * C::WM + (vhalf * (C::RB / THB) + wr) * TWB + half;
                    a += stat_lds[(wv * 64 + (c & 63)) * 2 + 0];
                    q2 += stat_lds[(wv * 64 + (c & 63)) * 2 + 1];
                }
                const int64_t t16 = ((int64_t)t.b * (THB * p.tilesY) + THB * t.ty + vhalf) * tiles16 + tx16;
                dst[(t16 * 2 + 0) * p.N + t.n0 + c] = a;
                dst[(t16 * 2 + 1) * p.N + t.n0 + c] = q2;
            }
        }
    };

    // ---- prologue: (WRES) the whole weight pack into LDS; position 0 staged, position 1 in the registers -------------------
    if (WRES) {
#pragma unroll
        for (int s = 0; s < P::WRES_SLICES; ++s) {
            u32x4 wr[C::B_ITERS];
#pragma unroll
            for (int it = 0; it < C::B_ITERS; ++it)
                wr[it] = ig3_bload(rs_w, it < C::B_ITERS - 1 ? b_voff0 : b_voff_last, (unsigned)s * w_slice + it * b_it_bytes);
#pragma unroll
            for (int it = 0; it < C::B_ITERS; ++it)
                if (it < C::B_ITERS - 1 || b_last_live) *reinterpret_cast<u32x4*>(smem + s * C::B_BYTES + b_st + it * (256 * C::PSB)) = wr[it];
        }
    }
    set_load_tile(0);
    issue_loads();
    {
        u32x4 a0[C::A_ITERS], b0[C::B_ITERS];
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) a0[it] = areg[it];
        if (!WRES) {
#pragma unroll
            for (int it = 0; it < C::B_ITERS; ++it) b0[it] = breg[it];
        }
        advance();          // nsl >= 2: still item 0
        issue_loads();
        __syncthreads();    // the transform table is complete
        u32x4 a1[C::A_ITERS], b1[C::B_ITERS];
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) { a1[it] = areg[it]; areg[it] = a0[it]; }
        if (!WRES) {
#pragma unroll
            for (int it = 0; it < C::B_ITERS; ++it) { b1[it] = breg[it]; breg[it] = b0[it]; }
        }
        s_regs = 0;
        inb_regs = a_inb;
        store_regs();
#pragma unroll
        for (int it = 0; it < C::A_ITERS; ++it) areg[it] = a1[it];
        if (!WRES) {
#pragma unroll
            for (int it = 0; it < C::B_ITERS; ++it) breg[it] = b1[it];
        }
        s_regs = s_ld;
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);   // no prologue load may stay pending into the loop (conv_igemm3.inc header)
    __syncthreads();

    // ---- the stream: every wave runs [MFMAs of position g | its chunks of a later position: registers -> LDS (+ epilogue
    // at a tile's last slice), next loads], waves 4-7 (the SIMD partners of 0-3) one stage phase ahead -- and ONE barrier per
    // position: the first half takes it after its staging part, the second half after its MFMAs.  Between two barriers the
    // first half multiplies position g, then stages g+1; the second half stages g+1 (its part, from the registers it loaded
    // a position earlier), then multiplies g.  Why one is enough: position g's buffer is complete one barrier before
    // anybody reads it (the first half's part was stored before barrier g-1, the second half's a position earlier still),
    // and a buffer is rewritten only after the barrier that follows its last reader: the first half stores position g+1
    // into the buffer of g-1, whose readers finished before barrier g-1; the second half stores position g+2 into the buffer of
    // g after barrier g.  With the second barrier of round 1 (between a wave's MFMAs and its staging) every MFMA phase opened
    // behind a barrier round trip and the latency of its first fragment reads with the matrix pipe idle -- 460 of an
    // iteration's 5,580 cycles; now the partner's MFMAs run through them.
    const int second = wave >= 4 ? 1 : 0;   // waves 4-7 run one stage phase ahead
    if (second && 1 < G) stage_phase();
    int s_mma = 0, i_mma = 0;
#ifdef CMU_IG_STAMPS
    // diagnostic build: waves 0 and 4 of a few workgroups stamp s_memtime through LDS around the phases of 12 iterations
    // that straddle the first tile boundary (iterations nsl-3 ...)
    const int stamp_slot = (blockIdx.x % 61 == 0 && blockIdx.x / 61 < 4) ? (int)(blockIdx.x / 61) : -1;
    unsigned long long* stamp_lds = reinterpret_cast<unsigned long long*>(smem + P::STAMP_OFF);
    const int stamp_g0 = nsl - 3;
#define IG3P_STAMP(k_)                                                                                           \
    do {                                                                                                         \
        if (stamp_slot >= 0 && g >= stamp_g0 && g < stamp_g0 + P::STAMP_ITERS && (tid & 255) == 0)              \
            stamp_lds[((tid >> 8) * P::STAMP_ITERS + (g - stamp_g0)) * 8 + (k_)] = __builtin_amdgcn_s_memtime();  \
    } while (0)
#else
#define IG3P_STAMP(k_) do {} while (0)
#endif
#ifdef CMU_IG_STAMPS
    // shader clock under this load: delta s_memtime / delta s_memrealtime (100 MHz) around the stream
    unsigned long long clk0 = 0, rt0 = 0;
    if (stamp_slot >= 0 && tid == 0) { clk0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
#endif
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
        IG3P_STAMP(0);
        __builtin_amdgcn_s_setprio(2);
        if (WRES) mfma_step((unsigned)(g & 1) * P::A_STRIDE, (unsigned)s_mma * C::B_BYTES);
        else mfma_step((unsigned)(g & 1) * C::BUF_BYTES, (unsigned)(g & 1) * C::BUF_BYTES);
        __builtin_amdgcn_s_setprio(0);
        IG3P_STAMP(1);
        if (second) __syncthreads();
        IG3P_STAMP(2);
        // the staged registers are dead between their LDS store and the next loads: the epilogue sits there
        const bool staging = g + second + 1 < G;
        if (staging) store_regs();
        IG3P_STAMP(3);
        // the previous tile's slab rows: its second-half epilogues ran after the barrier of that tile's last position, i.e.
        // before the barrier that opened this iteration (the launcher sends nsl >= 4 here: the statistics strip is not
        // rewritten before this tile's last slice)
        if (s_mma == 1 && i_mma > 0) write_slab(decode(i_mma - 1));
        if (s_mma == nsl - 1) {
#if defined(CMU_IG_STAMPS) && defined(CMU_IG_STAMPS_EPI)
            epi_g = g;
#endif
            epilogue(decode(i_mma));
            zero_acc();
        }
#ifndef CMU_IG_STAMPS_EPI
        IG3P_STAMP(4);
#endif
        if (staging) {
            advance();
            issue_loads();
            s_regs = s_ld;
            inb_regs = a_inb;
        }
#ifndef CMU_IG_STAMPS_EPI
        IG3P_STAMP(5);
#endif
        if (++s_mma == nsl) {
            s_mma = 0;
            ++i_mma;
        }
        if (!second) __syncthreads();
#ifndef CMU_IG_STAMPS_EPI
        IG3P_STAMP(6);
#endif
    }
    __syncthreads();   // the second half's last staging part (its last epilogue) is done
#ifdef CMU_IG_STAMPS
    if (stamp_slot >= 0 && tid < 2 * P::STAMP_ITERS * 8) g_ig_stamps[stamp_slot * 256 + tid] = stamp_lds[tid];
    if (stamp_slot >= 0 && tid == 0) {
        g_ig_stamps[stamp_slot * 256 + 200] = __builtin_amdgcn_s_memtime() - clk0;
        g_ig_stamps[stamp_slot * 256 + 201] = __builtin_amdgcn_s_memrealtime() - rt0;
        g_ig_stamps[stamp_slot * 256 + 202] = (unsigned long long)G;
    }
#endif
    write_slab(decode(n_my - 1));
}

static int cmu_num_cus() {
    static int n[256] = {0};   // per device (the persistent grid is one workgroup per CU of the device launched on)
    const int dev = cmu_current_device() & 255;
    int v = __atomic_load_n(&n[dev], __ATOMIC_RELAXED);
    if (v == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        v = cus;
        __atomic_store_n(&n[dev], v, __ATOMIC_RELAXED);
    }
    return v;
}

template <class TR, int NB, bool TF, bool BST, int THB = 1, bool WRES = false, bool PART = false>
static int launch_igemm3p_cfg(IGParams p, hipStream_t st) {
    typedef IG3Cfg<TR, NB, 2, THB> C;
    typedef IG3PCfg<TR, NB, THB, WRES> P;
    static_assert(P::LDS_BYTES <= 163840, "LDS budget");
    constexpr const char* name = "cmu_conv3x3_fwd(wide, persistent)";
    p.tilesX = cmu_div_up(p.W, C::TW);
    p.tilesY = cmu_div_up(p.H, C::TH);
    p.nblk = p.N / NB;
    p.nslices32 = p.K / C::KC;
    p.nslices = p.nslices32;
    p.npad = cmu_conv3x3_npad(p.N);
    p.total_blocks = (int64_t)p.B * p.tilesX * p.tilesY * p.nblk;
    if (p.total_blocks >= (1ll << 30)) return launch_igemm3_cfg<TR, NB, TF, 2>(p, st);   // 32-bit item arithmetic in the kernel
    cmu_fastdiv_init((unsigned)p.nblk, p.fd_nblk);
    cmu_fastdiv_init((unsigned)p.tilesX, p.fd_tx);
    cmu_fastdiv_init((unsigned)p.tilesY, p.fd_ty);
    // CMU_CONV_PERSIST_GRID=n: test knob, forces n workgroups (long item lists per workgroup on small shapes)
    const int forced = cmu_knob(CMU_KNOB_CONV_PERSIST_GRID);
    const int64_t want = forced > 0 ? forced : cmu_num_cus();
    const int64_t grid = p.total_blocks < want ? p.total_blocks : want;
    if (int rc = cmu_launch_lds<&conv_igemm3p_kernel<TR, NB, TF, BST, THB, WRES, PART>>(dim3((unsigned)grid), dim3(512), P::LDS_BYTES, st, name, p)) return rc;
    cmu_set_kernel_tag("conv_igemm3p_kernel");
    CMU_CHECK_LAUNCH(name);
    return CMU_OK;
}

// CMU_CONV_PERSIST=0 keeps the one-tile-per-workgroup kernel (A/B switch)
static bool cmu_conv_persist_enabled() { return cmu_knob(CMU_KNOB_CONV_PERSIST); }
template <class TR> static bool igemm5_eligible(const IGParams& p);   // conv_igemm5.inc
template <class TR> static int launch_igemm5(const IGParams& p, hipStream_t st);
template <class TR> static bool igemm6_eligible(const IGParams& p);   // conv_igemm6.inc
template <class TR> static int launch_igemm6(const IGParams& p, hipStream_t st);
template <class TR>
static int launch_igemm3_any(const IGParams& p, hipStream_t st) {
    if (!cmu_conv_persist_enabled()) return launch_igemm3<TR>(p, st);
    if (igemm6_eligible<TR>(p)) return launch_igemm6<TR>(p, st);
    if (igemm5_eligible<TR>(p)) return launch_igemm5<TR>(p, st);
    const bool tf = p.in_scale != nullptr, bst = p.bstats != nullptr;
    if (tf && bst) return launch_igemm3<TR>(p, st);   // no entry asks for both; the one-tile kernel handles it
    if (p.K / (32 / (int)sizeof(typename TR::elem_t)) < 4) return launch_igemm3<TR>(p, st);   // fewer than four slices per tile (see the slab rows)
    if (p.H % 16 != 0 || p.W % 32 != 0) {
        // partial tiles: 16 x 16 pixel tiles where they pay (one-tile kernel), else the persistent kernel's predicated epilogue
        // (CMU_CONV_PERSIST_PART=0: the one-tile kernel, as before round 3's last session; read per launch for the tests)
        if (!igemm3_persist_part_enabled() || igemm3_slim_tiles(p, (int)sizeof(typename TR::elem_t))) return launch_igemm3<TR>(p, st);
        if (p.N % 128 == 0 && !igemm3_narrow_blocks(p))
            return tf ? launch_igemm3p_cfg<TR, 128, true, false, 1, false, true>(p, st)
                      : (bst ? launch_igemm3p_cfg<TR, 128, false, true, 1, false, true>(p, st) : launch_igemm3p_cfg<TR, 128, false, false, 1, false, true>(p, st));
        return tf ? launch_igemm3p_cfg<TR, 64, true, false, 1, false, true>(p, st)
                  : (bst ? launch_igemm3p_cfg<TR, 64, false, true, 1, false, true>(p, st) : launch_igemm3p_cfg<TR, 64, false, false, 1, false, true>(p, st));
    }
    if (p.N % 128 == 0 && !igemm3_narrow_blocks(p))
        return tf ? launch_igemm3p_cfg<TR, 128, true, false>(p, st)
                  : (bst ? launch_igemm3p_cfg<TR, 128, false, true>(p, st) : launch_igemm3p_cfg<TR, 128, false, false>(p, st));
    // 64 channels: a 16 x 32 tile gives a wave 36 MFMAs per phase against 5.25 staged chunks -- staging-bound.  A 32 x 32
    // pixel form (THB = 2: wave = 128 px x 64 ch, 72 MFMAs against 7.25 chunks) balanced the phases and shortened the main
    // loop by 15 % per output, but a pixel's 128-byte channel vector is read 32 bytes per K slice, and with 148 KB of halo per
    // CU the 32 CUs of an XCD outran its 4 MB L2 between two slices: PMC FETCH_SIZE of the three forward launches went from
    // 4.8 to 12.5 GB per step for +0 ... 3 % of speed.  Not instantiated any more (its LDS has no room for the second
    // epilogue strip).
    // 64 -> 64 at 16 bits (four slices, one channel block): the weight pack stays resident in LDS (IG3PCfg, WRES); CMU_CONV_WRES=0
    // keeps the streaming form (A/B switch)
    if constexpr (sizeof(typename TR::elem_t) == 2) {
        if (cmu_knob(CMU_KNOB_CONV_WRES) && p.N == 64 && p.K == 64)
            return tf ? launch_igemm3p_cfg<TR, 64, true, false, 1, true>(p, st)
                      : (bst ? launch_igemm3p_cfg<TR, 64, false, true, 1, true>(p, st) : launch_igemm3p_cfg<TR, 64, false, false, 1, true>(p, st));
    }
    return tf ? launch_igemm3p_cfg<TR, 64, true, false>(p, st)
              : (bst ? launch_igemm3p_cfg<TR, 64, false, true>(p, st) : launch_igemm3p_cfg<TR, 64, false, false>(p, st));
}
