// key_sort.hip -- cmu_sort_u64: a segmented ascending sort of 64-bit keys (no reference counterpart).  The
// tile sort and the merge passes are stated in key_sort.h, whose index arithmetic and partition search these kernels call; the same
// functions run serially in tools/sort_host_check.cpp.  One launch for the tile sort and one per merge pass, cmu_ks_passes(n) of
// them: the launch count depends on (S, n) alone.  No atomics, no host synchronisation; keys move, nothing is ever added: the result
// is the same on every call.
#include "common.h"
#include "key_sort.h"

// One tile per workgroup.  in and out may be the same buffer: a workgroup reads its tile into LDS before it writes the same slots.
__global__ __launch_bounds__(CMU_KS_THREADS) void ks_tile_sort_kernel(const uint64_t* in, uint64_t* out, int64_t n, int64_t tiles) {
    __shared__ uint64_t s[CMU_KS_TILE];
    const int64_t seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
    const int64_t base = seg * n + tile * CMU_KS_TILE;
    const int cnt = cmu_ks_tile_count(n, tile), m = cmu_ks_pow2(cnt);
    for (int i = threadIdx.x; i < m; i += CMU_KS_THREADS) s[i] = i < cnt ? in[base + i] : CMU_KS_PAD;
    __syncthreads();
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int q = threadIdx.x; q < (m >> 1); q += CMU_KS_THREADS) {
                const int lo = cmu_ks_bitonic_lo(q, stride);
                uint64_t a = s[lo], b = s[lo + stride];
                cmu_ks_compare_exchange(a, b, (lo & size) == 0);
                s[lo] = a;
                s[lo + stride] = b;
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < cnt; i += CMU_KS_THREADS) out[base + i] = s[i];
}

// One output tile per workgroup: lanes 0 and 1 search the tile's two ends in global memory, the cnt keys between them come into LDS
// (A's part, then B's), every lane finds its own start in LDS and merges CMU_KS_PER_LANE keys into registers; the tile goes back
// through LDS so that the store is coalesced.
__global__ __launch_bounds__(CMU_KS_THREADS) void ks_merge_kernel(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, int64_t n,
                                                                  int64_t run, int64_t tiles) {
    __shared__ uint64_t s[CMU_KS_TILE];             // (all 64 KB of a static allocation: the two ends pass through its first slots)
    const int64_t seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
    const CmuKsMerge g = cmu_ks_merge_geometry(n, run, tile);
    const int cnt = cmu_ks_tile_count(n, tile);
    const uint64_t* A = src + seg * n + g.a0;
    const uint64_t* B = A + g.na;
    if (threadIdx.x < 2) s[threadIdx.x] = (uint64_t)cmu_ks_merge_path(A, g.na, B, g.nb, g.d0 + (int64_t)threadIdx.x * cnt);
    __syncthreads();
    const int64_t a_lo = (int64_t)s[0], b_lo = g.d0 - a_lo;
    const int la = (int)((int64_t)s[1] - a_lo), lb = cnt - la;
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += CMU_KS_THREADS) s[i] = i < la ? A[a_lo + i] : B[b_lo + (i - la)];
    __syncthreads();
    const int d = min((int)threadIdx.x * CMU_KS_PER_LANE, cnt);
    int ia = (int)cmu_ks_merge_path(s, la, s + la, lb, d), ib = d - ia;
    uint64_t r[CMU_KS_PER_LANE];
    uint64_t ka = ia < la ? s[ia] : 0, kb = ib < lb ? s[la + ib] : 0;
#pragma unroll
    for (int i = 0; i < CMU_KS_PER_LANE; ++i) {
        const bool has_a = ia < la, has_b = ib < lb;
        if (cmu_ks_take_a(has_a, has_b, ka, kb)) {
            r[i] = ka;
            ++ia;
            ka = ia < la ? s[ia] : 0;
        } else {
            r[i] = kb;                  // (past both ends: a value that is not stored)
            ++ib;
            kb = ib < lb ? s[la + ib] : 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CMU_KS_PER_LANE; ++i)
        if (d + i < cnt) s[d + i] = r[i];
    __syncthreads();
    uint64_t* o = dst + seg * n + tile * CMU_KS_TILE;
    for (int i = threadIdx.x; i < cnt; i += CMU_KS_THREADS) o[i] = s[i];
}

extern "C" int cmu_sort_tile_keys(void) { return CMU_KS_TILE; }

extern "C" int cmu_sort_u64(const uint64_t* keys, uint64_t* out, uint64_t* scratch, int64_t S, int64_t n, void* stream) {
    CMU_CHECK_ARG(keys && out && S > 0 && n > 0, "cmu_sort_u64: bad args");
    CMU_CHECK_ARG(out != keys && out != scratch, "cmu_sort_u64: out is a buffer of its own");
    const int64_t tiles = cmu_ks_tiles(n);
    const int passes = cmu_ks_passes(n);
    CMU_CHECK_ARG(n < (int64_t(1) << 40) && S < (int64_t(1) << 31) && S * tiles < (int64_t(1) << 31),
                  "cmu_sort_u64: S * ceil(n / %d) workgroups must stay below 2^31 (S = %lld, n = %lld)", CMU_KS_TILE, (long long)S, (long long)n);
    CMU_CHECK_ARG(passes == 0 || scratch, "cmu_sort_u64: n = %lld > %d keys per segment needs the scratch buffer", (long long)n, CMU_KS_TILE);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(S * tiles)), block(CMU_KS_THREADS);
    // the tile sort writes where an even number of passes ends in out
    uint64_t* cur = (passes & 1) ? scratch : out;
    hipLaunchKernelGGL(ks_tile_sort_kernel, grid, block, 0, st, keys, cur, n, tiles);
    CMU_CHECK_LAUNCH("cmu_sort_u64(tile sort)");
    int64_t run = CMU_KS_TILE;
    for (int p = 0; p < passes; ++p, run *= 2) {
        uint64_t* nxt = cur == out ? scratch : out;
        hipLaunchKernelGGL(ks_merge_kernel, grid, block, 0, st, (const uint64_t*)cur, nxt, n, run, tiles);
        CMU_CHECK_LAUNCH("cmu_sort_u64(merge)");
        cur = nxt;
    }
    return CMU_OK;
}
