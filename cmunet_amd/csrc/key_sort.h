// key_sort.h -- the index arithmetic and the partition search of the segmented 64-bit key sort (csrc/key_sort.hip: cmu_sort_u64) as
// __host__ __device__ functions, so that the very same code runs inside the kernels and in a stand-alone host program
// (tools/sort_host_check.cpp).  No HIP header is needed to include it.  DESIGN.md section 4.26.
//
// S segments of n keys each, ascending, every segment on its own:
//   tile sort   a segment is cut into tiles of CMU_KS_TILE keys (the last one shorter); a workgroup sorts one tile in LDS with the
//               bitonic network over the next power of two of the tile's count, the tail padded with CMU_KS_PAD (the largest key:
//               it sorts behind every real one, or beside an equal one, and is cut off again);
//   merge pass  sorted runs of `run` keys (run = CMU_KS_TILE << pass) become runs of 2 * run: a workgroup produces one output tile;
//               which part of the two runs feeds it is found by the merge-path search below, in global memory for the tile's two
//               ends and in LDS for each lane's CMU_KS_PER_LANE outputs.  A run without a partner is copied.
// A tile never crosses a segment: tiles are counted per segment.  Ties go to the left run; the keys are plain integers, so the sorted
// keys are the same whichever way ties go.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CMU_KS_HD __host__ __device__ static inline
#else
#define CMU_KS_HD static inline
#endif

constexpr int CMU_KS_TILE = 8192;                  // keys per tile: 64 KB of LDS
constexpr int CMU_KS_THREADS = 1024;               // lanes per workgroup
constexpr int CMU_KS_PER_LANE = CMU_KS_TILE / CMU_KS_THREADS;
constexpr uint64_t CMU_KS_PAD = ~0ull;

CMU_KS_HD int64_t cmu_ks_tiles(int64_t n) { return (n + CMU_KS_TILE - 1) / CMU_KS_TILE; }
// merge passes behind the tile sort: the smallest p with CMU_KS_TILE << p >= n
CMU_KS_HD int cmu_ks_passes(int64_t n) {
    int p = 0;
    for (int64_t run = CMU_KS_TILE; run < n; run *= 2) ++p;
    return p;
}
CMU_KS_HD int cmu_ks_tile_count(int64_t n, int64_t tile) {
    const int64_t left = n - tile * CMU_KS_TILE;
    return (int)(left < CMU_KS_TILE ? left : CMU_KS_TILE);
}
// the network's size for a tile of cnt keys: the next power of two (1 for a single key: no stage at all)
CMU_KS_HD int cmu_ks_pow2(int cnt) {
    int m = 1;
    while (m < cnt) m <<= 1;
    return m;
}

// Bitonic network over m = 2^k slots: for size = 2, 4, .., m and stride = size / 2, .., 1, compare-exchange q = 0 .. m / 2 - 1 takes
// the slots lo = cmu_ks_bitonic_lo(q, stride) and lo + stride, ascending iff (lo & size) == 0.
CMU_KS_HD int cmu_ks_bitonic_lo(int q, int stride) { return ((q & ~(stride - 1)) << 1) | (q & (stride - 1)); }
CMU_KS_HD void cmu_ks_compare_exchange(uint64_t& a, uint64_t& b, bool ascending) {
    if ((a > b) == ascending) {
        const uint64_t t = a;
        a = b;
        b = t;
    }
}

// The two runs behind output tile `tile` of a pass over runs of `run` keys in a segment of n keys: A = [a0, a0 + na), B = [a0 + na,
// a0 + na + nb) (nb = 0: A has no partner), both merged to [a0, ..); the tile's first output is number d0 of that merge.
struct CmuKsMerge {
    int64_t a0, na, nb, d0;
};
CMU_KS_HD CmuKsMerge cmu_ks_merge_geometry(int64_t n, int64_t run, int64_t tile) {
    CmuKsMerge g;
    const int64_t out0 = tile * CMU_KS_TILE;
    g.a0 = out0 / (2 * run) * (2 * run);
    g.na = n - g.a0 < run ? n - g.a0 : run;
    const int64_t left = n - g.a0 - g.na;
    g.nb = left < run ? left : run;
    g.d0 = out0 - g.a0;
    return g;
}
// Merge path: how many of the first d outputs of merge(a[0..na), b[0..nb)) come from a, ties to a; 0 <= d <= na + nb.  Every index
// read lies inside its run: mid < hi <= na, and d - 1 - mid < nb because mid >= lo >= d - nb.
CMU_KS_HD int64_t cmu_ks_merge_path(const uint64_t* a, int64_t na, const uint64_t* b, int64_t nb, int64_t d) {
    int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// one step of the serial merge: does the next output come from a?
CMU_KS_HD bool cmu_ks_take_a(bool has_a, bool has_b, uint64_t ka, uint64_t kb) { return has_a && (!has_b || ka <= kb); }
