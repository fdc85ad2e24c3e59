// components_uf.h -- the find / union / canonical-label logic of csrc/components.hip as __host__ __device__ functions, so that the
// very same code runs inside the kernels (parent array behind agent-scope / workgroup-scope atomics) and in a stand-alone host
// program that visits the tiles serially (tools/components_host_check.cpp, plain ints).  No HIP header is needed to include it.
//
// Parent array convention: parent[i] <= i for every foreground pixel i (row-major index inside its image or its tile), -1 on
// background.  A root is an i with parent[i] == i.  A union only ever LOWERS a parent (atomic min), so
//   * parent[i] <= i holds for ever, hence the smallest index of a tree is its root: when all unions are done the root of a
//     component is its smallest row-major index, whatever the order of the unions -- label = root + 1 is canonical;
//   * any value ever read from parent[i], however stale, is an ancestor-or-self of i in the final forest that is <= i.
// ``A`` is an accessor with  int load(int i)  and  int fetch_min(int i, int v)  (returns the value before the min).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CMU_UF_HD __host__ __device__ static inline
#else
#define CMU_UF_HD static inline
#endif

constexpr int CMU_CC_TILE = 32;       // tiles of 32 x 32 pixels are labelled in LDS; seams lie at multiples of 32

// foreground rule of cmu_label_components: cls in 0..255: v == cls; cls == -1: v != 0; cls <= -2: v != (-cls - 2), the complement of
// class (-cls - 2) (what hole filling labels)
CMU_UF_HD bool cmu_uf_foreground(int v, int cls) { return cls >= 0 ? v == cls : (cls == -1 ? v != 0 : v != -cls - 2); }

// Root of x.  Every step goes to a strictly smaller index (parent[x] < x off the root), so the walk ends after at most ``limit``
// (= number of pixels) steps; the counter is a second, independent guard: on overrun *over is set and the walk stops.
template <class A>
CMU_UF_HD int cmu_uf_find(A& a, int x, int limit, int* over) {
    int steps = 0;
    int p = a.load(x);
    while (p != x) {
        if (p < 0 || p > x || ++steps > limit) {      // (p < 0 / p > x cannot happen on a foreground pixel; never follow them)
            *over = 1;
            break;
        }
        x = p;
        p = a.load(x);
    }
    return x;
}

// Merge the sets of x and y; the smaller root wins.  Loop: hi = the larger of the two supposed roots, lo the smaller;
// old = fetch_min(parent[hi], lo).
//   old == hi: hi really was a root and now hangs under lo: done.
//   old != hi: another union (or a stale read) got there first, hi hung under old < hi already.  parent[hi] is now min(old, lo);
//              whichever of the two lost that min is no longer linked through hi, so the pair (old, lo) still has to be merged:
//              continue with it.  A stale read therefore costs a trip, never a wrong merge: nothing is concluded from a load, only
//              from the value the atomic min returns.
// Termination: max(x, y) strictly decreases on every trip (old < hi and lo < hi) and is bounded below by 0, so there are at most
// ``limit`` trips; the counter is the independent guard (sets *over and leaves).
template <class A>
CMU_UF_HD void cmu_uf_union(A& a, int x, int y, int limit, int* over) {
    int trips = 0;
    for (;;) {
        x = cmu_uf_find(a, x, limit, over);
        y = cmu_uf_find(a, y, limit, over);
        if (x == y || *over) return;
        const int hi = x > y ? x : y, lo = x > y ? y : x;
        const int old = a.fetch_min(hi, lo);
        if (old == hi) return;
        if (old < 0 || old > hi || ++trips > limit) {
            *over = 1;
            return;
        }
        x = old;
        y = lo;
    }
}

// Step 1, per pixel (lx, ly) of a tw x th tile (tw, th <= 32) whose parent array ``a`` is indexed ly * 32 + lx: union with the
// already-visited neighbours W, N (and NW, NE for connectivity 8) INSIDE the tile.  fg[i] != 0 marks foreground.
template <class A>
CMU_UF_HD void cmu_uf_tile_link(A& a, const uint8_t* fg, int lx, int ly, int tw, int conn, int* over) {
    constexpr int T = CMU_CC_TILE, LIM = T * T;
    const int i = ly * T + lx;
    if (!fg[i]) return;
    if (lx > 0 && fg[i - 1]) cmu_uf_union(a, i, i - 1, LIM, over);
    if (ly > 0) {
        if (fg[i - T]) cmu_uf_union(a, i, i - T, LIM, over);
        if (conn == 8) {
            if (lx > 0 && fg[i - T - 1]) cmu_uf_union(a, i, i - T - 1, LIM, over);
            if (lx + 1 < tw && fg[i - T + 1]) cmu_uf_union(a, i, i - T + 1, LIM, over);
        }
    }
}

// Step 2, per pixel (x, y) of an H x W image whose parent array ``a`` is indexed y * W + x: union with those of the neighbours
// W, N (NW, NE) that lie in ANOTHER tile (the ones step 1 could not see).  img: the image's source bytes.
template <class A>
CMU_UF_HD void cmu_uf_seam_link(A& a, const uint8_t* img, int cls, int x, int y, int W, int H, int conn, int* over) {
    constexpr int T = CMU_CC_TILE;
    const int lx = x % T, ly = y % T;
    if (ly != 0 && lx != 0 && lx != T - 1) return;              // every neighbour looked at lies in the pixel's own tile
    const int i = y * W + x, limit = H * W;
    if (!cmu_uf_foreground(img[i], cls)) return;
    if (lx == 0 && x > 0 && cmu_uf_foreground(img[i - 1], cls)) cmu_uf_union(a, i, i - 1, limit, over);
    if (y > 0) {
        if (ly == 0 && cmu_uf_foreground(img[i - W], cls)) cmu_uf_union(a, i, i - W, limit, over);
        if (conn == 8) {
            if ((ly == 0 || lx == 0) && x > 0 && cmu_uf_foreground(img[i - W - 1], cls)) cmu_uf_union(a, i, i - W - 1, limit, over);
            if ((ly == 0 || lx == T - 1) && x + 1 < W && cmu_uf_foreground(img[i - W + 1], cls)) cmu_uf_union(a, i, i - W + 1, limit, over);
        }
    }
}

// order of cmu_select_largest: larger size first, ties to the smaller index; as ONE unsigned key whose maximum is the winner
CMU_UF_HD uint64_t cmu_uf_rank_key(int size, int index) { return ((uint64_t)(uint32_t)size << 32) | (uint64_t)(0xffffffffu - (uint32_t)index); }
