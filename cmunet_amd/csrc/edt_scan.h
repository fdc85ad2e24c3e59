// edt_scan.h -- the site rule, the row-pass search, the morphology select and the rank selection of csrc/edt.hip as
// __host__ __device__ functions, so that the very same code runs inside the kernels and in a stand-alone host program
// (tools/edt_host_check.cpp).  No HIP header is needed to include it.  DESIGN.md section 4.23.
//
// Two separable passes give the exact squared Euclidean distance to the nearest site:
//   column pass  g(y, x)  = min over sites (y', x) of the pixel's own column of |y - y'|, CMU_EDT_GINF if the column has none;
//   row pass     d2(y, x) = min over x' of (x - x')^2 + g(y, x')^2.
// Everything is an int32: with H, W <= CMU_EDT_MAX_SIDE = 4096 a real squared distance is at most 2 * 4095^2 = 33 538 050 < 2^25, the
// sentinel's square is 2^28 -- above every real value, so it never wins the minimum against a site -- and the largest sum formed,
// 4095^2 + 2^28, is below 2^31.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CMU_EDT_HD __host__ __device__ static inline
#else
#define CMU_EDT_HD static inline
#endif

constexpr int CMU_EDT_MAX_SIDE = 4096;
constexpr int CMU_EDT_GINF = 1 << 14;                              // "no site in this column"
constexpr int CMU_EDT_D2INF = CMU_EDT_GINF * CMU_EDT_GINF;         // 2^28: a row minimum at or above it means "no site in the image's row band"
constexpr int CMU_EDT_NOT_BORDER = -2;                             // masked distance maps: the pixel is no border pixel (-1: infinitely far)

// the site rule, the codes of cmu_label_components: cls in 0..255: v == cls; -1: v != 0; -2 - c: v != c
CMU_EDT_HD bool cmu_edt_rule(int v, int cls) { return cls >= 0 ? v == cls : (cls == -1 ? v != 0 : v != -cls - 2); }

// Is pixel (y, x) of the H x W image a site?  border == 0: the rule itself.  border != 0: the rule's set minus its 4-erosion
// (outside the image counts as not in the set): a pixel of the set with a 4-neighbour that is outside the set or outside the image.
CMU_EDT_HD bool cmu_edt_site(const uint8_t* img, int y, int x, int H, int W, int cls, int border) {
    const int64_t i = (int64_t)y * W + x;
    if (!cmu_edt_rule(img[i], cls)) return false;
    if (!border) return true;
    if (y == 0 || x == 0 || y == H - 1 || x == W - 1) return true;
    return !(cmu_edt_rule(img[i - W], cls) && cmu_edt_rule(img[i + W], cls) && cmu_edt_rule(img[i - 1], cls) && cmu_edt_rule(img[i + 1], cls));
}

// one step of a column sweep: the distance to the nearest site met so far, saturating at the sentinel
CMU_EDT_HD int cmu_edt_col_step(int d, bool site) { return site ? 0 : (d + 1 < CMU_EDT_GINF ? d + 1 : CMU_EDT_GINF); }

// Row pass for pixel x of a row whose column distances are g[0..W): a scan outwards from x.  At step d both candidates cost at least
// d^2, so the scan stops once d^2 reaches the best value so far: exact, and at most W - 1 trips.  Returns the squared distance, or
// -1 if no column of the row holds a site (then no column of the image does: every g of a column is the sentinel or none is).
CMU_EDT_HD int cmu_edt_row_min(const int* g, int x, int W) {
    const int g0 = g[x];
    int best = g0 * g0;
    for (int d = 1; d < W; ++d) {
        const int dd = d * d;
        const int xl = x - d, xr = x + d;
        if (dd >= best || (xl < 0 && xr >= W)) break;
        if (xl >= 0) {
            const int v = g[xl], c = dd + v * v;
            best = c < best ? c : best;
        }
        if (xr < W) {
            const int v = g[xr], c = dd + v * v;
            best = c < best ? c : best;
        }
    }
    return best >= CMU_EDT_D2INF ? -1 : best;
}

// The fused morphology output of the row pass.  A site (d2 == 0) keeps ``base``.  Any other pixel is a hit if
//   gt == 0:  d2 <= t           (inside the dilation of the sites by the disk of squared radius t)
//   gt != 0:  d2 > t            (survives the erosion by that disk; the sites are the pixels outside the set)
// with d2 == -1 (no site at all) counting as infinitely far.  A hit writes v_hit, a miss v_miss; a negative value means ``base``.
CMU_EDT_HD int cmu_edt_select(int d2, int t, int gt, int base, int v_hit, int v_miss) {
    if (d2 == 0) return base;
    const bool hit = gt ? (d2 < 0 || d2 > t) : (d2 > 0 && d2 <= t);
    const int v = hit ? v_hit : v_miss;
    return v < 0 ? base : v;
}

// Exact rank selection over integers in [lo, hi]: the k-th smallest (k from 0) of ``total`` elements, by bisection on the VALUE.
// ``count(v)`` returns how many elements are <= v (negative elements are never counted); the caller knows that no element exceeds hi
// (their maximum, or any bound on it) and that the answer is not below lo (0, or the answer for a smaller rank).  Returns -1 if fewer than
// k + 1 elements exist.  The smallest v with count(v) > k is the answer; the interval halves on every trip: at most 32 trips.
template <class C>
CMU_EDT_HD int cmu_edt_kth(C& count, int64_t k, int lo, int hi, int64_t total) {
    if (k < 0 || k >= total || hi < lo) return -1;
    for (int trip = 0; trip < 32 && lo < hi; ++trip) {
        const int mid = lo + (hi - lo) / 2;
        if (count(mid) > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
