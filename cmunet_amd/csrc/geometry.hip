// geometry.hip -- the reference's CPU geometry metrics (Finetuning/metrics.py:224-395: hausdorff_distance_mask, compute_radius_arteries,
// scikit-image find_contours / skeletonize + scipy KD-trees) as exact lattice geometry on the device.
//
// Doubled lattice of an H x W mask: (2H-1) x (2W-1) cells; pixel centres at (even, even), crossings (midpoints of two 4-neighbour
// pixels that differ) at (even, odd) and (odd, even).  Every distance between such points is sqrt(integer) / 2.
//   * contour points (cmu_contour_points): find_contours(mask > 0) returns every crossing once plus one repeat of the first point
//     of every closed contour.  Each crossing gets an oriented successor (marching squares, fully_connected='low': the segments of
//     a saddle square cut off its two foreground pixels); pointer jumping carries max(last-square index) around each contour and
//     marks contours that reach a border crossing as open.  The repeat of a closed contour is in its row-major-last square M:
//     M's left-edge crossing if M's top-left pixel is foreground, else its top-edge crossing.  Output: a lattice weight map
//     (0 / 1 / 2) and per image (crossings, closed contours).
//   * nearest distances (cmu_lattice_nearest): integer squared EDT seeded by a weight map (column pass, then a per-row
//     Felzenszwalb-Huttenlocher lower envelope with exact integer breakpoints), gathered at query points with their weights,
//     reduced per image in fp64 (sum w*d, sum w, max d, min d).
//   * thinning (cmu_skeletonize): scikit-image's _fast_skeletonize, one workgroup per image, bit-packed mask in LDS (two
//     buffers: each sub-iteration reads the state before it), until a round removes nothing.
#include "common.h"

namespace {

constexpr int GEOM_BIG = 0x7fffffff;

// scikit-image's thinning table (skimage/morphology/_skeletonize_cy.pyx, _fast_skeletonize; BSD-3-Clause, (c) the scikit-image
// team).  Index: the 8 neighbours, bit 0 = top-left, then clockwise; 1: removed in the first sub-iteration, 2: in the second, 3: both.
__constant__ unsigned char kThinLut[256] = {
    0, 0, 0, 1, 0, 0, 1, 3, 0, 0, 3, 1, 1, 0, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 2, 0, 3, 0, 3, 3,
    0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 3, 0, 2, 2,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    2, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 3, 0, 2, 0,
    0, 0, 3, 1, 0, 0, 1, 3, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1,
    3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    2, 3, 1, 3, 0, 0, 1, 3, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    2, 3, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 3, 3, 0, 1, 0, 0, 0, 0, 2, 2, 0, 0, 2, 0, 0, 0,
};

constexpr int SKEL_THREADS = 1024;
constexpr int SKEL_MAX_WORDS = 8192;          // 512 x 512 bits per buffer (32 KiB)
constexpr int ROW_THREADS = 64;               // cmu_lattice_nearest row pass: one thread per lattice row
constexpr int MAX_LW = 1023;                  // 2 * 512 - 1

inline int grid_for(int64_t n, int per) { return (int)(cmu_div_up64(n, per) < 4096 ? cmu_div_up64(n, per) : 4096); }

// ------------------------------------------------------------------------------------------------------------------------------
// binarisation
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void argmax2_mask_kernel(const T* __restrict__ x, uint8_t* __restrict__ m, int H, int W, int64_t total, int clear) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = o / HW, p = o % HW;
        const int r = (int)(p / W), c = (int)(p % W);
        uint8_t v = x[(b * 2 + 1) * HW + p] > x[(b * 2 + 0) * HW + p] ? 1 : 0;      // np.argmax: ties -> channel 0
        if (clear && (r == 0 || c == 0 || r == H - 1 || c == W - 1)) v = 0;
        m[o] = v;
    }
}

template <typename T>
__global__ void plane_mask_kernel(const T* __restrict__ x, int C, int ch, uint8_t* __restrict__ m, int H, int W, int64_t total, int clear) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = o / HW, p = o % HW;
        const int r = (int)(p / W), c = (int)(p % W);
        uint8_t v = x[(b * C + ch) * HW + p] > (T)0 ? 1 : 0;
        if (clear && (r == 0 || c == 0 || r == H - 1 || c == W - 1)) v = 0;
        m[o] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// contour points
// ------------------------------------------------------------------------------------------------------------------------------
// crossing slot s of an image <-> lattice cell t = 2s + 1 (the lattice width is odd, so odd t <=> i + j odd <=> a crossing slot)
__global__ void contour_init_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ wmap, int* __restrict__ J, int* __restrict__ A,
                                    int H, int W) {
    const int LH = 2 * H - 1, LW = 2 * W - 1;
    const int64_t NL = (int64_t)LH * LW, NS = (NL - 1) / 2;
    const int b = blockIdx.y;
    const uint8_t* m = mask + (int64_t)b * H * W;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < NL; t += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(t / LW), j = (int)(t % LW);
        if (((i + j) & 1) == 0) { wmap[(int64_t)b * NL + t] = 0; continue; }
        const int64_t s = (t - 1) >> 1;
        const bool horiz = (i & 1) == 0;
        const int r = i >> 1, c = j >> 1;
        bool cross, fg_lo;
        if (horiz) { const uint8_t l = m[(int64_t)r * W + c], rr = m[(int64_t)r * W + c + 1]; cross = l != rr; fg_lo = l != 0; }
        else { const uint8_t tp = m[(int64_t)r * W + c], bt = m[(int64_t)(r + 1) * W + c]; cross = tp != bt; fg_lo = bt != 0; }
        wmap[(int64_t)b * NL + t] = cross ? 1 : 0;
        int* Jb = J + (int64_t)b * NS;
        int* Ab = A + (int64_t)b * NS;
        if (!cross) { Jb[s] = -1; Ab[s] = GEOM_BIG; continue; }
        // heading square (sr, sc) and the edge it is entered by: 0 top, 1 bottom, 2 left, 3 right
        int sr, sc, ein;
        if (horiz) { sr = fg_lo ? r : r - 1; sc = c; ein = fg_lo ? 0 : 1; }
        else { sr = r; sc = fg_lo ? c : c - 1; ein = fg_lo ? 2 : 3; }
        const bool border = horiz ? (i == 0 || i == LH - 1) : (j == 0 || j == LW - 1);
        Ab[s] = border ? GEOM_BIG : (i >> 1) * (W - 1) + (j >> 1);
        if (sr < 0 || sr > H - 2 || sc < 0 || sc > W - 2) { Jb[s] = (int)s; continue; }   // open end: absorbing
        const bool a = m[(int64_t)sr * W + sc], bb = m[(int64_t)sr * W + sc + 1];
        const bool d = m[(int64_t)(sr + 1) * W + sc], e = m[(int64_t)(sr + 1) * W + sc + 1];
        const bool has[4] = {a != bb, d != e, a != d, bb != e};
        int other = 0;
        if (a == e && bb == d && a != bb) {          // saddle, fully_connected='low'
            const int pa[4] = {2, 3, 0, 1}, pb[4] = {3, 2, 1, 0};
            other = a ? pa[ein] : pb[ein];
        } else {
            for (int q = 0; q < 4; ++q)
                if (has[q] && q != ein) other = q;
        }
        int oi, oj;
        switch (other) {
            case 0: oi = 2 * sr; oj = 2 * sc + 1; break;
            case 1: oi = 2 * sr + 2; oj = 2 * sc + 1; break;
            case 2: oi = 2 * sr + 1; oj = 2 * sc; break;
            default: oi = 2 * sr + 1; oj = 2 * sc + 2; break;
        }
        Jb[s] = (int)((((int64_t)oi * LW + oj) - 1) >> 1);
    }
}

__global__ void contour_jump_kernel(const int* __restrict__ J, const int* __restrict__ A, int* __restrict__ J2, int* __restrict__ A2, int64_t NS) {
    const int64_t base = (int64_t)blockIdx.y * NS;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < NS; s += (int64_t)gridDim.x * blockDim.x) {
        const int n = J[base + s];
        if (n < 0) { J2[base + s] = -1; A2[base + s] = GEOM_BIG; continue; }
        const int an = A[base + n], a = A[base + s];
        A2[base + s] = a > an ? a : an;
        J2[base + s] = J[base + n];
    }
}

__global__ __launch_bounds__(256) void contour_final_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ J, const int* __restrict__ A,
                                                            uint8_t* __restrict__ wmap, int* __restrict__ counts, int H, int W) {
    const int LW = 2 * W - 1;
    const int64_t NL = (int64_t)(2 * H - 1) * LW, NS = (NL - 1) / 2;
    const int b = blockIdx.y;
    const uint8_t* m = mask + (int64_t)b * H * W;
    int nc = 0, nr = 0;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < NS; s += (int64_t)gridDim.x * blockDim.x) {
        if (J[(int64_t)b * NS + s] < 0) continue;
        ++nc;
        const int M = A[(int64_t)b * NS + s];
        if (M == GEOM_BIG) continue;
        const int mr = M / (W - 1), mc = M % (W - 1);
        const bool fg = m[(int64_t)mr * W + mc] != 0;
        const int64_t target = fg ? (int64_t)(2 * mr + 1) * LW + 2 * mc : (int64_t)(2 * mr) * LW + 2 * mc + 1;
        if (target == 2 * s + 1) { wmap[(int64_t)b * NL + target] = 2; ++nr; }
    }
    __shared__ int red[2][4];
    for (int o = 32; o > 0; o >>= 1) { nc += __shfl_down(nc, o); nr += __shfl_down(nr, o); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = nc; red[1][threadIdx.x >> 6] = nr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c0 = red[0][0] + red[0][1] + red[0][2] + red[0][3], c1 = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (c0) atomicAdd(&counts[2 * b], c0);
        if (c1) atomicAdd(&counts[2 * b + 1], c1);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// nearest distances on the lattice
// ------------------------------------------------------------------------------------------------------------------------------
// column pass: G[b][i][j] = (distance along column j to the nearest seed)^2, or GEOM_BIG when the column holds no seed
__global__ void edt_cols_kernel(const uint8_t* __restrict__ seeds, int* __restrict__ G, int LH, int LW) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= LW) return;
    const int64_t NL = (int64_t)LH * LW;
    const uint8_t* sd = seeds + (int64_t)blockIdx.y * NL + j;
    int* g = G + (int64_t)blockIdx.y * NL + j;
    int last = -(1 << 20);
    for (int i = 0; i < LH; ++i) {
        if (sd[(int64_t)i * LW]) last = i;
        g[(int64_t)i * LW] = i - last;                       // distance to the seed above (huge when none yet)
    }
    int next = 1 << 21;
    for (int i = LH - 1; i >= 0; --i) {
        if (sd[(int64_t)i * LW]) next = i;
        int d = g[(int64_t)i * LW];
        if (next - i < d) d = next - i;
        g[(int64_t)i * LW] = d >= (1 << 19) ? GEOM_BIG : d * d;
    }
}

__device__ __forceinline__ int64_t fh_num(int fq, int q, int fp, int p) { return ((int64_t)fq + (int64_t)q * q) - ((int64_t)fp + (int64_t)p * p); }

// row pass: one thread per lattice row; lower envelope of the parabolas g(q) + (j - q)^2 over the columns q with a seed
// (Felzenszwalb-Huttenlocher, breakpoints compared exactly in integers), evaluated at the row's query points.
// qmode 0: queries = lattice weight map (weights 1 / 2); 1: queries = an H x W pixel mask at the lattice points (2r, 2c).
__global__ __launch_bounds__(ROW_THREADS) void edt_rows_kernel(const int* __restrict__ G, const uint8_t* __restrict__ q, int qmode,
                                                               double* __restrict__ part, int H, int W, int B) {
    __shared__ short vstk[MAX_LW * ROW_THREADS];
    const int LH = 2 * H - 1, LW = 2 * W - 1;
    const int64_t row = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
    if (row >= (int64_t)B * LH) return;
    const int b = (int)(row / LH), i = (int)(row % LH);
    const int* g = G + (int64_t)b * LH * LW + (int64_t)i * LW;
    double* out = part + row * 4;
    // queries of this row
    auto weight = [&](int j) -> int {
        if (qmode == 0) return q[(int64_t)b * LH * LW + (int64_t)i * LW + j];
        if ((i | j) & 1) return 0;
        return q[(int64_t)b * H * W + (int64_t)(i >> 1) * W + (j >> 1)];
    };
    bool any = false;
    if (qmode == 0 || (i & 1) == 0)
        for (int j = 0; j < LW && !any; ++j) any = weight(j) != 0;
    if (!any) { out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0; return; }
    short* v = vstk + threadIdx.x;                 // v[k] at vstk[k * ROW_THREADS + lane]
#define V(k) v[(k) * ROW_THREADS]
    int k = -1;
    for (int qq = 0; qq < LW; ++qq) {
        const int fq = g[qq];
        if (fq == GEOM_BIG) continue;
        while (k >= 0) {
            // drop v[k] when the parabola of qq overtakes it no later than v[k] overtook v[k-1]
            const int p = V(k);
            if (k == 0) break;
            const int pp = V(k - 1);
            // s(p, qq) <= s(pp, p)  <=>  num(p,qq) * 2(p-pp) <= num(pp,p) * 2(qq-p)
            if (fh_num(fq, qq, g[p], p) * (int64_t)(p - pp) <= fh_num(g[p], p, g[pp], pp) * (int64_t)(qq - p)) --k;
            else break;
        }
        V(++k) = (short)qq;
    }
    if (k < 0) { out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0; return; }    // no seed in the image (the finish kernels decide)
    // k + 1 parabolas; walk j, advancing while the next parabola is lower at j: s(v[c], v[c+1]) < j
    double sw = 0.0, ww = 0.0, mx = 0.0, mn = 1e300;
    int c = 0;
    for (int j = 0; j < LW; ++j) {
        while (c < k) {
            const int p = V(c), n = V(c + 1);
            if (fh_num(g[n], n, g[p], p) < (int64_t)j * 2 * (n - p)) ++c;
            else break;
        }
        const int w = weight(j);
        if (!w) continue;
        const int p = V(c);
        const int64_t d2 = (int64_t)g[p] + (int64_t)(j - p) * (j - p);
        const double d = sqrt((double)d2) * 0.5;
        sw += w * d;
        ww += w;
        mx = d > mx ? d : mx;
        mn = d < mn ? d : mn;
    }
#undef V
    out[0] = sw; out[1] = ww; out[2] = mx; out[3] = mn;
}

// per image, fixed order: (sum w*d, sum w, max d, min d) over the LH row partials
__global__ __launch_bounds__(256) void edt_reduce_kernel(const double* __restrict__ part, double* __restrict__ out4, int LH) {
    __shared__ double red[4][256];
    const double* p = part + (int64_t)blockIdx.x * LH * 4;
    double s = 0.0, w = 0.0, mx = 0.0, mn = 1e300;
    for (int i = threadIdx.x; i < LH; i += 256) {
        const double pw = p[4 * i + 1];
        s += p[4 * i];
        w += pw;
        if (pw > 0) { mx = fmax(mx, p[4 * i + 2]); mn = fmin(mn, p[4 * i + 3]); }
    }
    red[0][threadIdx.x] = s; red[1][threadIdx.x] = w; red[2][threadIdx.x] = mx; red[3][threadIdx.x] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
            red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + o]);
            red[3][threadIdx.x] = fmin(red[3][threadIdx.x], red[3][threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = out4 + (int64_t)blockIdx.x * 4;
        o[0] = red[0][0]; o[1] = red[1][0]; o[2] = red[2][0]; o[3] = red[1][0] > 0 ? red[3][0] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// thinning
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t skel_window(const uint32_t* buf, int r, int k, int H, int WW) {
    // bits: [0] = column 32k-1, [1..32] = the word, [33] = column 32k+32
    if (r < 0 || r >= H) return 0ull;
    const uint32_t* row = buf + r * WW;
    const uint64_t lo = k > 0 ? (row[k - 1] >> 31) : 0u;
    const uint64_t hi = k + 1 < WW ? (row[k + 1] & 1u) : 0u;
    return lo | ((uint64_t)row[k] << 1) | (hi << 33);
}

__global__ __launch_bounds__(SKEL_THREADS) void skeletonize_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ skel, int H, int W) {
    __shared__ uint32_t buf[2][SKEL_MAX_WORDS];
    __shared__ unsigned char lut[256];
    __shared__ int flag;
    const int WW = (W + 31) >> 5, NW = H * WW;
    const uint8_t* m = mask + (int64_t)blockIdx.x * H * W;
    if (threadIdx.x < 256) lut[threadIdx.x] = kThinLut[threadIdx.x];
    for (int w = threadIdx.x; w < NW; w += SKEL_THREADS) {
        const int r = w / WW, c0 = (w % WW) * 32;
        uint32_t bits = 0;
        for (int t = 0; t < 32 && c0 + t < W; ++t) bits |= (m[(int64_t)r * W + c0 + t] ? 1u : 0u) << t;
        buf[0][w] = bits;
    }
    int cur = 0;
    __syncthreads();
    while (true) {
        if (threadIdx.x == 0) flag = 0;
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            const int want = pass + 1;
            int removed_any = 0;
            for (int w = threadIdx.x; w < NW; w += SKEL_THREADS) {
                const uint32_t center = buf[cur][w];
                if (!center) { buf[cur ^ 1][w] = 0; continue; }
                const int r = w / WW, k = w % WW;
                const uint64_t up = skel_window(buf[cur], r - 1, k, H, WW), mid = skel_window(buf[cur], r, k, H, WW),
                               dn = skel_window(buf[cur], r + 1, k, H, WW);
                uint32_t rm = 0, bitsleft = center;
                while (bitsleft) {
                    const int bpos = __builtin_ctz(bitsleft);
                    bitsleft &= bitsleft - 1;
                    const int idx = (int)((up >> bpos) & 1) | (int)(((up >> (bpos + 1)) & 1) << 1) | (int)(((up >> (bpos + 2)) & 1) << 2) |
                                    (int)(((mid >> (bpos + 2)) & 1) << 3) | (int)(((dn >> (bpos + 2)) & 1) << 4) |
                                    (int)(((dn >> (bpos + 1)) & 1) << 5) | (int)(((dn >> bpos) & 1) << 6) | (int)(((mid >> bpos) & 1) << 7);
                    const int v = lut[idx];
                    if (v == 3 || v == want) rm |= 1u << bpos;
                }
                buf[cur ^ 1][w] = center & ~rm;
                removed_any |= rm != 0;
            }
            if (removed_any) flag = 1;
            __syncthreads();
            cur ^= 1;
        }
        const int f = flag;
        __syncthreads();
        if (!f) break;
    }
    uint8_t* o = skel + (int64_t)blockIdx.x * H * W;
    for (int64_t p = threadIdx.x; p < (int64_t)H * W; p += SKEL_THREADS) {
        const int r = (int)(p / W), c = (int)(p % W);
        o[p] = (buf[cur][r * WW + (c >> 5)] >> (c & 31)) & 1u;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// per-image results
// ------------------------------------------------------------------------------------------------------------------------------
__global__ void hausdorff_finish_kernel(const int* __restrict__ cnt_a, const int* __restrict__ cnt_b, const double* __restrict__ fwd4,
                                        const double* __restrict__ bwd4, double* __restrict__ out_mod, double* __restrict__ out_std, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double inf = __builtin_huge_val();
    const bool ea = cnt_a[2 * b] == 0, eb = cnt_b[2 * b] == 0;
    if (ea || eb) {
        const double v = (ea && eb) ? 0.0 : inf;
        if (out_mod) out_mod[b] = v;
        if (out_std) out_std[b] = v;
        return;
    }
    const double* f = fwd4 + 4 * b;
    const double* g = bwd4 + 4 * b;
    if (out_mod) { const double mf = f[0] / f[1], mb = g[0] / g[1]; out_mod[b] = mf > mb ? mf : mb; }
    if (out_std) out_std[b] = f[2] > g[2] ? f[2] : g[2];
}

__global__ void radius_finish_kernel(const int* __restrict__ cnt, const double* __restrict__ near4, double* __restrict__ out3, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* o = out3 + 3 * b;
    const double* n = near4 + 4 * b;
    if (cnt[2 * b] == 0) { o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; return; }
    if (n[1] == 0.0) { const double nan = __builtin_nan(""); o[0] = nan; o[1] = nan; o[2] = nan; return; }   // empty skeleton
    o[0] = 2.0 * n[3]; o[1] = 2.0 * (n[0] / n[1]); o[2] = 2.0 * n[2];
}

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int cmu_argmax2_mask(const void* x, int is_f64, uint8_t* mask, int B, int H, int W, int clear_border, void* stream) {
    CMU_CHECK_ARG(x && mask && B > 0 && H > 0 && W > 0, "cmu_argmax2_mask: bad args");
    const int64_t total = (int64_t)B * H * W;
    if (is_f64)
        hipLaunchKernelGGL(argmax2_mask_kernel<double>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)x, mask, H, W, total, clear_border);
    else
        hipLaunchKernelGGL(argmax2_mask_kernel<float>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x, mask, H, W, total, clear_border);
    CMU_CHECK_LAUNCH("cmu_argmax2_mask");
    return CMU_OK;
}

extern "C" int cmu_plane_mask(const void* x, int is_f64, int C, int channel, uint8_t* mask, int B, int H, int W, int clear_border, void* stream) {
    CMU_CHECK_ARG(x && mask && B > 0 && H > 0 && W > 0 && C > 0 && channel >= 0 && channel < C, "cmu_plane_mask: bad args");
    const int64_t total = (int64_t)B * H * W;
    if (is_f64)
        hipLaunchKernelGGL(plane_mask_kernel<double>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)x, C, channel, mask, H, W, total, clear_border);
    else
        hipLaunchKernelGGL(plane_mask_kernel<float>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x, C, channel, mask, H, W, total, clear_border);
    CMU_CHECK_LAUNCH("cmu_plane_mask");
    return CMU_OK;
}

extern "C" int64_t cmu_contour_points_ws_bytes(int B, int H, int W) {
    const int64_t NS = ((int64_t)(2 * H - 1) * (2 * W - 1) - 1) / 2;
    return 4 * align256(NS * B * (int64_t)sizeof(int));
}

extern "C" int cmu_contour_points(const uint8_t* mask, uint8_t* wmap, int* counts, int B, int H, int W, void* ws, void* stream) {
    CMU_CHECK_ARG(mask && wmap && counts && ws && B > 0 && B <= 65535 && H > 0 && W > 0 && H <= 4096 && W <= 4096,
                  "cmu_contour_points: bad args (B <= 65535, H, W <= 4096)");
    hipStream_t st = (hipStream_t)stream;
    const int64_t NL = (int64_t)(2 * H - 1) * (2 * W - 1), NS = (NL - 1) / 2;
    if (hipMemsetAsync(counts, 0, sizeof(int) * 2 * (size_t)B, st) != hipSuccess) { cmu_set_error("cmu_contour_points: memset"); return CMU_ERR_LAUNCH; }
    if (NS == 0) {   // a 1 x 1 mask: no crossing slot
        if (hipMemsetAsync(wmap, 0, (size_t)B * NL, st) != hipSuccess) { cmu_set_error("cmu_contour_points: memset"); return CMU_ERR_LAUNCH; }
        return CMU_OK;
    }
    const int64_t slab = align256(NS * B * (int64_t)sizeof(int));
    int* J0 = (int*)ws;
    int* A0 = (int*)((char*)ws + slab);
    int* J1 = (int*)((char*)ws + 2 * slab);
    int* A1 = (int*)((char*)ws + 3 * slab);
    const int gx = (int)(cmu_div_up64(NL, 256) < 1024 ? cmu_div_up64(NL, 256) : 1024);
    hipLaunchKernelGGL(contour_init_kernel, dim3(gx, B), dim3(256), 0, st, mask, wmap, J0, A0, H, W);
    CMU_CHECK_LAUNCH("cmu_contour_points(init)");
    int rounds = 0;
    while (((int64_t)1 << rounds) < NS) ++rounds;
    const int gs = (int)(cmu_div_up64(NS, 256) < 1024 ? cmu_div_up64(NS, 256) : 1024);
    for (int k = 0; k < rounds; ++k) {
        hipLaunchKernelGGL(contour_jump_kernel, dim3(gs, B), dim3(256), 0, st, (const int*)J0, (const int*)A0, J1, A1, NS);
        CMU_CHECK_LAUNCH("cmu_contour_points(jump)");
        int* t = J0; J0 = J1; J1 = t;
        t = A0; A0 = A1; A1 = t;
    }
    hipLaunchKernelGGL(contour_final_kernel, dim3(gs, B), dim3(256), 0, st, mask, (const int*)J0, (const int*)A0, wmap, counts, H, W);
    CMU_CHECK_LAUNCH("cmu_contour_points(final)");
    return CMU_OK;
}

extern "C" int64_t cmu_lattice_nearest_ws_bytes(int B, int H, int W) {
    const int64_t LH = 2 * H - 1, LW = 2 * W - 1;
    return align256(B * LH * LW * (int64_t)sizeof(int)) + align256(B * LH * 4 * (int64_t)sizeof(double));
}

extern "C" int cmu_lattice_nearest(const uint8_t* seeds, const uint8_t* queries, int query_pixels, double* out4, int B, int H, int W,
                                   void* ws, void* stream) {
    CMU_CHECK_ARG(seeds && queries && out4 && ws && B > 0 && B <= 65535 && H > 0 && W > 0, "cmu_lattice_nearest: bad args");
    CMU_CHECK_ARG(2 * W - 1 <= MAX_LW, "cmu_lattice_nearest: W <= 512 (lattice rows of at most %d points; got W = %d)", MAX_LW, W);
    hipStream_t st = (hipStream_t)stream;
    const int LH = 2 * H - 1, LW = 2 * W - 1;
    int* G = (int*)ws;
    double* part = (double*)((char*)ws + align256((int64_t)B * LH * LW * (int64_t)sizeof(int)));
    hipLaunchKernelGGL(edt_cols_kernel, dim3((LW + 255) / 256, B), dim3(256), 0, st, seeds, G, LH, LW);
    CMU_CHECK_LAUNCH("cmu_lattice_nearest(cols)");
    const int64_t rows = (int64_t)B * LH;
    hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)cmu_div_up64(rows, ROW_THREADS)), dim3(ROW_THREADS), 0, st, (const int*)G, queries,
                       query_pixels, part, H, W, B);
    CMU_CHECK_LAUNCH("cmu_lattice_nearest(rows)");
    hipLaunchKernelGGL(edt_reduce_kernel, dim3(B), dim3(256), 0, st, (const double*)part, out4, LH);
    CMU_CHECK_LAUNCH("cmu_lattice_nearest(reduce)");
    return CMU_OK;
}

extern "C" int cmu_skeletonize(const uint8_t* mask, uint8_t* skel, int B, int H, int W, void* stream) {
    CMU_CHECK_ARG(mask && skel && B > 0 && H > 0 && W > 0, "cmu_skeletonize: bad args");
    const int64_t words = (int64_t)H * ((W + 31) / 32);
    CMU_CHECK_ARG(words <= SKEL_MAX_WORDS, "cmu_skeletonize: H * ceil(W / 32) * 32 <= 512 * 512 (one workgroup's LDS); got %d x %d", H, W);
    hipLaunchKernelGGL(skeletonize_kernel, dim3(B), dim3(SKEL_THREADS), 0, (hipStream_t)stream, mask, skel, H, W);
    CMU_CHECK_LAUNCH("cmu_skeletonize");
    return CMU_OK;
}

extern "C" int cmu_hausdorff_finish(const int* counts_a, const int* counts_b, const double* fwd4, const double* bwd4, double* out_modified,
                                    double* out_standard, int B, void* stream) {
    CMU_CHECK_ARG(counts_a && counts_b && fwd4 && bwd4 && (out_modified || out_standard) && B > 0, "cmu_hausdorff_finish: bad args");
    hipLaunchKernelGGL(hausdorff_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, counts_a, counts_b, fwd4, bwd4,
                       out_modified, out_standard, B);
    CMU_CHECK_LAUNCH("cmu_hausdorff_finish");
    return CMU_OK;
}

extern "C" int cmu_radius_finish(const int* counts, const double* near4, double* out3, int B, void* stream) {
    CMU_CHECK_ARG(counts && near4 && out3 && B > 0, "cmu_radius_finish: bad args");
    hipLaunchKernelGGL(radius_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, counts, near4, out3, B);
    CMU_CHECK_LAUNCH("cmu_radius_finish");
    return CMU_OK;
}
