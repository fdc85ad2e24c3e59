// edt_host_check.cpp -- the site rule, the row-pass search, the morphology select and the rank selection of
// cmunet_amd/csrc/edt_scan.h on the CPU: the same functions the kernels of csrc/edt.hip call, with the columns and rows visited
// serially.  Built and run by tests/test_cpu_edt_ref.py (g++ or hipcc, with the host sanitizers) before anything runs on a GPU.
//
//   edt_host_check IN OUT
// IN : int32 n; then per case int32 H, W, cls, border, t and H * W bytes (the map).
// OUT: per case H * W int32 dist2 (the program's two passes), H * W int32 brute-force dist2, H * W bytes dilation map
//      (dist2 <= t writes 1, sites keep their value) and H * W bytes erosion map (dist2 > t keeps, else 0; sites keep theirs),
//      then int32 n_values and for k = 0, n / 2, n - 1 the k-th smallest value by bisection and by sorting.
// The program itself compares its two passes with the brute force and the bisection with the sort: exit status 6 / 7 on a difference.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmunet_amd/csrc/edt_scan.h"

struct HostCount {
    const std::vector<int>* v;
    int64_t operator()(int x) {
        int64_t c = 0;
        for (int e : *v) c += e >= 0 && e <= x;
        return c;
    }
};

static void transform(const uint8_t* img, int cls, int border, int H, int W, std::vector<int>& d2) {
    std::vector<int> g((size_t)H * W);
    for (int x = 0; x < W; ++x) {      // edt_col_kernel
        int d = CMU_EDT_GINF;
        for (int y = 0; y < H; ++y) {
            d = cmu_edt_col_step(d, cmu_edt_site(img, y, x, H, W, cls, border));
            g[(size_t)y * W + x] = d;
        }
        d = CMU_EDT_GINF;
        for (int y = H - 1; y >= 0; --y) {
            const int down = g[(size_t)y * W + x];
            d = cmu_edt_col_step(d, down == 0);
            if (d < down) g[(size_t)y * W + x] = d;
        }
    }
    for (int y = 0; y < H; ++y) {      // edt_row_kernel: the row is copied, as the kernel copies it into LDS
        std::vector<int> row(g.begin() + (size_t)y * W, g.begin() + (size_t)(y + 1) * W);
        for (int x = 0; x < W; ++x) d2[(size_t)y * W + x] = cmu_edt_row_min(row.data(), x, W);
    }
}

static void brute(const uint8_t* img, int cls, int border, int H, int W, std::vector<int>& d2) {
    std::vector<int> sy, sx;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (cmu_edt_site(img, y, x, H, W, cls, border)) {
                sy.push_back(y);
                sx.push_back(x);
            }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            long best = -1;
            for (size_t k = 0; k < sy.size(); ++k) {
                const long c = (long)(y - sy[k]) * (y - sy[k]) + (long)(x - sx[k]) * (x - sx[k]);
                if (best < 0 || c < best) best = c;
            }
            d2[(size_t)y * W + x] = (int)best;
        }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
        return 2;
    }
    int n = 0;
    if (fread(&n, 4, 1, in) != 1 || n < 0) return 3;
    for (int c = 0; c < n; ++c) {
        int hdr[5];
        if (fread(hdr, 4, 5, in) != 5) return 3;
        const int H = hdr[0], W = hdr[1], cls = hdr[2], border = hdr[3], t = hdr[4];
        if (H < 1 || W < 1 || H > CMU_EDT_MAX_SIDE || W > CMU_EDT_MAX_SIDE || t < 0) return 3;
        std::vector<uint8_t> img((size_t)H * W);
        if (fread(img.data(), 1, img.size(), in) != img.size()) return 3;
        std::vector<int> d2(img.size()), ref(img.size());
        transform(img.data(), cls, border, H, W, d2);
        brute(img.data(), cls, border, H, W, ref);
        if (d2 != ref) {
            fprintf(stderr, "case %d (%d x %d, cls %d, border %d): the two passes differ from the brute force\n", c, H, W, cls, border);
            return 6;
        }
        std::vector<uint8_t> dil(img.size()), ero(img.size());
        for (size_t i = 0; i < img.size(); ++i) {
            dil[i] = (uint8_t)cmu_edt_select(d2[i], t, 0, img[i], 1, -1);
            ero[i] = (uint8_t)cmu_edt_select(d2[i], t, 1, img[i], -1, 0);
        }
        fwrite(d2.data(), 4, d2.size(), out);
        fwrite(ref.data(), 4, ref.size(), out);
        fwrite(dil.data(), 1, dil.size(), out);
        fwrite(ero.data(), 1, ero.size(), out);
        // rank selection over the non-negative values, with entries of -1 and -2 mixed in as the masked maps hold them
        std::vector<int> vals(d2);
        for (size_t i = 0; i < vals.size(); i += 3) vals[i] = CMU_EDT_NOT_BORDER;
        std::vector<int> sorted;
        for (int e : vals)
            if (e >= 0) sorted.push_back(e);
        std::sort(sorted.begin(), sorted.end());
        const int m = (int)sorted.size();
        fwrite(&m, 4, 1, out);
        HostCount count{&vals};
        const int top = m ? sorted.back() : -1;
        const long ks[3] = {0, m / 2, (long)m - 1};
        int prev = 0;
        for (long k : ks) {      // (ascending ranks: each search starts from the answer before it, as the kernel's second rank does)
            const int got = cmu_edt_kth(count, k, prev >= 0 ? prev : 0, top, (int64_t)m);
            const int want = k >= 0 && k < m ? sorted[(size_t)k] : -1;
            if (got != want || got != cmu_edt_kth(count, k, 0, (H - 1) * (H - 1) + (W - 1) * (W - 1), (int64_t)m)) {
                fprintf(stderr, "case %d: rank %ld: bisection %d, sort %d\n", c, k, got, want);
                return 7;
            }
            prev = got;
            fwrite(&got, 4, 1, out);
        }
        if (cmu_edt_kth(count, (int64_t)m, 0, top, (int64_t)m) != -1 || cmu_edt_kth(count, -1, 0, top, (int64_t)m) != -1) return 7;
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    // the sentinel: its square is above every real squared distance and the largest sum formed stays below 2^31
    const long side = CMU_EDT_MAX_SIDE - 1, ginf = CMU_EDT_GINF;
    if (!(ginf * ginf > 2 * side * side && ginf * ginf + side * side < (1l << 31) && ginf * ginf == CMU_EDT_D2INF)) return 5;
    printf("%d cases\n", n);
    return 0;
}
