// components_host_check.cpp -- the find / union / canonical-label logic of cmunet_amd/csrc/components_uf.h on the CPU: the same
// functions the kernels of csrc/components.hip call, with the 32 x 32 tiles visited serially and a plain int array behind the
// accessor.  Built and run by tests/test_cpu_components_ref.py (g++ or hipcc, with the host sanitizers) before anything runs on a GPU.
//
//   components_host_check IN OUT
// IN : int32 n; then per case int32 H, W, cls, connectivity and H * W bytes (the label map).
// OUT: per case int32 count (-1: a walk overran its trip bound) and H * W int32 labels.
// The pixels of a tile are visited in a scrambled order (stride 37 mod 1024) to show that the result does not depend on it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmunet_amd/csrc/components_uf.h"

struct HostParents {
    int* p;
    int load(int i) { return p[i]; }
    int fetch_min(int i, int v) {
        const int old = p[i];
        if (v < old) p[i] = v;
        return old;
    }
};

static int label_image(const uint8_t* img, int cls, int conn, int H, int W, std::vector<int>& labels) {
    constexpr int T = CMU_CC_TILE;
    std::vector<int> parent((size_t)H * W, -1);
    int over = 0;
    for (int y0 = 0; y0 < H; y0 += T)
        for (int x0 = 0; x0 < W; x0 += T) {      // cc_tile_kernel
            const int tw = W - x0 < T ? W - x0 : T, th = H - y0 < T ? H - y0 : T;
            int lp[T * T];
            uint8_t fg[T * T];
            for (int i = 0; i < T * T; ++i) {
                const int lx = i % T, ly = i / T;
                const bool f = lx < tw && ly < th && cmu_uf_foreground(img[(size_t)(y0 + ly) * W + x0 + lx], cls);
                fg[i] = f;
                lp[i] = f ? i : -1;
            }
            HostParents a{lp};
            for (int k = 0; k < T * T; ++k) {
                const int i = (int)(((long)k * 37 + 11) % (T * T));
                cmu_uf_tile_link(a, fg, i % T, i / T, tw, conn, &over);
            }
            for (int i = 0; i < T * T; ++i) {
                const int lx = i % T, ly = i / T;
                if (lx < tw && ly < th && fg[i]) {
                    const int r = cmu_uf_find(a, i, T * T, &over);
                    parent[(size_t)(y0 + ly) * W + x0 + lx] = (y0 + r / T) * W + x0 + r % T;
                }
            }
        }
    HostParents g{parent.data()};
    const long HW = (long)H * W;
    for (long k = 0; k < HW; ++k) {              // cc_seam_kernel, pixels in a scrambled order as well
        const long i = HW - 1 - k;
        cmu_uf_seam_link(g, img, cls, (int)(i % W), (int)(i / W), W, H, conn, &over);
    }
    int count = 0;
    for (long i = 0; i < HW; ++i) {              // cc_flatten_kernel
        int lab = 0;
        if (parent[i] >= 0) {
            const int r = cmu_uf_find(g, (int)i, (int)HW, &over);
            count += r == i;
            lab = r + 1;
        }
        labels[i] = lab;
    }
    return over ? -1 : count;
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
        int hdr[4];
        if (fread(hdr, 4, 4, in) != 4) return 3;
        const int H = hdr[0], W = hdr[1], cls = hdr[2], conn = hdr[3];
        if (H < 1 || W < 1 || (long)H * W >= (1l << 31) || (conn != 4 && conn != 8)) return 3;
        std::vector<uint8_t> img((size_t)H * W);
        if (fread(img.data(), 1, img.size(), in) != img.size()) return 3;
        std::vector<int> labels(img.size());
        const int count = label_image(img.data(), cls, conn, H, W, labels);
        fwrite(&count, 4, 1, out);
        fwrite(labels.data(), 4, labels.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    // the order of cmu_select_largest: larger size first, then the smaller index
    if (!(cmu_uf_rank_key(5, 9) > cmu_uf_rank_key(4, 0) && cmu_uf_rank_key(5, 3) > cmu_uf_rank_key(5, 4) && cmu_uf_rank_key(1, 0) > 0)) return 5;
    printf("%d cases\n", n);
    return 0;
}
