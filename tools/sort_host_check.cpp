// sort_host_check.cpp -- the segmented key sort of csrc/key_sort.hip restated on the host with the index arithmetic and the partition
// search of csrc/key_sort.h, the very functions the kernels call: every workgroup's tile and every lane's share visited serially.
// Built with the host sanitizers and run by tests/test_cpu_lovasz.py; also compares itself with std::sort.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/sort_host_check.cpp -o sort_host_check
//   sort_host_check in.bin out.bin
// in.bin:  int64 jobs, then per job int64 S, int64 n and S * n uint64 keys.  out.bin: per job the S * n sorted keys.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../cmunet_amd/csrc/key_sort.h"

// ks_tile_sort_kernel: one tile of a segment, in an "LDS" of its own
static void tile_sort(const uint64_t* in, uint64_t* out, int64_t n, int64_t tile) {
    const int cnt = cmu_ks_tile_count(n, tile), m = cmu_ks_pow2(cnt);
    const int64_t base = tile * CMU_KS_TILE;
    std::vector<uint64_t> s(m);
    for (int i = 0; i < m; ++i) s[i] = i < cnt ? in[base + i] : CMU_KS_PAD;
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1)
            for (int q = 0; q < (m >> 1); ++q) {
                const int lo = cmu_ks_bitonic_lo(q, stride);
                cmu_ks_compare_exchange(s[lo], s[lo + stride], (lo & size) == 0);
            }
    for (int i = 0; i < cnt; ++i) out[base + i] = s[i];
}

// ks_merge_kernel: one output tile; "lanes" 0 and 1 find its ends, every lane its own start and CMU_KS_PER_LANE outputs
static void merge_tile(const uint64_t* src, uint64_t* dst, int64_t n, int64_t run, int64_t tile) {
    const CmuKsMerge g = cmu_ks_merge_geometry(n, run, tile);
    const int cnt = cmu_ks_tile_count(n, tile);
    const uint64_t* A = src + g.a0;
    const uint64_t* B = A + g.na;
    const int64_t a_lo = cmu_ks_merge_path(A, g.na, B, g.nb, g.d0), a_hi = cmu_ks_merge_path(A, g.na, B, g.nb, g.d0 + cnt);
    const int64_t b_lo = g.d0 - a_lo;
    const int la = (int)(a_hi - a_lo), lb = cnt - la;
    std::vector<uint64_t> s(cnt), o(cnt);
    for (int i = 0; i < cnt; ++i) s[i] = i < la ? A[a_lo + i] : B[b_lo + (i - la)];
    for (int lane = 0; lane < CMU_KS_THREADS; ++lane) {
        const int d = std::min(lane * CMU_KS_PER_LANE, cnt);
        int ia = (int)cmu_ks_merge_path(s.data(), la, s.data() + la, lb, d), ib = d - ia;
        for (int i = 0; i < CMU_KS_PER_LANE && d + i < cnt; ++i) {
            const bool has_a = ia < la, has_b = ib < lb;
            if (cmu_ks_take_a(has_a, has_b, has_a ? s[ia] : 0, has_b ? s[la + ib] : 0)) o[d + i] = s[ia++];
            else o[d + i] = s[la + ib++];
        }
    }
    for (int i = 0; i < cnt; ++i) dst[tile * CMU_KS_TILE + i] = o[i];
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int64_t jobs = 0;
    if (fread(&jobs, 8, 1, fi) != 1) return 2;
    for (int64_t j = 0; j < jobs; ++j) {
        int64_t hdr[2];
        if (fread(hdr, 8, 2, fi) != 2 || hdr[0] <= 0 || hdr[1] <= 0) return 2;
        const int64_t S = hdr[0], n = hdr[1];
        std::vector<uint64_t> keys(S * n), out(S * n), scratch(S * n);
        if ((int64_t)fread(keys.data(), 8, S * n, fi) != S * n) return 2;
        const int64_t tiles = cmu_ks_tiles(n);
        const int passes = cmu_ks_passes(n);
        for (int64_t s = 0; s < S; ++s) {
            uint64_t* cur = (passes & 1) ? scratch.data() + s * n : out.data() + s * n;
            for (int64_t t = 0; t < tiles; ++t) tile_sort(keys.data() + s * n, cur, n, t);
            int64_t run = CMU_KS_TILE;
            for (int p = 0; p < passes; ++p, run *= 2) {
                uint64_t* nxt = cur == out.data() + s * n ? scratch.data() + s * n : out.data() + s * n;
                for (int64_t t = 0; t < tiles; ++t) merge_tile(cur, nxt, n, run, t);
                cur = nxt;
            }
            if (cur != out.data() + s * n) return 3;
            std::vector<uint64_t> want(keys.begin() + s * n, keys.begin() + (s + 1) * n);
            std::sort(want.begin(), want.end());
            if (!std::equal(want.begin(), want.end(), out.begin() + s * n)) {
                fprintf(stderr, "job %lld segment %lld: not std::sort's order\n", (long long)j, (long long)s);
                return 1;
            }
        }
        if ((int64_t)fwrite(out.data(), 8, S * n, fo) != S * n) return 2;
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 2;
}
