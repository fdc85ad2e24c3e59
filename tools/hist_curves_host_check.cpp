// Stand-alone host program over csrc/hist_curves.h -- the very functions cmu_hist_curves calls -- for the host sanitizers
// (tests/test_cpu_prob_hist_ref.py builds it with -fsanitize=address,undefined and runs it; no GPU, no Python in the process).
//   hist_curves_host_check IN OUT
// IN : int32 jobs; per job int32 NB, select, nchunks; double eps, beta; int64 counts[2][NB+1]; uint64 conf[NB+1]
// OUT: per job int64 cum[4][NB+1]; double scores[5][NB+1]; double summary[6]
// The scan runs in nchunks chunks (as the kernel's lanes do) into buffers of exactly the documented sizes, and is compared here with a
// plain quadratic suffix sum; a mismatch is exit status 2.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmunet_amd/csrc/hist_curves.h"

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 64;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 65;
    int32_t jobs = 0;
    if (!rd(in, &jobs, 1)) return 66;
    for (int32_t q = 0; q < jobs; ++q) {
        int32_t hdr[3];
        double par[2];
        if (!rd(in, hdr, 3) || !rd(in, par, 2)) return 66;
        const int NB = hdr[0], select = hdr[1], nchunks = hdr[2], n = NB + 1;
        if (NB < 2 || NB > HC_MAX_BINS || nchunks < 1) return 67;
        std::vector<int64_t> counts(2 * (size_t)n), cum(4 * (size_t)n);
        std::vector<uint64_t> conf(n);
        std::vector<double> scores(HC_SCORES * (size_t)n), summary(HC_SUMMARY);
        if (!rd(in, counts.data(), counts.size()) || !rd(in, conf.data(), conf.size())) return 66;
        const int64_t* neg = counts.data();
        const int64_t* pos = counts.data() + n;
        // the kernel's order: chunk sums, the sum of the chunks above, then every chunk from the top down
        std::vector<int64_t> cp(nchunks), cn(nchunks);
        int64_t P = 0, N = 0;
        for (int c = 0; c < nchunks; ++c) {
            int lo, hi;
            hc_chunk_bounds(c, nchunks, n, &lo, &hi);
            cp[c] = cn[c] = 0;
            for (int i = lo; i < hi; ++i) {
                cp[c] += pos[i];
                cn[c] += neg[i];
            }
            P += cp[c];
            N += cn[c];
        }
        for (int c = 0; c < nchunks; ++c) {
            int lo, hi;
            hc_chunk_bounds(c, nchunks, n, &lo, &hi);
            int64_t tp = 0, tn = 0;
            for (int u = c + 1; u < nchunks; ++u) {
                tp += cp[u];
                tn += cn[u];
            }
            hc_scan_chunk(pos, neg, lo, hi, tp, tn, P, N, n, cum.data());
        }
        for (int j = 0; j < n; ++j) {
            int64_t tp = 0, fp = 0;
            for (int b = j + 1; b < n; ++b) {
                tp += pos[b];
                fp += neg[b];
            }
            if (cum[j] != tp || cum[n + j] != fp || cum[2 * n + j] != P - tp || cum[3 * n + j] != N - fp) {
                fprintf(stderr, "job %d: the chunked scan differs from the plain suffix sum at j = %d\n", (int)q, j);
                return 2;
            }
            double s[HC_SCORES];
            hc_scores(cum[j], cum[n + j], cum[2 * n + j], cum[3 * n + j], par[0], par[1], s);
            for (int k = 0; k < HC_SCORES; ++k) scores[(size_t)k * n + j] = s[k];
        }
        hc_summary(pos, neg, conf.data(), cum.data(), NB, par[0], par[1], select, summary.data());
        fwrite(cum.data(), sizeof(int64_t), cum.size(), out);
        fwrite(scores.data(), sizeof(double), scores.size(), out);
        fwrite(summary.data(), sizeof(double), summary.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 68;
    return 0;
}
