// hist_curves.h -- from the probability histogram of one (image or pool, class) row to its confusion counts at every threshold j / NB, the
// reference's scores there (Finetuning/metrics.py:135-198) and the threshold-free summaries, as plain functions that the kernel
// (prob_hist.hip: cmu_hist_curves) and a stand-alone host program (tools/hist_curves_host_check.cpp, built with the host sanitizers) both
// call.  n = NB + 1 bins; pos[b] / neg[b] = pixels of bin b with a positive / negative target; conf[b] = their sum of floor(p * 2^32).
// Every sum of doubles below runs over non-negative terms in ascending bin order; every expression is written as the reference's Python
// statement and is compiled without contraction (csrc/Makefile), so a score is the Python float's bits.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIP__
#define HC_FN __host__ __device__ static inline
#else
#define HC_FN static inline
#endif

constexpr int HC_MAX_BINS = 1024;
constexpr int HC_SCORES = 5;       // F-beta, IoU, precision, recall, specificity
constexpr int HC_SUMMARY = 6;      // AUROC, average precision, ECE, MCE, best j, the selected score at best j
constexpr int HC_SELECT_FBETA = 0, HC_SELECT_IOU = 1, HC_SELECT_YOUDEN = 2;

// bins [lo, hi) of chunk i when n bins are cut into nchunks runs of equal length (the last ones may be short or empty)
HC_FN void hc_chunk_bounds(int i, int nchunks, int n, int* lo, int* hi) {
    const int len = (n + nchunks - 1) / nchunks;
    const int a = i * len, b = a + len;
    *lo = a < n ? a : n;
    *hi = b < n ? b : n;
}

// the suffix scan over bins [lo, hi), from the top down: tail_pos / tail_neg are the sums over the bins >= hi, P / N the sums over all.
// cum (4, n): tp[j] = sum of pos over bins > j ("predicted positive at j / NB" is "bin > j"), fp[j] likewise of neg, fn = P - tp, tn = N - fp
HC_FN void hc_scan_chunk(const int64_t* pos, const int64_t* neg, int lo, int hi, int64_t tail_pos, int64_t tail_neg, int64_t P, int64_t N,
                         int n, int64_t* cum) {
    int64_t tp = tail_pos, fp = tail_neg;
    for (int j = hi - 1; j >= lo; --j) {
        cum[j] = tp;
        cum[n + j] = fp;
        cum[2 * n + j] = P - tp;
        cum[3 * n + j] = N - fp;
        tp += pos[j];
        fp += neg[j];
    }
}

// the five scores of one threshold, metrics.py:135-198: out[0] F-beta, [1] IoU, [2] precision, [3] recall, [4] specificity
HC_FN void hc_scores(int64_t tp_, int64_t fp_, int64_t fn_, int64_t tn_, double eps, double beta, double* out) {
    const double tp = (double)tp_, fp = (double)fp_, fn = (double)fn_, tn = (double)tn_;
    const double b2 = beta * beta;
    out[0] = ((1.0 + b2) * tp + eps) / ((1.0 + b2) * tp + b2 * fn + fp + eps);
    out[1] = (tp + eps) / (tp + fp + fn + eps);
    out[2] = (tp + eps) / (tp + fp + eps);
    out[3] = (tp + eps) / (tp + fn + eps);
    out[4] = (tn + eps) / (tn + fp + eps);
}

// the score best_j maximises: F-beta, IoU (both with eps, as above) or Youden's J = recall + specificity - 1 without eps (NaN when a
// class is empty)
HC_FN double hc_selected(int select, int64_t tp_, int64_t fp_, int64_t fn_, int64_t tn_, double eps, double beta) {
    const double tp = (double)tp_, fp = (double)fp_, fn = (double)fn_, tn = (double)tn_;
    if (select == HC_SELECT_YOUDEN) return tp / (tp + fn) + tn / (tn + fp) - 1.0;
    if (select == HC_SELECT_IOU) return (tp + eps) / (tp + fp + fn + eps);
    const double b2 = beta * beta;
    return ((1.0 + b2) * tp + eps) / ((1.0 + b2) * tp + b2 * fn + fp + eps);
}

// |pos - conf / 2^32| of one bin with ONE rounding: the difference is formed in integers (conf = hi * 2^32 + lo), never as the difference
// of two nearly equal doubles.  Counts below 2^52.
HC_FN double hc_gap(int64_t pos, uint64_t conf) {
    const int64_t d = pos - (int64_t)(conf >> 32);
    const double lo = (double)(conf & 0xffffffffull);
    const double two32 = 4294967296.0;
    // d * 2^32 - lo: for d > 0 it is (d - 1) * 2^32 + (2^32 - lo), else its magnitude is (-d) * 2^32 + lo -- sums of non-negative exact parts
    const double v = d > 0 ? (double)(d - 1) * two32 + (two32 - lo) : (double)(-d) * two32 + lo;
    return v / two32;
}

// summary[6] of one row: AUROC, average precision, ECE, MCE, best j, the selected score there.  conf may be null (ECE = MCE = NaN).
HC_FN void hc_summary(const int64_t* pos, const int64_t* neg, const uint64_t* conf, const int64_t* cum, int NB, double eps, double beta,
                      int select, double* summary) {
    const int n = NB + 1;
    const double nan = (double)NAN;
    const int64_t P = cum[0] + pos[0], N = cum[n] + neg[0];
    double auc = 0.0, ap = 0.0, ece = 0.0, mce = 0.0;
    for (int b = 0; b < n; ++b) {
        // trapezoid over the NB + 2 operating points: a negative of bin b is outranked by the positives above it, and ties with half of its own
        auc += (double)neg[b] * ((double)cum[b] + 0.5 * (double)pos[b]);
        // sum (R_i - R_{i+1}) * Prec_i: predicting "bin >= b" gains pos[b] / P of recall at precision tp / (tp + fp) of that point
        if (pos[b] > 0) {
            const double tp = (double)(cum[b] + pos[b]);
            ap += (double)pos[b] * (tp / (tp + (double)(cum[n + b] + neg[b])));
        }
        if (conf) {
            const double gap = hc_gap(pos[b], conf[b]);
            ece += gap;
            const int64_t cnt = pos[b] + neg[b];
            if (cnt > 0) {
                const double g = gap / (double)cnt;
                mce = g > mce ? g : mce;
            }
        }
    }
    summary[0] = (P > 0 && N > 0) ? auc / ((double)P * (double)N) : nan;
    summary[1] = P > 0 ? ap / (double)P : nan;
    summary[2] = (conf && P + N > 0) ? ece / (double)(P + N) : nan;
    summary[3] = (conf && P + N > 0) ? mce : nan;
    int best = 1;
    double best_s = hc_selected(select, cum[1], cum[n + 1], cum[2 * n + 1], cum[3 * n + 1], eps, beta);
    for (int j = 2; j < NB; ++j) {
        const double s = hc_selected(select, cum[j], cum[n + j], cum[2 * n + j], cum[3 * n + j], eps, beta);
        if (s > best_s) {      // the first maximum wins a tie; a NaN never replaces anything
            best_s = s;
            best = j;
        }
    }
    summary[4] = (double)best;
    summary[5] = best_s;
}
