// map_loss_math.h -- the per-pixel arithmetic of csrc/map_loss.hip that a host program or a test may want to restate bit for bit, as
// __host__ __device__ functions: the modulating factor q^gamma of the focal loss and the two distance fields that cmu_distance_field
// derives from the integer squared distances of cmu_edt_rows.  No HIP header is needed to include it.  DESIGN.md section 4.25.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CMU_ML_HD __host__ __device__ static inline
#else
#define CMU_ML_HD static inline
#endif

// q^gamma for q in [0, 1] (fp64, a quotient of fp32 sums): exactly 1 for gamma = 0 (also at q = 0), by multiplication for gamma = 1
// and 2; otherwise ONE fp32 exp(gamma log q) on q rounded to fp32 (relative error about 2 U gamma |ln q| + 2 U), and 0 at q = 0.
CMU_ML_HD double cmu_ml_pow_gamma(double q, double gamma) {
    if (gamma == 0.0) return 1.0;
    if (gamma == 1.0) return q;
    if (gamma == 2.0) return q * q;
    const float qf = (float)q;
    return qf > 0.f ? (double)expf((float)gamma * logf(qf)) : 0.0;
}

// Signed distance of a pixel to the boundary of a set S (Kervadec et al., one_hot2dist): d2_to is the squared distance to S (0 on S),
// d2_from the squared distance to S's complement (0 outside S).  Outside S: sqrt(d2_to); inside: 1 - sqrt(d2_from); each formed in
// fp64 and rounded once.  An empty or a full S (either map holds -1, at every pixel of the image): 0.
CMU_ML_HD float cmu_ml_signed_field(int32_t d2_to, int32_t d2_from) {
    if (d2_to < 0 || d2_from < 0) return 0.f;
    return d2_to > 0 ? (float)sqrt((double)d2_to) : (float)(1.0 - sqrt((double)d2_from));
}

// Unsigned distance to the boundary to the power alpha (MONAI's HausdorffDTLoss.distance_field, raised): one of the two roots is 0 at
// every pixel, so the base is sqrt(d2) with d2 = d2_to + d2_from.  alpha = 2: the integer itself, converted once; alpha = 1: the
// fp64 root rounded once; otherwise ONE fp32 exp((alpha / 2) log d2), 0 at d2 = 0.  An empty or a full S: 0.
CMU_ML_HD float cmu_ml_unsigned_field(int32_t d2_to, int32_t d2_from, double alpha) {
    if (d2_to < 0 || d2_from < 0) return 0.f;
    const int32_t d2 = d2_to + d2_from;
    if (alpha == 2.0) return (float)d2;
    if (alpha == 1.0) return (float)sqrt((double)d2);
    return d2 > 0 ? expf((float)(0.5 * alpha) * logf((float)d2)) : 0.f;
}
