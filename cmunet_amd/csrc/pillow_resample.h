// pillow_resample.h -- Pillow's separable bicubic resampling weights (libImaging/Resample.c, a = -0.5), shared by the resize
// kernels of augment.hip and ft_augment.hip.  Per output index the window [int(c - s + .5), int(c + s + .5)) around
// c = (i + .5) * scale with s = 2 * max(scale, 1), Keys cubic weights normalised by their sum.  Every double operation is an
// explicit round-to-nearest mul / add / div; the including files are compiled with -ffp-contract=off (Makefile).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#pragma clang fp contract(off)

__device__ static inline double aug_cubic(double x) {
    // Pillow bicubic_filter with a = -0.5: ((a+2)x - (a+3))x^2 + 1 on [0,1), (((x-5)x + 8)x - 4)a on [1,2)
    x = fabs(x);
    if (x < 1.0) return __dadd_rn(__dmul_rn(__dmul_rn(__dadd_rn(__dmul_rn(1.5, x), -2.5), x), x), 1.0);
    if (x < 2.0) return __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(x, -5.0), x), 8.0), x), -4.0), -0.5);
    return 0.0;
}

struct AugWin {
    int xmin, count;
    double center, ss, ww;
};
// the window and the normalisation sum of output index xx for a resize in_size -> out_size
__device__ static inline AugWin aug_window(int xx, int in_size, int out_size) {
    AugWin w;
    const double scale = __ddiv_rn((double)in_size, (double)out_size);
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = __dmul_rn(2.0, filterscale);
    w.ss = __ddiv_rn(1.0, filterscale);
    w.center = __dmul_rn(__dadd_rn((double)xx, 0.5), scale);
    int xmin = (int)__dadd_rn(__dadd_rn(w.center, -support), 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)__dadd_rn(__dadd_rn(w.center, support), 0.5);
    if (xmax > in_size) xmax = in_size;
    w.xmin = xmin;
    w.count = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < w.count; ++x) ww = __dadd_rn(ww, aug_cubic(__dmul_rn(__dadd_rn(__dadd_rn((double)(x + xmin), -w.center), 0.5), w.ss)));
    w.ww = ww;
    return w;
}
__device__ static inline double aug_coeff(const AugWin& w, int x) {
    const double k = aug_cubic(__dmul_rn(__dadd_rn(__dadd_rn((double)(x + w.xmin), -w.center), 0.5), w.ss));
    return w.ww != 0.0 ? __ddiv_rn(k, w.ww) : k;
}
