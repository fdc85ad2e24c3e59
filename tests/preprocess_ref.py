"""Numpy-only float64 restatement of cmunet_amd.preprocess (csrc/preprocess.hip): what every kernel is held to.

Images are 2-D arrays (uint8 or float32); every function returns float64 unless it says otherwise, so a test can measure the kernel's
float32 result against an (almost) exact value.  The Gaussian is a direct tap loop over an explicit reflect-index function -- nothing
here calls scipy, skimage or sklearn (tests/test_cpu_preprocess.py pins this file to them where they are installed).
"""
import numpy as np

U = 2.0 ** -24      # float32 unit roundoff
PRE_MAX_RADIUS = 16


def reflect_index(i, n):
    """Index of sample ``i`` of an axis of ``n`` under scipy's 'reflect' (half-sample symmetric: d c b a | a b c d), any distance."""
    p = 2 * n
    i = i % p      # (Python's and numpy's modulo: non-negative); an int or an integer array
    if isinstance(i, np.ndarray):
        return np.where(i < n, i, p - 1 - i)
    return i if i < n else p - 1 - i


def gaussian_taps(radius):
    """(lw, w): lw = int(4 * radius + 0.5); w[k + lw] = exp(-0.5 k^2 / radius^2) over k = -lw..lw, normalised to sum 1."""
    lw = int(4.0 * float(radius) + 0.5)
    if lw == 0:
        return 0, np.ones(1)
    k = np.arange(-lw, lw + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(radius) ** 2) * k ** 2)
    return lw, w / w.sum()


def blur_axis(a, radius, axis):
    """One axis of gaussian_filter(a, sigma=radius, mode='reflect', truncate=4.0): out[i] = sum_k w[k] a[reflect(i + k)]."""
    a = np.asarray(a, dtype=np.float64)
    lw, w = gaussian_taps(radius)
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k in range(-lw, lw + 1):
        idx = reflect_index(np.arange(n) + k, n)
        out += w[k + lw] * np.take(a, idx, axis=axis)
    return out


def gaussian(a, radius):
    """gaussian_filter of a 2-D image: scipy filters axis 0 first, then axis 1 (the order changes the result by roundoff only)."""
    return blur_axis(blur_axis(a, radius, 0), radius, 1)


def image_stats(x):
    """(mean, std, min, max) as numpy gives them in float64."""
    x64 = np.asarray(x).astype(np.float64) if np.asarray(x).dtype != np.uint8 else np.asarray(x)
    return float(np.mean(x64)), float(np.std(x64)), float(np.min(x64)), float(np.max(x64))


def standardize(x, mean=None, std=None):
    """float64 (x - mean) / std -- cast to float32 by the caller for the kernel's value."""
    m, s, _, _ = image_stats(x)
    mean = m if mean is None else mean
    std = s if std is None else std
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(x).astype(np.float64) - np.float64(mean)) / np.float64(std)


def minmax(x):
    """The reference's own expression, evaluated by numpy in its own dtypes: float32."""
    x = np.asarray(x)
    lo, hi = np.min(x), np.max(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (x - lo) / (hi - lo).astype("float32")


def row_normalize(x):
    x = np.asarray(x).astype(np.float64)
    n = np.sqrt((x * x).sum(axis=1))
    n[n == 0.0] = 1.0
    return x / n[:, None]


def unsharp_parts(x, radius, preserve_range):
    """(f, blurred, blurred_abs): the float image skimage works on, its Gaussian blur and the blur of |f| (for the roundoff bound)."""
    x = np.asarray(x)
    f = x.astype(np.float64)
    if x.dtype == np.uint8 and not preserve_range:
        f = f / 255.0
    return f, gaussian(f, radius), gaussian(np.abs(f), radius)


def unsharp_mask(x, radius=1.0, amount=1.0, preserve_range=False):
    f, blurred, _ = unsharp_parts(x, radius, preserve_range)
    res = f + (f - blurred) * amount
    if preserve_range:
        return res
    return np.clip(res, -1.0 if (f < 0).any() else 0.0, 1.0)


def unsharp_bound(x, radius, amount, preserve_range):
    """The a-priori bound on |kernel - unsharp_mask| per element: c U (|f| + |amount| (|f| + sum w |f|)) with c = 2 lw + 12.

    c counts the kernel's float32 roundings, each relative to a magnitude that the bracket dominates:
      1       f itself (uint8 / 255 is one division; it enters f, f - blurred and the blur)
      lw + 3  per blur pass: the tap rounded to float32 (1), the pair sum t[-k] + t[+k] (1), and lw + 1 accumulation steps of
              acc += w * pair (fused or not: at most one rounding of the running sum per step, which is below sum w |f|)
      3       the combine: f - blurred, * amount, f + ...
      2       slack for the second-order terms of the above
    i.e. 1 + 2 (lw + 3) + 3 + 2 = 2 lw + 12.  The clip is 1-Lipschitz and adds nothing."""
    lw, _ = gaussian_taps(radius)
    f, _, babs = unsharp_parts(x, radius, preserve_range)
    return (2 * lw + 12) * U * (np.abs(f) + abs(amount) * (np.abs(f) + babs))


def center_crop(x, size):
    H, W = x.shape[-2:]
    if H < size or W < size:
        raise ValueError("crop larger than the image")
    y0, x0 = (H - size) // 2, (W - size) // 2
    return x[..., y0:y0 + size, x0:x0 + size]


def integrate_masks(masks):
    return (np.asarray(masks) != 0).any(axis=0).astype(np.uint8)


def ulp32(v):
    """Spacing of float32 at |v| (float64 array)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)
