"""numpy restatement of the finetuning training augmentation (Finetuning/dataset.py:134-165, csrc/ft_augment.hip), driven by explicit
records (cmunet_amd.ft_augment.REC_DTYPE) and explicit float64 noise.  Each rule is written out with the device kernels' arithmetic (the
rules themselves are restated from albumentations 1.4.18 / OpenCV 4.x documentation: DESIGN.md 4.13; neither library is available to
check them against)."""
import numpy as np

OP_NOISE, OP_BLUR, OP_BC, OP_DOWN, OP_ONEOF = 1, 2, 4, 8, 16


def crop_offset(n, crop, u):
    """RandomCrop: int((n - crop + 1) * u), u uniform on [0, 1)."""
    return int((n - crop + 1) * u)


def ksize_from_draw(k, khi):
    """GaussianBlur's kernel size from the uniform integer k in [lo, hi]: an even k becomes (k + 1) mod (hi + 1)."""
    return k if k % 2 == 1 else (k + 1) % (khi + 1)


def gaussian_weights(k, sigma):
    """OpenCV getGaussianKernel in float64: t_i = exp(-0.5 / sigma^2 * x_i * x_i), x_i = i - (k - 1) / 2, w = t * (1 / sum t)."""
    scale2 = -0.5 / (sigma * sigma)
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    t = np.exp(scale2 * x * x)
    s = 0.0
    for v in t:
        s += v
    return t * (1.0 / s)


def correlate_reflect101(a, w, axis, store=np.float32):
    """Taps of ``w`` along ``axis`` with a reflect-101 border, accumulated in float64 in tap order, stored as ``store``."""
    a = np.asarray(a, dtype=np.float64)
    h = (len(w) - 1) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (h, h)
    p = np.pad(a, pad, mode="reflect")
    n = a.shape[axis]
    acc = np.zeros(a.shape, np.float64)
    for t in range(len(w)):
        sl = p[:, t:t + n] if axis == 1 else p[t:t + n, :]
        acc = acc + w[t] * sl
    return acc.astype(store)


def blur(img, k, sigma, store=np.float32):
    """GaussianBlur: the horizontal pass, then the vertical pass (``store`` after each)."""
    w = gaussian_weights(k, sigma)
    return correlate_reflect101(correlate_reflect101(img, w, 1, store), w, 0, store)


def gauss_noise(img, var, z, clip=True):
    """GaussNoise: img + sqrt(var) * z in float64, clipped to [0, 1] (the reference's float32 maximum), stored as float32."""
    out = np.asarray(img, np.float32).astype(np.float64) + np.sqrt(var) * z
    if clip:
        out = np.clip(out, 0.0, 1.0)
    return out.astype(np.float32)


def brightness_contrast(img, alpha, beta, clip=True):
    """RandomBrightnessContrast (brightness_by_max): img * alpha + beta * 1.0 in float32, clipped to [0, 1]."""
    out = np.asarray(img, np.float32) * np.float32(alpha) + np.float32(beta)
    if clip:
        out = np.clip(out, np.float32(0.0), np.float32(1.0))
    return out.astype(np.float32)


def downscale_index(n, s):
    """Downscale with INTER_NEAREST both ways: the source index of each output index.  small = cvRound(n * s) (half to even);
    down: resizeNN reads min(floor(j * (1 / s)), n - 1); up to n: min(floor(i * (1 / (n / small))), small - 1)."""
    small = max(1, int(np.rint(n * s)))
    i = np.arange(n)
    u = np.minimum(np.floor(i * (1.0 / (n / small))).astype(np.int64), small - 1)
    return np.minimum(np.floor(u * (1.0 / s)).astype(np.int64), n - 1)


def downscale(img, s):
    idx = downscale_index(img.shape[0], s)
    return img[np.ix_(idx, idx)]


def geometry(a, oneof, rot_k):
    """OneOf's HorizontalFlip / VerticalFlip / RandomRotate90 (np.rot90(a, k)); 3 (GaussNoise) leaves the geometry alone."""
    if oneof == 0:
        return a[:, ::-1]
    if oneof == 1:
        return a[::-1, :]
    if oneof == 2:
        return np.rot90(a, int(rot_k))
    return a


def augment(image, mask, rec, noise=None, crop=475, clip=True):
    """The whole chain for one image (H,W) float32 and mask (H,W) uint8 with record ``rec``; ``noise`` (2, crop, crop) float64 (plane 0
    GaussNoise, plane 1 OneOf's GaussNoise).  -> (image (crop,crop) float32, mask (crop,crop) uint8), the augmented crop before the
    resize."""
    ops = int(rec["ops"])
    y0, x0 = int(rec["y0"]), int(rec["x0"])
    a = np.asarray(image, np.float32)[y0:y0 + crop, x0:x0 + crop]
    m = np.asarray(mask)[y0:y0 + crop, x0:x0 + crop]
    if ops & OP_NOISE:
        a = gauss_noise(a, float(rec["var_noise"]), noise[0], clip)
    if ops & OP_BLUR:
        a = blur(a, int(rec["ksize"]), float(rec["sigma"]))
    if ops & OP_BC:
        a = brightness_contrast(a, float(rec["alpha"]), float(rec["beta"]), clip)
    if ops & OP_DOWN:
        a = downscale(a, float(rec["scale"]))
    if ops & OP_ONEOF:
        oneof = int(rec["oneof"])
        if oneof == 3:
            a = gauss_noise(a, float(rec["var_oneof"]), noise[1], clip)
        else:
            a = geometry(a, oneof, int(rec["rot_k"]))
            m = geometry(m, oneof, int(rec["rot_k"]))
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(m)


def augment_batch(images, masks, recs, noise=None, crop=475, clip=True):
    """``augment`` over a batch; noise (2, B, crop, crop) or None."""
    out = [augment(images[b], masks[b], recs[b], None if noise is None else noise[:, b], crop, clip) for b in range(len(recs))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
