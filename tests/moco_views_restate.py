"""CPU statement of MoCo's ``tau_g`` (moco_data_module.py:119-132) for the tests of cmunet_amd.moco_views, written from the rules of
torchvision 0.14.0's tensor path with torch's own CPU functions: every transform ends in ``F.grid_sample``,
``F.interpolate`` or ``F.pad`` + ``F.conv2d``, so those calls are the oracle for the pixels.  torchvision itself is not a dependency and
was not available to check the steps that lead up to those calls (the rotation's matrix and base grid, the crop law, the blur's weights).

Every function takes ``dtype``: float32 is the reference's arithmetic, float64 the same statement in double (the distance between the two
is the rounding floor the GPU tests measure).  ``*_explicit`` are index-and-weight statements of the resize and the blur that the CPU
tests hold against the torch calls.  This module does not import cmunet_amd.moco_views."""
import math

import numpy as np
import torch
import torch.nn.functional as F

OP_ROTATION, OP_BLUR, OP_HFLIP, OP_VFLIP, OP_NOISE = 1, 2, 4, 8, 16


# ------------------------------------------------------------------------------------------------
# 1. RandomRotation: NEAREST, expand=False, centre = image centre, fill 0
# ------------------------------------------------------------------------------------------------
def rotation_grid(H, W, angle, dtype=torch.float32):
    """F.rotate's sampling grid (1, H, W, 2): theta = [[cos r, sin r, 0], [-sin r, cos r, 0]], r = radians(-angle) in Python floats, then
    in ``dtype``: base grid linspace(-W/2 + 0.5, W/2 - 0.5, W) (same in y), times theta^T / (W/2, H/2)."""
    r = math.radians(-float(angle))
    theta = torch.tensor([[math.cos(r), math.sin(r), 0.0], [-math.sin(r), math.cos(r), 0.0]], dtype=dtype).reshape(1, 2, 3)
    base = torch.empty(1, H, W, 3, dtype=dtype)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + 0.5, W * 0.5 + 0.5 - 1, steps=W, dtype=dtype))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + 0.5, H * 0.5 + 0.5 - 1, steps=H, dtype=dtype).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=dtype)
    return base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)


def rotate(img, angle, dtype=torch.float32):
    """img (H, W) -> the rotated image in ``dtype`` (grid_sample nearest, zeros, align_corners=False)."""
    H, W = img.shape
    x = img.to(dtype)[None, None]
    return F.grid_sample(x, rotation_grid(H, W, angle, dtype), mode="nearest", padding_mode="zeros", align_corners=False)[0, 0]


def rotation_tie_band(H, W, angle, tol=1e-3):
    """Pixels of the rotated image whose unnormalised source coordinate, in float64, lies within ``tol`` of a half-integer in x or y:
    where float32 rounding, not the rule, picks the neighbour.  -> bool (H, W)."""
    g = rotation_grid(H, W, angle, torch.float64)[0]
    ix = ((g[..., 0] + 1) * W - 1) / 2
    iy = ((g[..., 1] + 1) * H - 1) / 2
    near = lambda c: ((c - torch.floor(c)) - 0.5).abs() <= tol
    return near(ix) | near(iy)


# ------------------------------------------------------------------------------------------------
# 2. RandomResizedCrop: crop (i, j, h, w), interpolate to (out, out) bilinear, align_corners=False
# ------------------------------------------------------------------------------------------------
def resized_crop(img, box, out, antialias=False, dtype=torch.float32):
    i, j, h, w = (int(v) for v in box)
    x = img.to(dtype)[i:i + h, j:j + w][None, None]
    return F.interpolate(x, size=(out, out), mode="bilinear", align_corners=False, antialias=bool(antialias))[0, 0]


def resize_taps(n, out, antialias, f32=True):
    """Per output index of a resize n -> out: (first source index, weights) by ATen's rule.  ``f32``: the coordinate arithmetic in float32
    (what ATen does for float32 images), else float64."""
    t = np.float32 if f32 else np.float64
    scale = t(n) / t(out)
    taps = []
    for o in range(out):
        if not antialias:
            # scale * (o + 0.5) - 0.5 with ONE rounding: ATen's CPU kernels are compiled with fused multiply-add
            src = max(t(np.float64(scale) * (o + 0.5) - 0.5), t(0))
            i0 = min(int(np.floor(src)), n - 1)
            lam = min(max(t(src - t(i0)), t(0)), t(1))
            i1 = i0 + (1 if i0 < n - 1 else 0)
            taps.append(([i0, i1], [t(1) - lam, lam]))
        else:
            support = scale if scale >= 1 else t(1)
            inv = t(1) / scale if scale >= 1 else t(1)
            center = scale * (t(o) + t(0.5))
            xmin = max(int(t(center - support) + t(0.5)), 0)
            xmax = min(int(t(center + support) + t(0.5)), n)
            ws = []
            for k in range(xmax - xmin):
                x = abs(t(t(t(k + xmin) - center) + t(0.5)) * inv)
                ws.append(t(1) - x if x < 1 else t(0))
            total = t(0)
            for v in ws:
                total = t(total + v)
            taps.append((list(range(xmin, xmax)), [t(v / total) for v in ws]))
    return taps


def resized_crop_explicit(img, box, out, antialias=False, f32=True):
    """The same resize as sums over ``resize_taps`` (horizontal, then vertical), accumulated in float32 (``f32``) or float64."""
    t = np.float32 if f32 else np.float64
    i, j, h, w = (int(v) for v in box)
    a = np.asarray(img, dtype=t)[i:i + h, j:j + w]
    cols, rows = resize_taps(w, out, antialias, f32), resize_taps(h, out, antialias, f32)
    hor = np.zeros((h, out), t)
    for o, (idx, ws) in enumerate(cols):
        acc = a[:, idx[0]] * t(ws[0])
        for k in range(1, len(idx)):
            acc = (acc + a[:, idx[k]] * t(ws[k])).astype(t)
        hor[:, o] = acc
    res = np.zeros((out, out), t)
    for o, (idx, ws) in enumerate(rows):
        acc = hor[idx[0]] * t(ws[0])
        for k in range(1, len(idx)):
            acc = (acc + hor[idx[k]] * t(ws[k])).astype(t)
        res[o] = acc
    return res


# ------------------------------------------------------------------------------------------------
# 3. GaussianBlur(kernel_size=(kx, ky), sigma): reflect padding, conv2d with the outer-product kernel
# ------------------------------------------------------------------------------------------------
def gaussian_kernel1d(k, sigma):
    """float32 whatever the image's dtype (the kernel is computed first and cast afterwards)."""
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k)
    pdf = torch.exp(-0.5 * (x / float(sigma)).pow(2))
    return pdf / pdf.sum()


def blur(img, ksize, sigma, dtype=torch.float32):
    kx, ky = ksize
    wx, wy = gaussian_kernel1d(kx, sigma).to(dtype), gaussian_kernel1d(ky, sigma).to(dtype)
    k2 = torch.mm(wy[:, None], wx[None, :])
    x = F.pad(img.to(dtype)[None, None], [kx // 2, kx // 2, ky // 2, ky // 2], mode="reflect")
    return F.conv2d(x, k2[None, None])[0, 0]


def blur_explicit(img, ksize, sigma):
    """The blur as 45 explicit float64 terms per pixel over reflected indices."""
    kx, ky = ksize
    wx, wy = gaussian_kernel1d(kx, sigma).double().numpy(), gaussian_kernel1d(ky, sigma).double().numpy()
    a = np.asarray(img, dtype=np.float64)
    H, W = a.shape
    refl = lambda i, n: np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
    ys, xs = np.arange(H), np.arange(W)
    res = np.zeros_like(a)
    for dy in range(ky):
        yy = refl(ys + dy - ky // 2, H)
        for dx in range(kx):
            xx = refl(xs + dx - kx // 2, W)
            res += wy[dy] * wx[dx] * a[np.ix_(yy, xx)]
    return res


# ------------------------------------------------------------------------------------------------
# 4. / 5. flips and GaussNoise; the chain
# ------------------------------------------------------------------------------------------------
def gauss_noise(img, z):
    """moco_data_module.py:199-213: sigma = max(image) / 10, out = image + sigma * randn."""
    sigma = torch.max(img) / 10
    return img + sigma * z.to(img.dtype)


def apply_view(img, rec, ksize=(5, 9), out=224, antialias=False, noise=None, dtype=torch.float32):
    """One view of img (H, W) for a record (anything indexable by field name) -> (view (out, out), its maximum before the noise)."""
    x = img.to(dtype)
    ops = int(rec["ops"])
    if ops & OP_ROTATION:
        x = rotate(x, float(rec["angle"]), dtype)
    x = resized_crop(x, (rec["top"], rec["left"], rec["height"], rec["width"]), out, antialias, dtype)
    if ops & OP_BLUR:
        x = blur(x, ksize, float(rec["sigma"]), dtype)
    if ops & OP_HFLIP:
        x = torch.flip(x, [-1])
    if ops & OP_VFLIP:
        x = torch.flip(x, [-2])
    m = torch.max(x)
    if ops & OP_NOISE and noise is not None:
        x = gauss_noise(x, noise)
    return x, m


def taint(img_shape, rec, ksize=(5, 9), out=224, antialias=False, tol=1e-3):
    """Output pixels of a view whose value depends on a tie-band pixel of the rotation (through the resize's and the blur's footprints):
    the band's indicator pushed through the same crop, resize, blur and flips in float64 (all weights are non-negative).  -> bool."""
    H, W = img_shape
    ops = int(rec["ops"])
    if not ops & OP_ROTATION:
        return torch.zeros(out, out, dtype=torch.bool)
    band = rotation_tie_band(H, W, float(rec["angle"]), tol).double()
    x = resized_crop(band, (rec["top"], rec["left"], rec["height"], rec["width"]), out, antialias, torch.float64)
    if ops & OP_BLUR:
        x = blur(x, ksize, float(rec["sigma"]), torch.float64)
    if ops & OP_HFLIP:
        x = torch.flip(x, [-1])
    if ops & OP_VFLIP:
        x = torch.flip(x, [-2])
    return x > 0


# ------------------------------------------------------------------------------------------------
# host mirror of the sampler's laws (numpy generator; not the device's stream)
# ------------------------------------------------------------------------------------------------
def crop_box(H, W, rng, scale=(0.2, 1.0), ratio=(3. / 4., 4. / 3.), attempts=10):
    """RandomResizedCrop.get_params -> (i, j, h, w, fell_back)."""
    area = H * W
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(attempts):
        target = area * rng.uniform(scale[0], scale[1])
        aspect = math.exp(rng.uniform(lo, hi))
        w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.randint(0, H - h + 1)), int(rng.randint(0, W - w + 1)), h, w, False
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w, True


def sample_records(n, H, W, rng, p_rotation=0.5, degrees=180.0, scale=(0.2, 1.0), ratio=(3. / 4., 4. / 3.), p_blur=0.5, sigma=(0.1, 2.0),
                   p_hflip=0.5, p_vflip=0.5, p_noise=0.5):
    """n records drawn by the reference's laws -> dict of arrays (ops, top, left, height, width, angle, sigma, fell_back)."""
    r = {k: np.zeros(n, np.int32) for k in ("ops", "top", "left", "height", "width")}
    r["angle"], r["sigma"], r["fell_back"] = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    for k in range(n):
        ops = OP_ROTATION if rng.uniform() < p_rotation else 0
        r["angle"][k] = rng.uniform(-degrees, degrees)
        r["top"][k], r["left"][k], r["height"][k], r["width"][k], r["fell_back"][k] = crop_box(H, W, rng, scale, ratio)
        ops |= OP_BLUR if rng.uniform() < p_blur else 0
        r["sigma"][k] = rng.uniform(sigma[0], sigma[1])
        ops |= OP_HFLIP if rng.uniform() < p_hflip else 0
        ops |= OP_VFLIP if rng.uniform() < p_vflip else 0
        ops |= OP_NOISE if rng.uniform() < p_noise else 0
        r["ops"][k] = ops
    return r
