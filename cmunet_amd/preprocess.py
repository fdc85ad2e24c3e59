"""The reference's image preprocessing (``data_processing/pre_processing.py``) on the GPU (csrc/preprocess.hip).

Batch functions, on ``(B,H,W)`` or ``(H,W)`` images, uint8 or float32 (other dtypes are cast to float32), numpy arrays or tensors;
host data is uploaded, the result is a device tensor in the input's layout:

  image_stats(x)                       -> (B,4) float64: mean, population std (np.std), min, max of every image
  standardize(x, mean=None, std=None)  -> float32((float64(x) - mean) / std); None: the image's own statistic
  minmax(x, lo=None, hi=None)          -> (x - lo) / float32(hi - lo), the reference's expression; None: the image's own min / max
  row_normalize(x)                     -> sklearn.preprocessing.normalize of every image: each row over its Euclidean norm
  unsharp_mask(x, radius=1.0, amount=1.0, preserve_range=False)   -> skimage.filters.unsharp_mask
  center_crop(x, size, mask=None)      -> albumentations' CenterCrop(size, size) of the image (and of the uint8 mask)
  integrate_masks(masks)               -> uint8 0/1: any of the (M,H,W) / (B,M,H,W) masks is non-zero

They only launch kernels (small host-to-device uploads aside): no host synchronisation, no device-to-host read, no CPU fallback --
without a GPU they raise ``RuntimeError``.  Every result is the same bits on every call.

Reference classes with their names, constructor signatures and ``fit_transform`` / ``transform`` contracts on the reference's
``{key: {"raw": image, "labelled": mask(s)}}`` dictionaries: ``PreProcessor``, ``Intensity_normalizer``, ``MinMax_normalizer``,
``skly_normalizer``, ``Unsharper``, ``Mask_Integrater``, ``Cropper``, ``Pipeline``.  Values may be numpy arrays or tensors; images of equal
shape and dtype run as one batch; results are device tensors.  Fitted statistics are kept per key (0-dim device tensors).

``Preprocess(steps)`` (= ``Pipeline(steps).batch``) is the device callable ``(n,H,W) -> (n,H',W') float32`` that ``infer.Segmenter``
takes: every image is normalised with its own statistics.

Where this differs from the reference, on purpose:
  * statistics are float64 whatever the image's dtype (numpy's ``np.mean`` of a float32 image accumulates in float32), and the
    standardisation subtracts and divides in float64 before one cast;
  * ``Unsharper`` returns float32 (skimage: float64); ``radius`` may not exceed ``PRE_MAX_RADIUS``; one radius for both axes;
  * ``Mask_Integrater`` returns uint8 0/1 (the reference: Python int, after a uint8 sum that wraps at 256 -- here any non-zero counts);
  * ``Cropper`` crops to its ``size`` (the reference's constructor takes ``size`` and then crops to 475 regardless); ``border_ratio`` and
    ``thresh`` are accepted for signature parity only: ``ReplaceWithBorderPixel`` (``cv2.inpaint`` with INPAINT_TELEA, a sequential
    fast-marching fill) is NOT built, and neither are ``Mask_Contour_Fillier`` (cv2 contours) and ``Unlabelled_Remover`` (host bookkeeping:
    ``{k: v for k, v in data.items() if len(v.get("labelled", ())) > 0}``).  After a successful crop ``PadIfNeeded`` never acts;
  * min / max ignore NaN pixels (numpy propagates them).
"""
from abc import ABC, abstractmethod

import numpy as np
import torch

from . import ops

PRE_MAX_RADIUS = ops.PRE_MAX_RADIUS      # largest Gaussian radius of unsharp_mask: half-width int(4 * 16 + 0.5) = 64 taps a side


def gaussian_weights(radius):
    """scipy.ndimage's 1-D Gaussian for ``sigma = radius``, ``truncate = 4``: the taps at distance 0..lw, lw = int(4 * radius + 0.5),
    ``exp(-0.5 k^2 / radius^2)`` normalised so that the full symmetric kernel sums to 1 (float64, on the host)."""
    radius = float(radius)
    if not 0.0 <= radius <= PRE_MAX_RADIUS:      # (also refuses nan)
        raise ValueError(f"preprocess: radius must lie in 0..PRE_MAX_RADIUS = {PRE_MAX_RADIUS}, got {radius!r}")
    lw = int(4.0 * radius + 0.5)
    if lw == 0:
        return np.ones(1, dtype=np.float64)
    k = np.arange(-lw, lw + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (radius * radius) * k ** 2)
    phi /= phi.sum()
    return phi[lw:].copy()


_WEIGHTS = {}


def _device_weights(radius, device):
    key = (float(radius), device)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = torch.from_numpy(gaussian_weights(radius).astype(np.float32)).to(device)
    return _WEIGHTS[key]


def _to_device(what, x, device=None):
    if not torch.cuda.is_available():
        raise RuntimeError(f"preprocess.{what} runs on the GPU only; there is no CPU fallback in this package")
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype != torch.uint8 and t.dtype != torch.float32:
        t = t.to(torch.float32)
    if not t.is_cuda:
        t = t.to(device or "cuda", non_blocking=True)
    return t


def _as_batch(what, x):
    t = _to_device(what, x)
    if t.dim() not in (2, 3):
        raise ValueError(f"preprocess.{what}: (H,W) or (B,H,W), got {tuple(t.shape)}")
    return (t if t.dim() == 3 else t.unsqueeze(0)).contiguous(), t.dim() == 3


def _column(what, v, B, device):
    """A per-image statistic given by the caller: a number, a sequence of B numbers or a tensor -> (B,) float64 on the device."""
    t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))
    t = t.to(device=device, dtype=torch.float64).reshape(-1)
    if t.numel() not in (1, B):
        raise ValueError(f"preprocess.{what}: a statistic must be one number or one per image ({B}), got {t.numel()}")
    return t.expand(B)


def _stats_with(what, x, cols):
    """(B,4) statistics of ``x`` with the given columns {index: value} replaced; nothing is measured when every column is given."""
    B = x.shape[0]
    given = {c: v for c, v in cols.items() if v is not None}
    if len(given) < len(cols):
        stats = ops.pre_stats(x)
    else:
        stats = torch.zeros(B, 4, dtype=torch.float64, device=x.device)
    for c, v in given.items():
        stats[:, c] = _column(what, v, B, x.device)
    return stats


def image_stats(x):
    """(B,4) float64 -- (4,) for an (H,W) image: mean, population standard deviation, min, max.  Sums run in float64 in a fixed order;
    the mean of a uint8 image is its exact integer sum divided once."""
    t, batched = _as_batch("image_stats", x)
    s = ops.pre_stats(t)
    return s if batched else s[0]


def standardize(x, mean=None, std=None):
    """``Intensity_normalizer``: float32((float64(x) - mean) / std); a zero ``std`` gives nan / inf as numpy does."""
    t, batched = _as_batch("standardize", x)
    out = ops.pre_standardize(t, _stats_with("standardize", t, {0: mean, 1: std}))
    return out if batched else out[0]


def minmax(x, lo=None, hi=None):
    """``MinMax_normalizer``: ``(x - lo) / float32(hi - lo)``.  uint8: the difference is an exact integer (never wrapped), the quotient
    one float32 division; float32: one float32 subtraction and one division.  A constant image gives nan."""
    t, batched = _as_batch("minmax", x)
    out = ops.pre_minmax(t, _stats_with("minmax", t, {2: lo, 3: hi}))
    return out if batched else out[0]


def row_normalize(x):
    """``skly_normalizer``: every row of every image over its Euclidean norm (float64 norm and quotient); a zero row stays zero."""
    t, batched = _as_batch("row_normalize", x)
    out = ops.pre_row_normalize(t)
    return out if batched else out[0]


def unsharp_mask(x, radius=1.0, amount=1.0, preserve_range=False):
    """``skimage.filters.unsharp_mask``: f + (f - gaussian(f, sigma=radius, mode='reflect', truncate=4)) * amount with f = x / 255 for a
    uint8 image unless ``preserve_range``; without ``preserve_range`` the result is clipped to [0,1], or to [-1,1] for an image that
    holds a negative value.  float32 taps and accumulation; 0 <= radius <= PRE_MAX_RADIUS (below 0.125 the blur is the identity)."""
    wts = gaussian_weights(radius)      # (refuses a bad radius before anything touches the device)
    t, batched = _as_batch("unsharp_mask", x)
    u8 = t.dtype == torch.uint8
    clip = not preserve_range
    stats = ops.pre_stats(t) if clip and not u8 else None      # the [-1,1] / [0,1] choice needs the image's min
    out = ops.pre_unsharp(t, _device_weights(radius, t.device), float(amount), 255.0 if u8 and not preserve_range else 1.0, clip, stats)
    return out if batched else out[0]


def _crop_offsets(what, H, W, size):
    size = int(size)
    if size < 1:
        raise ValueError(f"preprocess.{what}: size must be at least 1, got {size}")
    if H < size or W < size:
        raise ValueError(f"preprocess.{what}: requested crop size ({size}, {size}) is larger than the image size ({H}, {W})")
    return (H - size) // 2, (W - size) // 2, size


def center_crop(x, size, mask=None):
    """``A.CenterCrop(size, size)``: rows ``(H - size) // 2 ..``, columns ``(W - size) // 2 ..``; with ``mask`` (uint8, the image's
    shape) returns ``(image, mask)`` cropped alike.  A side shorter than ``size`` raises ValueError."""
    shape = tuple(x.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"preprocess.center_crop: (H,W) or (B,H,W), got {shape}")
    y0, x0, size = _crop_offsets("center_crop", shape[-2], shape[-1], size)
    if mask is not None and tuple(mask.shape) != shape:
        raise ValueError(f"preprocess.center_crop: the mask's shape {tuple(mask.shape)} is not the image's {shape}")
    t, batched = _as_batch("center_crop", x)
    out = ops.pre_crop(t, y0, x0, size, size)
    out = out if batched else out[0]
    if mask is None:
        return out
    m = torch.as_tensor(mask) if not torch.is_tensor(mask) else mask
    if m.dtype != torch.uint8:
        m = m.to(torch.uint8)
    m, _ = _as_batch("center_crop", m)
    mo = ops.pre_crop(m, y0, x0, size, size)
    return out, (mo if batched else mo[0])


def integrate_masks(masks):
    """``Mask_Integrater``: uint8 0/1, 1 where any mask of the stack is non-zero.  ``masks``: (M,H,W) -> (H,W), (B,M,H,W) -> (B,H,W), or a
    list of M (H,W) masks; values are read as uint8."""
    if isinstance(masks, (list, tuple)):
        masks = torch.stack([torch.as_tensor(m) for m in masks]) if any(torch.is_tensor(m) for m in masks) else np.stack(masks)
    t = masks if torch.is_tensor(masks) else torch.from_numpy(np.ascontiguousarray(masks))
    if t.dim() not in (3, 4):
        raise ValueError(f"preprocess.integrate_masks: (M,H,W) or (B,M,H,W), got {tuple(t.shape)}")
    if t.dtype != torch.uint8:
        t = (t != 0).to(torch.uint8)
    t = _to_device("integrate_masks", t)
    out = ops.pre_integrate_masks((t if t.dim() == 4 else t.unsqueeze(0)).contiguous())
    return out if t.dim() == 4 else out[0]


# ----------------------------------------------------------------------------------------------------------------------
# the reference's classes
# ----------------------------------------------------------------------------------------------------------------------
def _raw_batches(data):
    """Keys grouped by the (shape, dtype) of their "raw" image: [(keys, (n,H,W) device batch)]."""
    groups = {}
    for k, v in data.items():
        t = _to_device("transform", v["raw"])
        if t.dim() != 2:
            raise ValueError(f"preprocess: every raw image must be 2-D, got {tuple(t.shape)} for {k!r}")
        groups.setdefault((tuple(t.shape), t.dtype), []).append((k, t))
    return [([k for k, _ in g], torch.stack([t for _, t in g]).contiguous()) for g in groups.values()]


def _map_raw(data, fn):
    """``fn(keys, batch) -> batch`` over every group; the other fields of each entry are carried over."""
    out = {k: dict(v) for k, v in data.items()}
    for keys, batch in _raw_batches(data):
        res = fn(keys, batch)
        for i, k in enumerate(keys):
            out[k]["raw"] = res[i]
    return out


class PreProcessor(ABC):
    """Abstract class for pre-processing data"""

    def __init__(self) -> None:
        pass

    @abstractmethod
    def transform(self, data):
        """Transform ``{key: {"raw": image, "labelled": mask}}`` and return the transformed dictionary."""

    def fit_transform(self, data):
        """Fit the processor on the incoming data and return the transformed data."""
        return self.transform(data)


class skly_normalizer(PreProcessor):
    """sklearn's ``normalize`` of every raw image (rows over their L2 norm)."""

    def __init__(self) -> None:
        super().__init__()

    def _batch(self, x):
        return ops.pre_row_normalize(x)

    def transform(self, data):
        return _map_raw(data, lambda keys, x: self._batch(x))

    def fit_transform(self, data):
        return self.transform(data)


class Intensity_normalizer(PreProcessor):
    """z = (x - u) / s with the mean and standard deviation of each key's image at ``fit_transform`` time."""

    def __init__(self) -> None:
        super().__init__()

    def _batch(self, x):
        return ops.pre_standardize(x, ops.pre_stats(x))

    def transform(self, data):
        if not hasattr(self, "means") or not hasattr(self, "stds"):
            raise ValueError("The means and stds are not set, please call `fit_transform` first.")

        def run(keys, x):
            stats = torch.zeros(len(keys), 4, dtype=torch.float64, device=x.device)
            stats[:, 0] = torch.stack([self.means[k] for k in keys]).to(x.device)      # (an unseen key: KeyError, as the reference)
            stats[:, 1] = torch.stack([self.stds[k] for k in keys]).to(x.device)
            return ops.pre_standardize(x, stats)

        return _map_raw(data, run)

    def fit_transform(self, data):
        self.means, self.stds = {}, {}
        for keys, x in _raw_batches(data):
            stats = ops.pre_stats(x)
            for i, k in enumerate(keys):
                self.means[k], self.stds[k] = stats[i, 0], stats[i, 1]
        return self.transform(data)


class MinMax_normalizer(PreProcessor):
    """(x - min) / (max - min) with each key's own min and max at ``fit_transform`` time."""

    def __init__(self) -> None:
        super().__init__()

    def _batch(self, x):
        return ops.pre_minmax(x, ops.pre_stats(x))

    def transform(self, data):
        if not hasattr(self, "min") or not hasattr(self, "max"):
            raise ValueError("The means and stds are not set, please call `fit_transform` first.")

        def run(keys, x):
            stats = torch.zeros(len(keys), 4, dtype=torch.float64, device=x.device)
            stats[:, 2] = torch.stack([self.min[k] for k in keys]).to(x.device)
            stats[:, 3] = torch.stack([self.max[k] for k in keys]).to(x.device)
            return ops.pre_minmax(x, stats)

        return _map_raw(data, run)

    def fit_transform(self, data):
        self.min, self.max = {}, {}
        for keys, x in _raw_batches(data):
            stats = ops.pre_stats(x)
            for i, k in enumerate(keys):
                self.min[k], self.max[k] = stats[i, 2], stats[i, 3]
        return self.transform(data)


class Unsharper(PreProcessor):
    """skimage's unsharp mask of every raw image."""

    def __init__(self, radius: int, amount: int, preserve_range: bool) -> None:
        super().__init__()
        gaussian_weights(radius)      # (ValueError for a radius outside 0..PRE_MAX_RADIUS)
        self.radius = radius
        self.amount = amount
        self.preserve_range = preserve_range

    def _batch(self, x):
        return unsharp_mask(x, self.radius, self.amount, self.preserve_range)

    def transform(self, data):
        return _map_raw(data, lambda keys, x: self._batch(x))

    def fit_transform(self, data):
        return self.transform(data)


class Mask_Integrater(PreProcessor):
    """The masks of every key's "labelled" list combined into one uint8 0/1 mask."""

    def __init__(self) -> None:
        super().__init__()

    def transform(self, data):
        return {k: {**v, "labelled": integrate_masks(list(v["labelled"]) if not torch.is_tensor(v["labelled"]) else v["labelled"])}
                for k, v in data.items()}

    def fit_transform(self, data):
        return self.transform(data)


class Cropper(PreProcessor):
    """Centre crop of the raw image and of its mask to ``size`` x ``size``.  ``border_ratio`` / ``thresh`` belong to the reference's
    ``ReplaceWithBorderPixel`` inpainting step, which is not built: they are stored and unused."""

    def __init__(self, size=475, border_ratio=0.25, thresh=20) -> None:
        super().__init__()
        self.size = size
        self.border_ratio = border_ratio
        self.thresh = thresh

    def _batch(self, x):
        y0, x0, size = _crop_offsets("Cropper", x.shape[1], x.shape[2], self.size)
        return ops.pre_crop(x, y0, x0, size, size)

    def transform(self, data):
        size = self.aug      # (set by fit_transform; before it: AttributeError, as the reference's missing ``self.aug``)
        out = {k: dict(v) for k, v in data.items()}
        for k, v in data.items():
            if v.get("labelled") is not None:
                out[k]["raw"], out[k]["labelled"] = center_crop(v["raw"], size, v["labelled"])
            else:
                out[k]["raw"] = center_crop(v["raw"], size)
        return out

    def fit_transform(self, data):
        self.aug = int(self.size)
        return self.transform(data)


class Pipeline(PreProcessor):
    """A pipeline of PreProcessors: ``steps`` is a list of ``(class, keyword dict or None)``."""

    def __init__(self, steps: list) -> None:
        self.functions = []
        for step, arg in steps:
            if arg is not None:
                self.functions.append(step(**arg))
            else:
                self.functions.append(step())

    def transform(self, data):
        for function in self.functions:
            data = function.transform(data)
        return data

    def fit_transform(self, data):
        for function in self.functions:
            data = function.fit_transform(data)
        return data

    def batch(self, x):
        """The image steps on a device batch: (n,H,W) uint8 / float32 -> (n,H',W') float32, each image with its own statistics."""
        t, batched = _as_batch("Pipeline.batch", x)
        for function in self.functions:
            if not hasattr(function, "_batch"):
                raise ValueError(f"Pipeline.batch: {type(function).__name__} does not act on images")
            t = function._batch(t)
        if t.dtype != torch.float32:
            t = t.float()
        return t if batched else t[0]


class Preprocess:
    """``Preprocess(steps)(x)``: the callable form of ``Pipeline(steps).batch`` -- what ``infer.Segmenter(preprocess=...)`` takes."""

    def __init__(self, steps):
        self.pipeline = steps if isinstance(steps, Pipeline) else Pipeline(steps)
        for function in self.pipeline.functions:
            if not hasattr(function, "_batch"):
                raise ValueError(f"Preprocess: {type(function).__name__} does not act on images")

    def __call__(self, x):
        return self.pipeline.batch(x)


NORMALIZERS = {"none": None, "intensity": Intensity_normalizer, "minmax": MinMax_normalizer, "rows": skly_normalizer}


def from_options(crop=None, unsharp=None, preserve_range=False, normalize="none"):
    """The command line's pipeline, in the order crop -> unsharp -> normalise; None when no option is set.  ``unsharp``: (radius, amount)."""
    if normalize not in NORMALIZERS:
        raise ValueError(f"preprocess: normalize must be one of {sorted(NORMALIZERS)}, got {normalize!r}")
    steps = []
    if crop is not None:
        steps.append((Cropper, {"size": int(crop)}))
    if unsharp is not None:
        steps.append((Unsharper, {"radius": float(unsharp[0]), "amount": float(unsharp[1]), "preserve_range": bool(preserve_range)}))
    if NORMALIZERS[normalize] is not None:
        steps.append((NORMALIZERS[normalize], None))
    return Preprocess(steps) if steps else None
