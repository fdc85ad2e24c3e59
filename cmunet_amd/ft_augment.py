"""The finetuning training augmentation (Finetuning/dataset.py:134-165, ``get_training_augmentation``) on the GPU.

The reference trains every finetuning fold on an albumentations pipeline of six transforms, applied per sample on the host:

    RandomCrop(475, 475)                                          p = 1      image + mask
    GaussNoise(var_limit=(10, 50))                                p = 0.1    image
    GaussianBlur(blur_limit=(5, 11), sigma_limit=(0.5, 1.0))      p = 0.2    image
    RandomBrightnessContrast(brightness_limit=0.25)               p = 0.15   image
    Downscale(scale_min=0.5, scale_max=1.0)                       p = 0.25   image
    OneOf([HorizontalFlip, VerticalFlip, RandomRotate90, GaussNoise])  p = 0.75   flips / rot90: image + mask; noise: image

Here a batch is five launches of csrc/ft_augment.hip driven by one record per image (``REC_DTYPE``) that holds every random decision:
the Philox sampler writes the records, the photometric pass applies crop, noise, blur and brightness, and the resize pass composes
Downscale and OneOf into the source reads of SegmentationDataset's Pillow bicubic resize, gathers the mask through the same geometry
and writes its one-hot.  Nothing is synchronised with the host.  DESIGN.md 4.13 restates every rule (from the library's documented
behaviour; neither albumentations nor OpenCV is part of this build, so no rule has been checked against them).

The [0, 1] clip of GaussNoise and RandomBrightnessContrast (albumentations' maximum value of a float32 image) is replicated by default
(SURVEY Appendix A): on z-scored images it saturates every pixel of an image that either transform touches.  ``clip_float=False``
turns it off.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import call
from .dataset import apply_overrides, check_probabilities, epoch_permutation

OP_NOISE, OP_BLUR, OP_BRIGHTNESS_CONTRAST, OP_DOWNSCALE, OP_ONEOF = 1, 2, 4, 8, 16
ONEOF_HFLIP, ONEOF_VFLIP, ONEOF_ROT90, ONEOF_NOISE = 0, 1, 2, 3

# include/cmunet_hip.h CmuFtAugRec (72 bytes)
REC_DTYPE = np.dtype({
    "names": ["ops", "y0", "x0", "ksize", "var_noise", "var_oneof", "sigma", "alpha", "beta", "scale", "oneof", "rot_k"],
    "formats": ["<i4", "<i4", "<i4", "<i4", "<f8", "<f8", "<f8", "<f8", "<f8", "<f8", "<i4", "<i4"],
    "offsets": [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 68],
    "itemsize": 72})

MAX_CLASSES = 16        # csrc/ft_augment.hip FTA_MAX_CLASSES
MAX_KSIZE = 15          # FTA_MAX_K (cmu_ftaug_max_ksize)


def _pair(v, centre=0.0):
    """albumentations' to_tuple: a scalar limit l becomes (centre - l, centre + l)."""
    if np.isscalar(v):
        return (centre - float(v), centre + float(v))
    lo, hi = v
    return (float(lo), float(hi))


class FinetuneAugmentConfig:
    """The arguments of get_training_augmentation (dataset.py:146-161); every probability and limit can be overridden by keyword.
    ``clip_float``: the [0, 1] clip of the noise and brightness transforms (True = the reference's behaviour)."""

    def __init__(self, **kw):
        self.crop = 475                         # RandomCrop(height=475, width=475, always_apply=True)
        self.p_noise = 0.1                      # GaussNoise(var_limit=(10.0, 50.0), p=0.1)
        self.var_limit = (10.0, 50.0)
        self.p_blur = 0.2                       # GaussianBlur(blur_limit=(5, 11), sigma_limit=(0.5, 1.0), p=0.2)
        self.blur_limit = (5, 11)
        self.sigma_limit = (0.5, 1.0)
        self.p_brightness_contrast = 0.15       # RandomBrightnessContrast(brightness_limit=0.25, p=0.15); contrast_limit default 0.2
        self.brightness_limit = 0.25
        self.contrast_limit = 0.2
        self.p_downscale = 0.25                 # Downscale(scale_min=0.5, scale_max=1.0, p=0.25), INTER_NEAREST both ways
        self.scale_limit = (0.5, 1.0)
        self.p_oneof = 0.75                     # OneOf([HorizontalFlip, VerticalFlip, RandomRotate90, GaussNoise()], p=0.75)
        self.oneof_var_limit = (10.0, 50.0)     # GaussNoise()'s default var_limit
        self.clip_float = True
        apply_overrides(self, kw)
        klo, khi = (3, int(self.blur_limit)) if np.isscalar(self.blur_limit) else (int(v) for v in self.blur_limit)
        if not (1 <= klo <= khi) or khi % 2 != 1:
            raise ValueError(f"blur_limit {self.blur_limit}: needs 1 <= low <= high with an odd high")
        if khi > MAX_KSIZE:
            raise ValueError(f"blur_limit {self.blur_limit}: kernel sizes above {MAX_KSIZE} are not supported (the compile-time maximum "
                             "of the photometric pass's LDS halo)")
        self.blur_limit = (klo, khi)
        check_probabilities(self, ("p_noise", "p_blur", "p_brightness_contrast", "p_downscale", "p_oneof"))
        if int(self.crop) <= 0:
            raise ValueError("crop must be positive")
        if not 0.0 < _pair(self.scale_limit)[0] <= _pair(self.scale_limit)[1] <= 1.0:
            raise ValueError(f"scale_limit {self.scale_limit}: needs 0 < low <= high <= 1")

    def params(self):
        """The 19 float64 parameters of cmu_ftaug_sample, in the header's order."""
        b, c = _pair(self.brightness_limit), _pair(self.contrast_limit)
        return np.array([self.p_noise, *_pair(self.var_limit), self.p_blur, *self.blur_limit, *_pair(self.sigma_limit),
                         self.p_brightness_contrast, *b, *c, self.p_downscale, *_pair(self.scale_limit), self.p_oneof,
                         *_pair(self.oneof_var_limit)], dtype=np.float64)


def _check_records(recs, B, H, W, S):
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    if recs.shape != (B,):
        raise ValueError(f"records: expected ({B},) of REC_DTYPE, got {recs.shape}")
    if (recs["y0"] < 0).any() or (recs["y0"] > H - S).any() or (recs["x0"] < 0).any() or (recs["x0"] > W - S).any():
        raise ValueError("records: crop offsets outside the image")
    return recs


class DeviceTrainingAugmentation:
    """get_training_augmentation() followed by SegmentationDataset's resize and one-hot (dataset.py:44-55), for a batch on the GPU.

    ``aug(images, masks)``: images (B,H,W) float32 cuda (H, W >= config.crop), masks (B,H,W) uint8 cuda ->
    (image (B,size,size) float32, one-hot (B,n_cls,size,size) float64), the contract of ``DeviceSegmentationBatch``.  ``records``: a
    ``REC_DTYPE`` array that replaces the sampler; ``noise``: (2,B,crop,crop) float64 standard normals that replace the generator (plane 0:
    GaussNoise, plane 1: OneOf's GaussNoise).  Each call draws from (seed, offset) and advances the offset by one.
    ``aug(image=np, mask=np) -> {'image', 'mask'}``: albumentations' protocol for one sample (the augmented crop, before the resize), so
    the object can be handed to ``SegmentationDataset(augmentation=...)``.  Requires the HIP library (no CPU fallback)."""

    def __init__(self, config=None, size=256, class_values=(0, 1), seed=0, offset=0):
        self.config = config if config is not None else FinetuneAugmentConfig()
        self.size = int(size)
        vals = [int(np.asarray(v).reshape(-1)[0]) for v in class_values]
        if not 1 <= len(vals) <= MAX_CLASSES or any(v < 0 or v > 255 for v in vals):
            raise ValueError(f"class_values: 1 .. {MAX_CLASSES} values in 0 .. 255")
        self.class_values = vals
        self._cls = (ctypes.c_int * len(vals))(*vals)
        assert _lib.lib().cmu_ftaug_max_ksize() == MAX_KSIZE
        self._params = np.ascontiguousarray(self.config.params())
        self.seed, self.offset = int(seed) & (2 ** 64 - 1), int(offset)
        self.last_offset = None
        self._recs = None

    # -- checks ---------------------------------------------------------------------------------------------------------------------
    def _inputs(self, images, masks):
        if not torch.is_tensor(images) or not torch.is_tensor(masks):
            raise TypeError("images and masks must be torch tensors on the GPU")
        if not images.is_cuda or not masks.is_cuda:
            raise ValueError("DeviceTrainingAugmentation runs on the GPU: images and masks must be cuda tensors (there is no CPU path)")
        if images.dtype == torch.uint8:
            raise TypeError("uint8 images are not supported (the FAME2 images are z-scored float32)")
        if images.dtype != torch.float32 or images.dim() != 3:
            raise TypeError(f"images must be (B,H,W) float32, got {tuple(images.shape)} {images.dtype}")
        if masks.dim() != 3 or tuple(masks.shape) != tuple(images.shape):
            raise ValueError(f"masks {tuple(masks.shape)} must have the images' shape {tuple(images.shape)}")
        if masks.dtype != torch.uint8:
            if masks.dtype.is_floating_point or masks.dtype == torch.bool or masks.dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
                masks = masks.to(torch.uint8)
            else:
                raise TypeError(f"masks: unsupported dtype {masks.dtype}")
        if images.device != masks.device:
            raise ValueError("images and masks on different devices")
        S = int(self.config.crop)
        B, H, W = images.shape
        if H < S or W < S:
            raise ValueError(f"RandomCrop({S}, {S}) needs images of at least {S} x {S}, got {H} x {W}")
        return images.contiguous(), masks.contiguous(), B, H, W, S

    def _noise(self, noise, B, S, dev):
        if noise is None:
            return None
        noise = noise if torch.is_tensor(noise) else torch.from_numpy(np.ascontiguousarray(noise))
        if noise.dtype != torch.float64 or tuple(noise.shape) != (2, B, S, S):
            raise ValueError(f"noise must be (2, {B}, {S}, {S}) float64 standard normals")
        return noise.to(dev).contiguous()

    def sample(self, B, H, W, device=None):
        """Draw the records of a batch of B images of H x W with the device sampler (advances the offset; no host synchronisation).
        -> the records as a (B * 72,) uint8 device tensor (``records()`` reads them back)."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        S = int(self.config.crop)
        if H < S or W < S:
            raise ValueError(f"RandomCrop({S}, {S}) needs images of at least {S} x {S}, got {H} x {W}")
        with torch.cuda.device(dev):
            return self._records(None, int(B), int(H), int(W), S, dev)

    def _records(self, records, B, H, W, S, dev):
        """The batch's records on the device: uploaded from ``records`` or drawn by the sampler (no host synchronisation)."""
        if records is not None:
            recs = torch.from_numpy(_check_records(records, B, H, W, S).view(np.uint8).copy()).to(dev)
        else:
            recs = torch.empty(B * REC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            call("cmu_ftaug_sample", ops._p(recs), B, H, W, S, self._params.ctypes.data_as(ctypes.c_void_p), len(self._params), self.seed,
                 self.offset, ops._stream())
        self._recs = recs
        self.last_offset = self.offset
        self.offset += 1
        return recs

    def _photometric(self, images, recs, noise, B, H, W, S):
        P = torch.empty(B, S, S, dtype=torch.float32, device=images.device)
        call("cmu_ftaug_photometric", ops._p(images), B, H, W, ops._p(recs), ops._p(noise), self.seed, self.last_offset,
             int(bool(self.config.clip_float)), ops._p(P), S, ops._stream())
        return P

    # -- the batch paths ------------------------------------------------------------------------------------------------------------
    def __call__(self, images=None, masks=None, records=None, noise=None, **kw):
        if kw or images is None:
            return self._albumentations(**kw)
        images, masks, B, H, W, S = self._inputs(images, masks)
        dev = images.device
        with torch.cuda.device(dev):
            noise = self._noise(noise, B, S, dev)
            recs = self._records(records, B, H, W, S, dev)
            P = self._photometric(images, recs, noise, B, H, W, S)
            n = len(self.class_values)
            img = torch.empty(B, self.size, self.size, dtype=torch.float32, device=dev)
            onehot = torch.empty(B, n, self.size, self.size, dtype=torch.float64, device=dev)
            ws = ops.workspace("cmu_ftaug_resize_ws_bytes", dev, B, S, self.size)
            call("cmu_ftaug_resize_onehot", ops._p(P), ops._p(masks), B, H, W, ops._p(recs), ops._p(noise), self.seed, self.last_offset,
                 int(bool(self.config.clip_float)), self._cls, n, ops._p(img), ops._p(onehot), S, self.size, ops._p(ws), ops._stream())
        return img, onehot

    def augment_only(self, images, masks, records=None, noise=None):
        """The augmented crop before the resize: (image (B,crop,crop) float32, mask (B,crop,crop) uint8)."""
        images, masks, B, H, W, S = self._inputs(images, masks)
        dev = images.device
        with torch.cuda.device(dev):
            noise = self._noise(noise, B, S, dev)
            recs = self._records(records, B, H, W, S, dev)
            P = self._photometric(images, recs, noise, B, H, W, S)
            img = torch.empty(B, S, S, dtype=torch.float32, device=dev)
            lab = torch.empty(B, S, S, dtype=torch.uint8, device=dev)
            call("cmu_ftaug_apply", ops._p(P), ops._p(masks), B, H, W, ops._p(recs), ops._p(noise), self.seed, self.last_offset,
                 int(bool(self.config.clip_float)), ops._p(img), ops._p(lab), S, ops._stream())
        return img, lab

    def records(self):
        """The last batch's records as a REC_DTYPE array (synchronises: tests and diagnostics)."""
        if self._recs is None:
            raise RuntimeError("no batch has been augmented yet")
        return self._recs.cpu().numpy().view(REC_DTYPE).copy()

    def _albumentations(self, image=None, mask=None, **_):
        """albumentations' ``aug(image=, mask=) -> {'image', 'mask'}`` for one sample on the current GPU."""
        if image is None:
            raise TypeError("call as aug(image=..., mask=...) or aug(images, masks)")
        image = np.asarray(image)
        if image.dtype == np.uint8:
            raise TypeError("uint8 images are not supported (the FAME2 images are z-scored float32)")
        dev = torch.device("cuda", torch.cuda.current_device())
        m = np.zeros(image.shape, np.uint8) if mask is None else np.asarray(mask)
        if m.shape != image.shape:
            raise ValueError(f"mask {m.shape} must have the image's shape {image.shape}")
        if m.dtype != np.uint8:
            if not np.array_equal(m, np.round(m)) or m.min(initial=0) < 0 or m.max(initial=0) > 255:
                raise ValueError("mask values must be integers in 0 .. 255")
        x = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)[None]).to(dev)
        y = torch.from_numpy(np.ascontiguousarray(m.astype(np.uint8))[None]).to(dev)
        img, lab = self.augment_only(x, y)
        out = {"image": img[0].cpu().numpy()}
        if mask is not None:
            out["mask"] = lab[0].cpu().numpy().astype(m.dtype, copy=False)
        return out


def get_training_augmentation(seed=0):
    """The reference's factory name (Finetuning/dataset.py:134): the pipeline with the reference's arguments, on the GPU."""
    return DeviceTrainingAugmentation(FinetuneAugmentConfig(), seed=seed)


# ------------------------------------------------------------------------------------------------
# loaders for main_finetuning(make_loaders=...)
# ------------------------------------------------------------------------------------------------
class _DeviceLoader:
    """Batches of (image, one-hot) over ``idx`` of device-resident images / masks.  ``shuffle``: a fresh permutation per epoch drawn on
    the device from a seeded generator (every index once, the last partial batch kept, as DataLoader(shuffle=True)); ``transform``
    turns (images, masks) into the batch."""

    def __init__(self, images, masks, idx, batch_size, transform, shuffle, seed=0):
        self.images, self.masks = images, masks
        self.idx = torch.as_tensor(np.asarray(idx, dtype=np.int64)).to(images.device)
        self.batch_size, self.transform, self.shuffle = int(batch_size), transform, shuffle
        self.seed, self.epoch = int(seed), 0

    def __len__(self):
        return (len(self.idx) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.idx)
        order = self.idx
        if self.shuffle:
            order = self.idx.index_select(0, epoch_permutation(n, self.seed, self.epoch, self.images.device))
        self.epoch += 1
        for j in range(0, n, self.batch_size):
            sel = order[j:j + self.batch_size]
            yield self.transform(self.images.index_select(0, sel), self.masks.index_select(0, sel))


def device_finetune_loaders(image_paths, mask_paths, class_values, augmentation=None, device="cuda", seed=0):
    """A ``make_loaders(train_idx, val_idx, BATCH) -> (train_loader, test_loader)`` for ``train.main_finetuning`` that keeps the split in
    HBM: every ``.npy`` image (float32) and mask is loaded once.  The training loader augments each batch on the device (``augmentation``:
    a DeviceTrainingAugmentation, default get_training_augmentation(seed)); the validation loader runs DeviceSegmentationBatch in order.
    No device-to-host copy inside an epoch."""
    from .dataset import DeviceSegmentationBatch
    if len(image_paths) != len(mask_paths) or not len(image_paths):
        raise ValueError("image_paths and mask_paths must be non-empty lists of the same length")
    imgs = [np.load(p) for p in image_paths]
    msks = [np.load(p) for p in mask_paths]
    shape = imgs[0].shape
    for p, a, m in zip(image_paths, imgs, msks):
        if a.shape != shape or m.shape != shape:
            raise ValueError(f"{p}: image {a.shape} / mask {m.shape} differ from the first image's {shape}")
        if a.dtype != np.float32:
            raise TypeError(f"{p}: images must be float32 .npy files, got {a.dtype}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("device_finetune_loaders keeps the data on the GPU: device must be a cuda device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    images = torch.from_numpy(np.stack(imgs)).to(dev)
    m = np.stack(msks)
    if m.dtype != np.uint8:
        if not np.array_equal(m, np.round(m)) or m.min() < 0 or m.max() > 255:
            raise ValueError("mask values must be integers in 0 .. 255")
        m = m.astype(np.uint8)
    masks = torch.from_numpy(m).to(dev)
    class_values = list(class_values) if class_values is not None else [0, 1]
    aug = augmentation if augmentation is not None else DeviceTrainingAugmentation(class_values=class_values, seed=seed)
    val = DeviceSegmentationBatch(size=aug.size, class_values=class_values)
    calls = [0]

    def make_loaders(train_idx, val_idx, BATCH):
        calls[0] += 1
        train = _DeviceLoader(images, masks, train_idx, BATCH, aug, True, seed=seed * 7919 + calls[0])
        test = _DeviceLoader(images, masks, val_idx, BATCH, val, False)
        return train, test

    make_loaders.images, make_loaders.masks = images, masks
    return make_loaders
