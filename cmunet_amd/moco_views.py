"""MoCo-v2's two augmented views (Pretraining/MoCo/pl_bolts/models/self_supervised/moco/moco_data_module.py:119-132, ``tau_g``) on the GPU.

The reference makes the query / key pair of every image with a torchvision pipeline applied twice per sample on the host:

    RandomApply([RandomRotation(180)], p=0.5)                                   NEAREST, centre, fill 0
    RandomResizedCrop(224, scale=(0.2, 1.0))                                    ratio (3/4, 4/3), bilinear, no antialias (0.14.0)
    RandomApply([GaussianBlur(kernel_size=(5, 9), sigma=(0.1, 2.0))], p=0.5)    reflect padding
    RandomHorizontalFlip(), RandomVerticalFlip()                                p = 0.5 each
    RandomApply([GaussNoise()], p=0.5)                                          out = image + max(image) / 10 * randn

Here a batch is three launches of csrc/moco_views.hip driven by one record per (image, view) (``REC_DTYPE``) that holds every random
decision: the Philox sampler writes the records, one pass does rotation, crop, resize, blur and flips and leaves each view's maximum in
device memory, and the noise pass reads it from there.  Nothing is synchronised with the host.  DESIGN.md 4.14 restates every rule; they
are torchvision 0.14.0's (the version the reference pins for MoCo) on a float tensor.  torchvision >= 0.17 antialiases tensor resizes by
default: ``MocoViewConfig(antialias=True)`` gives that behaviour (ATen's ``_upsample_bilinear2d_aa``).

The reference's ``tau_l`` (local crops) is built by its data module and never used (``MoCoDataset`` takes only ``tau_g``): it is left out.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import call
from .dataset import apply_overrides, check_probabilities, epoch_permutation

OP_ROTATION, OP_BLUR, OP_HFLIP, OP_VFLIP, OP_NOISE = 1, 2, 4, 8, 16

# include/cmunet_hip.h CmuMocoViewRec (40 bytes)
REC_DTYPE = np.dtype({
    "names": ["ops", "top", "left", "height", "width", "angle", "sigma"],
    "formats": ["<i4", "<i4", "<i4", "<i4", "<i4", "<f8", "<f8"],
    "offsets": [0, 4, 8, 12, 16, 24, 32],
    "itemsize": 40})

MAX_KSIZE = 9           # csrc/moco_views.hip MV_MAX_K (cmu_mocoviews_max_ksize)


def _range(v, name):
    lo, hi = (float(x) for x in v)
    if not 0.0 < lo <= hi:
        raise ValueError(f"{name} {v}: needs 0 < low <= high")
    return lo, hi


class MocoViewConfig:
    """The arguments of ``tau_g`` (moco_data_module.py:119-132); every probability and limit can be overridden by keyword.  ``size``: the
    side the raw images are resized to first (moco_data_set.py:31), ``out``: the views' side, ``antialias``: False = torchvision 0.14.0's
    tensor resize (the pinned version), True = the default of torchvision >= 0.17."""

    def __init__(self, **kw):
        self.p_rotation = 0.5                   # RandomApply([RandomRotation(180)], p=0.5)
        self.degrees = 180.0
        self.scale = (0.2, 1.0)                 # RandomResizedCrop(224, scale=(0.2, 1.0)); ratio default (3/4, 4/3)
        self.ratio = (3.0 / 4.0, 4.0 / 3.0)
        self.p_blur = 0.5                       # RandomApply([GaussianBlur(kernel_size=(5, 9), sigma=(0.1, 2.0))], p=0.5)
        self.kernel_size = (5, 9)               # (x, y)
        self.sigma = (0.1, 2.0)
        self.p_hflip = 0.5                      # RandomHorizontalFlip(), RandomVerticalFlip()
        self.p_vflip = 0.5
        self.p_noise = 0.5                      # RandomApply([GaussNoise()], p=0.5)
        self.size = 256
        self.out = 224
        self.antialias = False
        apply_overrides(self, kw)
        check_probabilities(self, ("p_rotation", "p_blur", "p_hflip", "p_vflip", "p_noise"))
        ks = (int(self.kernel_size),) * 2 if np.isscalar(self.kernel_size) else tuple(int(v) for v in self.kernel_size)
        if len(ks) != 2 or any(k < 1 or k % 2 != 1 for k in ks):
            raise ValueError(f"kernel_size {self.kernel_size}: needs two odd positive sizes (x, y)")
        if max(ks) > MAX_KSIZE:
            raise ValueError(f"kernel_size {self.kernel_size}: kernel sizes above {MAX_KSIZE} are not supported (the compile-time maximum "
                             "of the geometry pass's LDS halo)")
        self.kernel_size = ks
        self.scale = _range(self.scale, "scale")
        self.ratio = _range(self.ratio, "ratio")
        self.sigma = _range(self.sigma, "sigma")
        self.degrees = float(self.degrees)
        if self.degrees < 0.0:
            raise ValueError("degrees must not be negative")
        self.size, self.out = int(self.size), int(self.out)
        if self.size <= 0 or self.out <= max(ks) // 2:
            raise ValueError(f"size {self.size} / out {self.out}: size must be positive and out larger than the blur's reflection")
        self.antialias = bool(self.antialias)
        if self.antialias and self.size > 2 * self.out:
            raise ValueError(f"antialias takes crops of at most twice the output side (size {self.size}, out {self.out})")

    def params(self):
        """The 12 float64 parameters of cmu_mocoviews_sample, in the header's order."""
        return np.array([self.p_rotation, self.degrees, *self.scale, *self.ratio, self.p_blur, *self.sigma, self.p_hflip, self.p_vflip,
                         self.p_noise], dtype=np.float64)


def rec_layout():
    """(itemsize, offsets...) of CmuMocoViewRec as the library reports them."""
    buf = (ctypes.c_int64 * 16)()
    n = _lib.lib().cmu_mocoviews_rec_layout(buf, 16)
    return [int(buf[i]) for i in range(n)]


def _check_records(recs, B, S):
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    if recs.shape != (B, 2):
        raise ValueError(f"records: expected ({B}, 2) of REC_DTYPE, got {recs.shape}")
    t, l, h, w = (recs[k].astype(np.int64) for k in ("top", "left", "height", "width"))
    if (h < 1).any() or (w < 1).any() or (t < 0).any() or (l < 0).any() or (t + h > S).any() or (l + w > S).any():
        raise ValueError("records: crop boxes outside the image")
    if (recs["ops"] & OP_BLUR).astype(bool).any() and not (recs["sigma"][(recs["ops"] & OP_BLUR).astype(bool)] > 0).all():
        raise ValueError("records: a blurred view needs sigma > 0")
    return recs


class DeviceMocoViews:
    """``tau_g`` applied twice to every image of a batch on the GPU.

    ``views(raw)``: raw (B,H,W) float32 or uint8 cuda (resized to ``config.size`` with the Pillow bicubic of ``ops.resize_bicubic`` when
    it has another shape) -> (img_q, img_k), each (B,1,out,out) float32: what ``Moco_v2.training_step`` takes.  ``records``: a (B, 2)
    ``REC_DTYPE`` array that replaces the sampler; ``noise``: (2,B,out,out) float32 standard normals that replace the generator.  Each
    call draws from (seed, offset) and advances the offset by one: the same seed and offset give the same bits.  Requires the HIP
    library (no CPU fallback)."""

    def __init__(self, config=None, seed=0, offset=0):
        self.config = config if config is not None else MocoViewConfig()
        if not isinstance(self.config, MocoViewConfig):
            raise TypeError("config must be a MocoViewConfig")
        self._params = np.ascontiguousarray(self.config.params())
        self.seed, self.offset = int(seed) & (2 ** 64 - 1), int(offset)
        self.last_offset = None
        self._recs = self._vmax = None

    def _base(self, raw):
        if not torch.is_tensor(raw):
            raise TypeError("raw must be a torch tensor on the GPU")
        if not raw.is_cuda:
            raise ValueError("DeviceMocoViews runs on the GPU: raw must be a cuda tensor (there is no CPU path)")
        if raw.dtype not in (torch.float32, torch.uint8) or raw.dim() != 3:
            raise TypeError(f"raw must be (B,H,W) float32 or uint8, got {tuple(raw.shape)} {raw.dtype}")
        if raw.shape[0] < 1:
            raise ValueError("raw: empty batch")
        S = self.config.size
        raw = raw.contiguous()
        base = raw if tuple(raw.shape[1:]) == (S, S) else ops.resize_bicubic(raw, S, S)
        return base.float() if base.dtype == torch.uint8 else base

    def sample(self, B, device=None):
        """Draw the (B, 2) records with the device sampler (advances the offset; no host synchronisation) -> a (B * 2 * 40,) uint8
        device tensor (``records()`` reads them back)."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(dev):
            return self._records(None, int(B), dev)

    def _records(self, records, B, dev):
        S = self.config.size
        if records is not None:
            recs = torch.from_numpy(_check_records(records, B, S).view(np.uint8).reshape(-1).copy()).to(dev)
        else:
            recs = torch.empty(B * 2 * REC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            call("cmu_mocoviews_sample", ops._p(recs), B, S, S, self._params.ctypes.data_as(ctypes.c_void_p), len(self._params), self.seed,
                 self.offset, ops._stream())
        self._recs = recs
        self.last_offset = self.offset
        self.offset += 1
        return recs

    def views(self, raw, records=None, noise=None):
        base = self._base(raw)
        B, dev, O = base.shape[0], base.device, self.config.out
        if noise is not None:
            noise = noise if torch.is_tensor(noise) else torch.from_numpy(np.ascontiguousarray(noise))
            if noise.dtype != torch.float32 or tuple(noise.shape) != (2, B, O, O):
                raise ValueError(f"noise must be (2, {B}, {O}, {O}) float32 standard normals")
            noise = noise.to(dev).contiguous()
        with torch.cuda.device(dev):
            recs = self._records(records, B, dev)
            out = torch.empty(2, B, 1, O, O, dtype=torch.float32, device=dev)
            vmax = torch.empty(2 * B, dtype=torch.int32, device=dev)
            kx, ky = self.config.kernel_size
            S = self.config.size
            call("cmu_mocoviews_geometry", ops._p(base), B, S, S, ops._p(recs), kx, ky, int(self.config.antialias), ops._p(out), O,
                 ops._p(vmax), ops._stream())
            call("cmu_mocoviews_noise", ops._p(out), B, O, ops._p(recs), ops._p(vmax), ops._p(noise), self.seed, self.last_offset,
                 ops._stream())
            self._vmax = vmax
        return out[0], out[1]

    __call__ = views

    def records(self):
        """The last batch's records as a (B, 2) REC_DTYPE array (synchronises: tests and diagnostics)."""
        if self._recs is None:
            raise RuntimeError("no batch has been drawn yet")
        return self._recs.cpu().numpy().view(REC_DTYPE).reshape(-1, 2).copy()

    def maxima(self):
        """The last batch's per-view maxima before the noise, (B, 2) float32 on the device."""
        if self._vmax is None:
            raise RuntimeError("no batch has been augmented yet")
        B = self._vmax.numel() // 2
        out = torch.empty(B, 2, dtype=torch.float32, device=self._vmax.device)
        call("cmu_mocoviews_max", ops._p(self._vmax), ops._p(out), B, ops._stream())
        return out


class _ViewTransform:
    """One element of ``tau_g``: t(image (1,H,W)) -> one (1,out,out) view on the GPU (the first view of a one-image batch)."""

    def __init__(self, views):
        self.views = views

    def __call__(self, image):
        image = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        if image.dim() != 3 or image.shape[0] != 1:
            raise ValueError(f"expected one (1,H,W) image, got {tuple(image.shape)}")
        if not image.is_cuda:
            image = image.to(torch.device("cuda", torch.cuda.current_device()))
        if image.dtype not in (torch.float32, torch.uint8):
            image = image.float()
        return self.views.views(image)[0][0]


def get_moco_augmentation(seed=0, config=None):
    """The list the reference calls ``tau_g`` (moco_data_module.py:119-132): the same transform twice, each call an independent draw, so
    ``dataset.MoCoDataset(paths, get_moco_augmentation())`` works as in the reference."""
    t = _ViewTransform(DeviceMocoViews(config, seed=seed))
    return [t, t]


class _ViewLoader:
    """Batches ``((x_g0, x_g1), 0)`` over device-resident images: a fresh permutation per epoch drawn on the device from a seeded generator
    (every index once; ``drop_last`` drops the partial batch, as DataLoader does)."""

    def __init__(self, images, batch_size, views, shuffle, drop_last, seed=0):
        self.images, self.batch_size, self.views = images, int(batch_size), views
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self.seed, self.epoch = int(seed), 0
        self.idx = torch.arange(images.shape[0], device=images.device)
        self.last_order = None

    def __len__(self):
        n = self.images.shape[0]
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = self.idx
        if self.shuffle:
            order = epoch_permutation(len(order), self.seed, self.epoch, order.device)
        self.last_order = order
        self.epoch += 1
        for k in range(len(self)):
            sel = order[k * self.batch_size:(k + 1) * self.batch_size]
            yield self.views.views(self.images.index_select(0, sel)), 0


class MoCoDataModule:
    """moco_data_module.py:82-181 with the data on the device: ``data_dir`` is the list of ``.npy`` paths (what the reference ends up
    passing); ``setup("fit")`` loads every image once, resizes it to 256 x 256 on the GPU (Pillow bicubic, moco_data_set.py:31) and keeps
    the set in HBM; ``train_dataloader()`` yields ``((x_g0, x_g1), 0)`` per batch, each view (B,1,crop,crop) float32.  ``tau_l`` is not
    built (the reference never uses it); loader-process arguments (num_workers, pin_memory, ...) are accepted and ignored."""

    def __init__(self, data_dir=None, batch_size=64, shuffle=True, drop_last=True, global_crop_size=224, global_crop_scale=(0.2, 1.0),
                 device="cuda", seed=0, **kwargs):
        if data_dir is None or isinstance(data_dir, (str, bytes)) or not len(data_dir):
            raise ValueError("data_dir must be a non-empty list of .npy paths")
        self.data_dir = list(data_dir)
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), shuffle, drop_last
        self.global_crop_size, self.global_crop_scale = int(global_crop_size), tuple(global_crop_scale)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("MoCoDataModule keeps the data on the GPU: device must be a cuda device")
        self.device, self.seed = dev, int(seed)
        self.config = MocoViewConfig(out=self.global_crop_size, scale=self.global_crop_scale)
        self.views = DeviceMocoViews(self.config, seed=seed)
        self.tau_g = [_ViewTransform(self.views)] * 2
        self.images = self._loader = None

    def prepare_data(self):
        pass

    def setup(self, stage=None):
        if stage != "fit":
            print("Not implemented")
            return
        dev = self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        S = self.config.size
        out = []
        for p in self.data_dir:
            a = np.load(p)
            if a.ndim != 2:
                raise ValueError(f"{p}: expected a 2-D image, got {a.shape}")
            if a.dtype != np.uint8:
                a = a.astype(np.float32, copy=False)
            t = torch.from_numpy(np.ascontiguousarray(a))[None].to(dev)
            t = t if tuple(t.shape[1:]) == (S, S) else ops.resize_bicubic(t, S, S)
            out.append(t.float())
        self.images = torch.cat(out)
        self._loader = None

    def train_dataloader(self):
        if self.images is None:
            raise RuntimeError('call setup("fit") first')
        if self._loader is None:
            self._loader = _ViewLoader(self.images, self.batch_size, self.views, self.shuffle, self.drop_last, seed=self.seed)
        return self._loader


def pretrain_moco(data_dir, max_epochs=2, batch_size=64, model=None, seed=0, device="cuda", checkpoint=None, loss_scale=1.0, log=print,
                  **model_kw):
    """MoCo-v2 pretraining from a list of ``.npy`` images: MoCoDataModule + ``Moco_v2(**model_kw)`` + ``MocoPretrainer``, the cosine
    learning rate set per epoch.  ``checkpoint``: a ``.ckpt`` path written after the last epoch in Lightning's layout
    (``train.export_checkpoint(..., 'moco')``).  -> dict(losses = the per-epoch mean losses, model, trainer, datamodule)."""
    from .moco import Moco_v2
    from .pretrain import MocoPretrainer
    dm = MoCoDataModule(data_dir, batch_size=batch_size, device=device, seed=seed)
    dm.setup("fit")
    dev = dm.images.device
    if model is None:
        model = Moco_v2(batch_size=batch_size, **model_kw)
    model = model.to(dev)
    tr = MocoPretrainer(model)
    loader = dm.train_dataloader()
    if len(loader) == 0:
        raise ValueError(f"{len(dm.data_dir)} images make no batch of {batch_size} (drop_last)")
    losses = []
    buf = torch.zeros(len(loader), dtype=torch.float32, device=dev)
    for epoch in range(max_epochs):
        tr.set_epoch(epoch, max_epochs)
        for it, ((img_q, img_k), _) in enumerate(loader):
            buf[it:it + 1].copy_(tr.step(img_q, img_k, loss_scale=loss_scale).reshape(1))
        losses.append(float(buf.mean().item()))            # the epoch's one read-back
        log(f"Epoch {epoch + 1}/{max_epochs}, training loss {losses[-1]:.4f}, lr {tr.opt.lr:.5f}")
    if checkpoint is not None:
        from .train import export_checkpoint
        export_checkpoint(model.encoder_q.state_dict(), checkpoint, "moco", epoch=max_epochs,
                          extra={"global_step": max_epochs * len(loader)})
    return {"losses": losses, "model": model, "trainer": tr, "datamodule": dm}
