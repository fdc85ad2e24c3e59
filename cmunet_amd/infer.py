"""Segmentation with a finetuned UNet: the step after ``train()`` has written ``best_model.pth``.

  load_segmentation_model(path_or_state, dtype, device)   a pickled module, a state dict, or a path to either -> UNet on the GPU
  Segmenter(model, size=256, batch=32, ...).segment(images)   images of any size -> uint8 masks at the images' own sizes
  segment_files(model, paths, out_dir)                    ``.npy`` images -> ``<stem>_mask.npy``
  python -m cmunet_amd.infer --model M --images DIR --out DIR [--size 256] [--batch 32] [--dtype f16] [--threshold 0.5]

Per chunk of same-sized images: the training pipeline's resize (``ops.resize_bicubic``: Pillow's bicubic in the image's own
arithmetic, mode 'F' for float32 / mode 'L' for uint8, as ``dataset.DeviceSegmentationBatch`` feeds finetuning) -> ``UNet.predict``
(the fused prediction head: no logits, no int64 argmax map) -> ``ops.resize_nearest`` back to the source size.  Everything runs on
the HIP kernels; there is no CPU fallback.
"""
import argparse
import os

import numpy as np
import torch

from . import ops
from .model import UNet, _EngineOwner, class_value_table


def _unet_geometry(sd):
    """(out_classes, base_ch, depth) of a UNet state dict (the reference's key names, Finetuning/model.py:84-108)."""
    try:
        out_classes = int(sd["conv_last.weight"].shape[0])
        base_ch = int(sd["down_conv1.double_conv.double_conv.0.weight"].shape[0])
    except KeyError as e:
        raise ValueError(f"not a UNet state dict: {e.args[0]} is missing") from None
    n_down = 0
    while f"down_conv{n_down + 1}.double_conv.double_conv.0.weight" in sd:
        n_down += 1
    return out_classes, base_ch, n_down + 1


def load_segmentation_model(path_or_state, dtype="f32", device="cuda"):
    """A UNet ready for ``predict``: from a pickled module (``torch.save(model)``, what ``train()`` writes), a state dict, or a path
    to either.  From a state dict the structure is inferred: ``out_classes`` from ``conv_last.weight``, ``base_ch`` from the first
    conv of ``down_conv1``, ``depth`` from the number of ``down_conv*`` blocks.  ``dtype``: the activations' storage type."""
    obj = path_or_state
    if isinstance(obj, (str, os.PathLike)):
        obj = torch.load(obj, map_location="cpu", weights_only=False)
    if isinstance(obj, torch.nn.Module):
        if not isinstance(obj, UNet):
            raise ValueError(f"expected a cmunet_amd UNet, got {type(obj).__name__}")
        model = obj
        for m in model.modules():      # the storage type is a property of the run, not of the checkpoint
            if isinstance(m, _EngineOwner):
                m.dtype = dtype
    elif isinstance(obj, dict):
        sd = obj["state_dict"] if "state_dict" in obj and "conv_last.weight" not in obj else obj
        out_classes, base_ch, depth = _unet_geometry(sd)
        model = UNet(out_classes=out_classes, base_ch=base_ch, depth=depth, dtype=dtype)
        model.load_state_dict(sd)
    else:
        raise ValueError(f"cannot load a segmentation model from {type(obj).__name__}")
    return model.to(device).eval()


def _depth(model):
    n = 0
    while hasattr(model, f"down_conv{n + 1}"):
        n += 1
    return n + 1


class Segmenter:
    """``segment(images)``: uint8 masks at each image's own size.

    ``size``: side the network runs at (the training pipeline's 256; None = each image's native size); ``batch``: images per
    network call; ``threshold``: probability threshold of a one-channel head; ``class_values``: max(out_classes, 2) integers in
    0..255 written instead of the class indices.  ``size`` -- every image under ``size=None`` -- must be a multiple of
    2**(depth-1)."""

    def __init__(self, model, size=256, batch=32, threshold=0.5, class_values=None):
        self.model, self.size, self.batch, self.threshold = model, size, int(batch), threshold
        self.mult = 1 << (_depth(model) - 1)
        if size is not None and (int(size) <= 0 or int(size) % self.mult):
            raise ValueError(f"Segmenter: size={size} must be a positive multiple of {self.mult} (UNet depth {_depth(model)})")
        if self.batch < 1:
            raise ValueError(f"Segmenter: batch={batch} must be at least 1")
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"Segmenter: threshold must lie inside (0, 1), got {threshold}")
        self.class_values = None if class_values is None else [int(v) for v in class_values]
        self._lut = None

    def _table(self, device):
        if self.class_values is None:
            return None
        if self._lut is None or self._lut.device != device:
            self._lut = class_value_table(self.class_values, self.model.conv_last.weight.shape[0], device)
        return self._lut

    def _chunk(self, src):
        """src (n,H,W) float32 / uint8 on the device -> (n,H,W) uint8.  Launches only: no host synchronisation."""
        H, W = src.shape[1:]
        S = self.size
        x = src if S is None or (H, W) == (S, S) else ops.resize_bicubic(src, S, S)
        if x.dtype == torch.uint8:      # 8-bit sources are resized in Pillow's mode-'L' arithmetic; the network reads float32
            x = x.float()
        lab = self.model.predict(x, threshold=self.threshold, class_values=self._table(src.device))
        return lab if tuple(lab.shape[1:]) == (H, W) else ops.resize_nearest(lab, H, W)

    def segment(self, images):
        """``images``: a list of 2-D arrays / tensors, or one (N,H,W) tensor; float32 or uint8, host or device, any sizes.  Returns
        a list of (H,W) uint8 cuda tensors in input order.  Images are grouped by (shape, dtype) and run in chunks of ``batch``."""
        dev = self.model.conv_last.weight.device
        if dev.type != "cuda":
            raise RuntimeError("Segmenter: the model must live on a CUDA/ROCm device; there is no CPU fallback in this package")
        items = []
        for im in (images.unbind(0) if torch.is_tensor(images) and images.dim() == 3 else images):
            t = im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))
            if t.dim() != 2:
                raise ValueError(f"Segmenter: every image must be 2-D, got {tuple(t.shape)}")
            if t.dtype != torch.uint8:
                t = t.float()
            if self.size is None and (t.shape[0] % self.mult or t.shape[1] % self.mult):
                raise ValueError(f"Segmenter(size=None): image {tuple(t.shape)} is not a multiple of {self.mult}")
            items.append(t)
        groups = {}
        for i, t in enumerate(items):
            groups.setdefault((tuple(t.shape), t.dtype), []).append(i)
        out = [None] * len(items)
        for idx in groups.values():
            for c0 in range(0, len(idx), self.batch):
                part = idx[c0:c0 + self.batch]
                src = torch.stack([items[i].to(dev, non_blocking=True) for i in part]).contiguous()
                for i, m in zip(part, self._chunk(src).unbind(0)):
                    out[i] = m
        return out


def segment_files(model, paths, out_dir, **kw):
    """Segment ``.npy`` images (2-D, float32 or uint8): writes ``<stem>_mask.npy`` (uint8, the image's size) into ``out_dir`` and
    returns the written paths in input order.  ``kw``: the ``Segmenter`` arguments."""
    seg = Segmenter(model, **kw)
    paths = [os.fspath(p) for p in paths]
    os.makedirs(out_dir, exist_ok=True)
    written = []
    step = seg.batch * 8      # bounded host memory: a few network batches of files at a time
    for c0 in range(0, len(paths), step):
        part = paths[c0:c0 + step]
        masks = seg.segment([np.load(p) for p in part])
        for p, m in zip(part, masks):
            dst = os.path.join(out_dir, os.path.splitext(os.path.basename(p))[0] + "_mask.npy")
            np.save(dst, m.cpu().numpy())
            written.append(dst)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cmunet_amd.infer", description="Segment .npy images with a finetuned UNet on the GPU.")
    ap.add_argument("--model", required=True, help="best_model.pth of train() (a pickled module) or a state-dict file")
    ap.add_argument("--images", required=True, help="directory of 2-D .npy images (float32 or uint8)")
    ap.add_argument("--out", required=True, help="directory the <stem>_mask.npy files are written to")
    ap.add_argument("--size", type=int, default=256, help="side the network runs at; 0 = each image's native size")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16", "bf16"], help="storage type of the activations")
    ap.add_argument("--threshold", type=float, default=0.5, help="probability threshold of a one-channel head")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("cmunet_amd.infer needs a ROCm GPU; there is no CPU fallback in this package")
    model = load_segmentation_model(args.model, dtype=args.dtype)
    paths = sorted(os.path.join(args.images, f) for f in os.listdir(args.images) if f.endswith(".npy"))
    written = segment_files(model, paths, args.out, size=args.size or None, batch=args.batch, threshold=args.threshold)
    print(f"{len(written)} masks written to {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
