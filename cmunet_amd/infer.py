"""Segmentation with a finetuned UNet: the step after ``train()`` has written ``best_model.pth``.

  load_segmentation_model(path_or_state, dtype, device)   a pickled module, a state dict, or a path to either -> UNet on the GPU
  Segmenter(model, size=256, batch=32, ...).segment(images)   images of any size -> uint8 masks at the images' own sizes
  segment_files(model, paths, out_dir)                    ``.npy`` images -> ``<stem>_mask.npy``
  calibrate_threshold(segmenter, images, masks)           the threshold of ``Segmenter(threshold=, threshold_class=)`` from a validation split
  python -m cmunet_amd.infer --model M --images DIR --out DIR [--size 256] [--batch 32] [--dtype f16] [--threshold 0.5]
                              [--threshold-class C]
                              [--tile 256 [--stride 128] [--window gaussian] [--pad reflect]] [--tta d4]
                              [--min-size 50] [--keep-largest 2] [--fill-holes] [--connectivity 8] [--opening R] [--closing R]
                              [--crop 475] [--unsharp RADIUS AMOUNT [--preserve-range]] [--normalize {none,intensity,minmax,rows}]

Per chunk of same-sized images: the training pipeline's resize (``ops.resize_bicubic``: Pillow's bicubic in the image's own
arithmetic, mode 'F' for float32 / mode 'L' for uint8, as ``dataset.DeviceSegmentationBatch`` feeds finetuning) -> ``UNet.predict``
(the fused prediction head: no logits, no int64 argmax map) -> ``ops.resize_nearest`` back to the source size.  Everything runs on
the HIP kernels; there is no CPU fallback.

With ``tile`` and / or ``tta`` the chunk runs the tiled path instead (csrc/tiled_predict.hip): ``ops.extract_tiles`` cuts overlapping
windows (in every flip / rotation asked for) out of the padded image, ``UNet.predict_probs`` writes every class's probability of each
tile back in the image's frame, ``ops.blend_tiles`` sums them under a window in a fixed order and takes the argmax / threshold.
``size=None`` then means the image's own resolution, whatever its size.

With ``preprocess`` (a callable such as ``preprocess.Preprocess``: the reference's data_processing steps, csrc/preprocess.hip) every
device chunk of raw images passes through it first, so raw image -> mask is one call that never leaves the device; the masks then have
the PREPROCESSED size (the cropped one).
"""
import argparse
import math
import os

import numpy as np
import torch

from . import ops, postprocess
from . import preprocess as _preprocess
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


def tile_starts(L, T, stride):
    """Window starts along a side of length ``L`` for tiles of ``T``: ``[0]`` if the side fits in one tile (the tile is padded),
    else every ``stride`` from 0 while the tile ends before the side does, plus the last tile clamped to the end:
    tile_starts(475, 256, 128) == [0, 128, 219]."""
    L, T, stride = int(L), int(T), int(stride)
    if L < 1 or T < 1 or not 1 <= stride <= T:
        raise ValueError(f"tile_starts: need L >= 1, T >= 1 and 1 <= stride <= T, got L={L}, T={T}, stride={stride}")
    return [0] if L <= T else list(range(0, L - T, stride)) + [L - T]


WINDOWS = ("uniform", "gaussian")


def blend_window(T, kind="gaussian"):
    """The blending window along one side of a tile, (T,) float32 on the host: ``'uniform'`` all ones; ``'gaussian'`` centred on
    (T - 1) / 2 with sigma T / 8, normalised to maximum 1 (computed in float64, then cast)."""
    T = int(T)
    if T < 1:
        raise ValueError(f"blend_window: T={T} must be at least 1")
    if kind == "uniform":
        return torch.ones(T, dtype=torch.float32)
    if kind != "gaussian":
        raise ValueError(f"blend_window: kind must be one of {WINDOWS}, got {kind!r}")
    d = (np.arange(T, dtype=np.float64) - (T - 1) / 2.0) / (T / 8.0)
    w = np.exp(-0.5 * d * d)
    return torch.from_numpy((w / w.max()).astype(np.float32))


TTA_CODES = {"flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
# The probabilities of every (tile, copy) of the images blended together live in one float32 buffer (tiles x K' x T x T); images are
# blended in groups whose buffer stays under this many bytes (a single image may exceed it: it is then a group of its own).
PROB_BUDGET_BYTES = 1 << 30


class Segmenter:
    """``segment(images)``: uint8 masks at each image's own size.

    ``size``: side the network runs at (the training pipeline's 256; None = each image's native size); ``batch``: images per
    network call; ``threshold``: probability threshold of a one-channel head; ``class_values``: max(out_classes, 2) integers in
    0..255 written instead of the class indices.  ``size`` -- every image under ``size=None`` without ``tile`` -- must be a
    multiple of 2**(depth-1).

    Tiled path (``tile`` or ``tta`` given; with both None the calls above run exactly as before):
    ``tile``: side T of the square sliding window, a multiple of 2**(depth-1).  ``size``, when not None, is applied first (resize, then
    tile); ``size=None`` runs at the image's own resolution, for ANY image size (a side shorter than T is padded: ``pad`` =
    'reflect', without repeating the edge, or 'zero').  ``stride``: step of the window (default T // 2; 1 <= stride <= T); the last
    window is clamped to the image's end.  ``window``: 'gaussian' (sigma T / 8) or 'uniform' weights of a tile's pixels in the blend.
    ``tta``: None, 'flips' (the four flips), 'd4' (flips and 90-degree rotations: 8 copies) or a list of distinct dihedral codes (bit
    0 flips W, bit 1 flips H, bit 2 transposes): the class probabilities are averaged over the copies.  With ``tile=None`` and
    ``tta`` set every (resized) image is one tile of its own size (blended with uniform weights: one tile covers every pixel);
    transposing codes then need square images (ValueError).  The network runs on at most ``batch`` tiles per call.  A one-channel
    head thresholds the BLENDED probability.

    Clean-up (``min_size``, ``keep_largest`` or ``fill_holes`` given; with none of them the calls above run exactly as before):
    ``postprocess.clean_mask`` runs on every mask AT THE IMAGE'S OWN SIZE (after the nearest-neighbour resize back, so ``min_size``
    counts source pixels), on the plain and the tiled path, for every class but 0: components (``connectivity`` 4 or 8) of fewer
    than ``min_size`` pixels are removed, then only the ``keep_largest`` (1..8) largest stay, then holes are filled.  The network and
    blend passes then write class indices and the clean-up's last pass applies ``class_values``.  ``prob`` outputs are untouched.
    ``opening`` / ``closing`` (None, or the radius >= 0 of a Euclidean disk) belong to the same clean-up and switch it on as well: every
    class is opened, then closed (csrc/edt.hip: an exact distance transform, the cost does not grow with the radius), before the three
    steps above, so a vessel broken by a gap of a pixel or two is one component when ``keep_largest`` looks at it.

    ``preprocess`` (None: the calls above run exactly as before): a callable ``(n,H,W) uint8 / float32 device batch -> (n,H',W')`` --
    ``preprocess.Preprocess`` -- applied to every chunk before the resize / tiling.  Masks (and ``min_size``) are then at the
    preprocessed size H' x W', e.g. the cropped one, not the raw image's; the ``size=None`` multiple-of-2**(depth-1) rule applies to
    H' x W'.

    ``threshold_class`` (None: the calls above run exactly as before, the same bits): for a head of K >= 2 classes the mask is class C =
    ``threshold_class`` where the probability of class C exceeds ``threshold`` and class 0 elsewhere, instead of the argmax (on the tiled
    path the BLENDED probability): that class's probability is requested internally and ``ops.threshold_mask`` runs before the resize back
    and the clean-up; ``class_values`` and the clean-up apply as before.  ``calibrate_threshold`` picks the threshold.  ValueError for a
    one-channel head (its ``threshold`` already applies), C outside 1..K-1, and ``segment(prob_class=)`` naming another class."""

    def __init__(self, model, size=256, batch=32, threshold=0.5, class_values=None, tile=None, stride=None, window="gaussian",
                 pad="reflect", tta=None, min_size=None, keep_largest=None, fill_holes=False, connectivity=8, preprocess=None, opening=None, closing=None,
                 threshold_class=None):
        self.model, self.size, self.batch, self.threshold = model, size, int(batch), threshold
        self.threshold_class = None
        if threshold_class is not None:
            K = int(model.conv_last.weight.shape[0])
            if K < 2:
                raise ValueError("Segmenter: threshold_class is for a head of two or more classes; a one-channel head's threshold already applies")
            if isinstance(threshold_class, bool) or int(threshold_class) != threshold_class or not 1 <= int(threshold_class) <= K - 1:
                raise ValueError(f"Segmenter: threshold_class must lie in 1..{K - 1}, got {threshold_class!r}")
            self.threshold_class = int(threshold_class)
        self.mult = 1 << (_depth(model) - 1)
        if size is not None and (int(size) <= 0 or int(size) % self.mult):
            raise ValueError(f"Segmenter: size={size} must be a positive multiple of {self.mult} (UNet depth {_depth(model)})")
        if self.batch < 1:
            raise ValueError(f"Segmenter: batch={batch} must be at least 1")
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"Segmenter: threshold must lie inside (0, 1), got {threshold}")
        self.class_values = None if class_values is None else [int(v) for v in class_values]
        self._lut = None
        self.tile = None if tile is None else int(tile)
        if self.tile is not None and (self.tile <= 0 or self.tile % self.mult):
            raise ValueError(f"Segmenter: tile={tile} must be a positive multiple of {self.mult} (UNet depth {_depth(model)})")
        if stride is not None and self.tile is None:
            raise ValueError("Segmenter: stride needs tile")
        self.stride = None if self.tile is None else (self.tile // 2 if stride is None else int(stride))
        if self.stride is not None and not 1 <= self.stride <= self.tile:
            raise ValueError(f"Segmenter: stride={stride} must lie in 1..tile={self.tile}")
        if window not in WINDOWS:
            raise ValueError(f"Segmenter: window must be one of {WINDOWS}, got {window!r}")
        if pad not in ops.PAD_MODES:
            raise ValueError(f"Segmenter: pad must be one of {sorted(ops.PAD_MODES)}, got {pad!r}")
        self.window, self.pad = window, pad
        if tta is None:
            self.codes = None
        elif isinstance(tta, str):
            if tta not in TTA_CODES:
                raise ValueError(f"Segmenter: tta must be None, one of {sorted(TTA_CODES)} or a list of codes, got {tta!r}")
            self.codes = list(TTA_CODES[tta])
        else:
            self.codes = [int(c) for c in tta]
            if not self.codes or len(set(self.codes)) != len(self.codes) or any(not 0 <= c <= 7 for c in self.codes):
                raise ValueError(f"Segmenter: tta codes must be distinct integers in 0..7, got {list(tta)}")
        self.tiled = self.tile is not None or self.codes is not None
        self._grids = {}
        if min_size is not None and (isinstance(min_size, bool) or int(min_size) != min_size or int(min_size) < 0):
            raise ValueError(f"Segmenter: min_size must be None or an integer >= 0, got {min_size!r}")
        if keep_largest is not None and (isinstance(keep_largest, bool) or int(keep_largest) != keep_largest
                                         or not 1 <= int(keep_largest) <= ops.CC_MAX_KEEP):
            raise ValueError(f"Segmenter: keep_largest must be None or lie in 1..{ops.CC_MAX_KEEP}, got {keep_largest!r}")
        if not isinstance(fill_holes, bool):
            raise ValueError(f"Segmenter: fill_holes must be True or False, got {fill_holes!r}")
        if connectivity not in (4, 8):
            raise ValueError(f"Segmenter: connectivity must be 4 or 8, got {connectivity!r}")
        self.min_size = None if min_size is None else int(min_size)
        self.keep_largest = None if keep_largest is None else int(keep_largest)
        self.fill_holes, self.connectivity = fill_holes, connectivity
        for name, r in (("opening", opening), ("closing", closing)):
            if r is not None and (isinstance(r, bool) or not isinstance(r, (int, float)) or not math.isfinite(r) or r < 0):
                raise ValueError(f"Segmenter: {name} must be None or a real radius >= 0, got {r!r}")
        self.opening = None if opening is None else float(opening)
        self.closing = None if closing is None else float(closing)
        self.post = (self.min_size is not None or self.keep_largest is not None or self.fill_holes or self.opening is not None
                     or self.closing is not None)
        if preprocess is not None and not callable(preprocess):
            raise ValueError(f"Segmenter: preprocess must be None or a callable, got {type(preprocess).__name__}")
        self.preprocess = preprocess

    def _table(self, device, head=True):
        """The class-value table; ``head``: for the prediction head / the blend, which write class indices when the mask is cleaned
        afterwards (``cmu_filter_components`` applies the table instead: components are those of class indices)."""
        if self.class_values is None or (head and self.post):
            return None
        if self._lut is None or self._lut.device != device:
            self._lut = class_value_table(self.class_values, self.model.conv_last.weight.shape[0], device)
        return self._lut

    def _grid(self, H, W, device):
        """The tile grid + the two window vectors for (resized) images of H x W, built once per size (host checks, small uploads)."""
        key = (H, W, device)
        if key not in self._grids:
            TH, TW = (self.tile, self.tile) if self.tile is not None else (H, W)
            ys = tile_starts(H, TH, self.stride) if self.tile is not None else [0]
            xs = tile_starts(W, TW, self.stride) if self.tile is not None else [0]
            grid = ops.TileGrid(H, W, TH, TW, ys, xs, self.codes or (0,), device)
            kind = self.window if self.tile is not None else "uniform"
            self._grids[key] = (grid, blend_window(TH, kind).to(device), blend_window(TW, kind).to(device))
        return self._grids[key]

    def _chunk_tiled(self, x, prob_class):
        """x (n,H,W) float32 / uint8 on the device, any H, W -> (labels (n,H,W) uint8, prob (n,H,W) f32 or None)."""
        n, H, W = x.shape
        grid, wy, wx = self._grid(H, W, x.device)
        KP = max(int(self.model.conv_last.weight.shape[0]), 1)
        labels = torch.empty((n, H, W), dtype=torch.uint8, device=x.device)
        prob = torch.empty((n, H, W), dtype=torch.float32, device=x.device) if prob_class is not None else None
        per_image = grid.per_image * KP * grid.TH * grid.TW * 4
        group = max(1, min(n, PROB_BUDGET_BYTES // per_image))
        probs = torch.empty((group * grid.per_image, KP, grid.TH, grid.TW), dtype=torch.float32, device=x.device)
        tiles = torch.empty((group * grid.per_image, grid.TH, grid.TW), dtype=torch.float32, device=x.device)
        for g0 in range(0, n, group):
            g = min(group, n - g0)
            nt = g * grid.per_image
            ops.extract_tiles(x[g0:g0 + g], grid, self.pad, tiles[:nt])
            codes = grid.tile_codes(g) if self.codes is not None else None
            for c0 in range(0, nt, self.batch):
                c1 = min(c0 + self.batch, nt)
                self.model.predict_probs(tiles[c0:c1], None if codes is None else codes[c0:c1], probs[c0:c1])
            ops.blend_tiles(probs[:nt], grid, wy, wx, labels[g0:g0 + g], None if prob is None else prob[g0:g0 + g],
                            prob_class or 0, self.threshold, self._table(x.device))
        return labels, prob

    def _threshold_class_mask(self, prob):
        """Class ``threshold_class`` where its probability exceeds the threshold, class 0 elsewhere -- as class values when the head
        would have written them (no clean-up behind it)."""
        C = self.threshold_class
        v = self.class_values if self.class_values is not None and not self.post else None
        return ops.threshold_mask(prob, self.threshold, C if v is None else v[C], 0 if v is None else v[0])

    def _chunk(self, src, prob_class=None):
        """src (n,H,W) float32 / uint8 on the device -> (n,H,W) uint8, or (labels, prob) with ``prob_class`` (prob at the size the
        network ran at).  Launches only: no host synchronisation."""
        H, W = src.shape[1:]
        S = self.size
        x = src if S is None or (H, W) == (S, S) else ops.resize_bicubic(src, S, S)
        want_prob = prob_class is not None
        if self.threshold_class is not None:
            prob_class = self.threshold_class
        if self.tiled:
            lab, prob = self._chunk_tiled(x, prob_class)
        else:
            if x.dtype == torch.uint8:      # 8-bit sources are resized in Pillow's mode-'L' arithmetic; the network reads float32
                x = x.float()
            lab = self.model.predict(x, threshold=self.threshold, prob_class=prob_class, class_values=self._table(src.device))
            lab, prob = lab if prob_class is not None else (lab, None)
        if self.threshold_class is not None:
            lab = self._threshold_class_mask(prob)
            if not want_prob:
                prob_class = prob = None
        lab = lab if tuple(lab.shape[1:]) == (H, W) else ops.resize_nearest(lab, H, W)
        if self.post:      # on the mask at the image's own size: min_size counts source pixels
            K = max(int(self.model.conv_last.weight.shape[0]), 2)
            lab = postprocess.clean_mask(lab, range(1, K), self.min_size or 0, self.keep_largest, self.fill_holes, self.connectivity,
                                         self._table(src.device, head=False), opening=self.opening or 0, closing=self.closing or 0)
        return lab if prob_class is None else (lab, prob)

    def segment(self, images, prob_class=None):
        """``images``: a list of 2-D arrays / tensors, or one (N,H,W) tensor; float32 or uint8, host or device, any sizes.  Returns
        a list of (H,W) uint8 cuda tensors in input order.  Images are grouped by (shape, dtype) and run in chunks of ``batch``.
        With ``prob_class`` the list holds ``(mask, prob)`` pairs: ``prob`` is the float32 probability of that class (class 0 = the
        sigmoid for a one-channel head; on the tiled path the blended one) AT THE SIZE THE NETWORK RAN AT: the image's own size
        under ``size=None``, else ``size`` x ``size`` -- it is not resampled back."""
        K1 = max(int(self.model.conv_last.weight.shape[0]), 1)
        if prob_class is not None and not 0 <= int(prob_class) < K1:
            raise ValueError(f"Segmenter.segment: prob_class {prob_class} outside 0..{K1 - 1}")
        prob_class = None if prob_class is None else int(prob_class)
        if self.threshold_class is not None and prob_class not in (None, self.threshold_class):
            raise ValueError(f"Segmenter.segment: prob_class {prob_class} is not the threshold_class {self.threshold_class} of this Segmenter")
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
            if self.preprocess is None and self.size is None and self.tile is None and (t.shape[0] % self.mult or t.shape[1] % self.mult):
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
                if self.preprocess is not None:
                    src = self.preprocess(src)
                    if src.dim() != 3 or src.shape[0] != len(part) or src.dtype not in (torch.uint8, torch.float32):
                        raise ValueError(f"Segmenter: preprocess must return (n,H,W) uint8 / float32, got {tuple(src.shape)} {src.dtype}")
                    if self.size is None and self.tile is None and (src.shape[1] % self.mult or src.shape[2] % self.mult):
                        raise ValueError(f"Segmenter(size=None): preprocessed image {tuple(src.shape[1:])} is not a multiple of {self.mult}")
                    src = src.contiguous()
                res = self._chunk(src, prob_class)
                for j, i in enumerate(part):
                    out[i] = res[j] if prob_class is None else (res[0][j], res[1][j])
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


def calibrate_threshold(segmenter, images, masks, cls=1, bins=256, score="dice", beta=1.0):
    """The threshold of class ``cls`` that maximises ``score`` ('dice': F-beta with ``beta``, 'iou', 'youden') over a validation split:
    ``segmenter.segment(images, prob_class=cls)``; every uint8 label mask brought to its probability's size (the size the network ran at)
    with ``ops.resize_nearest``, the training pipeline's rule; ONE histogram pooled over all images, of any mix of sizes, on the device;
    ``metrics.best_threshold``.  Returns (threshold, sweep): the threshold j / bins as a Python float -- the single host synchronisation
    -- which lies inside (0, 1) and is valid for ``Segmenter(threshold=, threshold_class=cls)`` (one-channel head: ``threshold=``), and the
    ``metrics.threshold_sweep`` of the pooled histogram.  The sweep describes the probabilities (see ``metrics.threshold_sweep``)."""
    from . import metrics
    bins = ops.check_bins("calibrate_threshold", bins)
    items = list(images.unbind(0)) if torch.is_tensor(images) and images.dim() == 3 else list(images)
    labels = list(masks.unbind(0)) if torch.is_tensor(masks) and masks.dim() == 3 else list(masks)
    if not items or len(items) != len(labels):
        raise ValueError(f"calibrate_threshold: {len(items)} images for {len(labels)} masks")
    res = segmenter.segment(items, prob_class=cls)
    hist = None
    for (_, prob), m in zip(res, labels):
        m = m if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m))
        if m.dtype != torch.uint8 or m.dim() != 2:
            raise ValueError(f"calibrate_threshold: every mask must be a 2-D uint8 label map, got {tuple(m.shape)} {m.dtype}")
        m = m.to(prob.device)[None].contiguous()
        if tuple(m.shape[1:]) != tuple(prob.shape):
            m = ops.resize_nearest(m, prob.shape[0], prob.shape[1])
        # the one probability plane's "foreground" (label != 0): the pixels of class cls (a one-channel head: every non-zero label)
        y = m if int(segmenter.model.conv_last.weight.shape[0]) < 2 else (m == int(cls)).to(torch.uint8)
        hist = metrics.prob_histogram(prob[None].contiguous(), y, bins, None, pooled=True, out=hist)
    thr, _ = metrics.best_threshold(hist, 0, score, beta)
    return float(thr.item()), metrics.threshold_sweep(hist, beta=beta, score=score)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m cmunet_amd.infer", description="Segment .npy images with a finetuned UNet on the GPU.")
    ap.add_argument("--model", required=True, help="best_model.pth of train() (a pickled module) or a state-dict file")
    ap.add_argument("--images", required=True, help="directory of 2-D .npy images (float32 or uint8)")
    ap.add_argument("--out", required=True, help="directory the <stem>_mask.npy files are written to")
    ap.add_argument("--size", type=int, default=None,
                    help="side the network runs at (default 256; with --tile the default is the image's native size); 0 = native size")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16", "bf16"], help="storage type of the activations")
    ap.add_argument("--threshold", type=float, default=0.5, help="probability threshold of a one-channel head")
    ap.add_argument("--threshold-class", type=int, default=None, metavar="C",
                    help="K >= 2 classes: the mask is class C where its probability exceeds --threshold, class 0 elsewhere (not the argmax)")
    ap.add_argument("--tile", type=int, default=None, help="sliding-window inference with square tiles of this side (any image size)")
    ap.add_argument("--stride", type=int, default=None, help="step of the sliding window (default tile // 2)")
    ap.add_argument("--window", default="gaussian", choices=list(WINDOWS), help="weights of a tile's pixels where tiles overlap")
    ap.add_argument("--pad", default="reflect", choices=sorted(ops.PAD_MODES), help="fill of a tile past an image smaller than it")
    ap.add_argument("--tta", default="none", choices=["none"] + sorted(TTA_CODES),
                    help="test-time augmentation: average the probabilities over the flips / over flips and 90-degree rotations")
    ap.add_argument("--min-size", type=int, default=None, help="remove components of fewer than this many pixels of the source image")
    ap.add_argument("--keep-largest", type=int, default=None, help="keep only this many (1..8) largest components of each class")
    ap.add_argument("--fill-holes", action="store_true", help="fill the holes of each class")
    ap.add_argument("--connectivity", type=int, default=8, choices=[4, 8], help="connectivity of the components")
    ap.add_argument("--opening", type=float, default=None, metavar="R", help="open each class with a Euclidean disk of this radius first")
    ap.add_argument("--closing", type=float, default=None, metavar="R", help="then close each class with a disk of this radius (joins gaps)")
    ap.add_argument("--crop", type=int, default=None, metavar="SIZE", help="centre-crop every raw image to SIZE x SIZE first (the reference: 475)")
    ap.add_argument("--unsharp", type=float, nargs=2, default=None, metavar=("RADIUS", "AMOUNT"),
                    help=f"unsharp mask (skimage.filters.unsharp_mask) with this Gaussian radius (<= {_preprocess.PRE_MAX_RADIUS}) and amount")
    ap.add_argument("--preserve-range", action="store_true", help="with --unsharp: keep a uint8 image's 0..255 range and do not clip")
    ap.add_argument("--normalize", default="none", choices=sorted(_preprocess.NORMALIZERS),
                    help="per-image normalisation after crop and unsharp: (x - mean) / std, (x - min) / (max - min), or rows over their L2 norm")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.preserve_range and args.unsharp is None:
        raise SystemExit("--preserve-range needs --unsharp")
    pre = _preprocess.from_options(args.crop, args.unsharp, args.preserve_range, args.normalize)      # (None: the calls of before)
    if not torch.cuda.is_available():
        raise RuntimeError("cmunet_amd.infer needs a ROCm GPU; there is no CPU fallback in this package")
    model = load_segmentation_model(args.model, dtype=args.dtype)
    paths = sorted(os.path.join(args.images, f) for f in os.listdir(args.images) if f.endswith(".npy"))
    size = (None if args.tile else 256) if args.size is None else (args.size or None)
    written = segment_files(model, paths, args.out, size=size, batch=args.batch, threshold=args.threshold, tile=args.tile,
                            stride=args.stride, window=args.window, pad=args.pad, tta=None if args.tta == "none" else args.tta,
                            min_size=args.min_size, keep_largest=args.keep_largest, fill_holes=args.fill_holes, connectivity=args.connectivity,
                            preprocess=pre, opening=args.opening, closing=args.closing, threshold_class=args.threshold_class)
    print(f"{len(written)} masks written to {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
