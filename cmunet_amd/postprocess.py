"""Connected-component clean-up of predicted masks on the GPU (csrc/components.hip).

  label(mask, connectivity=8, cls=-1)          -> (labels int32, counts int32 per image)
  component_sizes(labels)                      -> int32 in the shape of ``labels``
  remove_small_objects(mask, min_size, connectivity=8)
  keep_largest(mask, n=1, connectivity=8)
  fill_holes(mask)
  clean_mask(label_map, classes=None, min_size=0, keep_largest=None, fill_holes=False, connectivity=8, class_values=None,
             opening=0, closing=0)

and the exact Euclidean distance transform with the disk morphology built on it (csrc/edt.hip):

  squared_distance_transform(mask, cls=-1, to="background")   -> int32, -1 where there is nothing to measure to
  distance_transform_edt(mask, cls=-1, to="background")       -> float32 (inf there)
  binary_dilation / binary_erosion / binary_opening / binary_closing(mask, radius)

Masks and label maps are uint8 ``(B,H,W)`` or ``(H,W)`` CUDA tensors; the result has the input's shape.  Every function only launches
kernels: no host synchronisation, no device-to-host read, no CPU fallback.  Every value is an integer, so results are exact and the
same on every call.

Labels are canonical: 0 on background, else 1 + the smallest row-major index ``y * W + x`` of the pixel's component within its image.
``counts[b]`` is -1 if the labelling of image ``b`` overran its trip bound (a defect of the kernels, never expected).
A binary mask's foreground is ``mask != 0``: kept foreground pixels keep their value, removed ones become 0, filled ones become 1.
"""
import math

import torch

from . import ops


def _as_batch(what, mask):
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise RuntimeError(f"postprocess.{what} runs on the GPU only; there is no CPU fallback in this package")
    if mask.dim() not in (2, 3):
        raise ValueError(f"postprocess.{what}: (H,W) or (B,H,W), got {tuple(mask.shape)}")
    return (mask if mask.dim() == 3 else mask.unsqueeze(0)).contiguous(), mask.dim() == 3


def _check(what, connectivity=8, n=None, min_size=0):
    if connectivity not in (4, 8):
        raise ValueError(f"postprocess.{what}: connectivity must be 4 or 8, got {connectivity!r}")
    if n is not None and (isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= ops.CC_MAX_KEEP):
        raise ValueError(f"postprocess.{what}: the number of components to keep must lie in 1..{ops.CC_MAX_KEEP}, got {n!r}")
    if min_size is None or isinstance(min_size, bool) or int(min_size) != min_size or int(min_size) < 0:
        raise ValueError(f"postprocess.{what}: min_size must be an integer >= 0, got {min_size!r}")


def label(mask, connectivity=8, cls=-1):
    """Connected components of ``mask != 0`` (``cls=-1``) or of ``mask == cls``: (labels int32 in the mask's shape, counts int32
    (B,), or 0-dim for an (H,W) mask)."""
    _check("label", connectivity)
    m, batched = _as_batch("label", mask)
    if m.dtype != torch.uint8:
        raise ValueError(f"postprocess.label: a uint8 mask, got {m.dtype}")
    labels, counts = ops.label_components(m, cls, connectivity)
    return (labels, counts) if batched else (labels[0], counts[0])


def component_sizes(labels):
    """``labels`` of ``label`` -> int32 of the same shape: flat entry ``r`` of an image is the pixel count of label ``r + 1``, 0 where no
    component has that label."""
    lab, batched = _as_batch("component_sizes", labels)
    sizes = ops.component_sizes(lab)
    return sizes if batched else sizes[0]


def _clean_class(cur, c, min_size, n, fill, connectivity, lut):
    """The three steps for class ``c`` of the (B,H,W) uint8 map ``cur``; ``lut`` rides on the last pass."""
    if min_size > 0 or n is not None:
        labels, _ = ops.label_components(cur, c, connectivity)
        sizes = ops.component_sizes(labels)
        keep = ops.select_largest(sizes, n) if n is not None else None
        cur = ops.filter_components(cur, c, labels, sizes, min_size, keep, 0, class_values=None if fill else lut)
    if fill:
        # holes of class c: 4-connected components of (cur != c) that do not touch the frame (scipy.ndimage.binary_fill_holes)
        hl, _ = ops.label_components(cur, -2 - c, 4)
        cur = ops.filter_components(cur, c, hole_labels=hl, hole_touches=ops.border_components(hl), class_values=lut)
    return cur


def _disk_t(what, name, radius):
    """floor(radius^2) of a real radius >= 0, computed once on the host: the disk is {dy^2 + dx^2 <= radius^2} and the squared
    distances are integers."""
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not math.isfinite(radius) or radius < 0:
        raise ValueError(f"postprocess.{what}: {name} must be a real number >= 0, got {radius!r}")
    return min(int(math.floor(float(radius) * float(radius))), 2 ** 31 - 1)


def _complement(cls):
    """The site-rule code of the pixels that do NOT satisfy ``cls``."""
    cls = int(cls)
    return 0 if cls == -1 else (-2 - cls if cls >= 0 else -cls - 2)


def _open_class(cur, c, t, g):
    """Opening of class ``c`` of the (B,H,W) map by the disk of squared radius ``t``: pixels the opening drops go to class 0."""
    ops.edt_columns(cur, _complement(c), g=g)                 # erosion: what lies within the disk of a pixel outside the class goes
    er = ops.edt_rows(g, "map", cur, True, t, -1, 0)
    ops.edt_columns(er, c, g=g)                               # dilation of what is left (never beyond the class: an opening)
    return ops.edt_rows(g, "map", er, False, t, c, -1)


def _close_class(cur, c, t, g):
    """Closing of class ``c``: pixels the closing adds take the class, whatever class they held."""
    ops.edt_columns(cur, c, g=g)
    di = ops.edt_rows(g, "map", cur, False, t, c, -1)
    ops.edt_columns(di, _complement(c), g=g)                  # erosion of the dilated class; what it drops falls back to its own value
    return ops.edt_rows(g, "map", cur, True, t, c, -1)


def _clean(what, mask, classes, min_size, n, fill, connectivity, lut, t_open=0, t_close=0):
    _check(what, connectivity, n, min_size)
    m, batched = _as_batch(what, mask)
    if m.dtype != torch.uint8:
        raise ValueError(f"postprocess.{what}: a uint8 map, got {m.dtype}")
    ops._cc_check(what, m, torch.uint8)
    classes = [int(c) for c in classes]
    if any(not 0 <= c <= 255 for c in classes):
        raise ValueError(f"postprocess.{what}: classes must lie in 0..255, got {classes}")
    active = int(min_size) > 0 or n is not None or fill
    cur = m
    if classes and (t_open > 0 or t_close > 0):
        ops._edt_check(what, m, torch.uint8)
        g = torch.empty(m.shape, dtype=torch.int32, device=m.device)
        for k, c in enumerate(classes):
            if t_open > 0:
                cur = _open_class(cur, c, t_open, g)
            if t_close > 0:
                cur = _close_class(cur, c, t_close, g)
            if active:
                cur = _clean_class(cur, c, int(min_size), None if n is None else int(n), bool(fill), connectivity,
                                   lut if k == len(classes) - 1 else None)
        if lut is not None and not active:
            cur = ops.filter_components(cur, 0, class_values=lut)
    elif classes and active:
        for k, c in enumerate(classes):
            cur = _clean_class(cur, c, int(min_size), None if n is None else int(n), bool(fill), connectivity, lut if k == len(classes) - 1 else None)
    elif lut is not None:
        cur = ops.filter_components(cur, 0, class_values=lut)
    else:
        cur = cur.clone()
    return cur if batched else cur[0]


def remove_small_objects(mask, min_size, connectivity=8):
    """Components of ``mask != 0`` with fewer than ``min_size`` pixels become 0 (a size equal to ``min_size`` stays).  Components are
    those of the whole foreground, whatever non-zero values it holds."""
    _check("remove_small_objects", connectivity, None, min_size)
    m, batched = _as_batch("remove_small_objects", mask)
    if m.dtype != torch.uint8:
        raise ValueError(f"postprocess.remove_small_objects: a uint8 mask, got {m.dtype}")
    labels, _ = ops.label_components(m, -1, connectivity)
    out = ops.filter_components(m, 0, labels, ops.component_sizes(labels), int(min_size))
    return out if batched else out[0]


def keep_largest(mask, n=1, connectivity=8):
    """Only the ``n`` (1..8) largest components of ``mask != 0`` stay; of equal sizes the one with the smaller label (the one whose
    first pixel in row-major order comes first) wins."""
    _check("keep_largest", connectivity, n)
    m, batched = _as_batch("keep_largest", mask)
    if m.dtype != torch.uint8:
        raise ValueError(f"postprocess.keep_largest: a uint8 mask, got {m.dtype}")
    labels, _ = ops.label_components(m, -1, connectivity)
    sizes = ops.component_sizes(labels)
    out = ops.filter_components(m, 0, labels, sizes, 0, ops.select_largest(sizes, int(n)))
    return out if batched else out[0]


def fill_holes(mask):
    """Background pixels that no 4-connected background path joins to the image's frame become 1 (the rule of
    ``scipy.ndimage.binary_fill_holes`` with its default structure)."""
    m, batched = _as_batch("fill_holes", mask)
    if m.dtype != torch.uint8:
        raise ValueError(f"postprocess.fill_holes: a uint8 mask, got {m.dtype}")
    hl, _ = ops.label_components(m, 0, 4)
    out = ops.filter_components(m, 1, hole_labels=hl, hole_touches=ops.border_components(hl))
    return out if batched else out[0]


def clean_mask(label_map, classes=None, min_size=0, keep_largest=None, fill_holes=False, connectivity=8, class_values=None, num_classes=None,
               opening=0, closing=0):
    """Clean a class-index map class by class: for every class of ``classes``, in turn, (1) components with fewer than ``min_size``
    pixels go to class 0, (2) of the rest only the ``keep_largest`` largest stay (None: all), (3) with ``fill_holes`` the holes of
    what is left take the class -- whatever class they held.  ``connectivity`` (4 / 8) is the foreground's in (1) and (2); holes
    are always 4-connected background.

    ``classes=None``: every class except 0, i.e. 1 .. K - 1 with K = ``num_classes``, else the length of ``class_values``, else 2
    (a binary map: class 1) -- the class count is not read back from the device.  ``class_values``: a sequence of integers in
    0..255, or a uint8 device table; index ``k`` of the cleaned map is written as ``class_values[k]``.

    ``opening`` / ``closing`` (radii of a Euclidean disk, 0 = off, the default: the calls are then exactly those above): for every class
    in turn the order is opening, closing, then the three steps.  Pixels of the class that its opening drops go to class 0; pixels that
    its closing adds take the class whatever class they held (the rule of ``fill_holes``).  A closing joins what a gap of up to about
    twice the radius separates, so ``keep_largest`` then keeps the whole vessel instead of its larger half."""
    t_open, t_close = _disk_t("clean_mask", "opening", opening), _disk_t("clean_mask", "closing", closing)
    lut = class_values
    if lut is not None and not torch.is_tensor(lut):
        vals = [int(v) for v in lut]
        if not vals or len(vals) > 256 or any(not 0 <= v <= 255 for v in vals):
            raise ValueError(f"postprocess.clean_mask: class_values must be 1..256 integers in 0..255, got {vals}")
        dev = label_map.device if torch.is_tensor(label_map) else "cuda"
        lut = torch.tensor(vals, dtype=torch.uint8).to(dev)
    elif lut is not None and (lut.dtype != torch.uint8 or lut.dim() != 1 or not 1 <= lut.numel() <= 256):
        raise ValueError("postprocess.clean_mask: a class_values tensor must be a uint8 vector of 1..256 entries")
    if classes is None:
        K = int(num_classes) if num_classes is not None else (int(lut.numel()) if lut is not None else 2)
        classes = range(1, K)
    return _clean("clean_mask", label_map, classes, min_size, keep_largest, fill_holes, connectivity, lut, t_open, t_close)


# ---- exact Euclidean distance transform and disk morphology (csrc/edt.hip) ----------------------------
def _edt_input(what, mask, cls=-1):
    m, batched = _as_batch(what, mask)
    if m.dtype != torch.uint8:
        raise ValueError(f"postprocess.{what}: a uint8 mask, got {m.dtype}")
    ops._edt_check(what, m, torch.uint8, cls)
    return m, batched


def _sites(what, cls, to):
    if to not in ("background", "foreground"):
        raise ValueError(f"postprocess.{what}: to must be 'background' or 'foreground', got {to!r}")
    return int(cls) if to == "foreground" else _complement(cls)


def squared_distance_transform(mask, cls=-1, to="background"):
    """Exact squared Euclidean distance, int32 in the mask's shape.  The rule ``cls`` names a set of pixels (``-1``: ``mask != 0``;
    0..255: ``mask == cls``; ``-2 - c``: ``mask != c``).  ``to="background"``: from every pixel to the nearest pixel of its image NOT
    in the set -- 0 outside the set, scipy's ``distance_transform_edt(mask) ** 2`` inside.  ``to="foreground"``: to the nearest pixel
    of the set.  An image with nothing to measure to holds -1 at every pixel."""
    sites = _sites("squared_distance_transform", cls, to)
    m, batched = _edt_input("squared_distance_transform", mask, cls)
    d2 = ops.edt_rows(ops.edt_columns(m, sites), "dist2")
    return d2 if batched else d2[0]


def distance_transform_edt(mask, cls=-1, to="background"):
    """``sqrt`` of ``squared_distance_transform`` as float32: the float64 root of the integer rounded once, bit for bit
    ``np.sqrt(d2.astype(np.float64)).astype(np.float32)``; ``inf`` where the squared distance is -1."""
    sites = _sites("distance_transform_edt", cls, to)
    m, batched = _edt_input("distance_transform_edt", mask, cls)
    d = ops.edt_rows(ops.edt_columns(m, sites), "dist")
    return d if batched else d[0]


def _dilate(m, t, base, v_hit, v_miss):
    return ops.edt_rows(ops.edt_columns(m, -1), "map", base, False, t, v_hit, v_miss)


def _erode(m, t, base, v_hit, v_miss):
    return ops.edt_rows(ops.edt_columns(m, 0), "map", base, True, t, v_hit, v_miss)


def _morph(what, mask, radius):
    t = _disk_t(what, "radius", radius)
    m, batched = _edt_input(what, mask)
    return m, batched, t, float(radius) == 0.0


def binary_dilation(mask, radius):
    """Dilation of ``mask != 0`` by the Euclidean disk ``dy^2 + dx^2 <= radius^2`` (``radius`` a real number >= 0; 0 returns a copy).
    Outside the image counts as background (scipy's ``border_value=0``).  Foreground pixels keep their value, added ones become 1.
    One transform, whatever the radius."""
    m, batched, t, copy = _morph("binary_dilation", mask, radius)
    out = m.clone() if copy else _dilate(m, t, m, 1, -1)
    return out if batched else out[0]


def binary_erosion(mask, radius):
    """Erosion of ``mask != 0`` by the disk.  Outside the image counts as foreground (scipy's ``border_value=1``): a vessel that leaves
    the frame is not eaten from there.  Kept pixels keep their value, removed ones become 0."""
    m, batched, t, copy = _morph("binary_erosion", mask, radius)
    out = m.clone() if copy else _erode(m, t, m, -1, 0)
    return out if batched else out[0]


def binary_opening(mask, radius):
    """Erosion, then dilation, with the border rules of ``binary_erosion`` and ``binary_dilation``: the result never exceeds the mask
    (anti-extensive).  Kept pixels keep their value."""
    m, batched, t, copy = _morph("binary_opening", mask, radius)
    out = m.clone() if copy else _dilate(_erode(m, t, m, -1, 0), t, m, -1, 0)
    return out if batched else out[0]


def binary_closing(mask, radius):
    """Dilation, then erosion, with the same border rules: the result always contains the mask (extensive).  Foreground pixels keep
    their value, added ones become 1."""
    m, batched, t, copy = _morph("binary_closing", mask, radius)
    if copy:
        out = m.clone()
    else:
        di = _dilate(m, t, m, 1, -1)
        out = _erode(di, t, di, -1, 0)
    return out if batched else out[0]
