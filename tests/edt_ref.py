"""Numpy / scipy reference for the exact Euclidean distance transform, the disk morphology and the surface-distance scores of
cmunet_amd (csrc/edt.hip), written independently of the kernels: a brute-force minimum over all sites where that is affordable,
``scipy.ndimage.distance_transform_edt`` beyond (tests/test_cpu_edt_ref.py pins the two to each other and the morphology to
scipy's).  Squared distances are exact integers; -1 at every pixel of an image that holds no site (the library's rule).
"""
import numpy as np

import components_ref as CR

BRUTE_LIMIT = 2 * 10 ** 7      # pixels x sites up to which the brute force runs


def rule(img, cls=-1):
    """cls in 0..255: img == cls; -1: img != 0; -2 - c: img != c (the codes of cmu_label_components)."""
    return CR.foreground(img, cls)


def complement(cls):
    return 0 if cls == -1 else (-2 - cls if cls >= 0 else -cls - 2)


def dist2_brute(sites):
    """(H,W) bool -> int32 squared distance to the nearest True pixel, by trying every one of them."""
    sites = np.asarray(sites, dtype=bool)
    H, W = sites.shape
    sy, sx = np.nonzero(sites)
    if sy.size == 0:
        return np.full((H, W), -1, np.int32)
    py, px = np.divmod(np.arange(H * W, dtype=np.int64), W)
    out = np.empty(H * W, np.int64)
    step = max(1, 4_000_000 // sy.size)
    for p0 in range(0, H * W, step):
        dy = py[p0:p0 + step, None] - sy[None, :]
        dx = px[p0:p0 + step, None] - sx[None, :]
        out[p0:p0 + step] = (dy * dy + dx * dx).min(1)
    return out.reshape(H, W).astype(np.int32)


def dist2_scipy(sites):
    from scipy import ndimage as ndi
    sites = np.asarray(sites, dtype=bool)
    if not sites.any():
        return np.full(sites.shape, -1, np.int32)
    d = ndi.distance_transform_edt(~sites)
    return np.rint(d * d).astype(np.int32)


def dist2(sites):
    sites = np.asarray(sites, dtype=bool)
    return dist2_brute(sites) if sites.size * int(sites.sum()) <= BRUTE_LIMIT else dist2_scipy(sites)


def squared_distance_transform(img, cls=-1, to="background"):
    return dist2(rule(img, cls if to == "foreground" else complement(cls)))


def edt(d2):
    """float32 root of an int32 squared-distance map, inf where it is -1."""
    with np.errstate(invalid="ignore"):
        r = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    return np.where(d2 < 0, np.float32(np.inf), r)


def disk_t(radius):
    return int(np.floor(float(radius) * float(radius)))


def disk(radius):
    """The structuring element {dy^2 + dx^2 <= radius^2} as a boolean array."""
    R = int(np.floor(radius))
    y, x = np.mgrid[-R:R + 1, -R:R + 1]
    return y * y + x * x <= disk_t(radius)


def _dilated(fg, t):
    d = dist2(fg)
    return (d >= 0) & (d <= t)


def _eroded(fg, t):
    d = dist2(~fg)
    return (d < 0) | (d > t)


def binary_dilation(mask, radius):
    m = np.asarray(mask, dtype=np.uint8)
    grown = _dilated(m != 0, disk_t(radius))
    return np.where(m != 0, m, grown.astype(np.uint8))


def binary_erosion(mask, radius):
    m = np.asarray(mask, dtype=np.uint8)
    return np.where(_eroded(m != 0, disk_t(radius)), m, 0).astype(np.uint8)


def binary_opening(mask, radius):
    m = np.asarray(mask, dtype=np.uint8)
    t = disk_t(radius)
    return np.where(_dilated(_eroded(m != 0, t), t), m, 0).astype(np.uint8)


def binary_closing(mask, radius):
    m = np.asarray(mask, dtype=np.uint8)
    t = disk_t(radius)
    closed = _eroded(_dilated(m != 0, t), t)
    return np.where(m != 0, m, closed.astype(np.uint8))


def clean_mask(label_map, classes=None, min_size=0, keep_largest=None, fill_holes=False, connectivity=8, class_values=None, num_classes=None,
               opening=0, closing=0):
    """components_ref.clean_mask with the two morphology steps in front of each class's three: pixels the opening drops go to class
    0, pixels the closing adds take the class."""
    cur = np.array(label_map, dtype=np.uint8)
    if classes is None:
        K = num_classes if num_classes is not None else (len(class_values) if class_values is not None else 2)
        classes = range(1, K)
    to, tc = disk_t(opening), disk_t(closing)
    for c in classes:
        if to > 0:
            cur[(cur == c) & ~_dilated(_eroded(cur == c, to), to)] = 0
        if tc > 0:
            cur[_eroded(_dilated(cur == c, tc), tc)] = c
        cur = CR.clean_mask(cur, [c], min_size, keep_largest, fill_holes, connectivity)
    if class_values is not None:
        lut = np.arange(256, dtype=np.uint8)
        lut[:len(class_values)] = np.asarray(class_values, dtype=np.uint8)
        cur = lut[cur]
    return cur


# ---- surface distances -------------------------------------------------------------------------------------------------------
def border(mask):
    """mask & ~binary_erosion(mask, cross, border_value=0): the rule of medpy and MONAI."""
    from scipy import ndimage as ndi
    m = np.asarray(mask) > 0
    return m & ~ndi.binary_erosion(m, structure=ndi.generate_binary_structure(2, 1), border_value=0)


def directed_dist2(a, b):
    """int32 squared distances from a's border pixels (row-major order) to the nearest border pixel of b; -1 if b has none."""
    return dist2(border(b))[border(a)]


def surface_distances(a, b, tolerance=1.0, percentile=95.0):
    """The scores of metrics.surface_distances for one image pair, as a dict of Python / numpy scalars, plus the two directed
    squared-distance vectors ('d2_ab', 'd2_ba')."""
    ab, ba = directed_dist2(a, b), directed_dist2(b, a)
    na, nb = int(ab.size), int(ba.size)
    out = {"n_pr": na, "n_gt": nb, "d2_ab": ab, "d2_ba": ba}
    if na == 0 and nb == 0:
        out.update(hd=0.0, hd_percentile=0.0, assd=0.0, nsd=1.0, mean_pr_to_gt=0.0, mean_gt_to_pr=0.0)
    elif na == 0 or nb == 0:
        inf = float("inf")
        out.update(hd=inf, hd_percentile=inf, assd=inf, nsd=0.0, mean_pr_to_gt=inf, mean_gt_to_pr=inf)
    else:
        dab, dba = np.sqrt(ab.astype(np.float64)), np.sqrt(ba.astype(np.float64))
        t2 = disk_t(tolerance)
        m_ab, m_ba = float(dab.mean()), float(dba.mean())
        out.update(hd=float(max(dab.max(), dba.max())), hd_percentile=float(np.percentile(np.hstack((dab, dba)), percentile)),
                   assd=(m_ab + m_ba) / 2.0, nsd=(int((ab <= t2).sum()) + int((ba <= t2).sum())) / (na + nb),
                   mean_pr_to_gt=m_ab, mean_gt_to_pr=m_ba)
    return out
