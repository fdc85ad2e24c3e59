"""Pure-numpy / pure-Python reference for cmunet_amd.postprocess (csrc/components.hip), written independently of the kernels: a
raster-order flood fill instead of a union-find.  tests/test_cpu_components_ref.py pins it against scipy.ndimage.

Canonical labelling: 0 on background, else 1 + the smallest row-major index y * W + x of the pixel's component.  A raster scan meets
the smallest index of every component first, so the label of a fill is known when it starts.
"""
import numpy as np

N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def foreground(img, cls=-1):
    """cls in 0..255: img == cls; -1: img != 0; -2 - c: img != c."""
    img = np.asarray(img)
    if cls >= 0:
        return img == cls
    return img != 0 if cls == -1 else img != (-cls - 2)


def label(img, connectivity=8, cls=-1):
    """(H,W) -> (labels int32 (H,W), number of components)."""
    assert connectivity in (4, 8)
    fg = foreground(img, cls)
    H, W = fg.shape
    P = W + 2                                           # flat padded grid: a background frame makes every neighbour index valid
    pad = np.zeros((H + 2, P), dtype=bool)
    pad[1:-1, 1:-1] = fg
    todo = pad.ravel().tolist()
    offs = [dy * P + dx for dy, dx in (N4 if connectivity == 4 else N8)]
    out = [0] * len(todo)
    count = 0
    for s in np.flatnonzero(pad.ravel()).tolist():      # ascending: raster order
        if not todo[s]:
            continue
        count += 1
        lab = (s // P - 1) * W + (s % P - 1) + 1
        todo[s] = False
        out[s] = lab
        stack = [s]
        while stack:
            p = stack.pop()
            for o in offs:
                q = p + o
                if todo[q]:
                    todo[q] = False
                    out[q] = lab
                    stack.append(q)
    lab2 = np.asarray(out, dtype=np.int32).reshape(H + 2, P)[1:-1, 1:-1]
    return np.ascontiguousarray(lab2), count


def label_batch(imgs, connectivity=8, cls=-1):
    """(B,H,W) -> (labels (B,H,W) int32, counts (B,) int32)."""
    res = [label(m, connectivity, cls) for m in imgs]
    return np.stack([r[0] for r in res]), np.asarray([r[1] for r in res], dtype=np.int32)


def component_sizes(labels):
    """sizes in the shape of ``labels`` (H,W): flat entry r holds the pixel count of label r + 1."""
    n = labels.size
    return np.bincount(labels.ravel(), minlength=n + 1)[1:n + 1].astype(np.int32).reshape(labels.shape)


def select_largest(sizes, n):
    """The labels of the n largest components, largest first, ties to the smaller label; -1 in unused slots."""
    flat = sizes.ravel()
    idx = [int(i) for i in np.flatnonzero(flat)]
    idx.sort(key=lambda i: (-int(flat[i]), i))
    keep = [i + 1 for i in idx[:n]]
    return keep + [-1] * (n - len(keep))


def remove_small_objects(mask, min_size, connectivity=8, cls=-1):
    """Boolean (H,W): the foreground pixels whose component has at least ``min_size`` pixels."""
    lab, _ = label(mask, connectivity, cls)
    sizes = component_sizes(lab).ravel()
    return (lab > 0) & (sizes[np.maximum(lab, 1) - 1] >= min_size)


def keep_largest(mask, n=1, connectivity=8, cls=-1):
    lab, _ = label(mask, connectivity, cls)
    keep = [k for k in select_largest(component_sizes(lab), n) if k > 0]
    return np.isin(lab, keep) & (lab > 0)


def holes(fg):
    """Boolean (H,W): background pixels whose 4-connected background component does not touch the image's frame."""
    fg = np.asarray(fg, dtype=bool)
    lab, _ = label((~fg).astype(np.uint8), 4, -1)
    frame = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
    return (lab > 0) & ~np.isin(lab, frame[frame > 0])


def fill_holes(mask, cls=-1):
    fg = foreground(mask, cls)
    return fg | holes(fg)


def clean_mask(label_map, classes=None, min_size=0, keep_largest=None, fill_holes=False, connectivity=8, class_values=None, num_classes=None):
    """(H,W) uint8 class-index map -> cleaned uint8 map.  Per class of ``classes`` (default 1 .. number of classes - 1, the number
    being ``num_classes``, else len(class_values), else 2), in turn: remove components below ``min_size``, keep the ``keep_largest``
    largest (both send pixels to class 0), fill holes (filled pixels take the class).  ``class_values`` maps the indices at the end."""
    cur = np.array(label_map, dtype=np.uint8)
    if classes is None:
        K = num_classes if num_classes is not None else (len(class_values) if class_values is not None else 2)
        classes = range(1, K)
    for c in classes:
        lab, _ = label(cur, connectivity, c)
        sizes = component_sizes(lab).ravel()
        ok = lab > 0
        if min_size > 0:
            ok &= sizes[np.maximum(lab, 1) - 1] >= min_size
        if keep_largest is not None:
            left = np.where(sizes >= min_size, sizes, 0)            # the largest of what the first step left
            ok &= np.isin(lab, [k for k in select_largest(left, keep_largest) if k > 0])
        cur[(lab > 0) & ~ok] = 0
        if fill_holes:
            cur[holes(cur == c)] = c
    if class_values is not None:
        lut = np.arange(256, dtype=np.uint8)
        lut[:len(class_values)] = np.asarray(class_values, dtype=np.uint8)
        cur = lut[cur]
    return cur
