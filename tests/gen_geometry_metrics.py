#!/usr/bin/env python3
"""Writes tests/golden/geometry_metrics.npz: the reference's own ``hausdorff_distance_mask`` and ``compute_radius_arteries``
(Finetuning/metrics.py:224-293, 352-395) and scikit-image's ``find_contours`` / ``skeletonize`` on a set of binary masks, for
tests/test_cpu_geometry_metrics.py (the lattice restatement) and tests/test_gpu_geometry_metrics.py (the HIP kernels).

Needs an interpreter with scikit-image, scipy and numpy (torch is not needed: ``metrics.py`` is imported behind a minimal torch stub
created in a temp dir) and the reference tree:   python3 tests/gen_geometry_metrics.py /path/to/reference
The recorded library versions are an unpinned boundary: the reference pins scikit-image 0.24.0 (its requirements.txt).

Per mask: crossing count and closed-contour count (``find_contours(mask > 0)``: points = crossings + one repeat per closed contour),
the skeleton of the mask (bit-packed) and the radius triple (nan where the reference raises on an empty skeleton).
Per pair (prediction, ground truth): the modified and standard Hausdorff distances.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "geometry_metrics.npz")

_TORCH_STUB = '''
class _Any:
    def __init__(self, *a, **k): pass
    def __call__(self, *a, **k): return _Any()
    def __getattr__(self, n): return _Any()
def __getattr__(name): return _Any
'''
_NN_STUB = '''
from torch import _Any
class Module(_Any): pass
def __getattr__(name): return type(name, (Module,), {})
'''


def import_reference(ref):
    stub = tempfile.mkdtemp(prefix="torch_stub_")
    os.makedirs(os.path.join(stub, "torch", "nn"))
    with open(os.path.join(stub, "torch", "__init__.py"), "w") as f:
        f.write(_TORCH_STUB)
    with open(os.path.join(stub, "torch", "nn", "__init__.py"), "w") as f:
        f.write(_NN_STUB)
    with open(os.path.join(stub, "torch", "nn", "functional.py"), "w") as f:
        f.write("from torch import _Any\ndef __getattr__(name): return _Any\n")
    sys.path.insert(0, stub)
    sys.path.insert(0, os.path.join(ref, "Finetuning"))
    import metrics as ref_metrics  # noqa
    return ref_metrics


def disk_stamp(m, r, c, rad):
    H, W = m.shape
    r0, r1, c0, c1 = max(0, int(r - rad)), min(H, int(r + rad) + 2), max(0, int(c - rad)), min(W, int(c + rad) + 2)
    if r1 <= r0 or c1 <= c0:
        return
    yy, xx = np.mgrid[r0:r1, c0:c1]
    m[r0:r1, c0:c1] |= (yy - r) ** 2 + (xx - c) ** 2 <= rad * rad


def vessels(rs, H, W, n_trees=3, depth=3):
    """Thick branching random polylines, 1-8 px wide (half-widths 0.5-4), tapering with depth."""
    m = np.zeros((H, W), bool)

    def grow(r, c, ang, width, d):
        for _ in range(rs.randint(4, 9)):
            step = rs.uniform(4, 10)
            ang += rs.uniform(-0.5, 0.5)
            nr, nc = r + step * np.sin(ang), c + step * np.cos(ang)
            for t in np.linspace(0, 1, int(step * 2) + 2):
                disk_stamp(m, r + t * (nr - r), c + t * (nc - c), width)
            r, c = nr, nc
            if d > 0 and rs.rand() < 0.25:
                grow(r, c, ang + rs.choice([-1, 1]) * rs.uniform(0.5, 1.2), max(0.5, width * 0.7), d - 1)
    for _ in range(n_trees):
        grow(rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0, 2 * np.pi), rs.uniform(1.5, 4.0), depth)
    return m


def blobs(rs, H, W, n=4, holes=3):
    m = np.zeros((H, W), bool)
    for _ in range(n):
        disk_stamp(m, rs.uniform(0, H), rs.uniform(0, W), rs.uniform(H / 10, H / 4))
    for _ in range(holes):
        h = np.zeros_like(m)
        disk_stamp(h, rs.uniform(0, H), rs.uniform(0, W), rs.uniform(H / 30, H / 10))
        m &= ~h
    return m


def noisy(rs, gt, flip):
    """A first-epoch-like prediction: the ground truth with a fraction of its pixels flipped."""
    return gt ^ (rs.rand(*gt.shape) < flip)


def cases():
    rs = np.random.RandomState(20261016)
    masks, names, pairs = [], [], []

    def add(name, m):
        masks.append(np.ascontiguousarray(m, dtype=bool))
        names.append(name)
        return len(masks) - 1

    for p in (0.1, 0.5, 0.9):
        add(f"noise{p}_64", rs.rand(64, 64) < p)
    cb = (np.add.outer(np.arange(48), np.arange(48)) % 2) == 0
    add("checker_noise_48", cb ^ (rs.rand(48, 48) < 0.1))
    add("checker_48x40", ((np.add.outer(np.arange(48), np.arange(40)) % 2) == 0) ^ (rs.rand(48, 40) < 0.03))
    for k in range(3):
        add(f"vessels{k}_128", vessels(rs, 128, 128))
    for k in range(2):
        add(f"blobs{k}_96", blobs(rs, 96, 96))
    add("empty_16", np.zeros((16, 16), bool))
    add("full_16", np.ones((16, 16), bool))
    s = np.zeros((16, 16), bool)
    s[7, 9] = True
    add("single_16", s)
    s = np.zeros((16, 16), bool)
    s[0, 5] = True
    add("single_edge_16", s)
    b = np.zeros((8, 8), bool)
    b[3:5, 3:5] = True
    add("block2_8", b)
    b = np.zeros((9, 9), bool)
    b[3:6, 3:6] = True
    add("block3_9", b)
    t = blobs(rs, 64, 64, n=6, holes=2)
    t[:, :3] = True
    t[-2:, 20:40] = True
    add("border_touch_64", t)
    add("vessels_96x160", vessels(rs, 96, 160))
    add("noise_96x160", rs.rand(96, 160) < 0.3)
    add("vessels_160x96", vessels(rs, 160, 96))
    # pairs: (prediction, ground truth) as the metric is called
    a, b = add("pair_small_a", blobs(rs, 64, 64)), add("pair_small_b", blobs(rs, 64, 64))
    pairs.append((a, b))
    pairs.append((names.index("noise0.1_64"), names.index("noise0.5_64")))
    pairs.append((names.index("empty_16"), names.index("full_16")))          # both point sets empty -> 0
    pairs.append((names.index("empty_16"), names.index("single_16")))        # one empty -> inf
    pairs.append((names.index("single_16"), names.index("single_edge_16")))
    pairs.append((names.index("vessels_96x160"), names.index("noise_96x160")))
    for k, flip in enumerate((0.45, 0.2, 0.05, 0.0)):
        gt = vessels(rs, 256, 256, n_trees=4)
        pr = noisy(rs, gt, flip) if flip > 0 else blobs(rs, 256, 256)
        g, p = add(f"gt256_{k}", gt), add(f"pr256_{k}", pr)
        pairs.append((p, g))
    gt = vessels(rs, 512, 512, n_trees=6, depth=4)
    g, p = add("gt512", gt), add("pr512", noisy(rs, gt, 0.3))
    pairs.append((p, g))
    return masks, names, pairs


def main(ref):
    import scipy
    import skimage
    from skimage.measure import find_contours
    from skimage.morphology import skeletonize
    M = import_reference(ref)
    masks, names, pairs = cases()
    out = {"names": np.array(names), "pairs": np.array(pairs, dtype=np.int32),
           "versions": np.array([f"scikit-image {skimage.__version__}", f"scipy {scipy.__version__}", f"numpy {np.__version__}"])}
    n_cross, n_closed, radius = [], [], []
    for i, m in enumerate(masks):
        cs = find_contours(m > 0)
        closed = sum(1 for c in cs if len(c) > 1 and (c[0] == c[-1]).all())
        pts = sum(len(c) for c in cs)
        n_cross.append(pts - closed)
        n_closed.append(closed)
        try:
            rad = M.compute_radius_arteries(m.copy())
        except ValueError:              # np.min of an empty skeleton's radii
            rad = (np.nan, np.nan, np.nan)
        radius.append([float(v) for v in rad])
        out[f"mask_{i}"] = np.packbits(m, axis=None)
        out[f"skel_{i}"] = np.packbits(skeletonize(m), axis=None)
        out[f"shape_{i}"] = np.array(m.shape, np.int32)
        print(f"{names[i]:18s} {m.shape}  crossings {pts - closed:6d}  closed {closed:4d}  radius {radius[-1]}", flush=True)
    out["n_cross"] = np.array(n_cross, np.int64)
    out["n_closed"] = np.array(n_closed, np.int64)
    out["radius"] = np.array(radius, np.float64)
    hd = []
    for p, g in pairs:
        hd.append([float(M.hausdorff_distance_mask(masks[p], masks[g], method="modified")),
                   float(M.hausdorff_distance_mask(masks[p], masks[g], method="standard"))])
        print(f"pair {names[p]} / {names[g]}: modified {hd[-1][0]!r} standard {hd[-1][1]!r}", flush=True)
    out["hausdorff"] = np.array(hd, np.float64)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


def load(path=OUT):
    """The fixture as Python objects: masks / skeletons (bool arrays), names, pairs and the recorded values."""
    z = np.load(path)
    masks, skels = [], []
    for i in range(len(z["names"])):
        shp = tuple(int(v) for v in z[f"shape_{i}"])
        n = shp[0] * shp[1]
        masks.append(np.unpackbits(z[f"mask_{i}"])[:n].reshape(shp).astype(bool))
        skels.append(np.unpackbits(z[f"skel_{i}"])[:n].reshape(shp).astype(bool))
    return {"masks": masks, "skeletons": skels, "names": [str(s) for s in z["names"]], "pairs": z["pairs"].tolist(),
            "n_cross": z["n_cross"], "n_closed": z["n_closed"], "radius": z["radius"], "hausdorff": z["hausdorff"],
            "versions": [str(s) for s in z["versions"]]}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
