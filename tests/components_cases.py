"""The case list of the connected-component tests (tests/test_cpu_components_ref.py, tests/test_gpu_components.py): the smallest
shapes at which a union-find on 32 x 32 tiles can still go wrong.  Masks are (H,W) uint8 0 / 1; references come from
tests/components_ref.py, computed once per (case, connectivity) and shared."""
import functools

import numpy as np

import components_ref as R

T = 32      # the kernels' tile side (csrc/components_uf.h CMU_CC_TILE): seams lie at multiples of it


def _rand(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


def _serpentine(n=96):
    m = np.zeros((n, n), np.uint8)
    m[::2] = 1                                        # every other row, joined alternately at the right and the left end
    for k, y in enumerate(range(1, n - 1, 2)):
        m[y, n - 1 if k % 2 == 0 else 0] = 1
    return m


def _spiral(n=96):
    m = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    while True:
        ny, nx = y + dy, x + dx
        # turn when the wall or an earlier arm (two ahead) is met
        ay, ax = ny + dy, nx + dx
        if not (0 <= ny < n and 0 <= nx < n) or (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                break
        y, x = ny, nx
        m[y, x] = 1
    return m


def _comb(H=70, W=45):
    m = np.zeros((H, W), np.uint8)
    m[:, ::2] = 1
    m[H - 1] = 1
    return m


def _ring(H, W, y0, x0, y1, x1, m=None, v=1):
    m = np.zeros((H, W), np.uint8) if m is None else m
    m[y0:y1 + 1, x0:x1 + 1] = v
    m[y0 + 1:y1, x0 + 1:x1] = 0
    return m


def _nested():
    m = _ring(70, 45, 2, 2, 66, 42)
    m[20:50, 10:36] = 1                               # island inside the hole ...
    m[25:45, 15:30] = 0                               # ... with a hole of its own
    m[33:36, 20:24] = 1                               # and an island in that
    return m


def _open_ring():
    m = _ring(70, 45, 0, 5, 40, 40)                   # its top side lies on the frame ...
    m[0, 20] = 0                                      # ... and a gap there opens the inside to the frame
    return m


def _diag_closed():
    m = np.zeros((40, 40), np.uint8)                  # a diamond outline: 8-connected, closed only diagonally
    c, r = 20, 9
    for d in range(r + 1):
        for sy, sx in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
            m[c + sy * d, c + sx * (r - d)] = 1
    return m


def _corner(points):
    m = np.zeros((2 * T, 2 * T), np.uint8)
    for y, x in points:
        m[y, x] = 1
    return m


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (H,W) uint8 mask; insertion order is the test order."""
    c = {}
    c["1x1_fg"] = np.ones((1, 1), np.uint8)
    c["1x1_bg"] = np.zeros((1, 1), np.uint8)
    c["1x70"] = _rand(1, 70, 0.6, 1)
    c["70x1"] = _rand(70, 1, 0.6, 2)
    for k, (H, W) in enumerate(((31, 33), (32, 32), (33, 65), (64, 64), (70, 45))):
        c[f"seam_{H}x{W}"] = _rand(H, W, 0.55, 10 + k)
    c["all_fg"] = np.ones((70, 45), np.uint8)
    c["all_bg"] = np.zeros((70, 45), np.uint8)
    c["corner_diag"] = _corner(((T - 1, T - 1), (T, T)))
    c["corner_anti"] = _corner(((T - 1, T), (T, T - 1)))
    c["corner_both"] = _corner(((T - 1, T - 1), (T, T), (T - 1, T), (T, T - 1)))
    c["checker_66"] = (np.add.outer(np.arange(66), np.arange(66)) % 2).astype(np.uint8)
    c["serpentine_96"] = _serpentine()
    c["spiral_96"] = _spiral()
    c["comb"] = _comb()
    c["ring"] = _ring(70, 45, 5, 5, 60, 40)
    c["nested_rings"] = _nested()
    c["open_ring"] = _open_ring()
    c["hole_near_frame"] = _ring(70, 45, 0, 0, 2, 2, _ring(70, 45, 30, 42, 34, 44))    # holes at (1,1) and one pixel from the right edge
    c["diag_closed"] = _diag_closed()
    for d in (0.3, 0.5, 0.59, 0.7):
        for seed in (0, 1, 2):
            c[f"rand_{d}_{seed}"] = _rand(130, 97, d, 100 + seed)
    c["rand_512"] = _rand(512, 512, 0.59, 7)
    return c


SMALL = tuple(k for k in cases() if k != "rand_512")      # the cases the clean-up steps are checked on as well


@functools.lru_cache(maxsize=None)
def ref_label(name, connectivity):
    """(labels int32 (H,W), count) of the reference, computed once; treat as read-only."""
    lab, n = R.label(cases()[name], connectivity)
    lab.setflags(write=False)
    return lab, n


def batch3():
    """Three different 70 x 45 images in one batch."""
    c = cases()
    return np.stack([c["seam_70x45"], c["comb"], c["nested_rings"]])
