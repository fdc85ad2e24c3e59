"""Numpy restatement of the Genesis / MAE apply semantics driven by per-image records (cmunet_amd.genesis.REC_DTYPE): what
csrc/genesis.hip computes, written as the reference's array operations (utils.py:69-253).  Used by tests/test_cpu_genesis.py (against the
recorded reference batches) and tests/test_gpu_genesis.py (against the kernels fed with device-sampled records)."""
import math

import numpy as np

from cmunet_amd.genesis import GF_FLIP0, GF_FLIP1, GF_LOCAL, GF_NONLIN, GF_SORTY, NT


def bezier(points, n=NT):
    """bezier_curve (utils.py:25-50) with math.comb (exact small integers, as scipy's comb returns them)."""
    xp = np.array([p[0] for p in points])
    yp = np.array([p[1] for p in points])
    t = np.linspace(0.0, 1.0, n)
    poly = np.array([math.comb(3, i) * (t ** (3 - i)) * (1 - t) ** i for i in range(4)])
    return np.dot(xp, poly), np.dot(yp, poly)


def nonlinear(x, bez, sort_y):
    mn, mx = np.min(x), np.max(x)
    r = [float(v) for v in bez]
    points = [[mn, mn], [r[0] * (mx - mn) + mn, r[1] * (mx - mn) + mn], [r[2] * (mx - mn) + mn, r[3] * (mx - mn) + mn], [mx, mx]]
    xv, yv = bezier(points)
    if sort_y:
        xv, yv = np.sort(xv), np.sort(yv)
    else:
        xv = np.sort(xv)
    return np.interp(x, xv, yv).astype(np.float32)


def flip(img, flags):
    if flags & GF_FLIP0:
        img = np.flip(img, axis=0)
    if flags & GF_FLIP1:
        img = np.flip(img, axis=1)
    return np.ascontiguousarray(img)


def shuffle(orig, blocks, perms):
    """local_pixel_shuffling: the last block covering a pixel wins; its value is orig[block origin + perm(p)]."""
    H, W = orig.shape
    owner = np.full((H, W), -1, np.int64)
    for k, (x0, y0, bx, by) in enumerate(blocks.astype(np.int64)):
        owner[x0:x0 + bx, y0:y0 + by] = k
    ii, jj = np.nonzero(owner >= 0)
    k = owner[ii, jj]
    x0, y0, by = blocks[k, 0].astype(np.int64), blocks[k, 1].astype(np.int64), blocks[k, 3].astype(np.int64)
    q = perms[k, (ii - x0) * by + (jj - y0)].astype(np.int64)
    out = orig.copy()
    out[ii, jj] = orig[x0 + q // by, y0 + q % by]
    return out


def paint(x, rec, noise):
    H, W = x.shape
    inside = np.zeros((H, W), bool)
    for q in range(int(rec["nrect"])):
        x0, y0, sx, sy = (int(v) for v in rec["rect"][q])
        inside[x0:x0 + sx, y0:y0 + sy] = True
    sel = inside if int(rec["paint"]) == 1 else ~inside
    out = x.copy()
    out[sel] = noise[sel]
    return out


def apply_genesis(src, recs, blocks, perms, noise, stages=("local", "nonlinear", "paint")):
    """-> (x, y) float32 (B, H, W).  ``noise`` (B, H, W): the paint values (the host replay's, or None to leave painted pixels
    as NaN -- for comparing device batches outside their Philox noise)."""
    B = len(recs)
    H, W = src.shape[1:]
    xs, ys = np.empty((B, H, W), np.float32), np.empty((B, H, W), np.float32)
    for b in range(B):
        r = recs[b]
        f = int(r["flags"])
        y = flip(src[int(r["src"])], f)
        x = y.copy()
        if f & GF_LOCAL and "local" in stages:
            x = shuffle(y, blocks[b], perms[b])
        if f & GF_NONLIN and "nonlinear" in stages:
            x = nonlinear(x, r["bez"], bool(f & GF_SORTY))
        if int(r["paint"]) and "paint" in stages:
            x = paint(x, r, noise[b] if noise is not None else np.full((H, W), np.nan, np.float32))
        xs[b], ys[b] = x, y
    return xs, ys


def apply_mae(src, recs, mask):
    y = src[recs["src"].astype(np.int64)]
    return y * (1 - mask), y
