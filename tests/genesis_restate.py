"""Numpy restatement of the Genesis / MAE apply semantics driven by per-image records (cmunet_amd.genesis.REC_DTYPE): what
csrc/genesis.hip computes, written as the reference's array operations (utils.py:69-253).  Used by tests/test_cpu_genesis.py (against the
recorded reference batches) and tests/test_gpu_genesis.py (against the kernels fed with device-sampled records).  The Bezier helpers
(``bezier_kernel_order``, ``controls``, ``runs``) and the table ``BEZIER_CASES`` restate the kernel's own table arithmetic for
tests/test_gpu_genesis_tables.py; tests/test_cpu_genesis.py proves them against ``bezier`` and checks every case's run category."""
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


def bezier_kernel_order(P, n=NT):
    """The n samples of one cubic with control values P[0..3] in the order csrc/genesis.hip's gen_bezier evaluates them, in fp64:
    t = k / (n - 1) with the last t = 1, u = 1 - t, ((P0 t^3 + P1 3 t^2 u) + P2 3 t u^2) + P3 u^3 (k = 0 is the P3 end)."""
    P = [np.float64(v) for v in P]
    t = np.arange(n, dtype=np.float64) / np.float64(n - 1)
    t[-1] = 1.0
    u = 1.0 - t
    b0, b1, b2, b3 = t ** 3.0, (3.0 * (t * t)) * u, (3.0 * t) * (u * u), u ** 3.0
    return ((P[0] * b0 + P[1] * b1) + P[2] * b2) + P[3] * b3


def controls(mn, mx, bez):
    """-> (cx, cy): the control values of the x and the y cubic as gen_controls rounds them: c = float32(float32(r) * (mx - mn)) + mn
    in float32, every operation rounded on its own; cx = (mn, c0, c2, mx), cy = (mn, c1, c3, mx), as fp64 arrays."""
    mn, mx = np.float32(mn), np.float32(mx)
    with np.errstate(over="ignore"):
        d = np.float32(mx - mn)
        c = [np.float32(np.float32(np.float32(r) * d) + mn) for r in bez]
    return np.array([mn, c[0], c[2], mx], np.float64), np.array([mn, c[1], c[3], mx], np.float64)


def runs(v):
    """-> (number of monotone runs of v, the index of the first sample of every run but the first): a run ends where the sign of
    the next non-zero difference changes (zero differences belong to the run they sit in; no non-zero difference: one run)."""
    d = np.diff(np.asarray(v, np.float64))
    k = np.nonzero(d != 0)[0]
    s = np.sign(d[k])
    turn = np.nonzero(s[1:] != s[:-1])[0] + 1
    b = k[turn] + 1
    return len(b) + 1, b


def ulp32(x, n):
    """float32(x) moved n float32 steps up."""
    x = np.float32(x)
    for _ in range(n):
        x = np.nextafter(x, np.float32(np.inf))
    return x


# The Bezier tables the CPU proofs (test_cpu_genesis.py) and the kernel tests (test_gpu_genesis_tables.py) share:
# (group, name, mn, mx, the four draws, category of the x table, category of the y table).  A category is the number of monotone runs
# of the sampled cubic: "one", "few" (2 .. 16: the kernel's rank merge across runs) or "many" (> 16: its general sort).
# Draws in [0, 1) give monotone cubics; draws outside it give genuine three-run ones; ranges of a few float32 steps give cubics whose
# flat ends are rounding noise; one-step ranges and constant images give noise all along (a constant 0 gives 100,000 equal samples).
_D = (0.3, 0.6, 0.2, 0.9)
_LO, _HI = np.float32(-1.7), np.float32(2.9)
BEZIER_CASES = [
    ("ordinary", "draws", _LO, _HI, _D, "one", "one"),
    ("ordinary", "zeros", _LO, _HI, (0.0, 0.0, 0.0, 0.0), "one", "one"),
    ("ordinary", "ends", _LO, _HI, (0.999999, 0.0, 0.0, 0.999999), "one", "one"),
    ("ordinary", "halves", _LO, _HI, (0.5, 0.5, 0.5, 0.5), "one", "one"),
    ("three", "x", _LO, _HI, (1.5, 0.5, -0.5, 0.5), "few", "one"),
    ("three", "y", _LO, _HI, (0.5, 1.5, 0.5, -0.5), "one", "few"),
    ("three", "both", _LO, _HI, (1.5, 1.5, -0.5, -0.5), "few", "few"),
    ("three", "wide", _LO, _HI, (2.0, -1.0, -1.0, 2.0), "few", "few"),
    ("three", "x reversed", _LO, _HI, (-0.5, 0.5, 1.5, 0.5), "few", "one"),
    ("three", "double root", _LO, _HI, (1.0, 0.0, 0.0, 1.0), "few", "one"),
    # three-run cubics of the family (1.5, 0.5, -a, 0.5) (a scanned in steps of 0.0005) with a run that starts on the last (97) or the
    # first (0) sample of a thread's chunk, or one behind it (1: the sign change sits on the chunk's first difference, which only the
    # sign carried across the threads shows); the differences next to the turn are 1e-9, a million times the rounding noise
    ("seam", "97", _LO, _HI, (1.5, 0.5, -0.311, 0.5), "few", "one"),
    ("seam", "0", _LO, _HI, (1.5, 0.5, -0.379, 0.5), "few", "one"),
    ("seam", "1", _LO, _HI, (1.5, 0.5, -0.3315, 0.5), "few", "one"),
    ("fewulp", "0.75 + 2", ulp32(0.75, 0), ulp32(0.75, 2), _D, "one", "few"),
    ("fewulp", "100 + 2", ulp32(100, 0), ulp32(100, 2), _D, "one", "few"),
    ("fewulp", "-3 + 2", ulp32(-3, 0), ulp32(-3, 2), _D, "one", "few"),
    ("fewulp", "-3 + 3", ulp32(-3, 0), ulp32(-3, 3), _D, "one", "few"),
    ("overflow", "1.0 + 1", ulp32(1.0, 0), ulp32(1.0, 1), _D, "many", "many"),
    ("overflow", "0.75 + 1", ulp32(0.75, 0), ulp32(0.75, 1), _D, "many", "many"),
    ("overflow", "constant 1.0", np.float32(1.0), np.float32(1.0), _D, "many", "many"),
    ("overflow", "constant 0.3", np.float32(0.3), np.float32(0.3), _D, "many", "many"),
    ("overflow", "constant 1000", np.float32(1000), np.float32(1000), _D, "many", "many"),
    ("overflow", "constant 1e-3", np.float32(1e-3), np.float32(1e-3), _D, "many", "many"),
    ("overflow", "constant 0", np.float32(0), np.float32(0), _D, "one", "one"),
]
CHUNK = 98        # samples per thread of genesis_bezier_kernel's run scan: (NT + 1023) // 1024


def in_category(n, cat):
    return {"one": n == 1, "few": 2 <= n <= 16, "many": n > 16}[cat]


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
