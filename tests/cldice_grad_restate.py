"""Helpers of the differentiable soft-clDice tests (no test in here).

1. The AUTOGRAD restatement: K-class softmax -> kept channels -> ``oracle.losses.soft_skel`` -> clDice, in whatever dtype the
   logits have (fp64 is the reference; fp32 on the CPU measures what fp32 arithmetic costs, ``e32`` of the GPU tests).
2. The EXPLICIT restatement of the reverse sweep through the skeleton in numpy fp64, in gather form -- the model of
   ``cmu_soft_skeleton_bwd`` (csrc/cldice_grad.hip), with PyTorch autograd's sub-gradient rules written out:
     dilate (3x3 max, padding never wins): the whole gradient to the FIRST maximum in row-major window order;
     erode = min(column min, row min): the column window's gradient to its first minimum (top, centre, bottom), the row window's
     to its first (left, centre, right); equal minima take half each, else the smaller takes all;
     relu'(0) = 0.
3. The tie-rich input planes both test files use.
"""
import numpy as np
import torch

from oracle import losses as OL


# ------------------------------------------------------------------------------------------------
# 1. autograd restatement
# ------------------------------------------------------------------------------------------------
def kept_channels(K, ignore_channels=None, exclude_background=False):
    """Channels that reach the skeletons: _take_channels(ignore_channels), then [:, 1:] if exclude_background."""
    keep = [c for c in range(K) if c not in (ignore_channels or ())]
    return keep[1:] if exclude_background else keep


def cldice_of_planes(yp, yt, smooth=1.0, num_iter=10):
    """clDice of (B,Kk,H,W) prediction / target planes (metrics.py:424-429)."""
    sp, st = OL.soft_skel(yp, num_iter), OL.soft_skel(yt, num_iter)
    tprec = ((sp * yt).sum() + smooth) / (sp.sum() + smooth)
    tsens = ((st * yp).sum() + smooth) / (st.sum() + smooth)
    return 1.0 - 2.0 * (tprec * tsens) / (tprec + tsens)


def cldice(logits, y, ignore_channels=None, exclude_background=False, smooth=1.0, num_iter=10, threshold=None):
    """The reference's soft_cldice(activation='softmax') on (B,K,H,W) logits and targets of one dtype."""
    keep = torch.tensor(kept_channels(logits.shape[1], ignore_channels, exclude_background))
    p = torch.softmax(logits, dim=1)
    if threshold is not None:
        p = (p > threshold).to(p.dtype)
    return cldice_of_planes(p.index_select(1, keep), y.index_select(1, keep), smooth, num_iter)


def skel_grad_autograd(img, g, num_iter, dtype=torch.float64):
    """d<g, soft_skel(img)>/dimg by autograd; img, g: (P,H,W) arrays."""
    x = torch.as_tensor(np.asarray(img)).to(dtype).unsqueeze(1).clone().requires_grad_(True)
    sk = OL.soft_skel(x, num_iter)
    sk.backward(torch.as_tensor(np.asarray(g)).to(dtype).unsqueeze(1))
    return x.grad[:, 0].numpy(), sk.detach()[:, 0].numpy()


# ------------------------------------------------------------------------------------------------
# 2. explicit reverse sweep, gather form (numpy fp64)
# ------------------------------------------------------------------------------------------------
def _sh(a, dy, dx, pad):
    """b[..., y, x] = a[..., y + dy, x + dx], ``pad`` outside."""
    H, W = a.shape[-2:]
    b = np.full_like(a, pad)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        b[..., ys:ye, xs:xe] = a[..., ys + dy:ye + dy, xs + dx:xe + dx]
    return b


def _erode(a):
    m = a
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        m = np.minimum(m, _sh(a, dy, dx, np.inf))
    return m


def _dilate(a):
    m = a
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m = np.maximum(m, _sh(a, dy, dx, -np.inf))
    return m


def _dilate_first(a):
    """Code 3 (dy + 1) + (dx + 1) of the first maximum of every 3x3 window, row-major, strict '>' (padding never wins)."""
    mx = np.full_like(a, -np.inf)
    sel = np.full(a.shape, -1, np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v = _sh(a, dy, dx, -np.inf)
            win = v > mx
            mx = np.where(win, v, mx)
            sel = np.where(win, 3 * (dy + 1) + (dx + 1), sel)
    return sel


def _dilate_gather(gD, im):
    """Pixel q collects gD[p] from every window p (a 3x3 neighbour of q, inside the image) whose first maximum is q."""
    sel = _dilate_first(im)
    out = np.zeros_like(gD)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            # p = q + (dy, dx); q sits at (-dy, -dx) of p's window
            hit = _sh(sel, dy, dx, -1) == 3 * (1 - dy) + (1 - dx)
            out = out + np.where(hit, _sh(gD, dy, dx, 0.0), 0.0)
    return out


def _erode_select(im):
    """Per window p: index (0, 1, 2) of the first minimum of (top, centre, bottom) and of (left, centre, right), and the weights
    of the column and the row window (1 / 0.5 / 0)."""
    col = [_sh(im, -1, 0, np.inf), im, _sh(im, 1, 0, np.inf)]
    row = [_sh(im, 0, -1, np.inf), im, _sh(im, 0, 1, np.inf)]

    def first_min(c):
        m, s = c[0], np.zeros(im.shape, np.int64)
        for i in (1, 2):
            less = c[i] < m
            m = np.where(less, c[i], m)
            s = np.where(less, i, s)
        return m, s
    m1, cs = first_min(col)
    m2, rs = first_min(row)
    wc = np.where(m1 < m2, 1.0, np.where(m1 == m2, 0.5, 0.0))
    return cs, rs, wc, 1.0 - wc


def _erode_gather(T, im):
    """Pixel q collects from the five windows whose column or row contains it."""
    cs, rs, wc, wr = _erode_select(im)
    cT, rT = wc * T, wr * T
    out = np.where(_sh(cs, -1, 0, -1) == 2, _sh(cT, -1, 0, 0.0), 0.0)          # bottom of the window above
    out = out + np.where(_sh(rs, 0, -1, -1) == 2, _sh(rT, 0, -1, 0.0), 0.0)    # right end of the window to the left
    out = out + np.where(cs == 1, cT, 0.0) + np.where(rs == 1, rT, 0.0)       # centre of its own windows
    out = out + np.where(_sh(rs, 0, 1, -1) == 0, _sh(rT, 0, 1, 0.0), 0.0)      # left end of the window to the right
    out = out + np.where(_sh(cs, 1, 0, -1) == 0, _sh(cT, 1, 0, 0.0), 0.0)      # top of the window below
    return out


def skel_forward(img, num_iter):
    """(levels img_0..img_{N+1}, running skeletons skel_0..skel_N), fp64."""
    lev = [np.asarray(img, np.float64)]
    for _ in range(num_iter + 1):
        lev.append(_erode(lev[-1]))
    sk = []
    for j in range(num_iter + 1):
        delta = np.maximum(lev[j] - _dilate(lev[j + 1]), 0.0)
        sk.append(delta if j == 0 else sk[-1] + np.maximum(delta - sk[-1] * delta, 0.0))
    return lev, sk


def skel_grad_explicit(img, g, num_iter):
    """d<g, soft_skel(img)>/dimg: levels deepest first.  A_j: what delta_j hands to img_j directly; gD_j: what it hands to
    dilate(img_{j+1}); T_m: the whole gradient of img_m = gD_{m-1} gathered through the dilate + A_m + T_{m+1} gathered through
    the erode (one erode per level stands for the reference's two: same function of img_j, their gradients add)."""
    N = num_iter
    lev, sk = skel_forward(img, N)
    gs = np.asarray(g, np.float64)
    A, gD = [None] * (N + 1), [None] * (N + 1)
    for j in range(N, -1, -1):
        raw = lev[j] - _dilate(lev[j + 1])
        delta = np.maximum(raw, 0.0)
        if j > 0:
            s = sk[j - 1]
            on = (delta - s * delta) > 0.0
            gd = np.where(on, gs - gs * s, 0.0)
            gs = np.where(on, gs - gs * delta, gs)
        else:
            gd = gs
        A[j] = np.where(raw > 0.0, gd, 0.0)
        gD[j] = np.where(raw > 0.0, -gd, 0.0)
    T = _dilate_gather(gD[N], lev[N + 1])                                      # T_{N+1}
    for m in range(N, 0, -1):
        T = _dilate_gather(gD[m - 1], lev[m]) + A[m] + _erode_gather(T, lev[m])
    return A[0] + _erode_gather(T, lev[0])


# ------------------------------------------------------------------------------------------------
# 3. inputs chosen for ties (all values fp32-representable)
# ------------------------------------------------------------------------------------------------
KINDS = ("ones", "zeros", "vessels", "lines", "saturated", "smooth")


def _vessel_mask(rs, P, H, W):
    m = np.zeros((P, H, W), np.float32)
    for p in range(P):
        for _ in range(3):
            y, x, a = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0, 2 * np.pi)
            wd = int(rs.randint(1, 4))
            for _ in range(2 * (H + W)):
                a += rs.uniform(-0.4, 0.4)
                y, x = y + np.sin(a), x + np.cos(a)
                iy, ix = int(round(y)), int(round(x))
                m[p, max(0, iy):max(0, iy + wd), max(0, ix):max(0, ix + wd)] = 1.0
    return m


def tie_planes(kind, shape, seed=0):
    """(P,H,W) float32 planes in [0, 1]."""
    P, H, W = shape
    rs = np.random.RandomState(1000 * seed + 7 * H + W + KINDS.index(kind))
    if kind == "ones":
        return np.ones(shape, np.float32)
    if kind == "zeros":
        return np.zeros(shape, np.float32)
    if kind == "vessels":
        return _vessel_mask(rs, P, H, W)
    if kind == "lines":                      # one-pixel-wide lines that touch every border and corner
        m = np.zeros(shape, np.float32)
        m[:, 0, :] = 1.0
        m[:, :, W - 1] = 1.0
        m[:, H // 2, :] = 1.0
        m[:, :, W // 3] = 1.0
        d = np.arange(min(H, W))
        m[:, H - 1 - d, d] = 1.0
        if P > 1:                            # the other planes: other borders, a soft line too
            m[1] = 0.0
            m[1, H - 1, :] = 1.0
            m[1, :, 0] = 1.0
            m[1, d, d] = 0.75
        return m
    soft = rs.uniform(0.02, 0.98, shape).astype(np.float32)
    if kind == "smooth":
        return soft
    if kind == "saturated":                  # at least 20 % exact zeros and ones, in plateaus and as single pixels
        v = _vessel_mask(rs, P, H, W)
        u = rs.uniform(0, 1, shape)
        out = np.where(u < 0.3, v, soft)
        out = np.where(u > 0.9, np.float32(rs.randint(0, 2)), out).astype(np.float32)
        frac = np.mean((out == 0) | (out == 1))
        if frac < 0.2:
            out.reshape(-1)[: max(1, int(np.ceil(0.25 * out.size)))] = 1.0
        return out
    raise ValueError(kind)


def upstream(shape, seed, sign=0):
    """Upstream gradient of the skeleton, fp32-representable: mixed signs (0), all positive (+1) or all negative (-1)."""
    g = np.random.RandomState(77 + seed).standard_normal(shape).astype(np.float32)
    return g if sign == 0 else (np.abs(g) + np.float32(0.125)) * np.float32(sign)
