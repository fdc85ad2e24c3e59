"""numpy / float64 restatement of the tiled-prediction passes (csrc/tiled_predict.hip) and of the whole pipeline around them.

Nothing here imports the package: the tile starts, the reflection fold, the dihedral views and their inverses, the windows and the
blend are written again from their definitions, so that the tests compare two independent statements.

Dihedral code: bit 0 flips W, bit 1 flips H, bit 2 transposes.  Forward view: flip W, then flip H, then transpose.  Inverse view:
transpose, then flip H, then flip W.  Tile index = ((img * ny + iy) * nx + ix) * A + a."""
import numpy as np


def tile_starts(L, T, stride):
    if L <= T:
        return [0]
    return list(range(0, L - T, stride)) + [L - T]


def fold(i, L):
    """Reflection without repeating the edge: the triangle fold of period 2 (L - 1)."""
    if L == 1:
        return 0
    m = 2 * (L - 1)
    i = i % m                      # Python: non-negative
    return m - i if i >= L else i


def view(a, code):
    """Forward dihedral view over the last two axes."""
    if code & 1:
        a = a[..., :, ::-1]
    if code & 2:
        a = a[..., ::-1, :]
    if code & 4:
        a = np.swapaxes(a, -1, -2)
    return a


def inverse_view(a, code):
    if code & 4:
        a = np.swapaxes(a, -1, -2)
    if code & 2:
        a = a[..., ::-1, :]
    if code & 1:
        a = a[..., :, ::-1]
    return a


def window(T, kind):
    if kind == "uniform":
        return np.ones(T, np.float32)
    assert kind == "gaussian"
    d = (np.arange(T, dtype=np.float64) - (T - 1) / 2.0) / (T / 8.0)
    w = np.exp(-0.5 * d * d)
    return (w / w.max()).astype(np.float32)


def canvas(img, Hp, Wp, pad):
    """(H,W) -> (Hp,Wp): the image in the top-left corner, the rest zero or folded."""
    H, W = img.shape
    out = np.zeros((Hp, Wp), img.dtype)
    out[:H, :W] = img
    if pad == "reflect":
        ys = [y if y < H else fold(y, H) for y in range(Hp)]
        xs = [x if x < W else fold(x, W) for x in range(Wp)]
        out = img[np.ix_(ys, xs)]
    else:
        assert pad == "zero"
    return out


def extract_tiles(src, ystarts, xstarts, codes, TH, TW, pad):
    """src (N,H,W) -> (N * ny * nx * A, TH, TW) float32."""
    N, H, W = src.shape
    out = []
    for img in range(N):
        c = canvas(src[img], max(H, TH), max(W, TW), pad)
        for y0 in ystarts:
            for x0 in xstarts:
                for code in codes:
                    out.append(view(c[y0:y0 + TH, x0:x0 + TW], code).astype(np.float32))
    return np.stack(out)


def uncovered(starts, T, L):
    hit = np.zeros(L, bool)
    for s in starts:
        hit[max(s, 0):s + T] = True
    miss = np.nonzero(~hit)[0]
    return None if miss.size == 0 else int(miss[0])


def cover_count(H, W, ystarts, xstarts, A, TH, TW):
    """Largest number of (tile, copy) pairs over one pixel."""
    cy, cx = np.zeros(H, int), np.zeros(W, int)
    for s in ystarts:
        cy[s:s + TH] += 1
    for s in xstarts:
        cx[s:s + TW] += 1
    return int(cy.max() * cx.max() * A)


def blend(probs, N, H, W, ystarts, xstarts, A, wy, wx):
    """probs (N * ny * nx * A, K', TH, TW), already in the un-augmented frame -> (num (N,K',H,W), den (N,H,W)) float64, summed in
    the order iy, ix, a."""
    probs = np.asarray(probs, np.float64)
    KP, TH, TW = probs.shape[1:]
    ny, nx = len(ystarts), len(xstarts)
    wgt = np.asarray(wy, np.float64)[:, None] * np.asarray(wx, np.float64)[None, :]
    num, den = np.zeros((N, KP, H, W)), np.zeros((N, H, W))
    for img in range(N):
        for iy, y0 in enumerate(ystarts):
            for ix, x0 in enumerate(xstarts):
                hh, ww = min(TH, H - y0), min(TW, W - x0)       # the part of the tile inside the image
                for a in range(A):
                    t = ((img * ny + iy) * nx + ix) * A + a
                    num[img, :, y0:y0 + hh, x0:x0 + ww] += wgt[:hh, :ww] * probs[t, :, :hh, :ww]
                    den[img, y0:y0 + hh, x0:x0 + ww] += wgt[:hh, :ww]
    return num, den


def labels_of(num, den, threshold=0.5):
    """K' >= 2: the first maximum; K' == 1: num / den > threshold."""
    if num.shape[1] == 1:
        return (num[:, 0] / den > threshold).astype(np.uint8)
    return np.argmax(num, axis=1).astype(np.uint8)


def softmax_planes(logits):
    """logits (n,K,h,w) -> float64 probabilities (n,K',h,w): softmax over K >= 2, the sigmoid for K == 1."""
    l = np.asarray(logits, np.float64)
    if l.shape[1] == 1:
        return 1.0 / (1.0 + np.exp(-l))
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def pipeline(src, tile_logits, TH, TW, ystarts, xstarts, codes, kind, pad):
    """The whole tiled path: src (N,H,W); ``tile_logits`` maps the (n,TH,TW) float32 stack of views to (n,K,TH,TW) logits.  Returns
    (num, den) in float64."""
    N, H, W = src.shape
    tiles = extract_tiles(src, ystarts, xstarts, codes, TH, TW, pad)
    p = softmax_planes(tile_logits(tiles))
    A = len(codes)
    back = np.stack([inverse_view(p[t], codes[t % A]) for t in range(p.shape[0])])
    return blend(back, N, H, W, ystarts, xstarts, A, window(TH, kind), window(TW, kind))
