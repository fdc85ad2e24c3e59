"""Float64 restatement of the Lovasz-Softmax loss (Berman et al., 2018) as cmunet_amd/metrics.py's LovaszSoftmaxLoss defines it, in
numpy / torch, and the case list of the key sort.  The reference of tests/test_gpu_lovasz.py; tests/test_cpu_lovasz.py pins it.

Per kept class c and segment (the whole batch, or one image), over the pixels whose label is not ``ignore_index``:
  e_i = 1 - p_c(i) where the label is c (foreground), else p_c(i);
  order: descending e, equal errors by ascending pixel index (b, h, w) within the segment;
  J_r = 1 - (G - F_r) / (G + r - F_r), g_1 = J_1, g_r = J_r - J_(r-1)     (G foreground pixels, F_r of them among the first r);
  class loss = sum_r e_(r) g_r.
'present' averages the classes with G > 0 in the segment, 'all' (or a list of ids) all kept classes; per_image averages the images.
"""
import numpy as np
import torch


def jaccard_grad(fg_sorted):
    """g of the definition, in float64: differences of J_r."""
    fg = np.asarray(fg_sorted, dtype=np.int64)
    n = fg.size
    if n == 0:
        return np.zeros(0)
    G, F, r = int(fg.sum()), np.cumsum(fg), np.arange(1, n + 1)
    J = 1.0 - (G - F).astype(np.float64) / (G + r - F).astype(np.float64)
    g = J.copy()
    g[1:] = J[1:] - J[:-1]
    return g


def jaccard_grad_closed(fg_sorted):
    """The same g without the difference's cancellation (the form csrc/lovasz.hip evaluates): a foreground key leaves the union
    U_r = G + r - F_r as it is, g_r = 1 / U_r; a background key leaves N = G - F_r, g_r = N / ((U_r - 1) U_r), and 1 where U_r = 1."""
    fg = np.asarray(fg_sorted, dtype=np.int64)
    n = fg.size
    if n == 0:
        return np.zeros(0)
    G, F, r = int(fg.sum()), np.cumsum(fg), np.arange(1, n + 1)
    U = (G + r - F).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bg = np.where(U == 1, 1.0, (G - F).astype(np.float64) / ((U - 1.0) * U))
    return np.where(fg != 0, 1.0 / U, bg)


def error_order(e):
    """Descending e, ties by ascending index."""
    e = np.asarray(e)
    return np.lexsort((np.arange(e.size), -e))


def class_loss(e, fg):
    """-> (loss, order, g) of one (segment, class) row: e float64 errors, fg 0/1, both over the valid pixels in index order."""
    order = error_order(e)
    g = jaccard_grad(np.asarray(fg)[order])
    return float(np.dot(np.asarray(e, dtype=np.float64)[order], g)), order, g


def kept_classes(K, classes):
    return list(range(K)) if isinstance(classes, str) else sorted(set(int(c) for c in classes))


def lovasz_softmax(x, labels, classes="present", per_image=False, ignore_index=-100, orders=None, probs=None):
    """The loss as a differentiable float64 torch scalar, and what it was made of.

    x (B,K,H,W) torch float64 logits (may require grad; ``probs``: use these probabilities instead of softmax(x)); labels (B,H,W)
    integer tensor.  ``orders``: {(s, c): int64 array of the segment's pixel indices, valid pixels only, in sorted order} -- the order
    is then GIVEN (the device's), else it is computed from the float64 errors.  -> (loss, info) with info['L_sc'] (S,K) class losses
    (0 where the class does not count), info['coef'] (S,), info['L_s'] (S,), info['orders'], info['g'] {(s, c): g along the order},
    info['e'] {(s, c): float64 errors along the order}, info['counts'] (S, K + 1) valid and per-class pixels.
    A label outside [0, K) that is not ignore_index: the loss is NaN (nothing else is computed)."""
    B, K, H, W = x.shape
    p = torch.softmax(x, 1) if probs is None else probs
    lab = labels.reshape(B, H * W).long()
    keep = kept_classes(K, classes)
    all_count = classes != "present"
    bad = (lab != ignore_index) & ((lab < 0) | (lab >= K))
    S = B if per_image else 1
    info = {"L_sc": np.zeros((S, K)), "coef": np.zeros(S), "L_s": np.zeros(S), "orders": {}, "g": {}, "e": {}, "counts": np.zeros((S, K + 1), np.int64)}
    if bool(bad.any()):
        return x.sum() * float("nan"), info
    pp = p.reshape(B, K, H * W)
    total = x.sum() * 0.0
    for s in range(S):
        lab_s = lab[s] if per_image else lab.reshape(-1)                                   # (n,), pixel index (b, h, w) within the segment
        p_s = pp[s] if per_image else pp.permute(1, 0, 2).reshape(K, -1)                   # (K, n)
        valid = (lab_s != ignore_index).numpy()
        vidx = np.nonzero(valid)[0]
        info["counts"][s, 0] = vidx.size
        for c in range(K):
            info["counts"][s, 1 + c] = int((lab_s == c).sum())
        counted = [c for c in keep if all_count or info["counts"][s, 1 + c] > 0]
        if not counted:
            continue
        info["coef"][s] = 1.0 / (S * len(counted))
        seg_loss = x.sum() * 0.0
        for c in counted:
            fg = (lab_s == c).numpy()[vidx]
            e = torch.where(torch.from_numpy(fg), 1.0 - p_s[c][vidx], p_s[c][vidx])
            if orders is None:
                o = error_order(e.detach().numpy())
            else:
                o = np.searchsorted(vidx, np.asarray(orders[(s, c)], dtype=np.int64))
                assert np.array_equal(np.sort(o), np.arange(vidx.size)), "the given order is no permutation of the valid pixels"
            g = jaccard_grad(fg[o])
            l = (e[o] * torch.from_numpy(g)).sum() if vidx.size else x.sum() * 0.0
            info["L_sc"][s, c] = float(l.detach())
            info["orders"][(s, c)], info["g"][(s, c)], info["e"][(s, c)] = vidx[o], g, e.detach().numpy()[o]
            seg_loss = seg_loss + l
        info["L_s"][s] = float(seg_loss.detach())
        total = total + info["coef"][s] * seg_loss
    return total, info


# ---- the key sort's cases (shared by the GPU test of cmu_sort_u64 and the host program's CPU test) --------------------------------
SORT_DATA = ("random", "shared_high", "ascending", "descending", "four_high")


def sort_sizes(T):
    """1, 2, around one tile, and 5 T + 7: six tiles, three merge passes over an odd tile count at the second pass."""
    return [1, 2, T - 1, T, T + 1, 2 * T + 3, 5 * T + 7]


def sort_keys(kind, S, n, seed=0):
    """(S,n) uint64.  random: any 64 bits; shared_high: one high word, distinct low words (only the index field decides);
    ascending / descending: already in / in the reverse order; four_high: four distinct high words, so that runs of equal high
    words are long and partitions land inside them."""
    rng = np.random.default_rng(seed * 7919 + n * 31 + S)
    lo = np.stack([rng.permutation(n) for _ in range(S)]).astype(np.uint64) * np.uint64(2) + (rng.integers(0, 2, (S, n)).astype(np.uint64))
    if kind == "random":
        return rng.integers(0, 2 ** 64, (S, n), dtype=np.uint64)
    if kind == "shared_high":
        return (np.uint64(0x3F123456) << np.uint64(32)) | lo
    if kind == "four_high":
        hi = np.array([0x00000000, 0x3F800000, 0x7FFFFFFF, 0xFFFFFFFF], np.uint64)[rng.integers(0, 4, (S, n))]
        return (hi << np.uint64(32)) | lo
    a = np.sort(rng.integers(0, 2 ** 64, (S, n), dtype=np.uint64), axis=1)
    return a if kind == "ascending" else a[:, ::-1].copy()


def sort_cases(T):
    return [(kind, S, n) for n in sort_sizes(T) for S in (1, 3) for kind in SORT_DATA]
