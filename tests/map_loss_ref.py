"""Float64 restatement of csrc/map_loss.hip as plain torch / numpy on the CPU (no GPU import): the focal sums and gradient, both kinds
of map-weighted softmax sums and their gradient, the two distance-field modes from integer squared distances, and
``tversky_from_counters``.  Every function takes what the kernel takes -- fp32 logits, targets in their own dtype, fp32 weights --
computes in float64 and returns, next to the values, the MAGNITUDES the error bounds are built from: for a sum, sum |term|; for a
gradient element, the sum of the absolute values of the terms that enter it.  tests/test_cpu_map_losses.py proves these against
torch autograd in float64 and scipy; tests/test_gpu_map_losses_fp64.py holds the kernels to them.

Forms without cancellation, so that float64 keeps its precision where a probability saturates:
  q = 1 - p_t        as the sum of the other classes' probabilities;
  p_c - y_c          as (1 - y_c) p_c - y_c sum_{j != c} p_j  (for a one-hot y one of the two products);
  focal gradient     j == t: -g a_t (C + q^(gamma+1));  j != t: g a_t ((p_j / q) C + p_j q^gamma),  C = gamma p_t (-log p_t) q^gamma,
                     0 / 0 := 0: the expansion of g a_t (d_jt - p_j) (gamma p_t q^(gamma-1) log p_t - q^gamma), both addends of one sign
                     -- so the magnitude of an element is |dx| itself."""
import numpy as np
import torch

U = 2.0 ** -24                      # fp32 unit roundoff


def _softmax_parts(x):
    """p and, per class, the sum of the OTHER classes' probabilities (never 1 - p_c), float64."""
    p = torch.softmax(x.double(), 1)
    K = p.shape[1]
    others = torch.stack([p[:, [j for j in range(K) if j != c]].sum(1) for c in range(K)], 1)
    return p, others


def pow_gamma(q, gamma):
    """q^gamma with the kernel's conventions: exactly 1 for gamma = 0 (also at q = 0), 0 at q = 0 otherwise."""
    return torch.ones_like(q) if gamma == 0 else q ** gamma


def focal_ref(x, labels, alpha=None, gamma=2.0, ignore_index=-100, g=1.0):
    """-> dict(T = (sum a_t q^gamma (-log p_t), sum a_t, pixels not ignored), T_mag, dx, dx_mag, lnq = |ln q| of the pixel's label,
    broadcast over the classes, 0 where q is 0) in float64 for x (B,K,H,W) fp32 logits and an int64 label plane (B,H,W).  A label
    outside [0, K) that is not ignore_index: NaN in T[0], counted in T[2], a zero gradient at that pixel."""
    assert x.dtype == torch.float32 and x.dim() == 4 and labels.dtype == torch.int64 and labels.shape == (x.shape[0],) + x.shape[2:]
    B, K, H, W = x.shape
    a = torch.ones(K, dtype=torch.float64) if alpha is None else alpha.double()
    ignored = labels == ignore_index
    bad = ~ignored & ((labels < 0) | (labels >= K))
    live = ~ignored & ~bad
    t = labels.clamp(0, K - 1)
    onehot = torch.nn.functional.one_hot(t, K).permute(0, 3, 1, 2).double() * live.unsqueeze(1)
    lv = live.unsqueeze(1).double()
    p, others = _softmax_parts(x)
    nlp = -torch.log_softmax(x.double(), 1)
    at = (a.view(1, K, 1, 1) * onehot).sum(1, keepdim=True)                 # a_t at live pixels, 0 elsewhere
    pt, q, n = (p * onehot).sum(1, keepdim=True), (others * onehot).sum(1, keepdim=True), (nlp * onehot).sum(1, keepdim=True)
    qg = pow_gamma(q, gamma) * lv
    term = at * qg * n
    T0 = term.sum() + (float("nan") if bool(bad.any()) else 0.0)
    T = torch.stack((T0, (at * lv).sum(), (~ignored).double().sum()))
    T_mag = torch.stack((term.abs().sum(), (at * lv).abs().sum(), (~ignored).double().sum()))
    C = gamma * pt * n * qg
    ratio = torch.where(q > 0, p / torch.where(q > 0, q, torch.ones_like(q)), torch.zeros_like(p))
    mag = at * (onehot * (C + q * qg) + (lv - onehot) * (ratio * C + p * qg))
    dx = g * at * (-onehot * (C + q * qg) + (lv - onehot) * (ratio * C + p * qg))
    lnq = torch.where(q > 0, torch.log(torch.where(q > 0, q, torch.ones_like(q))).abs(), torch.zeros_like(q)) * lv
    return dict(T=T, T_mag=T_mag, dx=dx, dx_mag=abs(g) * mag, lnq=lnq.expand_as(dx))


def softmax_map_ref(logits, wmap, y, keep, kind, g=None):
    """-> dict(T (K), T_mag, dx, dx_mag) in float64.  kind 'linear': T_c = sum Wm_c p_c; 'squared': T_c = sum Wm_c (p_c - y_c)^2; over
    the classes ``keep`` (None: all), 0 for the others.  wmap fp32 or None (ones); y fp32 / fp64; g: K upstream gradients (None: zeros).
    dx_j = p_j (G_j - sum_c p_c G_c), G_c = g_c Wm_c or 2 g_c Wm_c (p_c - y_c); dx_mag_j = p_j (|G_j| + sum_c p_c |G_c|)."""
    assert logits.dtype == torch.float32 and logits.dim() == 4 and kind in ("linear", "squared")
    B, K, H, W = logits.shape
    kept = torch.zeros(K, dtype=torch.float64)
    kept[list(range(K)) if keep is None else list(keep)] = 1.0
    kept = kept.view(1, K, 1, 1)
    w = torch.ones(logits.shape, dtype=torch.float64) if wmap is None else wmap.double()
    gv = (torch.zeros(K, dtype=torch.float64) if g is None else torch.as_tensor(g, dtype=torch.float64)).view(1, K, 1, 1)
    p, others = _softmax_parts(logits)
    if kind == "linear":
        term, G = w * p, gv * w
    else:
        yd = y.double()
        d = (1 - yd) * p - yd * others
        term, G = w * d * d, 2 * gv * w * d
    term, G = term * kept, G * kept
    spg, spg_mag = (p * G).sum(1, keepdim=True), (p * G.abs()).sum(1, keepdim=True)
    return dict(T=term.sum((0, 2, 3)), T_mag=term.abs().sum((0, 2, 3)), dx=p * (G - spg), dx_mag=p * (G.abs() + spg_mag))


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def signed_field_ref(d2_to, d2_from):
    """float32 (numpy) signed distance from int squared distances: sqrt(d2_to) outside the set (d2_to > 0), 1 - sqrt(d2_from) inside,
    in float64 and rounded once; 0 wherever either map holds -1 (an empty or a full set)."""
    a, b = np.asarray(d2_to, dtype=np.int64), np.asarray(d2_from, dtype=np.int64)
    phi = np.where(a > 0, np.sqrt(np.maximum(a, 0).astype(np.float64)), 1.0 - np.sqrt(np.maximum(b, 0).astype(np.float64)))
    return np.where((a < 0) | (b < 0), 0.0, phi).astype(np.float32)


def unsigned_field_ref(d2_to, d2_from, alpha):
    """-> (float32 field, float64 exact value, d2): (sqrt(d2_to) + sqrt(d2_from))^alpha with d2 = d2_to + d2_from (one root is 0).
    alpha = 2: float32(d2); alpha = 1: float32(sqrt(float64(d2))): both what the kernel writes, bit for bit.  Any other alpha: the
    float64 value rounded once -- the kernel's single fp32 exp((alpha / 2) log d2) is held to a bound against ``exact``."""
    a, b = np.asarray(d2_to, dtype=np.int64), np.asarray(d2_from, dtype=np.int64)
    off = (a < 0) | (b < 0)
    d2 = np.where(off, 0, a + b)
    if alpha == 2:
        exact = d2.astype(np.float64)
    elif alpha == 1:
        exact = np.sqrt(d2.astype(np.float64))
    else:
        exact = np.where(d2 > 0, np.maximum(d2, 1).astype(np.float64) ** (alpha / 2.0), 0.0)
    return _f32(exact), exact, d2


def tversky_ref(tp, spr, sgt, alpha=0.5, beta=0.5, eps=1e-7, ignore_channels=None):
    """The Tversky index in Python floats from per-class counters (sequences), pooled over the kept channels."""
    keep = [c for c in range(len(tp)) if c not in set(ignore_channels or ())]
    t, s, gsum = (float(sum(float(v[c]) for c in keep)) for v in (tp, spr, sgt))
    return (t + eps) / (t + alpha * (s - t) + beta * (gsum - t) + eps)
