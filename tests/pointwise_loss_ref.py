"""Float64 restatement of csrc/pointwise_loss.hip: the element-wise losses (L1 / MSE / BCE / BCE-with-logits) and the class-index
cross entropy, as plain torch on the CPU (no GPU import).  Every function takes what the kernel takes -- the fp32 predictions, the
targets in their own dtype, the fp32 weight vectors -- computes in float64 and returns, next to the sums and the gradient, the
MAGNITUDES the error bounds are built from: for a sum, sum |w term| (not |sum|); for a gradient element, the sum of the absolute
values of the terms that enter it.  tests/test_cpu_pointwise_losses.py proves these against torch.nn in float64 (autograd
included); tests/test_gpu_pointwise_losses_fp64.py holds the kernels to them.

Terms and derivatives are those of torch (c = 1 + (pw - 1) y):

    kind              term                                                    dterm                               |dterm| magnitude
    l1                |x - y|                                                 sign(x - y), 0 at ties              [x != y]
    mse               (x - y)^2                                               2 (x - y)                           2 (|x| + |y|)
    bce               -[y max(log x, -100) + (1 - y) max(log(1 - x), -100)]    (x - y) / max(x (1 - x), 1e-12)     (|x| + |y|) / max(x (1 - x), 1e-12)
    bce_with_logits   (1 - y) x + c (log1p(e^-|x|) + max(-x, 0))              (1 - y) - c sigmoid(-x)             |1 - y| + c sigmoid(-x)

The BCE-with-logits term and derivative are evaluated here in the forms without cancellation for 0 <= y <= 1
(c l + (x >= 0 ? (1 - y) x : pw y |x|);  x >= 0 ? (1 - y) - c s : c s - pw y  with s = sigmoid(-|x|)), which equal the table's."""
import torch

U = 2.0 ** -24                      # fp32 unit roundoff
KINDS = ("l1", "mse", "bce", "bce_with_logits")
BCE_EPS = float(torch.tensor(1e-12, dtype=torch.float32))      # torch's EPSILON is a float constant: 9.99999996e-13 in float64


def _per_channel(v, x):
    """An fp32 weight vector over x.shape[1] (or one element, or None = ones) as float64, broadcast against x."""
    if v is None:
        return torch.ones((), dtype=torch.float64)
    v = v.double().reshape(-1)
    if v.numel() == 1:
        return v.reshape(())
    assert x.dim() >= 2 and x.shape[1] == v.numel()
    return v.view(1, -1, *([1] * (x.dim() - 2)))


def pointwise_ref(kind, x, y, chan_w=None, chan_pw=None, g=1.0):
    """-> dict(S = sum w term, S_mag = sum |w term|, dx = g w dterm, dx_mag) in float64; x fp32, y fp32 / fp64, g a float."""
    assert kind in KINDS and x.dtype == torch.float32 and y.dtype in (torch.float32, torch.float64) and x.shape == y.shape
    x, y = x.double(), y.double()
    w, pw = _per_channel(chan_w, x), _per_channel(chan_pw, x)
    if kind == "l1":
        d = x - y
        term, dterm, dmag = d.abs(), torch.sign(d), (d != 0).double()
    elif kind == "mse":
        d = x - y
        term, dterm, dmag = d * d, 2 * d, 2 * (x.abs() + y.abs())
    elif kind == "bce":
        lx, l1x = torch.log(x).clamp_min(-100.0), torch.log1p(-x).clamp_min(-100.0)
        term = -(y * lx + (1 - y) * l1x)
        den = (x * (1 - x)).clamp_min(BCE_EPS)
        dterm, dmag = (x - y) / den, (x.abs() + y.abs()) / den
    else:
        ax = x.abs()
        e = torch.exp(-ax)
        l, s = torch.log1p(e), e / (1 + e)
        c = 1 + (pw - 1) * y
        pos = x >= 0
        term = c * l + torch.where(pos, (1 - y) * x, pw * y * ax)
        dterm = torch.where(pos, (1 - y) - c * s, c * s - pw * y)
        dmag = (1 - y).abs() + c.abs() * torch.where(pos, s, 1 - s)          # sigmoid(-x)
    wt = w * term
    return dict(S=wt.sum(), S_mag=wt.abs().sum(), dx=g * w * dterm, dx_mag=abs(g) * w.abs() * dmag)


def labels_of(target, onehot=False, keep=None):
    """The int64 label plane the kernel derives: a label plane truncated as ``.long()`` does, or the arg-max over the kept channels
    of K one-hot planes (the first maximum wins; all zeros -> the first kept channel), as an index into ALL K channels."""
    if not onehot:
        return target.long()
    keep = list(range(target.shape[1])) if keep is None else list(keep)
    return torch.tensor(keep)[torch.argmax(target[:, keep], dim=1)]


def index_ce_ref(x, labels, class_w=None, ignore_index=-100, log_input=False, keep=None, g0=1.0, g2=0.0):
    """-> dict(T = (sum w_t (-log p_t), sum w_t, sum_kept w_c (-log p_c)), T_mag = the same sums of absolute values, dx, dx_mag) in
    float64 for x (B,K,H,W) fp32 logits (``log_input``: log-probabilities) and an int64 label plane (B,H,W).  dx is the gradient of
    g0 T[0] + g2 T[2].  A label outside [0, K) that is not ignore_index: NaN in T[0], a zero gradient at that pixel."""
    assert x.dtype == torch.float32 and x.dim() == 4 and labels.dtype == torch.int64 and labels.shape == (x.shape[0],) + x.shape[2:]
    B, K, H, W = x.shape
    x = x.double()
    w = torch.ones(K, dtype=torch.float64) if class_w is None else class_w.double()
    kept = torch.zeros(K, dtype=torch.float64)
    kept[list(range(K)) if keep is None else list(keep)] = 1.0
    wk = (w * kept).view(1, K, 1, 1)
    ignored = labels == ignore_index
    bad = ~ignored & ((labels < 0) | (labels >= K))
    live = (~ignored & ~bad)
    t = labels.clamp(0, K - 1)                                          # (only read where live)
    onehot = torch.nn.functional.one_hot(t, K).permute(0, 3, 1, 2).double() * live.unsqueeze(1)
    p = torch.softmax(x, 1)
    nlp = -x if log_input else -torch.log_softmax(x, 1)
    wt = (w.view(1, K, 1, 1) * onehot).sum(1, keepdim=True)             # w_t at live pixels, 0 elsewhere
    lv = live.unsqueeze(1).double()
    T0, T0m = (wt * onehot * nlp).sum(), (wt * onehot * nlp).abs().sum()
    if bool(bad.any()):
        T0 = T0 + float("nan")
    T = torch.stack((T0, (wt * lv).sum(), (wk * nlp * lv).sum()))
    T_mag = torch.stack((T0m, (wt * lv).sum(), (wk * nlp * lv).abs().sum()))
    if log_input:
        dx = -g0 * wt * onehot - g2 * wk * lv
        mag = abs(g0) * wt * onehot + abs(g2) * wk * lv
    else:
        dx = g0 * wt * (p * lv - onehot) + g2 * (p * wk.sum() - wk) * lv
        mag = abs(g0) * wt * (p * lv + onehot) + abs(g2) * (p * wk.sum() + wk) * lv
    return dict(T=T, T_mag=T_mag, dx=dx, dx_mag=mag)


def reduce_ce(T, K, reduction="mean", label_smoothing=0.0):
    """torch's reductions of nn.CrossEntropyLoss from the three sums (works on the magnitudes too)."""
    e = label_smoothing
    v = (1 - e) * T[0] + (e / K) * T[2]
    return v / T[1] if reduction == "mean" else v
