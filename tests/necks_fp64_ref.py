"""Float64 references of the neck path (csrc/necks.hip: BatchNorm1d (+ReLU), the NCHW 1x1 convolution) and of the select / sum
kernels of the SparK path (csrc/sparse.hip, csrc/sparse_elem.hip: mask-select, the masked channel sums).  Plain torch on the CPU,
no GPU import; the conventions are those of tests/elem_fp64_ref.py: every function takes what the kernel takes (fp32 vectors as
the kernel receives them, activations already quantised to the storage type), computes in float64 and returns next to each result
the MAGNITUDE its error bound is built from (for a sum: sum |terms|).  tests/test_cpu_necks_ref.py proves them against torch's
float64 autograd; tests/test_gpu_necks_fp64.py and tests/test_gpu_spark_select_fp64.py hold the kernels to them.

BatchNorm1d is split the way the kernels split it, so that every stage can be evaluated at the fp32 values the previous stage
RETURNED: statistics (from the rows, from exchanged column sums, or the running ones) -> forward at (mean, invstd) -> backward column
sums at (mean, invstd) with the gate taken from y as data -> dx at (S0, S1, count).  The eval-mode backward is the same dx with
S0 = S1 = 0 and count = 1: the backward of a fixed affine map.
"""
import torch

from elem_fp64_ref import TORCH_DT, act_ref, expand_active, relu_on, vec  # noqa: F401  (re-exported for the tests)


def _d(t):
    return None if t is None else torch.as_tensor(t).double()


# ------------------------------------------------------------------------------------------------
# BatchNorm1d (+ ReLU) over the rows of (M, N)
# ------------------------------------------------------------------------------------------------
def bn1d_colsums_ref(x):
    """sums[0] = sum_m x, sums[1] = sum_m x^2 -> (sums (2, N), mags (2, N))."""
    x = _d(x)
    return torch.stack([x.sum(0), (x * x).sum(0)]), torch.stack([x.abs().sum(0), (x * x).sum(0)])


def bn1d_stats_local_ref(x):
    """Training statistics of the local rows: mean, BIASED variance, count = M -> dict with the magnitudes of the two sums."""
    x = _d(x)
    M = x.shape[0]
    mean = x.sum(0) / M
    d = x - mean
    return {"mean": mean, "var": (d * d).sum(0) / M, "count": M, "mag_mean": x.abs().sum(0) / M}


def bn1d_stats_exchanged_ref(sums, count, local_rows=None):
    """Training statistics from column sums added over the ranks (SyncBN): mean = S0 / count, var = max(S1 / count - mean^2, 0) with
    ``count`` the TOTAL number of rows -- not ``local_rows``, the rows of the block that is normalised (taken only so that the
    signature says which of the two numbers enters)."""
    s = _d(sums)
    mean = s[0] / count
    e2 = s[1] / count
    return {"mean": mean, "var": (e2 - mean * mean).clamp_min(0.0), "count": count, "e2": e2}


def bn1d_invstd_ref(var, eps):
    return 1.0 / torch.sqrt(_d(var) + eps)


def bn1d_running_ref(rm, rv, mean, var, count, momentum):
    """torch's update: running_mean <- (1 - m) rm + m mean; running_var <- (1 - m) rv + m var count / (count - 1) (the UNBIASED
    variance; a count of 1 keeps the biased one) -> (rm', rv', mag_rm, mag_rv)."""
    rm, rv, mean, var = _d(rm), _d(rv), _d(mean), _d(var)
    unb = count / (count - 1.0) if count > 1 else 1.0
    a, b = (1.0 - momentum) * rm, momentum * mean
    c, d = (1.0 - momentum) * rv, momentum * var * unb
    return a + b, c + d, a.abs() + b.abs(), c.abs() + d.abs()


def bn1d_fwd_ref(x, mean, invstd, gamma, beta, relu):
    """y = (x - mean) invstd gamma + beta (+ ReLU) at the given mean / invstd -> (y, m = |(x - mean) invstd gamma| + |beta|)."""
    x = _d(x)
    t = (x - _d(mean)) * _d(invstd)
    if gamma is not None:
        t = t * _d(gamma)
    b = torch.zeros(x.shape[1], dtype=torch.float64) if beta is None else _d(beta)
    y = t + b
    return (y.clamp_min(0.0) if relu else y), t.abs() + b.abs()


def bn1d_gate(y, relu):
    """The backward's ReLU gate, from y as DATA: y > 0, strictly (0.0 and -0.0 pass no gradient)."""
    y = _d(y)
    return (y > 0) if relu else torch.ones_like(y, dtype=torch.bool)


def bn1d_bwd_sums_ref(dy, x, y, mean, invstd, relu):
    """S0 = sum_m dz, S1 = sum_m dz xhat, dz = dy [y > 0], xhat = (x - mean) invstd -> (sums (2, N), mags (2, N)).  S0 is dbeta and
    S1 is dgamma of the local rows."""
    dz = torch.where(bn1d_gate(y, relu), _d(dy), torch.zeros((), dtype=torch.float64))
    t = dz * ((_d(x) - _d(mean)) * _d(invstd))
    return torch.stack([dz.sum(0), t.sum(0)]), torch.stack([dz.abs().sum(0), t.abs().sum(0)])


def bn1d_bwd_dx_ref(dy, x, y, mean, invstd, gamma, relu, sums, count):
    """dx = gamma invstd (dz - S0 / count - xhat S1 / count) -> (dx, m = |gamma invstd| (|dz| + |S0 / count| + |xhat S1 / count|)).
    ``sums`` None with count 1: the eval-mode backward (zero sums)."""
    dz = torch.where(bn1d_gate(y, relu), _d(dy), torch.zeros((), dtype=torch.float64))
    xh = (_d(x) - _d(mean)) * _d(invstd)
    s = torch.zeros(2, dz.shape[1], dtype=torch.float64) if sums is None else _d(sums)
    k = _d(invstd) if gamma is None else _d(gamma) * _d(invstd)
    c0, c1 = s[0] / count, s[1] / count
    return k * (dz - c0 - xh * c1), k.abs() * (dz.abs() + c0.abs() + (xh * c1).abs())


# ------------------------------------------------------------------------------------------------
# 1x1 convolution NHWC (dt, pending transform) -> NCHW fp32
# ------------------------------------------------------------------------------------------------
def conv1x1_operand_ref(x, sc, sh, relu_from, dt):
    """The A operand the kernel multiplies: x itself, or relu_on?(x sc + sh) rounded to the storage type (the transform runs in
    registers and is packed back to dt before the MFMA).  relu_from: cmu_relu_on of common.h, both signs."""
    if sc is None:
        return _d(x)
    a, _ = act_ref(x, sc, sh, relu_from)
    return a.to(TORCH_DT[dt]).double()


def conv1x1_nchw_ref(x, sc, sh, relu_from, w, bias, dt):
    """out[b, n, y, x] = sum_k a[b, y, x, k] round_dt(w[n, k]) + bias[n] -> (out (B, N, H, W), m = sum_k |a w| + |bias|)."""
    a = conv1x1_operand_ref(x, sc, sh, relu_from, dt)
    wq = w.to(TORCH_DT[dt]).double()
    b = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else _d(bias)
    out = torch.einsum("bhwk,nk->bnhw", a, wq) + b.view(1, -1, 1, 1)
    mag = torch.einsum("bhwk,nk->bnhw", a.abs(), wq.abs()) + b.abs().view(1, -1, 1, 1)
    return out, mag


# ------------------------------------------------------------------------------------------------
# mask-select and the masked sums
# ------------------------------------------------------------------------------------------------
def selection(active, H, W, invert=False):
    """(B, f, f) patch map -> (B, H, W) bool: the pixels a kernel treats as selected."""
    sel = expand_active(active, H, W)
    return ~sel if invert else sel


def ring_frame(active, H):
    """Pixels of the one-pixel border frame of MASKED patches (what the ring form zeroes) -> (B, H, H) bool."""
    f = active.shape[-1]
    s = H // f
    e = torch.arange(H) % s
    edge = (e == 0) | (e == s - 1)
    return (~expand_active(active, H, H)) & (edge.view(1, H, 1) | edge.view(1, 1, H))


def mask_select_ref(x, sc, sh, relu, sel, fill, dt):
    """out = selected ? relu?(x sc + sh) : round_dt(fill[c]) (fill None: 0) -> (out, m, moved): m = |x sc| + |sh| at selected positions
    (0 elsewhere: the fill is exact), moved = no arithmetic touches a selected element (no transform, no ReLU: a pure move)."""
    xd = _d(x)
    C = xd.shape[-1]
    if sc is None:
        t, m = xd, torch.zeros_like(xd)
    else:
        t, m = xd * vec(sc) + vec(sh), (xd * vec(sc)).abs() + vec(sh).abs()
    if relu:
        t = t.clamp_min(0.0)
    fl = torch.zeros(C, dtype=torch.float64) if fill is None else fill.to(TORCH_DT[dt]).double()
    s = sel.unsqueeze(-1)
    return torch.where(s, t, fl.view(1, 1, 1, -1).expand_as(t)), m * s, sc is None and not relu


def masked_sums_ref(x, sel):
    """Per-channel sum and sum of squares over the selected pixels -> (s1, s2, sum |x|, sum x^2)."""
    xs = _d(x) * sel.unsqueeze(-1)
    q = xs * xs
    return xs.sum((0, 1, 2)), q.sum((0, 1, 2)), xs.abs().sum((0, 1, 2)), q.sum((0, 1, 2))


# ------------------------------------------------------------------------------------------------
# the three products of the skinny GEMMs
# ------------------------------------------------------------------------------------------------
def gemm_fwd_ref(x, w, bias):
    """y (M, N) = x (M, K) . w (N, K)^T + bias, in float64 (exact for the integer and one-hot operands of the bit-for-bit tests)."""
    y = _d(x) @ _d(w).t()
    return y if bias is None else y + _d(bias)


def gemm_dgrad_ref(dy, w):
    """dx (M, K) = dy (M, N) . w (N, K)."""
    return _d(dy) @ _d(w)


def gemm_wgrad_ref(dy, x):
    """dw (N, K) = dy^T (N, M) . x (M, K), dbias (N) = sum_m dy."""
    return _d(dy).t() @ _d(x), _d(dy).sum(0)
