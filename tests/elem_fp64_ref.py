"""Float64 references of the element-wise / reduction kernels between the convolutions (csrc/elementwise.hip,
csrc/backward_elem.hip, the global-average-pool pair of csrc/heads.hip).  Plain torch / numpy on the CPU, no GPU import.

Every function takes what the kernel takes -- activations already quantised to the storage type, in the kernels' NHWC layout
(B, H, W, C), and the per-channel vectors as the fp32 values the kernel receives -- computes in float64, and returns next to each
result the MAGNITUDE its error bound is built from: the sum of the absolute values of the terms that enter the element (for a sum:
sum |terms|, not |sum|).  tests/test_cpu_elem_ref.py proves the references against torch's float64 autograd;
tests/test_gpu_elem_fp64.py holds the kernels to them.

Decisions (ReLU gate, pool arg-max) are taken in float64 from the same fp32 vectors: a correctly rounded fma has the sign of the
exact value, so the kernel's gate ``fmaf(v, sc, sh) > 0`` is the float64 sign of ``v * sc + sh`` unless the exact value lies below
the fp32 normal range (``gate_is_safe``).  The pool's arg-max follows ATen: the FIRST maximum of the window in the order (0,0),
(0,1), (1,0), (1,1), also when the whole window is 0.
"""
import numpy as np
import torch

U = 2.0 ** -24                      # fp32 unit roundoff
D = 2.0 ** -53                      # fp64 unit roundoff
U_DT = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}          # unit roundoff of the storage type (0: the output is fp32 itself)
TINY_DT = {"f32": 0.0, "f16": 2.0 ** -25, "bf16": 0.0}              # half the smallest f16 subnormal
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
F32_MIN_NORMAL = 2.0 ** -126


def quant(t, dt):
    """An fp32 tensor rounded to the storage type, back in fp32."""
    return t.to(TORCH_DT[dt]).to(torch.float32)


def elem_bound(ref, m, k, dt):
    """|got - ref| <= u_dt |ref| + k U m + tiny_dt: the storage rounding of the result, k fp32 roundings at magnitude m."""
    return U_DT[dt] * ref.abs() + k * U * m + TINY_DT[dt]


def vec(v):
    return v.double().view(1, 1, 1, -1)


def relu_on(C, relu_from):
    """cmu_relu_on of common.h: channels c >= relu_from are activated; a negative value -n activates the channels c < n."""
    c = torch.arange(C)
    return c >= relu_from if relu_from >= 0 else c < -relu_from


def nchw_to_nhwc_ref(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw_ref(x):
    return x.permute(0, 3, 1, 2).contiguous()


def expand_active(active, H, W):
    """Patch map (B, f, f) -> pixel selection (B, H, W): pixel (y, x) looks up active[b, y >> s, x >> s], f << s = H (sp_active)."""
    f = active.shape[-1]
    assert H % f == 0 and W % f == 0 and H // f == W // f
    return active.bool().repeat_interleave(H // f, 1).repeat_interleave(W // f, 2)


def rows_to_sel(rows, B, H, W):
    """Pixel list (dense pixel indices, -1 = padding) -> pixel selection (B, H, W)."""
    sel = torch.zeros(B * H * W, dtype=torch.bool)
    sel[rows[rows >= 0].long()] = True
    return sel.view(B, H, W)


# ------------------------------------------------------------------------------------------------
# pending transform, gate
# ------------------------------------------------------------------------------------------------
def act_ref(y, sc, sh, relu_from=0):
    """y * sc + sh with the ReLU on the channels ``relu_on`` selects -> (a, |y sc| + |sh|).  sc None: the identity."""
    y = y.double()
    if sc is None:
        return y, y.abs()
    t = y * vec(sc) + vec(sh)
    on = relu_on(y.shape[-1], relu_from).view(1, 1, 1, -1)
    return torch.where(on, t.clamp_min(0.0), t), (y * vec(sc)).abs() + vec(sh).abs()


def gate_ref(y, sc, sh):
    """The ReLU gate of the backward kernels: v * sc + sh > 0 (strictly: an activation of exactly 0 passes no gradient)."""
    return (y.double() * vec(sc) + vec(sh)) > 0


def gate_is_safe(y, sc, sh):
    """No exact pre-activation lies strictly between 0 and the smallest fp32 normal in magnitude: the only case in which the
    fp32 fma's sign may differ from the float64 one."""
    t = (y.double() * vec(sc) + vec(sh)).abs()
    return not bool(((t > 0) & (t < F32_MIN_NORMAL)).any())


# ------------------------------------------------------------------------------------------------
# BN + ReLU + MaxPool2d(2)
# ------------------------------------------------------------------------------------------------
def windows(x):
    """(B, H, W, C) -> (B, H/2, W/2, 4, C), window positions in the order (0,0), (0,1), (1,0), (1,1)."""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)


def unwindows(w):
    B, Ho, Wo, _, C = w.shape
    return w.reshape(B, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, C)


def pool_argmax(aw):
    """First maximum of each window (ATen's max_pool2d: a later element replaces the running maximum only when it is greater)."""
    best = aw[..., 0, :].clone()
    arg = torch.zeros(best.shape, dtype=torch.long)
    for q in range(1, 4):
        gt = aw[..., q, :] > best
        best = torch.where(gt, aw[..., q, :], best)
        arg = torch.where(gt, torch.full_like(arg, q), arg)
    return arg, best


def pool_ambiguous(aw, mw):
    """Windows whose arg-max the fp32 kernel may decide differently: some activation lies strictly below the maximum by no more
    than 4 U of the magnitudes entering the two values (distinct in float64, possibly equal after the kernel's fp32 rounding)."""
    best = aw.max(dim=3, keepdim=True).values
    thr = 4 * U * mw.max(dim=3, keepdim=True).values
    return ((aw < best) & (best - aw <= thr)).any(dim=3)


def pool_fwd_ref(y, sc, sh, active=None):
    """max over the 2 x 2 window of relu(y sc + sh) -> (out, magnitude = the window's largest |y sc| + |sh|); windows of masked
    patches (``active``: patch map) pool to exactly 0."""
    a, m = act_ref(y, sc, sh, 0)
    out, mag = windows(a).max(dim=3).values, windows(m).max(dim=3).values
    if active is not None:
        sel = expand_active(active, y.shape[1], y.shape[2])[:, ::2, ::2].unsqueeze(-1)
        out, mag = out * sel, mag * sel
    return out, mag


def pool_bwd_ref(dP, skips, y, sc, sh, active=None):
    """Gradient of the pool's input: the pooled gradient goes to the first maximum of its window, the skip gradients are added.
    -> dict: dA, mag (sum of |terms|), amb (B, H/2, W/2, C: windows with an ambiguous arg-max), written (B, H, W: False at the
    pixels of masked windows, which the masked kernel leaves untouched), k (fp32 additions on the element's path)."""
    a, m = act_ref(y, sc, sh, 0)
    aw = windows(a)
    arg, _ = pool_argmax(aw)
    hit = torch.stack([arg == q for q in range(4)], dim=3)
    g = unwindows(hit * dP.double().unsqueeze(3))
    dA, mag = g.clone(), g.abs()
    for s in skips:
        dA, mag = dA + s.double(), mag + s.double().abs()
    B, H, W, _ = y.shape
    written = torch.ones(B, H, W, dtype=torch.bool) if active is None else expand_active(active, H, W)
    return {"dA": dA, "mag": mag, "amb": pool_ambiguous(aw, windows(m)), "written": written, "k": len(skips)}


# ------------------------------------------------------------------------------------------------
# BatchNorm statistics finalisation
# ------------------------------------------------------------------------------------------------
def bn_finalize_ref(slab, count, bias, gamma, beta, rm, rv, momentum, eps, training):
    """cmu_bn_finalize: slab [rows][2][C] of partial (sum, sum of squares) -> dict of float64 numpy vectors scale, shift,
    save_mean, save_invstd, running_mean, running_var (None where the input is None) and ``mags``: S1 = sum |rows of sums| / count,
    S2 likewise.  Unbiased running variance (count == 1: the biased one), variance clamped at 0; eval: statistics from the running
    ones, save_mean = running_mean - bias.  Sums in extended precision (the slab rows may cancel: |mean| / std of 1e3)."""
    ld = np.longdouble
    f = lambda t, dflt, C: np.full(C, dflt, dtype=np.float64) if t is None else t.double().numpy()
    C = slab.shape[2] if training else rm.numel()
    g, b, cb = f(gamma, 1.0, C), f(beta, 0.0, C), f(bias, 0.0, C)
    mom, eps = float(np.float32(momentum)), float(np.float32(eps))
    out = {}
    if training:
        s = slab.double().numpy().astype(ld)
        s1, s2 = s[:, 0].sum(0), s[:, 1].sum(0)
        mean = s1 / count
        var = np.maximum(s2 / count - mean * mean, ld(0))
        out["mags"] = (np.abs(s[:, 0]).sum(0).astype(np.float64) / count, np.abs(s[:, 1]).sum(0).astype(np.float64) / count)
        mean, var = mean.astype(np.float64), var.astype(np.float64)
        invstd = 1.0 / np.sqrt(var + eps)
        out.update(scale=g * invstd, shift=b - mean * g * invstd, save_mean=mean, save_invstd=invstd, var=var)
        out["running_mean"] = None if rm is None else (1.0 - mom) * rm.double().numpy() + mom * (mean + cb)
        unb = var * count / (count - 1.0) if count > 1 else var
        out["running_var"] = None if rv is None else (1.0 - mom) * rv.double().numpy() + mom * unb
    else:
        rmn, rvn = rm.double().numpy(), rv.double().numpy()
        invstd = 1.0 / np.sqrt(rvn + eps)
        out.update(scale=g * invstd, shift=b + (cb - rmn) * g * invstd, save_mean=rmn - cb, save_invstd=invstd, running_mean=rmn,
                   running_var=rvn)
    return out


def bn_bwd_finalize_tiles_ref(slab, count):
    """cmu_bn_bwd_finalize_tiles: slab [rows][2][C] of partial (sum dz, sum dz xhat) -> dbeta, dgamma, coef (2, C) = sums / count,
    and the magnitudes sum |rows|."""
    s = slab.double()
    s1, s2 = s[:, 0].sum(0), s[:, 1].sum(0)
    return {"dbeta": s1, "dgamma": s2, "coef": torch.stack([s1, s2]) / count, "mag1": s[:, 0].abs().sum(0), "mag2": s[:, 1].abs().sum(0)}


# ------------------------------------------------------------------------------------------------
# BatchNorm + ReLU backward
# ------------------------------------------------------------------------------------------------
def bn_bwd_sums_ref(dA, y, sc, sh, mean, invstd, count=None, sel=None):
    """Phase 1: dz = gate * dA; dbeta = sum dz, dgamma = sum dz xhat, xhat = (y - mean) invstd; coef = (dbeta, dgamma) / count.
    ``sel`` (B, H, W): the pixels that enter (patch mask / pixel list); ``count`` defaults to the number of pixels."""
    dz = torch.where(gate_ref(y, sc, sh), dA.double(), torch.zeros((), dtype=torch.float64))
    if sel is not None:
        dz = dz * sel.unsqueeze(-1)
    if count is None:
        count = dz.shape[0] * dz.shape[1] * dz.shape[2]
    t2 = dz * ((y.double() - vec(mean)) * vec(invstd))
    s1, s2 = dz.sum((0, 1, 2)), t2.sum((0, 1, 2))
    return {"dbeta": s1, "dgamma": s2, "coef": torch.stack([s1, s2]) / count, "mag1": dz.abs().sum((0, 1, 2)), "mag2": t2.abs().sum((0, 1, 2)),
            "count": count}


def as_stored(stored, exact):
    """The gradient that enters a fused BatchNorm sum or a "never-stored" apply: the kernels take it rounded to the storage type,
    as the two-pass form stores it -- so the reference takes the stored bits (checked against ``exact`` on their own), not ``exact``."""
    assert stored.shape == exact.shape
    return stored.double()


def bn_bwd_apply_ref(dA, y, sc, sh, mean, invstd, coef, sel=None):
    """Phase 2: dY = sc (gate dA - c1 - xhat c2) -> (dY, m = |sc| (|dz| + |c1| + |xhat c2|)); exactly 0 outside ``sel``."""
    dz = torch.where(gate_ref(y, sc, sh), dA.double(), torch.zeros((), dtype=torch.float64))
    xh = (y.double() - vec(mean)) * vec(invstd)
    c1, c2 = vec(coef[0]), vec(coef[1])
    dY = vec(sc) * (dz - c1 - xh * c2)
    m = vec(sc).abs() * (dz.abs() + c1.abs() + (xh * c2).abs())
    if sel is not None:
        dY, m = dY * sel.unsqueeze(-1), m * sel.unsqueeze(-1)
    return dY, m


# ------------------------------------------------------------------------------------------------
# 1x1 head
# ------------------------------------------------------------------------------------------------
def head_fwd_ref(x, sc, sh, w, bias):
    """logits[b, k, y, x] = sum_c w[k, c] act(x)[b, y, x, c] + bias[k] (NCHW, fp32 output) -> (logits, sum |terms|).  The head's
    input is activated on every channel when a transform is pending, taken as it is otherwise."""
    a, m = act_ref(x, sc, sh, 0)
    w, bias = w.double(), bias.double()
    logits = torch.einsum("bhwc,kc->bkhw", a, w) + bias.view(1, -1, 1, 1)
    mag = torch.einsum("bhwc,kc->bkhw", m, w.abs()) + bias.abs().view(1, -1, 1, 1)
    return logits, mag


def head_bwd_ref(dl, x, sc, sh, w):
    """Gradients of the 1x1 head from dlogits (B, K, H, W): dX[p, c] = sum_k dl[p, k] w[k, c] (towards the head's activated
    input, before any storage rounding), dW[k, c] = sum_p dl[p, k] a[p, c], dbias[k] = sum_p dl[p, k], each with sum |terms|."""
    a, _ = act_ref(x, sc, sh, 0)
    dl, w = dl.double(), w.double()
    return {"dX": torch.einsum("bkhw,kc->bhwc", dl, w), "magX": torch.einsum("bkhw,kc->bhwc", dl.abs(), w.abs()),
            "dW": torch.einsum("bkhw,bhwc->kc", dl, a), "magW": torch.einsum("bkhw,bhwc->kc", dl.abs(), a.abs()),
            "db": dl.sum((0, 2, 3)), "magb": dl.abs().sum((0, 2, 3))}


# ------------------------------------------------------------------------------------------------
# first layer: Conv2d(1, Cout, 3, padding=1) with the patch mask multiplied into the image
# ------------------------------------------------------------------------------------------------
def c1_input(x, mask, per_sample):
    """The image the first layer sees: x (1 - mask); mask (1, H, W) for the whole batch, or (B, H, W) when ``per_sample``."""
    x = x.double()
    if mask is None:
        return x
    return x * (1.0 - (mask if per_sample else mask[:1]).double())


def c1_taps(xm):
    """(B, H, W) -> (B, H, W, 9): the nine zero-padded neighbours of each pixel, tap t = 3 kh + kw."""
    B, H, W = xm.shape
    xp = torch.zeros(B, H + 2, W + 2, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = xm
    return torch.stack([xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)], dim=-1)


def c1_fwd_ref(x, w, mask=None, per_sample=False):
    """-> (y NHWC, sum |terms|)."""
    taps, w9 = c1_taps(c1_input(x, mask, per_sample)), w.double().reshape(-1, 9)
    return torch.einsum("bhwt,ct->bhwc", taps, w9), torch.einsum("bhwt,ct->bhwc", taps.abs(), w9.abs())


def c1_wgrad_ref(x, dY, mask=None, per_sample=False, mdY=None):
    """dW[c, t] = sum_p dY[p, c] xm[p + t] -> (dW (Cout, 9), sum |terms|); ``mdY``: the magnitude that stands for |dY| (the fused
    BatchNorm-backward form passes the apply's m)."""
    taps = c1_taps(c1_input(x, mask, per_sample))
    dY = dY.double()
    return torch.einsum("bhwc,bhwt->ct", dY, taps), torch.einsum("bhwc,bhwt->ct", dY.abs() if mdY is None else mdY, taps.abs())


# ------------------------------------------------------------------------------------------------
# global average pool
# ------------------------------------------------------------------------------------------------
def gap_fwd_ref(y, sc, sh):
    """mean over the pixels of act(y) (all channels activated under a transform) -> (out (B, C), sum |terms| / HW)."""
    a, m = act_ref(y, sc, sh, 0)
    return a.mean((1, 2)), m.mean((1, 2))


def gap_bwd_ref(dout, H, W):
    """Every pixel of a channel gets dout / (H W) -> (dA (B, H, W, C), |dA|)."""
    B, C = dout.shape
    dA = (dout.double() / (H * W)).view(B, 1, 1, C).expand(B, H, W, C)
    return dA, dA.abs()
