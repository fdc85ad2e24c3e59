"""The float64 references of tests/elem_fp64_ref.py against torch's float64 autograd on the CPU: composed the way the step composes
the kernels (statistics -> pending transform -> pool / head -> BatchNorm backward sums -> apply), with the per-channel vectors left
unrounded, they must reproduce autograd to 1e-12 of each element's magnitude.  Exact positive ties and all-non-positive windows are
put into the data on purpose, so the first-maximum rule is proved against F.max_pool2d itself."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elem_fp64_ref as R

REL = 1e-12
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(got, ref, mag, what):
    got, ref, mag = (torch.as_tensor(t, dtype=torch.float64) for t in (got, ref, mag))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > REL * mag + 1e-300
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {ref.numel()} outside 1e-12 of the magnitude, worst {float((err / (mag + 1e-300)).max()):.3g}"


def nhwc(t):
    return R.nchw_to_nhwc_ref(t)


def slab_of(y, rows):
    """Per-channel (sum, sum of squares) of y (B, C, H, W) split into ``rows`` partial rows -> [rows][2][C]."""
    flat = y.permute(1, 0, 2, 3).reshape(y.shape[1], -1)
    parts = torch.tensor_split(flat, rows, dim=1)
    return torch.stack([torch.stack([p.sum(1), (p * p).sum(1)]) for p in parts])


def tied_input(g, B=2, C=6, H=8, W=10):
    """Random raw output with whole windows made equal (ties whatever the transform) and one strongly negative window."""
    y = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 1.5 + 0.3
    y[0, :, 0:2, 0:2] = 0.75
    y[0, :, 2:4, 0:2] = -50.0
    y[1, :, 4:6, 2:4] = y[1, :, 4:5, 2:3]
    y[1, :, 0, 0] = y[1, :, 1, 1]                      # a tie of the first and the last position of a window
    return y


@pytest.mark.parametrize("skips", [0, 1, 2])
def test_bn_relu_pool_forward_and_backward_match_autograd(skips):
    g = gen(10 + skips)
    y = tied_input(g)
    B, C, H, W = y.shape
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    gamma[1] = -gamma[1]                                # a negative scale
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    dP = torch.randn(B, C, H // 2, W // 2, generator=g, dtype=torch.float64)
    dS = [torch.randn(B, C, H, W, generator=g, dtype=torch.float64) for _ in range(skips)]
    yd, gd, bd = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a = F.relu(F.batch_norm(yd, None, None, gd, bd, True, MOM, EPS))
    a.retain_grad()
    p = F.max_pool2d(a, 2)
    ((p * dP).sum() + sum((a * s).sum() for s in dS)).backward()

    fin = R.bn_finalize_ref(slab_of(y, 7), B * H * W, None, gamma, beta, None, None, MOM, EPS, True)
    sc, sh, mean, invstd = (torch.from_numpy(fin[k]) for k in ("scale", "shift", "save_mean", "save_invstd"))
    yn = nhwc(y)
    out, mag = R.pool_fwd_ref(yn, sc, sh)
    close(out, nhwc(p.detach()), mag, "pool forward")
    pb = R.pool_bwd_ref(nhwc(dP), [nhwc(s) for s in dS], yn, sc, sh)
    close(pb["dA"], nhwc(a.grad), pb["mag"] + 1e-30, "pool backward + skips (ungated)")
    assert int(pb["amb"].sum()) == 0
    sums = R.bn_bwd_sums_ref(pb["dA"], yn, sc, sh, mean, invstd)
    close(sums["dbeta"], bd.grad, sums["mag1"], "dbeta")
    close(sums["dgamma"], gd.grad, sums["mag2"], "dgamma")
    dY, m = R.bn_bwd_apply_ref(pb["dA"], yn, sc, sh, mean, invstd, sums["coef"])
    close(dY, nhwc(yd.grad), m, "dY")


def test_pool_tie_rule_is_atens():
    """Dyadic values, scale and shift (exact products): all-equal positive windows, all-negative windows, windows of exact zeros,
    two-way ties at every pair of positions -- the gradient lands where F.max_pool2d's backward puts it, ungated."""
    g = gen(3)
    B, C, H, W = 2, 4, 12, 12
    y = torch.randint(-3, 4, (B, C, H, W), generator=g).double() / 4
    sc = torch.tensor([0.5, -0.25, 1.0, 0.0], dtype=torch.float64)
    sh = torch.tensor([0.0625, 0.0, -0.125, 0.0], dtype=torch.float64)
    y[0, :, 0:2, 0:2] = 0.25
    y[0, :, 2:4, 2:4] = -0.5
    y[0, :, 4:6, 4:6] = 0.0
    a = F.relu(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
    aw = R.windows(nhwc(a.detach()))
    srt = aw.sort(dim=3, descending=True).values
    assert int(((srt[..., 0, :] == srt[..., 1, :]) & (srt[..., 0, :] > 0)).sum()) > 50        # positive ties are there
    assert int((srt[..., 0, :] == 0).sum()) > 50                                             # and all-zero windows
    dP = torch.randn(B, C, H // 2, W // 2, generator=g, dtype=torch.float64)
    F.max_pool2d(a, 2).backward(dP)
    pb = R.pool_bwd_ref(nhwc(dP), [], nhwc(y), sc, sh)
    assert torch.equal(pb["dA"], nhwc(a.grad))
    arg, _ = R.pool_argmax(aw)
    _, idx = F.max_pool2d(a.detach(), 2, return_indices=True)
    q = (idx // W % 2) * 2 + idx % W % 2                # position inside the window of ATen's index
    assert torch.equal(arg, nhwc(q))


def test_pool_ambiguity_and_gate_safety_flags():
    y = torch.zeros(1, 2, 2, 1, dtype=torch.float64)
    y[0, 0, 0, 0], y[0, 0, 1, 0] = 1.0, 1.0 + 2.0 ** -30         # distinct in float64, equal in fp32
    one, zero = torch.ones(1), torch.zeros(1)
    pb = R.pool_bwd_ref(torch.ones(1, 1, 1, 1), [], y, one, zero)
    assert bool(pb["amb"].all())
    y[0, 0, 1, 0] = 1.0                                           # an exact tie is not ambiguous
    assert not bool(R.pool_bwd_ref(torch.ones(1, 1, 1, 1), [], y, one, zero)["amb"].any())
    assert R.gate_is_safe(y, one, zero)
    assert not R.gate_is_safe(torch.full((1, 1, 1, 1), 2.0 ** -100, dtype=torch.float64), torch.full((1,), 2.0 ** -40), zero)


@pytest.mark.parametrize("count_one", [False, True])
def test_bn_finalize_matches_batch_norm(count_one):
    g = gen(5)
    B, C, H, W = (1, 5, 1, 1) if count_one else (3, 5, 6, 4)
    y = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.5
    if count_one:
        y = (y * 8).round() / 8                      # squares exact in float64: the slab's sum of squares is mean^2 to the bit
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64) * 0.1, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    n = B * H * W
    # eval with a conv bias
    fin = R.bn_finalize_ref(None, n, bias, gamma, beta, rm, rv, MOM, EPS, False)
    ref = F.batch_norm(y + bias.view(1, -1, 1, 1), rm.clone(), rv.clone(), gamma, beta, False, MOM, EPS)
    sc, sh = torch.from_numpy(fin["scale"]).view(1, -1, 1, 1), torch.from_numpy(fin["shift"]).view(1, -1, 1, 1)
    close(y * sc + sh, ref, (y * sc).abs() + sh.abs() + ref.abs(), "eval with bias")
    close(fin["save_mean"], rm - bias, rm.abs() + bias.abs(), "eval save_mean = running_mean - bias")
    close(fin["save_invstd"], 1 / torch.sqrt(rv + EPS), 1 / torch.sqrt(rv), "eval save_invstd")
    # training: the transform and the running statistics (of the biased conv output)
    fin = R.bn_finalize_ref(slab_of(y, 1 if count_one else 5), n, bias, gamma, beta, rm, rv, MOM, EPS, True)
    sc, sh = torch.from_numpy(fin["scale"]).view(1, -1, 1, 1), torch.from_numpy(fin["shift"]).view(1, -1, 1, 1)
    if count_one:
        # torch refuses one value per channel in training mode: the statistics by hand (mean = the value, variance 0, no n - 1)
        close(fin["save_mean"], y.view(C), y.view(C).abs(), "mean of one value")
        close(fin["save_invstd"], np.full(C, 1 / np.sqrt(EPS)), np.full(C, 1 / np.sqrt(EPS)), "invstd = 1 / sqrt(eps)")
        close(fin["running_var"], (1 - MOM) * rv, rv + 1, "running_var with count 1: the biased (zero) variance")
        return
    rm2, rv2 = rm.clone(), rv.clone()
    ref = F.batch_norm(y + bias.view(1, -1, 1, 1), rm2, rv2, gamma, beta, True, MOM, EPS)
    close(y * sc + sh, ref, (y * sc).abs() + sh.abs() + ref.abs(), "train")
    close(fin["running_mean"], rm2, rm2.abs() + 1, "running_mean")
    close(fin["running_var"], rv2, rv2.abs() + 1, "running_var (unbiased)")
    close(fin["save_mean"], y.mean((0, 2, 3)), y.abs().mean((0, 2, 3)), "save_mean (bias-free)")


def test_bn_finalize_clamps_a_negative_variance():
    slab = torch.tensor([[[3.0], [2.9999999]]], dtype=torch.float64)       # sum 3, sum of squares < 3: variance < 0 for count 3
    fin = R.bn_finalize_ref(slab, 3, None, None, None, None, None, MOM, EPS, True)
    assert fin["var"][0] == 0.0 and abs(fin["save_invstd"][0] - 1 / np.sqrt(EPS)) < 1e-9


def test_masked_batchnorm_backward_is_batchnorm_over_the_selected_pixels():
    """Sparse BatchNorm (patch mask / pixel list): statistics and gradients over the selected pixels only, zeros elsewhere."""
    g = gen(7)
    B, C, H, W, f = 2, 5, 8, 8, 4
    y = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    dA = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    active = (torch.rand(B, f, f, generator=g) > 0.5).to(torch.uint8)
    sel = R.expand_active(active, H, W)
    assert torch.equal(sel[1, 5, 2], active[1, 2, 1].bool())
    rows = torch.cat([sel.flatten().nonzero().flatten(), torch.full((5,), -1)])
    assert torch.equal(R.rows_to_sel(rows, B, H, W), sel)
    ys = y[sel].clone().requires_grad_(True)
    gd, bd = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    (F.relu(F.batch_norm(ys, None, None, gd, bd, True, MOM, EPS)) * dA[sel]).sum().backward()
    n = int(sel.sum())
    mean, var = y[sel].mean(0), y[sel].var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + EPS)
    sc, sh = gamma * invstd, beta - mean * gamma * invstd
    sums = R.bn_bwd_sums_ref(dA, y, sc, sh, mean, invstd, count=n, sel=sel)
    close(sums["dbeta"], bd.grad, sums["mag1"], "masked dbeta")
    close(sums["dgamma"], gd.grad, sums["mag2"], "masked dgamma")
    dY, m = R.bn_bwd_apply_ref(dA, y, sc, sh, mean, invstd, sums["coef"], sel=sel)
    close(dY[sel], ys.grad, m[sel], "masked dY")
    assert bool((dY[~sel] == 0).all())
    t = R.bn_bwd_finalize_tiles_ref(torch.stack([torch.stack([sums["dbeta"] * 0.25, sums["dgamma"] * 0.25])] * 4), n)
    close(t["coef"], sums["coef"], sums["coef"].abs(), "finalize from a slab")


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("tf", [True, False])
def test_head_matches_conv2d(K, tf):
    g = gen(20 + K)
    B, C, H, W = 2, 16, 5, 7
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    sc = torch.randn(C, generator=g, dtype=torch.float64) if tf else None
    sh = torch.randn(C, generator=g, dtype=torch.float64) * 0.3 if tf else None
    w = torch.randn(K, C, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(K, generator=g, dtype=torch.float64).requires_grad_(True)
    a = (F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if tf else x.clone()).requires_grad_(True)
    logits = F.conv2d(a, w.view(K, C, 1, 1), b)
    dl = torch.randn(B, K, H, W, generator=g, dtype=torch.float64)
    logits.backward(dl)
    got, mag = R.head_fwd_ref(nhwc(x), sc, sh, w.detach(), b.detach())
    close(got, logits.detach(), mag, "logits")
    hb = R.head_bwd_ref(dl, nhwc(x), sc, sh, w.detach())
    close(hb["dX"], nhwc(a.grad), hb["magX"], "dX")
    close(hb["dW"], w.grad, hb["magW"], "dW")
    close(hb["db"], b.grad, hb["magb"], "dbias")


@pytest.mark.parametrize("masked", [0, 1, 2])
def test_first_layer_matches_conv2d(masked):
    g = gen(30 + masked)
    B, H, W, Cout = 3, 9, 7, 4
    x = torch.randn(B, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, 1, 3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    m = (torch.rand(B, H, W, generator=g) > 0.5).to(torch.uint8)
    mask = None if masked == 0 else (m[:1] if masked == 1 else m)
    xin = x if masked == 0 else x * (1 - (m[0] if masked == 1 else m).double())
    y = F.conv2d(xin.unsqueeze(1), w, padding=1)
    dY = torch.randn(B, Cout, H, W, generator=g, dtype=torch.float64)
    y.backward(dY)
    got, mag = R.c1_fwd_ref(x, w.detach(), mask, masked == 2)
    close(got, nhwc(y.detach()), mag, "first-layer conv")
    dW, magW = R.c1_wgrad_ref(x, nhwc(dY), mask, masked == 2)
    close(dW, w.grad.view(Cout, 9), magW, "first-layer dW")


def test_gap_layout_and_transform():
    g = gen(40)
    B, C, H, W = 2, 6, 3, 5
    y = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    sc, sh = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    a = F.relu(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
    out = a.mean((2, 3))
    dout = torch.randn(B, C, generator=g, dtype=torch.float64)
    out.backward(dout)
    got, mag = R.gap_fwd_ref(nhwc(y), sc, sh)
    close(got, out.detach(), mag, "gap")
    close(R.gap_fwd_ref(nhwc(y), None, None)[0], y.mean((2, 3)), y.abs().mean((2, 3)), "gap without a transform")
    dA, mA = R.gap_bwd_ref(dout, H, W)
    close(dA, nhwc(a.grad), mA, "gap backward")
    assert torch.equal(R.nhwc_to_nchw_ref(nhwc(y)), y)
    # relu_from: channels c >= 2 activated; -2: channels c < 2
    t = y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    pos, neg = t.clone(), t.clone()
    pos[:, 2:], neg[:, :2] = pos[:, 2:].clamp_min(0), neg[:, :2].clamp_min(0)
    assert torch.equal(R.act_ref(nhwc(y), sc, sh, 2)[0], nhwc(pos)) and torch.equal(R.act_ref(nhwc(y), sc, sh, -2)[0], nhwc(neg))
    assert not torch.equal(pos, neg)
