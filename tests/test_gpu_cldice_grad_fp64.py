"""The differentiable soft-clDice on the GPU (csrc/cldice_grad.hip, metrics.soft_cldice with threshold=None) against fp64.

u = 2^-24.  Gradients are held PER ELEMENT to max(4 e32, 8 u max|g64|), where e32 is measured inside each test as the largest error of
CPU fp32 autograd of the same restatement against its own fp64 run (the reference's arithmetic in fp32, not the code under test).
The skeleton backward runs on fp32-representable planes, so kernel and fp64 autograd make identical selections in every pooling
window and a wrong tie rule shows as an error of the order of max|g|.  The gradient to the logits is compared with a chain built
from the device's own probability planes (P = p32.double()): a chain that recomputes the softmax in fp64 selects other neighbours
at a handful of saturated pixels.  Every test prints ``PARITY <what> <worst error / bar>`` (profiles/cldice_grad_parity.txt).

Measured on an MI355X (worst error as a multiple of its bar): see profiles/cldice_grad_parity.txt.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cldice_grad_restate as R  # noqa: E402
import gen_cldice_grad as G  # noqa: E402
from oracle import losses as OL  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda"
ROWS = G.load()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    return o


@pytest.fixture(scope="module")
def metrics(ops):
    from cmunet_amd import metrics as m
    return m


def worst_ratio(got, ref, bound, what):
    """max |got - ref| / bound over the elements; asserts it is <= 1 and prints it."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    ratio = (got - ref).abs() / bound.clamp_min(1e-300)
    r = float(ratio.max()) if ratio.numel() else 0.0
    print(f"PARITY {what} {r:.3f}")
    if r > 1.0:
        i = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ref.numel()} elements outside the bound; worst at {idx}: got "
                             f"{got.flatten()[i].item():.9g}, ref {ref.flatten()[i].item():.9g}, bound {bound.flatten()[i].item():.3g} "
                             f"(err / bound {r:.3g})")
    return r


def grad_bar(g64, g32):
    g64, g32 = torch.as_tensor(g64).double(), torch.as_tensor(g32).double()
    e32 = float((g32 - g64).abs().max()) if g64.numel() else 0.0
    return max(4.0 * e32, 8.0 * U * float(g64.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------
# skeleton: forward bits and the reverse sweep
# ------------------------------------------------------------------------------------------------
SKEL_SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 2, 2), (3, 5, 7), (2, 17, 33), (2, 64, 65)]


def check_skeleton(ops, kind, shape, num_iters, signs):
    img = R.tie_planes(kind, shape, seed=2)
    x = torch.from_numpy(img).to(DEV)
    for N in num_iters:
        plain, saving = torch.empty_like(x), torch.empty_like(x)
        ops.soft_skeleton(x, plain, N)
        kept = ops.soft_skeleton_save(x, saving, N)
        assert torch.equal(plain, saving), f"saving forward differs from cmu_soft_skeleton ({kind} {shape} num_iter {N})"
        for sign in signs:
            g = R.upstream(shape, N, sign)
            want64, _ = R.skel_grad_autograd(img, g, N, torch.float64)
            want32, _ = R.skel_grad_autograd(img, g, N, torch.float32)
            dimg = torch.full_like(x, float("nan"))
            ops.soft_skeleton_bwd(x, kept, N, dimg, g_skel=torch.from_numpy(g).to(DEV))
            worst_ratio(dimg, want64, grad_bar(want64, want32), f"skel_bwd {kind} {'x'.join(map(str, shape))} N{N} sign{sign}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", SKEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_skeleton_forward_bits_and_backward(ops, kind, shape):
    check_skeleton(ops, kind, shape, (0, 1, 3, 10), (0, 1))


@pytest.mark.parametrize("kind", ["saturated", "vessels"])
def test_skeleton_backward_past_the_grid_cap(ops, kind):
    """5 x 512 x 512 = 1.25 grid passes of 4096 x 256 threads: the grid-stride loops of every kernel of the sweep."""
    check_skeleton(ops, kind, (5, 512, 512), (10,), (0,))


def test_skeleton_backward_with_the_cldice_tail(ops):
    """The fused tail: g = g4[0] y_true + g4[1] enters the deepest level and dimg gains g4[2] skel_true, g4 read on the device.
    (A binary y_true and dyadic g4 make the upstream gradient and the product g4[2] skel_true exact in fp32: the bar stays the sweep's.)"""
    shape, N = (3, 19, 23), 10
    img, yt, st = R.tie_planes("saturated", shape, 3), R.tie_planes("vessels", shape, 4), R.tie_planes("smooth", shape, 5)
    g4 = np.array([-0.375, 0.125, -0.0625, 0.9])
    g = np.float32(g4[0]).astype(np.float64) * yt + np.float32(g4[1]).astype(np.float64)
    want64, _ = R.skel_grad_autograd(img, g, N, torch.float64)
    want32, _ = R.skel_grad_autograd(img, g, N, torch.float32)
    want64 = want64 + np.float32(g4[2]).astype(np.float64) * st
    want32 = want32.astype(np.float64) + np.float32(g4[2]).astype(np.float64) * st
    x = torch.from_numpy(img).to(DEV)
    sk, dimg = torch.empty_like(x), torch.empty_like(x)
    kept = ops.soft_skeleton_save(x, sk, N)
    ops.soft_skeleton_bwd(x, kept, N, dimg, g4=torch.from_numpy(g4).to(DEV), y_true=torch.from_numpy(yt).to(DEV),
                          skel_true=torch.from_numpy(st).to(DEV))
    worst_ratio(dimg, want64, grad_bar(want64, want32), "skel_bwd with the clDice tail")


# ------------------------------------------------------------------------------------------------
# planes kernel and its backward
# ------------------------------------------------------------------------------------------------
def all_planes(ops, logits_dev):
    B, K, H, W = logits_dev.shape
    p = torch.empty(B * K, H, W, device=DEV)
    ops.softmax_planes(logits_dev, None, list(range(K)), None, p, None)
    return p.view(B, K, H, W)


PLANE_CASES = [(2, [1], (2, 33, 47)), (3, [0, 1, 2], (2, 33, 47)), (3, [1, 2], (2, 33, 47)), (8, list(range(8)), (2, 33, 47)),
               (8, list(range(1, 8)), (2, 33, 47)), (8, [2, 3, 4, 5, 6, 7], (2, 33, 47)), (4, [0, 2, 3], (1, 1, 1)),
               (2, [1], (5, 512, 512))]


@pytest.mark.parametrize("K,keep,bhw", PLANE_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, (list, tuple)) else str(v))
@pytest.mark.parametrize("f64_target", [False, True])
def test_planes_kernel(ops, K, keep, bhw, f64_target):
    B, H, W = bhw
    g = torch.Generator().manual_seed(100 * K + len(keep) + B)
    logits = torch.randn(B, K, H, W, generator=g) * torch.where(torch.rand(B, 1, H, W, generator=g) < 0.3, 30.0, 3.0)
    target = torch.rand(B, K, H, W, generator=g).float()
    target = torch.where(torch.rand(B, K, H, W, generator=g) < 0.5, target.round(), target)
    tgt = target.double() if f64_target else target
    ld = logits.to(DEV)
    n = B * len(keep)
    soft, tp = torch.full((n, H, W), float("nan"), device=DEV), torch.full((n, H, W), float("nan"), device=DEV)
    ops.softmax_planes(ld, tgt.to(DEV), keep, None, soft, tp)
    ref = torch.softmax(logits.double(), 1)[:, keep].reshape(n, H, W)
    worst_ratio(soft, ref, 8 * U, f"planes soft K{K} keep{keep} {bhw}")
    assert torch.equal(tp.cpu(), target[:, keep].reshape(n, H, W)), "target planes are not exact"
    assert torch.equal(soft, all_planes(ops, ld)[:, keep].reshape(n, H, W)), "kept planes differ from the all-channel planes"
    for t in (0.5, 0.3):
        hard = torch.full((n, H, W), float("nan"), device=DEV)
        ops.softmax_planes(ld, None, keep, t, hard, None)
        assert torch.equal(hard, (soft > t).float()), f"thresholded planes differ from (p32 > {t})"


@pytest.mark.parametrize("K,keep,bhw", PLANE_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, (list, tuple)) else str(v))
def test_planes_backward(ops, K, keep, bhw):
    """dlogit_k = p_k (G_k - sum_j p_j G_j) with the forward's own p32: an fma chain of Kk terms, a subtraction and a product ->
    (Kk + 4) u p_k (|G_k| + sum_j p_j |G_j|) per element."""
    B, H, W = bhw
    g = torch.Generator().manual_seed(7 * K + len(keep))
    logits = (torch.randn(B, K, H, W, generator=g) * 4.0).to(DEV)
    Gp = torch.randn(B, len(keep), H, W, generator=g)
    dl = torch.full((B, K, H, W), float("nan"), device=DEV)
    ops.softmax_planes_bwd(logits, Gp.reshape(-1, H, W).to(DEV).contiguous(), keep, dl)
    p = all_planes(ops, logits).double().cpu()
    Gf = torch.zeros(B, K, H, W, dtype=torch.float64)
    Gf[:, keep] = Gp.double()
    ref = p * (Gf - (p * Gf).sum(1, keepdim=True))
    bound = (len(keep) + 4) * U * p * (Gf.abs() + (p * Gf.abs()).sum(1, keepdim=True)) + 1e-37
    worst_ratio(dl, ref, bound, f"planes bwd K{K} keep{keep} {bhw}")


# ------------------------------------------------------------------------------------------------
# the module: value and gradient to the logits
# ------------------------------------------------------------------------------------------------
def vessel_logits(scale, seed, B=2, S=64):
    """Two-class vessel-like logits: the target's vessels, partly displaced, times ``scale``, plus noise."""
    rs = np.random.RandomState(seed)
    gt = R._vessel_mask(rs, B, S, S)
    pr = np.roll(gt, 1, axis=2) * (rs.rand(B, S, S) < 0.9) + (rs.rand(B, S, S) < 0.02)
    fg = scale * (2.0 * np.clip(pr, 0, 1) - 1.0) + 0.5 * rs.standard_normal((B, S, S))
    logits = np.stack([-0.5 * fg, 0.5 * fg], 1).astype(np.float32)
    y = np.stack([1.0 - gt, gt], 1).astype(np.float64)
    return logits.astype(np.float64), y


MODULE_CASES = [(key, K, ign, eb, lg, y) for key, K, ign, eb, _, lg, y, _, _ in ROWS]
MODULE_CASES += [("vessels64_soft", 2, [0], False) + vessel_logits(2.0, 31), ("vessels64_sat", 2, [0], False) + vessel_logits(12.0, 32)]


def value_bar(n_planes):
    return 4.0 * (n_planes / 131072 + 16) * U


def device_planes_reference(ops, logits_np, y_np, keep, dtype, smooth=1.0, num_iter=10):
    """(loss, dlogits) of the chain built on the device's own probabilities: P = p32 -> clDice by autograd -> the softmax formula
    with p32, all in ``dtype`` on the CPU."""
    p32 = all_planes(ops, torch.from_numpy(logits_np).float().to(DEV)).cpu()
    pa = p32.to(dtype)
    P = pa[:, keep].clone().requires_grad_(True)
    L = R.cldice_of_planes(P, torch.from_numpy(y_np).to(dtype)[:, keep], smooth, num_iter)
    Gk, = torch.autograd.grad(L, P)
    Gf = torch.zeros_like(pa)
    Gf[:, keep] = Gk
    return float(L), (pa * (Gf - (pa * Gf).sum(1, keepdim=True))).double()


def run_module(metrics, logits_np, y_np, **cfg):
    x = torch.from_numpy(logits_np).float().to(DEV).requires_grad_(True)
    m = metrics.soft_cldice(threshold=None, activation="softmax", **cfg)
    L = m(x, torch.from_numpy(y_np).to(DEV))
    assert L.dtype == torch.float64 and L.dim() == 0 and L.requires_grad
    L.backward()
    return float(L), x.grad.detach().cpu()


@pytest.mark.parametrize("case", MODULE_CASES, ids=[c[0] for c in MODULE_CASES])
def test_module_value_and_gradient(ops, metrics, case):
    key, K, ign, eb, lg, y = case
    keep = R.kept_channels(K, ign, eb)
    B, _, H, W = lg.shape
    L, dl = run_module(metrics, lg, y, ignore_channels=ign, exclude_background=eb)
    want = float(R.cldice(torch.from_numpy(lg), torch.from_numpy(y), ign, eb))
    worst_ratio(torch.tensor(L), torch.tensor(want), value_bar(B * len(keep) * H * W), f"module value {key}")
    _, g64 = device_planes_reference(ops, lg, y, keep, torch.float64)
    _, g32 = device_planes_reference(ops, lg, y, keep, torch.float32)
    assert float(g64.abs().max()) > 0
    worst_ratio(dl, g64, grad_bar(g64, g32), f"module gradient {key}")


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_module_against_the_reference_fixture(ops, metrics, row):
    """The reference's own fp64 loss and gradient (tests/golden/cldice_grad.npz).  The loss for every case; the gradient of the soft
    cases to 64 u max|g| (a soft case whose fp32 probabilities select another neighbour somewhere is named and held to the
    device-planes form instead)."""
    key, K, ign, eb, regime, lg, y, loss, dlogits = row
    keep = R.kept_channels(K, ign, eb)
    B, _, H, W = lg.shape
    L, dl = run_module(metrics, lg, y, ignore_channels=ign, exclude_background=eb)
    worst_ratio(torch.tensor(L), torch.tensor(loss), value_bar(B * len(keep) * H * W), f"fixture value {key}")
    if regime != "soft":
        return
    ref = torch.from_numpy(dlogits)
    bar = 64 * U * float(ref.abs().max())
    err = (dl.double() - ref).abs()
    print(f"PARITY fixture gradient {key} {float(err.max()) / bar:.3f}")
    if float(err.max()) > bar:
        for idx in (err > bar).nonzero()[:8].tolist():
            print(f"selection flip suspected at {key}{tuple(idx)}: got {dl[tuple(idx)].item():.9g}, reference {ref[tuple(idx)].item():.9g}")
        _, g64 = device_planes_reference(ops, lg, y, keep, torch.float64)
        _, g32 = device_planes_reference(ops, lg, y, keep, torch.float32)
        worst_ratio(dl, g64, grad_bar(g64, g32), f"fixture gradient {key} (device-planes form)")


def test_smooth_and_num_iter_are_honoured(ops, metrics):
    key, K, ign, eb, lg, y = MODULE_CASES[4]
    keep = R.kept_channels(K, ign, eb)
    x = torch.from_numpy(lg).float().to(DEV).requires_grad_(True)
    m = metrics.soft_cldice(threshold=None, activation="softmax2d", ignore_channels=ign, exclude_background=eb, smooth=0.25, iter_=50)
    m.num_iter = 3
    L = m(x, torch.from_numpy(y).float().to(DEV))          # an fp32 target this time
    L.backward()
    want, g64 = device_planes_reference(ops, lg, y, keep, torch.float64, smooth=0.25, num_iter=3)
    _, g32 = device_planes_reference(ops, lg, y, keep, torch.float32, smooth=0.25, num_iter=3)
    worst_ratio(L, torch.tensor(want), value_bar(lg.shape[0] * len(keep) * lg.shape[2] * lg.shape[3]), "module value smooth 0.25 num_iter 3")
    worst_ratio(x.grad, g64, grad_bar(g64, g32), "module gradient smooth 0.25 num_iter 3")


def test_backward_is_deterministic(metrics):
    _, K, ign, eb, lg, y = MODULE_CASES[-1]
    a = run_module(metrics, lg.copy(), y.copy(), ignore_channels=ign)
    b = run_module(metrics, lg.copy(), y.copy(), ignore_channels=ign)
    assert a[0] == b[0] and torch.equal(a[1], b[1])


def test_no_grad_and_detached_logits_give_the_same_value(metrics):
    _, K, ign, eb, lg, y = MODULE_CASES[2]
    m = metrics.soft_cldice(threshold=None, activation="softmax", ignore_channels=ign, exclude_background=eb)
    x, yd = torch.from_numpy(lg).float().to(DEV), torch.from_numpy(y).to(DEV)
    with_grad = m(x.clone().requires_grad_(True), yd)
    with torch.no_grad():
        a = m(x.clone().requires_grad_(True), yd)
    b = m(x, yd)
    assert with_grad.grad_fn is not None and a.grad_fn is None and b.grad_fn is None and not a.requires_grad and not b.requires_grad
    assert torch.equal(a, with_grad.detach()) and torch.equal(b, with_grad.detach())


def test_thresholded_driver_configuration_keeps_its_call_sequence(ops, metrics):
    from cmunet_amd import _lib
    _, K, ign, eb, lg, y = MODULE_CASES[-2]
    x, yd = torch.from_numpy(lg).float().to(DEV), torch.from_numpy(y).to(DEV)
    got = metrics.soft_cldice(threshold=0.5, activation="softmax", ignore_channels=[0])(x.clone().requires_grad_(True), yd)
    assert not got.requires_grad
    B, _, H, W = x.shape
    yp, yt = torch.empty(B, H, W, device=DEV), yd[:, 1].float().contiguous()
    ops.softmax2_threshold(x, 0.5, yp)
    ws = torch.empty(_lib.lib().cmu_soft_skeleton_ws_bytes(B * H * W), dtype=torch.uint8, device=DEV)
    sp, st, out4 = torch.empty_like(yp), torch.empty_like(yp), torch.empty(4, device=DEV)
    ops.soft_skeleton(yp, sp, 10, ws)
    ops.soft_skeleton(yt, st, 10, ws)
    ops.cldice_sums(sp, yt, st, yp, out4)
    s = out4.double()
    tprec, tsens = (s[0] + 1.) / (s[1] + 1.), (s[2] + 1.) / (s[3] + 1.)
    assert torch.equal(got, 1. - 2.0 * (tprec * tsens) / (tprec + tsens))


@pytest.mark.parametrize("ign,eb", [(None, False), ([0], False), ([1], True)])
def test_thresholded_three_class_value(metrics, ign, eb):
    """Logits on a grid of 1/4: no probability comes within 1e-5 of the threshold (asserted), so the fp32 and fp64 masks agree."""
    g = torch.Generator().manual_seed(5)
    B, K, H, W, t = 2, 3, 33, 47, 0.4
    logits = (torch.randn(B, K, H, W, generator=g) * 3).mul(4).round().div(4)
    y = torch.nn.functional.one_hot(torch.randint(0, K, (B, H, W), generator=g), K).permute(0, 3, 1, 2).contiguous().double()
    assert float((torch.softmax(logits.double(), 1) - t).abs().min()) > 1e-5
    got = metrics.soft_cldice(threshold=t, activation="softmax", ignore_channels=ign, exclude_background=eb)(logits.to(DEV), y.to(DEV))
    want = R.cldice(logits.double(), y, ign, eb, threshold=t)
    n = B * len(R.kept_channels(K, ign, eb)) * H * W
    worst_ratio(got, want, value_bar(n), f"thresholded K3 value ignore {ign} exclude_background {eb}")


# ------------------------------------------------------------------------------------------------
# integration: one training step with the whole tensor criterion of the reference's finetuning
# ------------------------------------------------------------------------------------------------
def test_train_step_with_the_combined_criterion(ops, metrics):
    from cmunet_amd import model as Mod, train as T
    M = metrics

    class Tap(torch.nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, x):
            self.out = self.net(x)
            self.out.retain_grad()
            return self.out

    torch.manual_seed(3)
    net = Mod.UNet(base_ch=8, depth=3)
    rs = np.random.RandomState(9)
    gt = R._vessel_mask(rs, 2, 32, 32)
    x = torch.from_numpy(gt + 0.3 * rs.standard_normal(gt.shape).astype(np.float32)).float()
    y = torch.from_numpy(np.stack([1.0 - gt, gt], 1)).double()
    soft = dict(activation="softmax", threshold=None, ignore_channels=[0])
    crit = M.DiceLoss(**soft) + M.CrossEntropyLoss() + 0.5 * M.soft_cldice(**soft)
    assert crit.__name__ == "dice_loss + cross_entropy_loss + 0.5 * soft_clDice"
    tap = Tap(net)
    tr = T.TrainEpoch(tap, loss=crit, metrics=[], optimizer=torch.optim.SGD(net.parameters(), lr=1e-3), device=DEV, verbose=False)
    net.train()
    M.clear_seg_cache()
    loss, pred = tr.batch_update(x.to(DEV), y.to(DEV))
    assert pred is tap.out and pred.shape == (2, 2, 32, 32)
    lg = pred.detach().cpu().double().numpy()

    def term(fn, dtype):
        z = torch.from_numpy(lg).to(dtype).requires_grad_(True)
        v = fn(z, y.to(dtype))
        g, = torch.autograd.grad(v, z)
        return float(v), g.double()
    total, ref, bar = 0.0, 0.0, 0.0
    for fn in (lambda z, t: OL.dice_loss(z, t, threshold=None, ignore_channels=(0,)), OL.cross_entropy_prob):
        v, g64 = term(fn, torch.float64)
        _, g32 = term(fn, torch.float32)
        total, ref, bar = total + v, ref + g64, bar + grad_bar(g64, g32)
    v, g64 = device_planes_reference(ops, lg, y.numpy(), [1], torch.float64)
    _, g32 = device_planes_reference(ops, lg, y.numpy(), [1], torch.float32)
    total, ref, bar = total + 0.5 * v, ref + 0.5 * g64, bar + 0.5 * grad_bar(g64, g32)
    assert abs(float(loss) - total) <= 1e-5 * abs(total), (float(loss), total)
    worst_ratio(pred.grad, ref, bar, "train step: logits.grad of dice + ce + 0.5 clDice")
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        # (the bias of a convolution in front of a training-mode BatchNorm has an identically zero gradient: the engine writes 0)
        if not (n.endswith("double_conv.0.bias") or n.endswith("double_conv.3.bias")):
            assert float(p.grad.abs().max()) > 0, n
