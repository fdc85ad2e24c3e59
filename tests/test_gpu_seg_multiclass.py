"""A three-class UNet trained with the differentiable Dice + CE criterion: the criterion's gradient reaches the engine exactly as
the backward kernel wrote it, and the drop-in Epoch classes run with three-class losses and metrics."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

K = 3


def batch(seed, B=2, S=32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, S, generator=g)
    y = F.one_hot(torch.randint(0, K, (B, S, S), generator=g), K).permute(0, 3, 1, 2).contiguous().double()
    return x, y


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_criterion_gradient_reaches_the_engine_unchanged(dtype):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import _lib, metrics as M, model as Mod, ops
    torch.manual_seed(7)
    net = Mod.UNet(out_classes=K, base_ch=16, depth=3, dtype=dtype).cuda().train()
    x, y = batch(1)
    x, y = x.cuda(), y.cuda()
    crit = M.DiceLoss(threshold=None, activation="softmax", ignore_channels=[0]) + M.CrossEntropyLoss()
    M.clear_seg_cache()
    logits = net(x)
    assert logits.shape == (2, K, 32, 32) and logits.dtype == torch.float32
    loss = crit(logits, y)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and math.isfinite(float(loss))
    loss.backward()
    first = {n: p.grad.clone() for n, p in net.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in first.values()) and any(float(g.abs().max()) > 0 for g in first.values())

    # the same gradient from the kernels called directly: counters -> d loss / d counters (autograd of the helper) -> dlogits
    lg = logits.detach()
    table = torch.empty(1 + 5 * K, dtype=torch.float64, device="cuda")
    ws = torch.empty(_lib.lib().cmu_seg_stats_ws_bytes(K), dtype=torch.uint8, device="cuda")
    ops.seg_stats_fwd(lg, y, None, 0.5, table, ws)
    table.requires_grad_(True)
    expr = (1.0 - M.f_score_from_counters(table[1:1 + K], table[1 + K:1 + 2 * K], table[1 + 4 * K:], 1.0, 1e-5, [0])) + table[0]
    assert torch.equal(expr.detach(), loss.detach())
    g, = torch.autograd.grad(expr, table)
    dl = torch.empty_like(lg)
    ops.seg_stats_bwd(lg, y, None, g[0:1], g[1:1 + K], g[1 + K:1 + 2 * K], dl)
    assert float(dl[:, 0].abs().max()) > 0          # the ignored channel still gets the CE term and the softmax coupling

    for p in net.parameters():
        p.grad = None
    logits2 = net(x)
    assert torch.equal(logits2, logits)
    logits2.backward(gradient=dl)
    for n, p in net.named_parameters():
        assert torch.equal(p.grad, first[n]), n


def test_epochs_run_with_three_classes():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import metrics as M, model as Mod, train as T
    torch.manual_seed(11)
    net = Mod.UNet(out_classes=K, base_ch=16, depth=3, dtype="f32")
    loader = [batch(21), batch(22)]
    soft = dict(threshold=None, activation="softmax", ignore_channels=[0])
    hard = dict(threshold=0.5, activation="softmax", ignore_channels=[0])
    crit = M.DiceLoss(**soft) + M.CrossEntropyLoss()
    mets = [M.DiceLoss(**hard), M.CrossEntropyLoss(), M.IoU(**hard)]
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    tr = T.TrainEpoch(net, loss=crit, metrics=mets, optimizer=opt, device="cuda", verbose=False)
    va = T.ValidEpoch(net, loss=crit, metrics=mets, device="cuda", verbose=False)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    for logs in (tr.run(loader), va.run(loader)):
        assert set(logs) == {"dice_loss + cross_entropy_loss", "dice_loss", "cross_entropy_loss", "iou_loss"}
        assert all(math.isfinite(v) for v in logs.values()), logs
        assert 0.0 <= logs["dice_loss"] <= 1.0 and 0.0 <= logs["iou_loss"] <= 1.0 and logs["cross_entropy_loss"] > 0
    changed = [n for n, p in net.named_parameters() if not torch.equal(p.detach(), before[n])]
    # (a convolution bias in front of a training-mode BatchNorm has a zero gradient: only the weights are required to move)
    assert {n for n in before if n.endswith("weight")} <= set(changed), sorted(set(before) - set(changed))
