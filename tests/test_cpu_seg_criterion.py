"""CPU suite of the K-class segmentation criterion: the counters-to-score helpers of cmunet_amd/metrics.py (pure torch, fp64) against
oracle/losses.py, and what the loss / metric constructors accept and refuse.  The kernels that produce the counters are pinned on
the GPU in tests/test_gpu_seg_criterion_fp64.py."""
import itertools

import pytest
import torch

from oracle import losses as OL


def counters(logits, y, threshold):
    """Per-class (tp, spr, sgt) of fp64 logits / targets with plain torch: soft (threshold None) or thresholded."""
    pr = torch.softmax(logits, 1)
    if threshold is not None:
        pr = (pr > threshold).double()
    return (y * pr).sum((0, 2, 3)), pr.sum((0, 2, 3)), y.sum((0, 2, 3))


def case(K, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(2, K, 7, 9, generator=g, dtype=torch.float64) * 2
    y = torch.nn.functional.one_hot(torch.randint(0, K, (2, 7, 9), generator=g), K).permute(0, 3, 1, 2).double()
    return logits, y


@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_scores_from_counters_match_the_oracle(K):
    """Every (ignore_channels, beta, eps, threshold) combination of the issue: values within 1e-12 of oracle.losses.dice_loss /
    iou_loss, and for the soft form the gradients w.r.t. the tp / spr counters within 1e-12 relative of the oracle expression's
    autograd (d loss / d counter through the same sums)."""
    from cmunet_amd import metrics as M
    logits, y = case(K, 10 + K)
    for ign, beta, eps, thr in itertools.product((None, [0], [1, K - 1]), (1.0, 0.5, 2.0), (1e-5, 1e-7, 1.0), (None, 0.5, 0.3)):
        tp, spr, sgt = counters(logits, y, thr)
        tp, spr = tp.clone().requires_grad_(True), spr.clone().requires_grad_(True)
        dice = 1 - M.f_score_from_counters(tp, spr, sgt, beta=beta, eps=eps, ignore_channels=ign)
        iou = 1 - M.iou_from_counters(tp, spr, sgt, eps=eps, ignore_channels=ign)
        assert dice.dtype == torch.float64 and dice.dim() == 0
        want_d = OL.dice_loss(logits, y, eps=eps, beta=beta, threshold=thr, ignore_channels=ign)
        want_i = OL.iou_loss(logits, y, eps=eps, threshold=thr, ignore_channels=ign)
        assert abs(float(dice.detach()) - float(want_d)) <= 1e-12, (ign, beta, eps, thr)
        assert abs(float(iou.detach()) - float(want_i)) <= 1e-12, (ign, beta, eps, thr)
        if thr is not None:
            continue
        # the oracle's own expression as a function of the per-class counters (the sums it forms from pr and gt)
        keep = [c for c in range(K) if c not in (ign or [])]
        for got, ref_fn in ((dice, lambda t, s: OL_dice_of(t, s, sgt[keep].sum(), beta, eps)), (iou, lambda t, s: OL_iou_of(t, s, sgt[keep].sum(), eps))):
            gtp, gspr = torch.autograd.grad(got, (tp, spr), retain_graph=True)
            t0, s0 = tp.detach()[keep].sum().requires_grad_(True), spr.detach()[keep].sum().requires_grad_(True)
            rt, rs = torch.autograd.grad(ref_fn(t0, s0), (t0, s0))
            for c in range(K):
                wt, wsp = (float(rt), float(rs)) if c in keep else (0.0, 0.0)
                assert abs(float(gtp[c]) - wt) <= 1e-12 * abs(wt), (ign, beta, eps, c)
                assert abs(float(gspr[c]) - wsp) <= 1e-12 * abs(wsp), (ign, beta, eps, c)


def OL_dice_of(tp, spr, sgt, beta, eps):
    """oracle.losses.dice_loss from its three sums (losses.py:32-36)."""
    fp, fn = spr - tp, sgt - tp
    return 1 - ((1 + beta ** 2) * tp + eps) / ((1 + beta ** 2) * tp + beta ** 2 * fn + fp + eps)


def OL_iou_of(inter, spr, sgt, eps):
    """oracle.losses.iou_loss from its three sums (losses.py:41-43)."""
    return 1 - (inter + eps) / (sgt + spr - inter + eps)


def test_oracle_expressions_restated_here_are_the_oracle():
    """The two expressions above, fed with the oracle's own sums, give the oracle's values (so the gradient check above is against
    the oracle's arithmetic), and autograd of the oracle through softmax agrees with the chain through the counters."""
    K = 3
    logits, y = case(K, 99)
    lo = logits.clone().requires_grad_(True)
    want = OL.dice_loss(lo, y, eps=1e-5, beta=2.0, threshold=None, ignore_channels=[0])
    tp, spr, sgt = counters(lo, y, None)
    got = OL_dice_of(tp[1:].sum(), spr[1:].sum(), sgt[1:].sum(), 2.0, 1e-5)
    assert abs(float(got) - float(want)) <= 1e-14
    ga, = torch.autograd.grad(want, lo, retain_graph=True)
    gb, = torch.autograd.grad(got, lo)
    assert float((ga - gb).abs().max()) <= 1e-15


def test_constructors_accept_the_new_configurations_and_keep_their_names():
    from cmunet_amd import metrics as M
    d = M.DiceLoss(activation="softmax", threshold=None)
    assert d.__name__ == "dice_loss" and d.threshold is None
    assert M.DiceLoss(eps=1.0, beta=0.5, activation="softmax2d", ignore_channels=[1, 2], threshold=0.3).__name__ == "dice_loss"
    assert M.IoU(eps=1e-3, threshold=None, activation="softmax").__name__ == "iou_loss"
    assert M.IoU(threshold=0.3, activation="softmax", ignore_channels=[0, 7]).__name__ == "iou_loss"
    assert M.DiceMetric().__name__ == "dice_loss"
    assert M.DiceMetric(beta=2.0, threshold=None, ignore_channels=None).__name__ == "dice_loss"
    ce = M.CrossEntropyLoss(weight=[1.0, 2.0, 0.5])
    assert ce.__name__ == "cross_entropy_loss" and ce.weight.dtype == torch.float32 and ce.weight.tolist() == [1.0, 2.0, 0.5]
    assert M.CrossEntropyLoss(weight=torch.tensor([1.0, 3.0], dtype=torch.float64)).weight.dtype == torch.float32
    crit = M.DiceLoss(activation="softmax", threshold=None, ignore_channels=[0]) + ce
    assert crit.__name__ == "dice_loss + cross_entropy_loss"
    assert (0.5 * crit).__name__ == "0.5 * (dice_loss + cross_entropy_loss)"


def test_constructors_refuse_what_the_kernels_do_not_cover():
    from cmunet_amd import metrics as M
    for cls in (M.DiceLoss, M.IoU, M.DiceMetric):
        for act in ("sigmoid", None, "tanh", "logsoftmax", torch.sigmoid):
            with pytest.raises(NotImplementedError):
                cls(activation=act, threshold=0.5, ignore_channels=[0])
        for thr in (0.0, 1.0, -0.1, 1.5):
            with pytest.raises(ValueError):
                cls(activation="softmax", threshold=thr)
        for ign in ([-1], [8], [0, 9], list(range(8))):
            with pytest.raises(ValueError):
                cls(activation="softmax", threshold=0.5, ignore_channels=ign)
        for eps in (0.0, -1e-5):
            with pytest.raises(ValueError):
                cls(activation="softmax", threshold=0.5, eps=eps)
    for cls in (M.DiceLoss, M.DiceMetric):
        for beta in (0.0, -1.0):
            with pytest.raises(ValueError):
                cls(activation="softmax", threshold=0.5, beta=beta)
    with pytest.raises(ValueError):
        M.CrossEntropyLoss(weight=[[1.0, 2.0]])


def test_helper_refuses_ignore_channels_that_do_not_fit_the_class_count():
    """The class count is known only when the counters exist: indices past it, or a list that covers every channel, raise there."""
    from cmunet_amd import metrics as M
    v = torch.ones(3, dtype=torch.float64)
    for ign in ([3], [0, 1, 2], [-1]):
        with pytest.raises(ValueError):
            M.f_score_from_counters(v, v, v, ignore_channels=ign)
        with pytest.raises(ValueError):
            M.iou_from_counters(v, v, v, ignore_channels=ign)
    assert float(M.iou_from_counters(v, v, v, eps=1e-7, ignore_channels=[0, 2])) == 1.0


def test_cpu_tensors_are_refused():
    from cmunet_amd import metrics as M
    lo, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4, dtype=torch.float64)
    crit = M.DiceLoss(activation="softmax", threshold=None, ignore_channels=[0]) + M.CrossEntropyLoss(weight=[1.0, 2.0, 3.0])
    for fn in (crit, M.IoU(threshold=0.3, activation="softmax"), M.DiceMetric(threshold=None), M.CrossEntropyLoss()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(lo, y)
