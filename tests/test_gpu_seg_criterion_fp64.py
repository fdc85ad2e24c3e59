"""The K-class segmentation criterion (cmu_seg_stats_fwd / _bwd of heads.hip and the loss / metric objects of cmunet_amd/metrics.py
on top of them) against float64 references computed on the CPU from the same fp32 logits: oracle/losses.py and its autograd.

Bounds are per element and built from the magnitudes of the terms that enter it (U = 2^-24, the fp32 unit roundoff), in the style of
test_softmax_ce_dice in tests/test_gpu_heads_optim_fp64.py:

* thresholded counters and sum gt are fp64 sums of exact 0/1 (or target) values: 2 U of the value;
* soft counters: every p_c is an fp32 exp (<= 2 U; the kernel gives the rounding of its argument l - max back, so that does not add),
  a sum of K <= 8 non-negative terms (<= 7 U, typically 2-3) and a correctly rounded division (U) -- under 16 U relative, and as all
  terms are non-negative the relative bound carries over to the sums: 16 U of the value;
* ce: the mean of per-pixel terms, each within 8 U of sum_c w_c y_c (|l_c| + |lse|);
* dlogits: the kernel combines the fp32 p in fp64, so the error of an element is that of p_j (< 8 U relative with typical sums)
  times |g_ce|/npix (p_j sum w y) + p_j |G_j|, plus that of p_j sum_c p_c G_c (two factors p: < 16 U), plus the final rounding to
  fp32 (U of the element).  One constant for the whole magnitude: 16, the largest of these, plus the issue's 2 U |l - lse| of the
  same magnitude for the argument of exp (which this kernel does not need: see above).

The worst error / bound ratio seen per K is printed, and written to the file named by CMU_SEG_PARITY_OUT when that is set
(profiles/seg_criterion_parity.txt holds one such run)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import losses as OL

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda"
C_GRAD = 16                              # see the module docstring; the issue's ceiling for it
SHAPES = {"odd": (2, 9, 13), "vec": (3, 64, 64), "issue_large": (5, 256, 256), "scalar_stride": (5, 257, 257), "vec4_stride": (5, 464, 464),
          "vec2_stride": (5, 328, 328), "misaligned": (3, 8, 8)}
THRESHOLD = {2: 0.5, 3: 0.3, 5: 0.5, 8: 0.3}
# The grid is capped at 1,024 blocks of 256 lanes, and a lane takes 4 pixels (K <= 4), 2 (K > 4) or 1 (H*W not a multiple of that):
# a lane runs its grid-stride loop a second time past 1,048,576 / 524,288 / 262,144 pixels.  The issue's (5,3,256,256) takes the
# 4-pixel path (81,920 groups: 320 blocks, one pass), so the passes past the cap have cases of their own, with fp64 targets:
#   scalar path, KT = 4:      (5,3,257,257)  330,245 pixels, 1,291 blocks' worth
#   4-pixel path, KT = 2 / 4: (5,K,464,464)  1,076,480 pixels, 1,052 blocks' worth
#   2-pixel path, KT = 8:     (5,8,328,328)  537,920 pixels, 1,051 blocks' worth
CASES = ([(K, s, t) for K in (2, 3, 5, 8) for s in ("odd", "vec") for t in ("onehot64", "onehot32", "soft64")]
         + [(3, "issue_large", t) for t in ("onehot64", "onehot32", "soft64")]
         + [(3, "scalar_stride", "onehot64"), (3, "scalar_stride", "soft64"), (3, "vec4_stride", "onehot64"), (2, "vec4_stride", "onehot32"),
            (8, "vec2_stride", "soft64")])
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    yield o
    lines = [f"K={K} worst |dlogits - fp64| / bound = {r:.4f}" for K, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    out = os.environ.get("CMU_SEG_PARITY_OUT")
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tests/test_gpu_seg_criterion_fp64.py: worst per-element error of cmu_seg_stats_bwd against oracle autograd in fp64,\n"
                    f"# as a fraction of the bound U * ({C_GRAD} + 2 |l - lse|) * magnitude; worst over the {len(CASES)} (K, shape, target) cases of the\n"
                    f"# test -- {sorted(set(c[1] for c in CASES))} -- and their gradient mixes\n")
            f.write("\n".join(lines) + "\n")


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(K, shape, target, thrs=None):
    """Logits randn * 2 with every fp64 softmax probability at least 1e-3 from the threshold(s) (offending pixels -- at most 2 % --
    get +4 on class pixel_index % K and -4 elsewhere); for K = 2, exact ties l0 == l1 on 5 % of the pixels (p = 0.5: not above 0.5)."""
    B, H, W = SHAPES[shape]
    thrs = thrs or (THRESHOLD[K],)
    thr = thrs[0]
    g = torch.Generator().manual_seed(1000 * K + H + len(target))
    logits = torch.randn(B, K, H, W, generator=g) * 2
    p0 = torch.softmax(logits.double(), 1)
    near = torch.stack([((p0 - t).abs() < 1e-3).any(1) for t in thrs]).any(0)                    # (B,H,W)
    assert float(near.double().mean()) <= 0.02
    pix = torch.arange(B * H * W).view(B, H, W)
    fixed = torch.where(F.one_hot(pix % K, K).permute(0, 3, 1, 2).bool(), 4.0, -4.0)
    logits = torch.where(near.unsqueeze(1), fixed, logits).contiguous()
    ties = torch.zeros(B, H, W, dtype=torch.bool)
    if K == 2:
        ties = torch.rand(B, H, W, generator=g) < 0.05
        logits[:, 1] = torch.where(ties, logits[:, 0], logits[:, 1])
    c = Case()
    c.K, c.B, c.H, c.W, c.thr, c.npix = K, B, H, W, thr, B * H * W
    c.logits = logits
    c.L = logits.double()
    c.p = torch.softmax(c.L, 1)
    clear = torch.stack([((c.p - t).abs() >= 1e-3).all(1) for t in thrs]).all(0)
    assert bool((clear | ties).all()), "a probability within 1e-3 of the threshold: the fp64 hard mask would be ambiguous"
    if K == 2:
        assert bool((c.p[:, 1][ties] == 0.5).all())
    c.lse = torch.logsumexp(c.L, 1, keepdim=True)
    if target.startswith("onehot"):
        y = F.one_hot(torch.randint(0, K, (B, H, W), generator=g), K).permute(0, 3, 1, 2).contiguous()
        c.y_dev = y.double() if target == "onehot64" else y.float()
    else:
        e = -torch.log(torch.rand(B, K, H, W, generator=g, dtype=torch.float64).clamp_min(1e-12))   # rows of a random simplex
        c.y_dev = (e / e.sum(1, keepdim=True)).contiguous()
    c.y = c.y_dev.double()
    c.w = torch.tensor([0.5, 2.0, 1.25, 0.75, 1.5, 1.0, 3.0, 0.25][:K])
    hard = (c.p > thr).double()
    c.tp_soft, c.spr_soft = (c.y * c.p).sum((0, 2, 3)), c.p.sum((0, 2, 3))
    c.tp_hard, c.spr_hard, c.sgt = (c.y * hard).sum((0, 2, 3)), hard.sum((0, 2, 3)), c.y.sum((0, 2, 3))
    return c


def ce_weighted(lo, y, w):
    return -(w.view(1, -1, 1, 1) * y * torch.log_softmax(lo, 1)).sum(1).mean()


def run_fwd(ops, c, weight, thr=None):
    from cmunet_amd import _lib
    K = c.K
    table = torch.empty(1 + 5 * K, dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.lib().cmu_seg_stats_ws_bytes(K), dtype=torch.uint8, device=DEV)
    ops.seg_stats_fwd(c.logits.to(DEV), c.y_dev.to(DEV), None if weight is None else weight.to(DEV), c.thr if thr is None else thr, table, ws)
    return table


@pytest.mark.parametrize("K,shape,target", CASES)
def test_seg_stats_forward(ops, K, shape, target):
    c = make_case(K, shape, target)
    for weight in (None, c.w):
        t = run_fwd(ops, c, weight).cpu()
        w = torch.ones(K, dtype=torch.float64) if weight is None else weight.double()
        ce = float(ce_weighted(c.L, c.y, w))
        ce_bound = 8 * U * float((w.view(1, K, 1, 1) * c.y * (c.L.abs() + c.lse.abs())).sum() / c.npix)
        print(f"K={K} {shape} {target}: ce {float(t[0]):.9g} ref {ce:.9g} err/bound {abs(float(t[0]) - ce) / ce_bound:.3g}")
        assert abs(float(t[0]) - ce) <= ce_bound
    for name, got, want, k in (("tp_soft", t[1:1 + K], c.tp_soft, 16), ("spr_soft", t[1 + K:1 + 2 * K], c.spr_soft, 16),
                               ("tp_hard", t[1 + 2 * K:1 + 3 * K], c.tp_hard, 2), ("spr_hard", t[1 + 3 * K:1 + 4 * K], c.spr_hard, 2),
                               ("sgt", t[1 + 4 * K:], c.sgt, 2)):
        err = (got - want).abs()
        print(f"K={K} {shape} {target}: {name} worst err / (U value) {float((err / (U * want.abs()).clamp_min(1e-300)).max()):.3g}")
        assert bool((err <= k * U * want.abs()).all()), (name, got.tolist(), want.tolist())
    # the same bits every run (fixed-order sums, no floating-point atomics)
    assert torch.equal(run_fwd(ops, c, c.w).cpu(), t)


# (a, b, c) of a * dice_soft + b * ce_w + c * iou_soft, with the Dice / IoU settings that go with it
MIXES = [((1.0, 1.0, 0.0), dict(ign=[0], beta=1.0, eps=1e-5)),
         ((0.7, 0.0, 0.4), dict(ign=None, beta=0.5, eps=1e-7)),
         ((0.0, 1.3, 0.0), dict(ign=[0], beta=1.0, eps=1e-5)),
         ((0.0, 0.0, 1.0), dict(ign=[1, -1], beta=2.0, eps=1.0)),
         ((3.0 * 0.5, 3.0 * 2.0, 3.0 * 0.25), dict(ign=[1, -1], beta=2.0, eps=1.0))]     # a loss scale of 3 on (0.5, 2, 0.25)


def soft_grads(c, a, cc, ign, beta, eps):
    """d (a * dice + cc * iou) / d (tp_soft, spr_soft) from the fp64 reference counters, through the product's own helper (which
    tests/test_cpu_seg_criterion.py holds to the oracle)."""
    from cmunet_amd import metrics as M
    tp, spr = c.tp_soft.clone().requires_grad_(True), c.spr_soft.clone().requires_grad_(True)
    v = a * (1 - M.f_score_from_counters(tp, spr, c.sgt, beta, eps, ign)) + cc * (1 - M.iou_from_counters(tp, spr, c.sgt, eps, ign))
    return torch.autograd.grad(v, (tp, spr))


def grad_bound(c, g_ce, g_tp, g_spr, w):
    K = c.K
    wy = w.view(1, K, 1, 1) * c.y
    G = (g_tp.view(1, K, 1, 1) * c.y + g_spr.view(1, K, 1, 1)).abs()
    mag = abs(g_ce) / c.npix * (c.p * wy.sum(1, keepdim=True) + wy) + c.p * (G + (c.p * G).sum(1, keepdim=True))
    return U * (C_GRAD + 2 * (c.L - c.lse).abs()) * mag


@pytest.mark.parametrize("K,shape,target", CASES)
def test_seg_stats_backward(ops, K, shape, target):
    c = make_case(K, shape, target)
    ld, yd, wd = c.logits.to(DEV), c.y_dev.to(DEV), c.w.to(DEV)
    w = c.w.double()
    mixes = MIXES if shape in ("odd", "vec") else MIXES[:2]
    for (a, b, cc), cfg in mixes:
        ign = None if cfg["ign"] is None else sorted({i % K for i in cfg["ign"]})      # [1, -1]: channels 1 and K - 1
        lo = c.L.clone().requires_grad_(True)
        loss = (a * OL.dice_loss(lo, c.y, eps=cfg["eps"], beta=cfg["beta"], threshold=None, ignore_channels=ign) + b * ce_weighted(lo, c.y, w)
                + cc * OL.iou_loss(lo, c.y, eps=cfg["eps"], threshold=None, ignore_channels=ign))
        loss.backward()
        if a == 0.0 and cc == 0.0:
            g_tp = g_spr = torch.zeros(K, dtype=torch.float64)
            gd = (None, None)                            # NULL pointers stand for zeros
        else:
            g_tp, g_spr = soft_grads(c, a, cc, ign, cfg["beta"], cfg["eps"])
            gd = (g_tp.to(DEV), g_spr.to(DEV))
        dl = torch.full(c.logits.shape, 7.0, device=DEV)
        ops.seg_stats_bwd(ld, yd, wd, torch.tensor([b], dtype=torch.float64, device=DEV), gd[0], gd[1], dl)
        bound = grad_bound(c, b, g_tp, g_spr, w)
        err = (dl.cpu().double() - lo.grad).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        RATIOS[K] = max(RATIOS.get(K, 0.0), ratio)
        print(f"K={K} {shape} {target} mix {(a, b, cc)} ignore {ign}: worst err / bound {ratio:.4f}")
        assert bool((err <= bound).all()), f"mix {(a, b, cc)}: worst err / bound {ratio:.3g}"
        if b == 0.0 and ign:
            # ignored channels: no Dice / IoU term of their own (G_j = 0), only the coupling through the softmax
            G = g_tp.view(1, K, 1, 1) * c.y + g_spr.view(1, K, 1, 1)
            assert bool((G[:, ign] == 0).all())
            want = -c.p[:, ign] * (c.p * G).sum(1, keepdim=True)
            got = dl.cpu().double()[:, ign]
            assert bool(((got - want).abs() <= bound[:, ign]).all())
            assert bool((got != 0).any()) and float(want.abs().max()) > 0


def test_loss_and_metric_objects_three_classes(ops, monkeypatch):
    """DiceLoss(threshold=None, ignore [0]) + CrossEntropyLoss(weight) on K = 3 costs ONE forward pass; its value is the oracle's
    within the propagated counter bounds; its gradient is the backward kernel's output for the gradients autograd hands it, bit for
    bit (also under a MultipliedLoss); thresholded metrics at the pass's threshold reuse it, another threshold costs one more pass."""
    from cmunet_amd import metrics as M
    K = 3
    c = make_case(K, "vec", "onehot64", (0.5, 0.3))
    calls = []
    real = ops.seg_stats_fwd
    monkeypatch.setattr(ops, "seg_stats_fwd", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    w = c.w.double()
    crit = M.DiceLoss(activation="softmax", threshold=None, ignore_channels=[0]) + M.CrossEntropyLoss(weight=c.w)
    M.clear_seg_cache()
    lo = c.logits.to(DEV).requires_grad_(True)
    y = c.y_dev.to(DEV)
    v = crit(lo, y)
    assert calls == [0.5] and v.dtype == torch.float64 and v.dim() == 0 and v.requires_grad
    # value: ce within its bound; 1 - f with f = N / D, N = 2 tp + eps, D = sgt + spr + eps (tp cancels), counters within 16 U / 2 U
    tp, spr, sgt = c.tp_soft[1:].sum(), c.spr_soft[1:].sum(), c.sgt[1:].sum()
    f = (2 * tp + 1e-5) / (sgt + spr + 1e-5)
    want = float(OL.dice_loss(c.L, c.y, threshold=None, ignore_channels=[0]) + ce_weighted(c.L, c.y, w))
    bound = float(32 * U * f + 8 * U * (w.view(1, K, 1, 1) * c.y * (c.L.abs() + c.lse.abs())).sum() / c.npix) + 2 ** -52 * abs(want)
    print(f"module value {float(v.detach()):.12g} ref {want:.12g} err/bound {abs(float(v.detach()) - want) / bound:.3g}")
    assert abs(float(v.detach()) - want) <= bound
    v.backward()

    def op_level(scale):
        table = run_fwd(ops, c, c.w, 0.5).requires_grad_(True)
        tps, sps, sg = table[1:1 + K], table[1 + K:1 + 2 * K], table[1 + 4 * K:]
        expr = (1.0 - M.f_score_from_counters(tps, sps, sg, 1.0, 1e-5, [0])) + table[0]
        if scale is not None:
            expr = scale * expr
        g, = torch.autograd.grad(expr, table)
        dl = torch.empty_like(lo)
        ops.seg_stats_bwd(lo.detach(), y, c.w.to(DEV), g[0:1], g[1:1 + K], g[1 + K:1 + 2 * K], dl)
        return dl

    assert torch.equal(lo.grad, op_level(None))
    n = len(calls)
    # metrics on the same tensors: the pass at 0.5 serves the first two, 0.3 needs its own
    d5 = M.DiceLoss(activation="softmax", threshold=0.5, ignore_channels=[0])(lo, y)
    i5 = M.IoU(activation="softmax", threshold=0.5, ignore_channels=[0])(lo, y)
    assert len(calls) == n
    i3 = M.IoU(activation="softmax", threshold=0.3, ignore_channels=[0])(lo, y)
    assert len(calls) == n + 1 and calls[-1] == pytest.approx(0.3)
    assert not d5.requires_grad and not i5.requires_grad and not i3.requires_grad
    # thresholded values: counters within 2 U; 1 - N / D with D = sgt + spr + eps for Dice (4 U of the score) and D = sgt + spr - tp
    # + eps >= (sgt + spr + tp) / 3 for IoU (2 U + 6 U of the score): 8 U
    for got, ref in ((d5, OL.dice_loss(c.L, c.y, threshold=0.5, ignore_channels=[0])), (i5, OL.iou_loss(c.L, c.y, threshold=0.5, ignore_channels=[0])),
                     (i3, OL.iou_loss(c.L, c.y, threshold=0.3, ignore_channels=[0]))):
        assert got.dtype == torch.float64 and abs(float(got) - float(ref)) <= 8 * U
    # a loss scale through MultipliedLoss reaches the kernel as scaled gradients of ce and the counters
    M.clear_seg_cache()
    lo.grad = None
    (3.0 * crit)(lo, y).backward()
    assert torch.equal(lo.grad, op_level(3.0))
    # the same bits on a second evaluation
    M.clear_seg_cache()
    assert torch.equal(crit(lo, y).detach(), v.detach())


def test_stride_cases_pass_their_grid_cap():
    """The arithmetic behind the *_stride cases: more pixel groups than 1,024 blocks of 256 lanes on the path each one takes.
    A guard on the CASE TABLE, not on the library: it restates plane_width (pixels per lane: 4 at K <= 4, 2 above, 1 when H*W is
    no multiple of that) and plane_grid (CE_MAX_BLOCKS = 1024 blocks of 256) of csrc/plane_stream.h -- change those and this with them."""
    for K, shape, _ in CASES:
        B, H, W = SHAPES[shape]
        V = 1 if (H * W) % (2 if K > 4 else 4) else (2 if K > 4 else 4)
        if shape.endswith("_stride"):
            assert B * H * W // V > 1024 * 256, (K, shape)
            assert V == {"scalar_stride": 1, "vec4_stride": 4, "vec2_stride": 2}[shape]


def dev_x(x, offset):
    """x on the device; ``offset``: starting one element past an allocation's (16-byte aligned) start."""
    if not offset:
        return x.to(DEV)
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
    buf[1:].copy_(x.reshape(-1))
    v = buf[1:].view(x.shape)
    assert v.data_ptr() % 16 == x.element_size() and v.is_contiguous()
    return v


@pytest.mark.parametrize("off", ["logits", "target"])
@pytest.mark.parametrize("K", [2, 5])
def test_misaligned_pointers_take_the_one_pixel_path(ops, K, off):
    """(3,K,8,8): H*W = 64 allows 4 (K = 2) and 2 (K = 5) pixels per lane, so a pointer one element past a 16-byte boundary is all that
    sends the pass down the one-pixel path (plane_width of csrc/plane_stream.h).  Forward and backward hold the bounds of the ``odd``
    cases against the same fp64 references.  Element by element the one-pixel path computes what the vector path does: dlogits and
    spr_hard (a sum of exact 0 / 1) equal the aligned tensors' bit for bit.  The other sums do not have to: a lane adds its
    four pixels before the block does, so rounded fp64 terms meet in another order -- as for the sum S of the pointwise suite."""
    from cmunet_amd import _lib
    (a, b, cc), cfg = MIXES[4]                                # Dice, CE and IoU at once
    ign = sorted({i % K for i in cfg["ign"]})
    for target in ("onehot64", "onehot32", "soft64"):
        c = make_case(K, "misaligned", target)
        w = c.w.double()
        g_tp, g_spr = soft_grads(c, a, cc, ign, cfg["beta"], cfg["eps"])
        tables, grads = [], []
        for lo_off, y_off in ((0, 0), (off == "logits", off == "target")):
            ld, yd, wd = dev_x(c.logits, lo_off), dev_x(c.y_dev, y_off), c.w.to(DEV)
            table = torch.empty(1 + 5 * K, dtype=torch.float64, device=DEV)
            ws = torch.empty(_lib.lib().cmu_seg_stats_ws_bytes(K), dtype=torch.uint8, device=DEV)
            ops.seg_stats_fwd(ld, yd, wd, c.thr, table, ws)
            tables.append(table.cpu())
            dl = torch.full(c.logits.shape, 7.0, device=DEV)
            ops.seg_stats_bwd(ld, yd, wd, torch.tensor([b], dtype=torch.float64, device=DEV), g_tp.to(DEV), g_spr.to(DEV), dl)
            grads.append(dl.cpu())
        t = tables[1]
        ce = float(ce_weighted(c.L, c.y, w))
        ce_bound = 8 * U * float((w.view(1, K, 1, 1) * c.y * (c.L.abs() + c.lse.abs())).sum() / c.npix)
        print(f"K={K} {off} {target}: ce {float(t[0]):.9g} ref {ce:.9g} err/bound {abs(float(t[0]) - ce) / ce_bound:.3g}")
        assert abs(float(t[0]) - ce) <= ce_bound
        for name, got, want, k in (("tp_soft", t[1:1 + K], c.tp_soft, 16), ("spr_soft", t[1 + K:1 + 2 * K], c.spr_soft, 16),
                                   ("tp_hard", t[1 + 2 * K:1 + 3 * K], c.tp_hard, 2), ("spr_hard", t[1 + 3 * K:1 + 4 * K], c.spr_hard, 2),
                                   ("sgt", t[1 + 4 * K:], c.sgt, 2)):
            assert bool(((got - want).abs() <= k * U * want.abs()).all()), (name, got.tolist(), want.tolist())
        lo = c.L.clone().requires_grad_(True)
        (a * OL.dice_loss(lo, c.y, eps=cfg["eps"], beta=cfg["beta"], threshold=None, ignore_channels=ign) + b * ce_weighted(lo, c.y, w)
         + cc * OL.iou_loss(lo, c.y, eps=cfg["eps"], threshold=None, ignore_channels=ign)).backward()
        bound = grad_bound(c, b, g_tp, g_spr, w)
        err = (grads[1].double() - lo.grad).abs()
        print(f"K={K} {off} {target}: dlogits worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.4f}")
        assert bool((err <= bound).all())
        assert torch.equal(grads[1], grads[0]) and torch.equal(tables[1][1 + 3 * K:1 + 4 * K], tables[0][1 + 3 * K:1 + 4 * K])


def test_criterion_and_metrics_do_not_wait_for_the_device(ops):
    """Loss, backward and metrics of a batch issue launches only: with torch's sync debug mode on 'error', any blocking copy or
    host read in the new path (an index tensor built per call, an .item()) raises."""
    from cmunet_amd import metrics as M
    K = 3
    c = make_case(K, "vec", "onehot64", (0.5, 0.3))
    cfg = dict(activation="softmax", ignore_channels=[0])
    crit = (M.DiceLoss(threshold=None, **cfg) + M.CrossEntropyLoss(weight=c.w)).to(DEV)
    mets = [M.DiceLoss(threshold=0.5, **cfg), M.CrossEntropyLoss(), M.IoU(threshold=0.3, **cfg), M.DiceMetric(threshold=None, ignore_channels=[1, 2])]
    lo, y = c.logits.to(DEV).requires_grad_(True), c.y_dev.to(DEV)
    crit(lo, y).backward()                                # first use: library load, allocator warm-up
    [m(lo, y) for m in mets]
    M.clear_seg_cache()
    lo.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        v = crit(lo, y)
        v.backward()
        vals = [m(lo, y) for m in mets]
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(torch.stack([v.detach()] + vals)).all()) and float(lo.grad.abs().max()) > 0


def test_two_class_metrics_reuse_the_soft_loss_pass(ops, monkeypatch):
    """DiceLoss(threshold=None) + CrossEntropyLoss() on two classes runs the K-class pass; reference-configuration metrics called on
    the same tensors afterwards read its counters instead of paying the fused two-class kernel on top."""
    from cmunet_amd import metrics as M
    c = make_case(2, "vec", "onehot64")
    old_calls, new_calls = [], []
    real_old, real_new = ops.softmax_ce_dice_fwd_bwd, ops.seg_stats_fwd
    monkeypatch.setattr(ops, "softmax_ce_dice_fwd_bwd", lambda *a, **k: (old_calls.append(1), real_old(*a, **k))[1])
    monkeypatch.setattr(ops, "seg_stats_fwd", lambda *a, **k: (new_calls.append(1), real_new(*a, **k))[1])
    mk = dict(activation="softmax", threshold=0.5, ignore_channels=[0])
    crit = M.DiceLoss(activation="softmax", threshold=None, ignore_channels=[0]) + M.CrossEntropyLoss()
    M.clear_seg_cache()
    lo, y = c.logits.to(DEV).requires_grad_(True), c.y_dev.to(DEV)
    crit(lo, y).backward()
    d, i, ce = M.DiceLoss(**mk)(lo, y), M.IoU(**mk)(lo, y), M.CrossEntropyLoss()(lo, y)
    assert (len(new_calls), len(old_calls)) == (1, 0)
    assert abs(float(d) - float(OL.dice_loss(c.L, c.y))) <= 8 * U and abs(float(i) - float(OL.iou_loss(c.L, c.y))) <= 8 * U
    assert abs(float(ce.detach()) - float(OL.cross_entropy_prob(c.L, c.y))) <= 8 * U * float((c.y * (c.L.abs() + c.lse.abs())).sum() / c.npix)


def test_reference_configuration_keeps_the_parent_kernel(ops):
    """(B,2,H,W) with the reference driver's configuration: criterion value, its gradient, IoU and DiceMetric are, bit for bit, what
    a direct cmu_softmax_ce_dice_fwd_bwd call on the same tensors gives."""
    from cmunet_amd import _lib, metrics as M
    g = torch.Generator().manual_seed(5)
    B, H, W = 4, 32, 32
    logits = (torch.randn(B, 2, H, W, generator=g) * 2).to(DEV)
    fg = (torch.rand(B, H, W, generator=g) > 0.6).double()
    y = torch.stack([1 - fg, fg], 1).to(DEV)
    out, dl = torch.empty(6, device=DEV), torch.empty(B, 2, H, W, device=DEV)
    ws = torch.empty(_lib.lib().cmu_softmax_ce_dice_ws_bytes(B, H, W), dtype=torch.uint8, device=DEV)
    ops.softmax_ce_dice_fwd_bwd(logits, y, out, dl, 1.0, ws)
    mk = dict(activation="softmax", threshold=0.5, ignore_channels=[0])
    crit = M.DiceLoss(**mk) + M.CrossEntropyLoss()
    M.clear_seg_cache()
    lo = logits.clone().requires_grad_(True)
    v = crit(lo, y)
    v.backward()
    assert torch.equal(v.detach(), out[1].double() + out[0].double())
    assert torch.equal(lo.grad, dl)
    assert torch.equal(M.IoU(**mk)(lo, y), out[2].double())
    assert torch.equal(M.DiceMetric()(lo, y), out[1].double())
