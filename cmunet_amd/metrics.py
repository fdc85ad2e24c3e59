"""Drop-in for the tensor losses / metrics of the reference's ``Finetuning/metrics.py`` that sit on the
training step: the ``Loss`` algebra (``DiceLoss(...) + CrossEntropyLoss()`` with the
reference's snake-case ``__name__``s, metrics.py:9-82), ``DiceLoss`` (:160-180), ``CrossEntropyLoss`` (:503)
and ``IoU`` (:200-220), computed by ONE fused kernel per (prediction, target) pair:
``cmu_softmax_ce_dice_fwd_bwd`` makes a single pass over the logits and yields the CE (with its gradient),
and the thresholded Dice / IoU counters -- the reference makes 4-5 elementwise passes and a host sync each.

The configuration the reference's driver uses (train.py:455-461: 2 classes, activation 'softmax', threshold 0.5, ignore_channels [0],
eps 1e-5 / 1e-7) runs on that kernel.  Every other softmax configuration of the same classes -- 2..8 classes, ``threshold=None`` (the
differentiable Dice / IoU: a Dice term that carries gradient) or any threshold, any ``ignore_channels`` / ``beta`` / ``eps``, per-class CE
weights -- runs on ``cmu_seg_stats_fwd`` / ``cmu_seg_stats_bwd``: one pass per (prediction, target) pair and threshold yields per-class
counters, the scores are a few fp64 flops on those K-vectors, and autograd through them hands the backward kernel its upstream
gradients on the device.  Other activations raise.
Which of the two kernels serves an object in the reference configuration on two-class logits depends on its context: inside a
combined Loss, the fused two-class kernel only if every Dice / CE term of the combination is in that configuration (``_planned``);
called on its own (a metric), the fused kernel unless the K-class pass has already run on the very same tensors (same objects,
versions and grad mode) -- then its cached counters are reused, so the choice follows the call order, as train.py has it: loss first,
metrics after.  Both kernels agree to rounding; only the reference configuration evaluated alone is bit-identical to earlier builds.
``hausdorff`` / ``radius_arteries`` (metrics.py:224-395: scikit-image contours and skeletons, scipy KD-trees on the host) run as
exact lattice geometry on the device (csrc/geometry.hip): no ``.cpu()``, no host sync; two classes only.
``soft_cldice`` takes 2..8 classes too, and with ``threshold=None`` it is a differentiable loss.
A thresholded Dice has no gradient, exactly like the reference's (SURVEY A-4).
The rest of the reference's loss surface (metrics.py:495-551), each a ``Loss`` that returns a 0-dim fp64 device
tensor and composes with ``+`` and a numeric factor:
``L1Loss(reduction)``, ``MSELoss(reduction)``, ``BCELoss(weight, reduction)`` and ``BCEWithLogitsLoss(weight, reduction, pos_weight)``
-- the criterion of a one-channel binary head, ``UNet(out_classes=1)`` -- run on ``cmu_pointwise_loss_fwd`` / ``_bwd``: one streaming
pass yields the fp64 sum, one more the gradient from the device-resident upstream gradient; ``reduction`` is 'mean' or 'sum' ('none'
raises), ``weight`` / ``pos_weight`` are one element or per channel ((C,1,1) / (1,C,1,1), C <= 8).
``RobustCrossEntropyLoss(weight, ignore_index, reduction, label_smoothing)`` takes CLASS-INDEX targets ((B,1,H,W) or (B,H,W) label maps
of int64 / int32 / uint8 / fp32 / fp64, read in their own dtype: 1-8 bytes per pixel instead of the 8K of fp64 one-hot planes) and
``NLLLoss(activation, ignore_channels, threshold)`` one-hot targets whose arg-max over the kept channels is taken in the kernel; both run
on ``cmu_index_ce_fwd`` / ``_bwd`` (2..8 classes), which yield three fp64 sums from which torch's reductions follow on the device.
Choosing the threshold (no reference counterpart): ``prob_histogram`` -- one pass of ``cmu_prob_hist`` -- then
``threshold_sweep`` / ``best_threshold`` (``cmu_hist_curves``: every threshold j / bins at once) and the threshold-free ``Metric``s
``AUROC``, ``AveragePrecision``, ``CalibrationError``.  New names only: every class above keeps its configuration checks.
Losses for thin, rare foregrounds (no reference counterpart), 2..8 classes, softmax: ``FocalLoss`` on
``cmu_focal_fwd`` / ``_bwd`` (label maps or one-hot planes), ``TverskyLoss`` from the pair's counter table (``tversky_from_counters``),
``BoundaryLoss`` and ``HausdorffDTLoss`` on ``cmu_softmax_map_fwd`` / ``_bwd`` with distance maps from the exact on-device transform
(``signed_distance_maps``, ``distance_fields``: ``cmu_edt_columns`` / ``cmu_edt_rows`` / ``cmu_distance_field``).
``LovaszSoftmaxLoss``, the surrogate of the Jaccard index itself: ``cmu_lovasz_keys`` -> ``cmu_sort_u64`` (a
hand-written segmented key sort) -> ``cmu_lovasz_grad``; its backward is ``cmu_softmax_map_bwd``.
"""
import collections
import math
import weakref

import torch
import torch.nn as nn

from . import _lib, ops


def _snake(name):
    """'CrossEntropyLoss' -> 'cross_entropy_loss': the log keys of the reference's drivers (train.py:455-461 prints and selects
    checkpoints by 'dice_loss'; metrics.py:9-24 derives them from the class names)."""
    out = []
    for i, ch in enumerate(name):
        if ch.isupper() and i and (name[i - 1].islower() or name[i - 1].isdigit() or (i + 1 < len(name) and name[i + 1].islower())):
            out.append("_")
        out.append(ch.lower())
    return "".join(out)


class BaseObject(nn.Module):
    """Named module: ``__name__`` is the explicit name or the snake-case class name (the reference's log-key contract)."""

    def __init__(self, name=None):
        super().__init__()
        self._name = name

    @property
    def __name__(self):
        return self._name if self._name is not None else _snake(type(self).__name__)


class Metric(BaseObject):
    pass


class Loss(BaseObject):
    """Losses combine with ``+`` and scale with a number (metrics.py:27-82): the result is again a Loss whose name spells the
    expression, e.g. 'dice_loss + cross_entropy_loss' (train.py:455) or '2 * (dice_loss + cross_entropy_loss)'."""

    def _terms(self):
        return [(1.0, self)]

    def _leaves(self):
        return [self]

    def __add__(self, other):
        if not isinstance(other, Loss):
            raise ValueError("Loss should be inherited from `Loss` class")
        return SumOfLosses(self, other)

    __radd__ = __add__

    def __mul__(self, value):
        if not isinstance(value, (int, float)):
            raise ValueError("Loss should be inherited from `BaseLoss` class")
        return MultipliedLoss(self, value)

    __rmul__ = __mul__


class SumOfLosses(Loss):
    def __init__(self, l1, l2):
        super().__init__(name=f"{l1.__name__} + {l2.__name__}")
        self.l1, self.l2 = l1, l2

    def _leaves(self):
        return self.l1._leaves() + self.l2._leaves()

    def forward(self, *inputs):
        return _planned(self, inputs, lambda: self.l1.forward(*inputs) + self.l2.forward(*inputs))

    __call__ = forward


class MultipliedLoss(Loss):
    def __init__(self, loss, multiplier):
        inner = loss.__name__
        super().__init__(name=f"{multiplier} * ({inner})" if "+" in inner else f"{multiplier} * {inner}")
        self.loss, self.multiplier = loss, multiplier

    def _leaves(self):
        return self.loss._leaves()

    def forward(self, *inputs):
        return _planned(self, inputs, lambda: self.multiplier * self.loss.forward(*inputs))

    __call__ = forward


# ---------------------------------------------------------------------------------------------------
# one fused pass per (logits, target) pair, shared by every loss / metric object evaluated on it
# ---------------------------------------------------------------------------------------------------
class _SegStatsFn(torch.autograd.Function):
    """out[0..2] = (ce, dice_loss, iou_loss); gradient flows through the CE entry only."""

    @staticmethod
    def forward(ctx, logits, y1h):
        B, K, H, W = logits.shape
        out = torch.empty(6, dtype=torch.float32, device=logits.device)
        dl = torch.empty_like(logits)
        ws = ops.workspace("cmu_softmax_ce_dice_ws_bytes", logits.device, B, H, W)
        ops.softmax_ce_dice_fwd_bwd(logits.detach().contiguous(), y1h.contiguous(), out, dl, 1.0, ws)
        ctx.save_for_backward(dl)
        return out

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g[0], None


# The loss and each metric object are called with the SAME (prediction, target) tensors one after the other
# (train.py:127-136); the fused pass runs once for the pair.  The pair is recognised by object identity through weak
# references (an address + version key would also match a LATER batch that the caching allocator placed at the same
# address once the earlier tensors were freed -- e.g. the first test batch after the last validation batch).
_cache = {"pr": None, "gt": None, "ver": None, "out": None}


def seg_stats(y_pr, y_gt):
    if not y_pr.is_cuda:
        raise RuntimeError("metrics: the HIP path needs CUDA/ROCm tensors (no CPU fallback)")
    if y_pr.dim() != 4 or y_pr.shape[1] != 2 or y_gt.shape != y_pr.shape:
        raise NotImplementedError("fused segmentation losses support (B,2,H,W) logits with one-hot targets of the same shape")
    ver = (y_pr._version, y_gt._version, y_pr.requires_grad and torch.is_grad_enabled())
    pr, gt = _cache["pr"], _cache["gt"]
    if pr is None or pr() is not y_pr or gt() is not y_gt or _cache["ver"] != ver:
        y = y_gt if y_gt.dtype == torch.float64 else y_gt.double()
        out = _SegStatsFn.apply(y_pr.float(), y)
        _cache.update(pr=weakref.ref(y_pr), gt=weakref.ref(y_gt), ver=ver, out=out)
    return _cache["out"]


def _check_cfg(activation, threshold, ignore_channels, what):
    if activation not in ("softmax", "softmax2d") or threshold != 0.5 or list(ignore_channels or []) != [0]:
        raise NotImplementedError(f"{what}: the HIP path implements the reference driver's configuration only "
                                  "(activation='softmax', threshold=0.5, ignore_channels=[0]; train.py:455-461)")


# ---------------------------------------------------------------------------------------------------
# any class count (2..8), threshold (None = the differentiable form), ignore_channels, beta, eps, class weights:
# cmu_seg_stats_fwd / _bwd yield per-class counters, the scores are a few fp64 flops on K-element device tensors
# ---------------------------------------------------------------------------------------------------
def _kept(K, ignore_channels):
    ign = sorted(set(int(c) for c in (ignore_channels or ())))
    if any(c < 0 or c >= K for c in ign):
        raise ValueError(f"ignore_channels {ign} out of range for {K} channels")
    keep = [c for c in range(K) if c not in ign]
    if not keep:
        raise ValueError("ignore_channels leaves no channel")
    return keep


def _kept_sums(ignore_channels, *vectors):
    K = vectors[0].shape[0]
    keep = _kept(K, ignore_channels)
    if len(keep) == K:
        return [v.sum() for v in vectors]
    # (element picks with Python indices: an index TENSOR built here would be a host-to-device copy, i.e. a host sync, per call)
    return [torch.stack([v[c] for c in keep]).sum() for v in vectors]


def f_score_from_counters(tp, spr, sgt, beta=1.0, eps=1e-5, ignore_channels=None):
    """metrics.py:135-157 from per-class fp64 counters (K,) -- tp = sum gt*pr, spr = sum pr, sgt = sum gt, soft or thresholded --
    over the channels that ``ignore_channels`` keeps.  Pure torch (CPU or device tensors), differentiable in tp / spr."""
    tp, spr, sgt = _kept_sums(ignore_channels, tp, spr, sgt)
    b2 = float(beta) ** 2
    return ((1 + b2) * tp + eps) / ((1 + b2) * tp + b2 * (sgt - tp) + (spr - tp) + eps)


def iou_from_counters(tp, spr, sgt, eps=1e-7, ignore_channels=None):
    """metrics.py:182-198 from the same counters: (intersection + eps) / (sum gt + sum pr - intersection + eps)."""
    tp, spr, sgt = _kept_sums(ignore_channels, tp, spr, sgt)
    return (tp + eps) / (sgt + spr - tp + eps)


def tversky_from_counters(tp, spr, sgt, alpha=0.5, beta=0.5, eps=1e-7, ignore_channels=None):
    """The Tversky index (Salehi et al.) from the same counters, pooled over the kept channels as ``f_score_from_counters`` pools
    them: (tp + eps) / (tp + alpha fp + beta fn + eps) with fp = spr - tp, fn = sgt - tp.  alpha = beta = 0.5 is the Dice score."""
    tp, spr, sgt = _kept_sums(ignore_channels, tp, spr, sgt)
    return (tp + eps) / (tp + alpha * (spr - tp) + beta * (sgt - tp) + eps)


class _SegTableFn(torch.autograd.Function):
    """table = [ce | tp_soft | spr_soft | tp_hard | spr_hard | sgt] (1 + 5K fp64); the backward kernel takes the incoming gradients
    of ce and of the soft counters straight from the device (the thresholded counters and sgt carry none)."""

    @staticmethod
    def forward(ctx, logits, y, class_w, threshold):
        K = logits.shape[1]
        table = torch.empty(1 + 5 * K, dtype=torch.float64, device=logits.device)
        ws = ops.workspace("cmu_seg_stats_ws_bytes", logits.device, K)
        lg = logits.detach().contiguous()
        ops.seg_stats_fwd(lg, y, class_w, threshold, table, ws)
        ctx.save_for_backward(lg, y, class_w)
        return table

    @staticmethod
    def backward(ctx, g):
        lg, y, class_w = ctx.saved_tensors
        K = lg.shape[1]
        g = g.contiguous()
        dl = torch.empty_like(lg)
        ops.seg_stats_bwd(lg, y, class_w, g[0:1], g[1:1 + K], g[1 + K:1 + 2 * K], dl)
        return dl, None, None, None


DEFAULT_THRESHOLD = 0.5     # the threshold of a pass that only soft losses / the CE asked for
_tables = {"pr": None, "gt": None, "ver": None, "entries": []}   # entries: (threshold, class weight or None, table)
_plan = None                # set while a combined Loss evaluates its terms: {"legacy": bool, "weight": tensor or None}


def _planned(loss, inputs, evaluate):
    """Evaluate a combined Loss with its terms agreed on ONE pass: the parent's fused two-class kernel only if every Dice / CE term
    is in the reference driver's configuration, and the class weights of its CE term known to the term that runs first."""
    global _plan
    if _plan is not None:
        return evaluate()
    seg = [l for l in loss._leaves() if hasattr(l, "_reference_cfg")]
    ces = [l for l in seg if isinstance(l, CrossEntropyLoss)]
    weight = None
    if len(ces) == 1 and inputs and torch.is_tensor(inputs[0]) and inputs[0].is_cuda:
        weight = ces[0]._weight_on(inputs[0].device)
    _plan = {"legacy": all(l._reference_cfg for l in seg), "weight": weight}
    try:
        return evaluate()
    finally:
        _plan = None


def clear_seg_cache():
    _cache.update(pr=None, gt=None, ver=None, out=None)
    _tables.update(pr=None, gt=None, ver=None, entries=[])


def seg_table(y_pr, y_gt, threshold=None, class_w=None, any_weight=False):
    """The counter table of the pair, from the cache when a pass with this threshold (``None``: any) and these class weights
    (``any_weight``: any) has run on the same tensors; one pass per distinct threshold otherwise."""
    if not y_pr.is_cuda:
        raise RuntimeError("metrics: the HIP path needs CUDA/ROCm tensors (no CPU fallback)")
    if y_pr.dim() != 4 or not 2 <= y_pr.shape[1] <= ops.SEG_MAX_K or y_gt.shape != y_pr.shape:
        raise NotImplementedError(f"segmentation losses support (B,K,H,W) logits, 2 <= K <= {ops.SEG_MAX_K}, with targets of the same shape")
    ver = (y_pr._version, y_gt._version, y_pr.requires_grad and torch.is_grad_enabled())
    pr, gt = _tables["pr"], _tables["gt"]
    if pr is None or pr() is not y_pr or gt() is not y_gt or _tables["ver"] != ver:
        _tables.update(pr=weakref.ref(y_pr), gt=weakref.ref(y_gt), ver=ver, entries=[])
    for t, w, table in _tables["entries"]:
        if (threshold is None or t == threshold) and (any_weight or w is class_w):
            return table
    if any_weight and _plan is not None:
        class_w = _plan["weight"]
    if class_w is not None and class_w.shape[0] != y_pr.shape[1]:
        raise ValueError(f"CrossEntropyLoss: {class_w.shape[0]} class weights for {y_pr.shape[1]} classes")
    t = DEFAULT_THRESHOLD if threshold is None else threshold
    y = y_gt if y_gt.dtype in (torch.float32, torch.float64) else y_gt.double()
    table = _SegTableFn.apply(y_pr.float(), y.contiguous(), class_w, t)
    _tables["entries"].append((t, class_w, table))
    return table


def _counters(table, threshold):
    K = (table.shape[0] - 1) // 5
    o = 1 if threshold is None else 1 + 2 * K
    return table[o:o + K], table[o + K:o + 2 * K], table[1 + 4 * K:1 + 5 * K]


def _check_seg_cfg(what, activation, threshold, ignore_channels, eps, beta=1.0):
    if activation not in ("softmax", "softmax2d"):
        raise NotImplementedError(f"{what}: activation 'softmax' / 'softmax2d' only on the HIP path (got {activation!r})")
    if threshold is not None and not 0.0 < float(threshold) < 1.0:
        raise ValueError(f"{what}: threshold must be None or inside (0, 1), got {threshold}")
    if not eps > 0 or not beta > 0:
        raise ValueError(f"{what}: eps and beta must be positive (got eps={eps}, beta={beta})")
    _kept(ops.SEG_MAX_K, ignore_channels)


def _pair_has_tables(y_pr, y_gt):
    """A counter table of exactly this pair (same tensors, versions and grad mode) is in the cache."""
    pr, gt = _tables["pr"], _tables["gt"]
    return (pr is not None and pr() is y_pr and gt() is y_gt and bool(_tables["entries"])
            and _tables["ver"] == (y_pr._version, y_gt._version, y_pr.requires_grad and torch.is_grad_enabled()))


def _use_legacy(obj, y_pr, y_gt):
    """The reference driver's configuration on two-class logits keeps the parent's fused kernel (the same bits as ever); inside a
    combined Loss only when every Dice / CE term of it is in that configuration, so that the combination still costs one pass.
    On its own (a metric), such an object reuses the counters of the pair when the loss before it ran the K-class pass on the same
    tensors -- e.g. DiceLoss(threshold=None) + CrossEntropyLoss() on two classes -- instead of paying the fused kernel on top."""
    if not (obj._reference_cfg and y_pr.dim() == 4 and y_pr.shape[1] == 2):
        return False
    return _plan["legacy"] if _plan is not None else not _pair_has_tables(y_pr, y_gt)


class _SegScore:
    """Shared by DiceLoss / DiceMetric / IoU: configuration and the loss value 1 - score from the pair's counters."""

    def _configure(self, what, activation, threshold, ignore_channels, eps, beta, ref_eps):
        _check_seg_cfg(what, activation, threshold, ignore_channels, eps, beta)
        self.eps, self.beta, self.threshold = float(eps), float(beta), None if threshold is None else float(threshold)
        self.activation, self.ignore_channels = activation, None if ignore_channels is None else list(ignore_channels)
        self._reference_cfg = threshold == 0.5 and list(ignore_channels or []) == [0] and eps == ref_eps and beta == 1.0

    def _dice(self, y_pr, y_gt):
        tp, spr, sgt = _counters(seg_table(y_pr, y_gt, self.threshold, any_weight=True), self.threshold)
        return 1.0 - f_score_from_counters(tp, spr, sgt, self.beta, self.eps, self.ignore_channels)

    def _iou(self, y_pr, y_gt):
        tp, spr, sgt = _counters(seg_table(y_pr, y_gt, self.threshold, any_weight=True), self.threshold)
        return 1.0 - iou_from_counters(tp, spr, sgt, self.eps, self.ignore_channels)


class DiceLoss(Loss, _SegScore):
    """metrics.py:160-180.  ``threshold=None`` is the differentiable Dice (its gradient reaches the logits through
    cmu_seg_stats_bwd); with a threshold the value is a step function of the logits and carries no gradient (SURVEY A-4)."""

    def __init__(self, eps=1e-5, beta=1.0, activation=None, ignore_channels=None, threshold=None, **kwargs):
        super().__init__(**kwargs)
        self._configure("DiceLoss", activation, threshold, ignore_channels, eps, beta, 1e-5)

    def forward(self, y_pr, y_gt):
        if _use_legacy(self, y_pr, y_gt):
            return seg_stats(y_pr, y_gt)[1].detach().double()
        v = self._dice(y_pr, y_gt)
        return v if self.threshold is None else v.detach()


class CrossEntropyLoss(Loss):
    """nn.CrossEntropyLoss(weight) with probability (one-hot float) targets, mean over B*H*W (metrics.py:503)."""

    def __init__(self, weight=None, **kwargs):
        super().__init__(**kwargs)
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).detach().clone().contiguous())
        if self.weight is not None and self.weight.dim() != 1:
            raise ValueError("CrossEntropyLoss: weight is a vector of one value per class")
        self._reference_cfg = weight is None

    def _weight_on(self, device):
        """The weight buffer, moved to ``device`` once (the cache recognises a pass by the identity of its weight tensor)."""
        if self.weight is not None and self.weight.device != device:
            self.weight = self.weight.to(device)
        return self.weight

    def forward(self, y_pr, y_gt):
        if _use_legacy(self, y_pr, y_gt):
            return seg_stats(y_pr, y_gt)[0].double()
        return seg_table(y_pr, y_gt, None, self._weight_on(y_pr.device))[0]


class IoU(Metric, _SegScore):
    __name__ = "iou_loss"

    def __init__(self, eps=1e-7, threshold=0.5, activation=None, ignore_channels=None, **kwargs):
        super().__init__(**kwargs)
        self._configure("IoU", activation, threshold, ignore_channels, eps, 1.0, 1e-7)

    def forward(self, y_pr, y_gt):
        if _use_legacy(self, y_pr, y_gt):
            return seg_stats(y_pr, y_gt)[2].detach().double()
        return self._iou(y_pr, y_gt).detach()


class DiceMetric(Metric, _SegScore):
    """The Dice loss value used as a metric (train.py:456-461 lists DiceLoss among the metrics)."""
    __name__ = "dice_loss"

    def __init__(self, eps=1e-5, beta=1.0, activation="softmax", ignore_channels=(0,), threshold=0.5, **kwargs):
        super().__init__(**kwargs)
        self._configure("DiceMetric", activation, threshold, ignore_channels, eps, beta, 1e-5)

    def forward(self, y_pr, y_gt):
        if _use_legacy(self, y_pr, y_gt):
            return seg_stats(y_pr, y_gt)[1].detach().double()
        return self._dice(y_pr, y_gt).detach()


def _cldice_planes_sums(logits, y, keep, threshold, num_iter, save):
    """(four clDice sums (fp32, device), what a backward needs or None): planes of the kept channels -> both soft skeletons -> sums."""
    B, K, H, W = logits.shape
    dev = logits.device
    yp = torch.empty(B * len(keep), H, W, dtype=torch.float32, device=dev)
    yt = torch.empty_like(yp)
    ops.softmax_planes(logits, y, keep, threshold, yp, yt)
    sp, st = torch.empty_like(yp), torch.empty_like(yp)
    ws = ops.workspace("cmu_soft_skeleton_ws_bytes", dev, yp.numel())
    kept = ops.soft_skeleton_save(yp, sp, num_iter) if save else ops.soft_skeleton(yp, sp, num_iter, ws)
    ops.soft_skeleton(yt, st, num_iter, ws)
    out4 = torch.empty(4, dtype=torch.float32, device=dev)
    ops.cldice_sums(sp, yt, st, yp, out4)
    return out4, ((yp, yt, st, kept) if save else None)


class _ClDiceSumsFn(torch.autograd.Function):
    """The four sums of the soft (threshold=None) clDice as fp64; the backward takes their incoming gradients g0..g3 straight from
    the device: dL/dskel_pred = g0 y_true + g1 runs down the skeleton's levels (cmu_soft_skeleton_bwd, which also adds the sums' own
    term g2 skel_true), and cmu_softmax_planes_bwd carries the planes' gradient to the logits.  The target has no gradient."""

    @staticmethod
    def forward(ctx, logits, y, keep, num_iter):
        lg = logits.detach().contiguous()
        out4, saved = _cldice_planes_sums(lg, y, keep, None, num_iter, True)
        ctx.save_for_backward(lg, *saved)
        ctx.keep, ctx.num_iter = keep, num_iter
        return out4.double()

    @staticmethod
    def backward(ctx, g):
        lg, yp, yt, st, kept = ctx.saved_tensors
        G = torch.empty_like(yp)
        ops.soft_skeleton_bwd(yp, kept, ctx.num_iter, G, g4=g.contiguous(), y_true=yt, skel_true=st)
        dl = torch.empty_like(lg)
        ops.softmax_planes_bwd(lg, G, ctx.keep, dl)
        return dl, None, None, None


class soft_cldice(Loss):
    """Soft clDice (metrics.py:401-431) on the device: softmax -> kept channels (``ignore_channels``, then ``exclude_background``
    drops the first channel left) -> soft skeletons of prediction and target by ``num_iter`` = 10 rounds of min/max pooling -> four
    sums (cmu_cldice_sums) -> 1 - 2*tprec*tsens/(tprec+tsens) in fp64.  2..8 classes.
    ``threshold=None`` is the differentiable loss: its gradient reaches the logits through one autograd.Function (a reverse sweep over
    the skeleton's levels and a softmax backward, csrc/cldice_grad.hip); nothing is kept for a backward under
    ``no_grad`` or for logits that need no gradient.  With a threshold the skeletons are those of the binarised prediction and the
    value carries no gradient, as in the reference; the driver's configuration (train.py:464: a threshold, ignore_channels [0]) on
    two-class logits runs its own kernel sequence (cmu_softmax2_threshold) as before.  Other activations raise."""
    __name__ = "soft_clDice"

    def __init__(self, iter_=3, smooth=1., exclude_background=False, threshold=0.5, activation=None, ignore_channels=None):
        super().__init__()
        if activation not in ("softmax", "softmax2d"):
            raise NotImplementedError(f"soft_cldice: activation 'softmax' / 'softmax2d' only on the HIP path (got {activation!r})")
        if not smooth > 0:
            raise ValueError(f"soft_cldice: smooth must be positive (got {smooth})")
        _kept(ops.SEG_MAX_K, ignore_channels)
        self.iter, self.smooth, self.num_iter = iter_, smooth, 10      # (iter_ is unused in the reference too: SoftSkeletonize(num_iter=10))
        self.threshold = None if threshold is None else float(threshold)
        self.activation, self.exclude_background = activation, bool(exclude_background)
        self.ignore_channels = None if ignore_channels is None else list(ignore_channels)

    def _keep(self, K):
        keep = _kept(K, self.ignore_channels)
        if self.exclude_background:
            keep = keep[1:]
            if not keep:
                raise ValueError("soft_cldice: exclude_background leaves no channel")
        return keep

    def _driver_sums(self, y_pred, y_true):
        """The driver's thresholded configuration on two classes: the kernel sequence (and the bits) it has always had."""
        B, K, H, W = y_pred.shape
        logits = y_pred.detach().float().contiguous()
        yt = y_true[:, 1].detach().float().contiguous()
        yp = torch.empty(B, H, W, dtype=torch.float32, device=y_pred.device)
        ops.softmax2_threshold(logits, self.threshold, yp)
        ws = ops.workspace("cmu_soft_skeleton_ws_bytes", y_pred.device, B * H * W)
        sp, st = torch.empty_like(yp), torch.empty_like(yp)
        ops.soft_skeleton(yp, sp, self.num_iter, ws)
        ops.soft_skeleton(yt, st, self.num_iter, ws)
        out4 = torch.empty(4, dtype=torch.float32, device=y_pred.device)
        ops.cldice_sums(sp, yt, st, yp, out4)
        return out4.double()

    def forward(self, y_pred, y_true):
        if not y_pred.is_cuda:
            raise RuntimeError("soft_cldice runs on the GPU only (no CPU fallback)")
        if y_pred.dim() != 4 or not 2 <= y_pred.shape[1] <= ops.SEG_MAX_K or y_true.shape != y_pred.shape:
            raise NotImplementedError(f"soft_cldice: (B,K,H,W) logits, 2 <= K <= {ops.SEG_MAX_K}, with targets of the same shape")
        K = y_pred.shape[1]
        keep = self._keep(K)
        if self.threshold is not None and K == 2 and keep == [1] and not self.exclude_background:
            s = self._driver_sums(y_pred, y_true)
        else:
            y = y_true.detach()
            y = (y if y.dtype in (torch.float32, torch.float64) else y.float()).contiguous()
            if self.threshold is None and y_pred.requires_grad and torch.is_grad_enabled():
                s = _ClDiceSumsFn.apply(y_pred.float(), y, keep, int(self.num_iter))
            else:
                s = _cldice_planes_sums(y_pred.detach().float().contiguous(), y, keep, self.threshold, int(self.num_iter), False)[0].double()
        tprec = (s[0] + self.smooth) / (s[1] + self.smooth)
        tsens = (s[2] + self.smooth) / (s[3] + self.smooth)
        return 1. - 2.0 * (tprec * tsens) / (tprec + tsens)


# ---------------------------------------------------------------------------------------------------
# geometry metrics: hausdorff, radius_arteries (metrics.py:224-395) on the doubled lattice (csrc/geometry.hip)
# ---------------------------------------------------------------------------------------------------
def _as_masks(image, clear_border=False):
    """(H,W) or (B,H,W) device tensor -> ((B,H,W) uint8 0/1 of ``image > 0``, batched?)."""
    if not image.is_cuda:
        raise RuntimeError("geometry metrics run on the GPU only (no CPU fallback)")
    batched = image.dim() == 3
    if image.dim() not in (2, 3):
        raise ValueError("masks must be (H, W) or (B, H, W)")
    x = image if batched else image.unsqueeze(0)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()
    x = x.contiguous()
    B, H, W = x.shape
    m = torch.empty(B, H, W, dtype=torch.uint8, device=x.device)
    _lib.call("cmu_plane_mask", ops._p(x), int(x.dtype == torch.float64), 1, 0, ops._p(m), B, H, W, int(clear_border), ops._stream())
    return m, batched


def _contour_points(m):
    """(lattice weight map (B,2H-1,2W-1) uint8, counts (B,2) int32 = (crossings, closed contours)) of find_contours(m > 0)."""
    B, H, W = m.shape
    wmap = torch.empty(B, 2 * H - 1, 2 * W - 1, dtype=torch.uint8, device=m.device)
    cnt = torch.empty(B, 2, dtype=torch.int32, device=m.device)
    ws = torch.empty(max(1, _lib.lib().cmu_contour_points_ws_bytes(B, H, W)), dtype=torch.uint8, device=m.device)
    _lib.call("cmu_contour_points", ops._p(m), ops._p(wmap), ops._p(cnt), B, H, W, ops._p(ws), ops._stream())
    return wmap, cnt


def _nearest(seeds, queries, query_pixels, H, W):
    """(B,4) fp64 (sum w*d, sum w, max d, min d): every query point's distance to the nearest seed point."""
    B = seeds.shape[0]
    if W > 512:
        raise NotImplementedError(f"geometry metrics: W <= 512 (got {W})")
    out = torch.empty(B, 4, dtype=torch.float64, device=seeds.device)
    ws = ops.workspace("cmu_lattice_nearest_ws_bytes", seeds.device, B, H, W)
    _lib.call("cmu_lattice_nearest", ops._p(seeds), ops._p(queries), int(query_pixels), ops._p(out), B, H, W, ops._p(ws), ops._stream())
    return out


def _check_geometry_size(H, W):
    if H * ((W + 31) // 32) * 32 > 512 * 512 or W > 512:
        raise NotImplementedError(f"geometry metrics support H * W <= 512 * 512 with W <= 512 (one workgroup per image holds the "
                                  f"bit-packed mask in LDS); got {H} x {W}")


def skeletonize(mask):
    """scikit-image 2-D ``skeletonize`` of (B,H,W) / (H,W) device masks (``mask > 0``) -> uint8 0/1 of the same shape."""
    m, batched = _as_masks(mask)
    B, H, W = m.shape
    _check_geometry_size(H, W)
    sk = torch.empty_like(m)
    _lib.call("cmu_skeletonize", ops._p(m), ops._p(sk), B, H, W, ops._stream())
    return sk if batched else sk[0]


def contour_counts(mask):
    """(B,2) int32 per image: (crossings, closed contours) of ``find_contours(mask > 0)``; the point count is their sum."""
    m, batched = _as_masks(mask)
    cnt = _contour_points(m)[1]
    return cnt if batched else cnt[0]


def _hausdorff_masks(a, b, modified=True, standard=True):
    B, H, W = a.shape
    _check_geometry_size(H, W)
    wa, ca = _contour_points(a)
    wb, cb = _contour_points(b)
    fwd = _nearest(wa, wb, 0, H, W)        # every point of b to the nearest point of a (cKDTree(a).query(b))
    bwd = _nearest(wb, wa, 0, H, W)
    om = torch.empty(B, dtype=torch.float64, device=a.device) if modified else None
    os_ = torch.empty(B, dtype=torch.float64, device=a.device) if standard else None
    _lib.call("cmu_hausdorff_finish", ops._p(ca), ops._p(cb), ops._p(fwd), ops._p(bwd), ops._p(om), ops._p(os_), B, ops._stream())
    return om, os_


def hausdorff_distance_mask(image0, image1, method='modified'):
    """metrics.py:224-293 on device masks ((H,W) or (B,H,W), foreground = ``> 0``): the Hausdorff distance between the contour
    point sets of ``find_contours``, per image as fp64 (a 0-dim tensor for (H,W) inputs).  0 when both sets are empty, inf when
    one is.  'modified' counts the repeated first point of every closed contour twice, as the reference's point arrays do."""
    if method not in ('standard', 'modified'):
        raise ValueError(f'unrecognized method {method}')
    a, batched = _as_masks(image0)
    b, _ = _as_masks(image1)
    if a.shape != b.shape:
        raise ValueError("both masks must have the same shape")
    om, os_ = _hausdorff_masks(a, b, modified=method == 'modified', standard=method == 'standard')
    out = om if method == 'modified' else os_
    return out if batched else out[0]


def _radius_of_masks(m):
    """m: (B,H,W) uint8 with the border already cleared -> (B,3) fp64."""
    B, H, W = m.shape
    _check_geometry_size(H, W)
    w, cnt = _contour_points(m)
    sk = torch.empty_like(m)
    _lib.call("cmu_skeletonize", ops._p(m), ops._p(sk), B, H, W, ops._stream())
    near = _nearest(w, sk, 1, H, W)
    out = torch.empty(B, 3, dtype=torch.float64, device=m.device)
    _lib.call("cmu_radius_finish", ops._p(cnt), ops._p(near), ops._p(out), B, ops._stream())
    return out


def compute_radius_arteries(mask):
    """metrics.py:378-395 on device masks ((H,W) or (B,H,W), foreground = ``> 0``): with the one-pixel border cleared, the distances
    from every skeleton pixel to the nearest contour point -> (2 min, 2 mean, 2 max) per image, (B,3) fp64 ((3,) for an (H,W) mask).
    (0, 0, 0) when the cleared mask has no contour.  Where the skeleton is empty but the contour is not the reference raises
    (``np.min`` of an empty list); here that image's row is nan.  The input is not modified (the reference clears its argument)."""
    m, batched = _as_masks(mask, clear_border=True)
    out = _radius_of_masks(m)
    return out if batched else out[0]


def _check_two_class(y_pr, y_gt, what):
    if not y_pr.is_cuda:
        raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")
    if y_pr.dim() != 4 or y_pr.shape[1] != 2 or y_gt.shape != y_pr.shape:
        raise NotImplementedError(f"{what}: two-class (B,2,H,W) logits with one-hot targets of the same shape")


class hausdorff(Metric):
    """metrics.py:295-331: per image, the modified Hausdorff distance between the contours of the thresholded prediction
    (softmax, > threshold, channel 1) and of the target's channel 1; the batch value is the mean over images (inf if any image
    is inf: one empty contour against a non-empty one).  The reference's ``torch.mean(torch.tensor(list))`` of per-image numpy
    float64 values is an fp64 mean; so is this one.  Only the driver's configuration (train.py:463) runs on the HIP path."""
    __name__ = "hausdorff"

    def __init__(self, threshold=0.5, activation=None, ignore_channels=None, **kwargs):
        super().__init__(**kwargs)
        _check_cfg(activation, threshold, ignore_channels, "hausdorff")
        self.threshold, self.ignore_channels = threshold, ignore_channels

    def per_image(self, y_pr, y_gt):
        """(B,) fp64: the reference's list ``hausdorff_distances`` (metrics.py:327-330)."""
        _check_two_class(y_pr, y_gt, "hausdorff")
        B, _, H, W = y_pr.shape
        logits = y_pr.detach().float().contiguous()
        yp = torch.empty(B, H, W, dtype=torch.float32, device=y_pr.device)
        ops.softmax2_threshold(logits, self.threshold, yp)
        a = torch.empty(B, H, W, dtype=torch.uint8, device=y_pr.device)
        _lib.call("cmu_plane_mask", ops._p(yp), 0, 1, 0, ops._p(a), B, H, W, 0, ops._stream())
        gt = y_gt.detach()
        if gt.dtype not in (torch.float32, torch.float64):
            gt = gt.float()
        gt = gt.contiguous()
        g = torch.empty(B, H, W, dtype=torch.uint8, device=y_pr.device)
        _lib.call("cmu_plane_mask", ops._p(gt), int(gt.dtype == torch.float64), 2, 1, ops._p(g), B, H, W, 0, ops._stream())
        return _hausdorff_masks(a, g, modified=True, standard=False)[0]

    def forward(self, y_pr, y_gt):
        return self.per_image(y_pr, y_gt).mean()


class radius_arteries(Metric):
    """metrics.py:333-347: per image |mean radius of argmax(prediction) - mean radius of argmax(target)| (compute_radius_arteries:
    border cleared, skeleton-to-contour distances), batch value = fp64 mean over images.  Two-class (B,2,H,W) inputs."""
    __name__ = "radius_arteries"

    def per_image(self, y_pr, y_gt):
        """(B, 2, 3) fp64: the radius triples of prediction and target."""
        _check_two_class(y_pr, y_gt, "radius_arteries")
        B, _, H, W = y_pr.shape
        m = torch.empty(2 * B, H, W, dtype=torch.uint8, device=y_pr.device)
        for k, x in enumerate((y_pr.detach(), y_gt.detach())):
            if x.dtype not in (torch.float32, torch.float64):
                x = x.float()
            x = x.contiguous()
            _lib.call("cmu_argmax2_mask", ops._p(x), int(x.dtype == torch.float64), ops._p(m[k * B:]), B, H, W, 1, ops._stream())
        r = _radius_of_masks(m)
        return torch.stack((r[:B], r[B:]), 1)

    def forward(self, y_pr, y_gt):
        r = self.per_image(y_pr, y_gt)
        return (r[:, 0, 1] - r[:, 1, 1]).abs().mean()


class components(Metric):
    """The Betti-0 error (no reference counterpart): per image |components of argmax(prediction) - components of argmax(target)|,
    batch value = fp64 mean over images.  Two-class (B,2,H,W) inputs, binarised by cmu_argmax2_mask as ``radius_arteries`` does (the
    border is kept); labelled by cmu_label_components (csrc/components.hip) with ``connectivity`` 4 or 8.  No host sync."""
    __name__ = "components"

    def __init__(self, connectivity=8, **kwargs):
        super().__init__(**kwargs)
        if connectivity not in (4, 8):
            raise ValueError(f"components: connectivity must be 4 or 8, got {connectivity!r}")
        self.connectivity = connectivity

    def per_image(self, y_pr, y_gt):
        """(B, 2) int32: the component counts of prediction and target."""
        _check_two_class(y_pr, y_gt, "components")
        B, _, H, W = y_pr.shape
        m = torch.empty(2 * B, H, W, dtype=torch.uint8, device=y_pr.device)
        for k, x in enumerate((y_pr.detach(), y_gt.detach())):
            if x.dtype not in (torch.float32, torch.float64):
                x = x.float()
            x = x.contiguous()
            _lib.call("cmu_argmax2_mask", ops._p(x), int(x.dtype == torch.float64), ops._p(m[k * B:]), B, H, W, 0, ops._stream())
        counts = ops.label_components(m, -1, self.connectivity)[1]
        return torch.stack((counts[:B], counts[B:]), 1)

    def forward(self, y_pr, y_gt):
        c = self.per_image(y_pr, y_gt).double()
        return (c[:, 0] - c[:, 1]).abs().mean()


# ---------------------------------------------------------------------------------------------------
# surface-distance scores on the exact distance transform (csrc/edt.hip; no reference counterpart)
# ---------------------------------------------------------------------------------------------------
SurfaceDistances = collections.namedtuple(
    "SurfaceDistances", "hd hd_percentile assd nsd mean_pr_to_gt mean_gt_to_pr n_pr n_gt")


def _check_surface_cfg(what, tolerance, percentile):
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not math.isfinite(tolerance) or tolerance < 0:
        raise ValueError(f"{what}: tolerance must be a real number >= 0, got {tolerance!r}")
    if isinstance(percentile, bool) or not isinstance(percentile, (int, float)) or not 0 <= percentile <= 100:
        raise ValueError(f"{what}: percentile must lie in 0..100, got {percentile!r}")


def _surface_of_masks(a, b, tolerance, percentile):
    """a, b (B,H,W) uint8 -> SurfaceDistances of (B,) tensors.  Launches only: no host read."""
    tol2 = min(int(math.floor(float(tolerance) * float(tolerance))), 2 ** 31 - 1)
    g = torch.empty(a.shape, dtype=torch.int32, device=a.device)
    to_b = ops.edt_rows(ops.edt_columns(b, -1, True, g), "dist2")          # every pixel's squared distance to b's border
    sa, ca, ma = ops.surface_reduce(a, to_b, tol2)                         # ... gathered on a's border
    to_a = ops.edt_rows(ops.edt_columns(a, -1, True, g), "dist2", out=to_b)
    sb, cb, mb = ops.surface_reduce(b, to_a, tol2)
    n_a, n_b = ca[:, 0], cb[:, 0]
    na, nb = n_a.double(), n_b.double()
    n = na + nb
    both_empty, one_empty = n == 0, (n_a == 0) != (n_b == 0)
    zero, one, inf = torch.zeros_like(n), torch.ones_like(n), torch.full_like(n, float("inf"))

    def dist(x):      # a distance: 0 when both borders are empty, inf when exactly one is
        return torch.where(both_empty, zero, torch.where(one_empty, inf, x))

    mean_ab, mean_ba = sa[:, 0] / na, sb[:, 0] / nb
    hd = torch.maximum(sa[:, 1], sb[:, 1])
    # np.percentile(hstack(d_ab, d_ba), q), numpy's default 'linear' method: virtual index (n - 1) * q / 100 between two exact order statistics
    vi = (n - 1.0) * (float(percentile) / 100.0)
    lo = vi.floor()
    k0 = torch.minimum(lo.clamp_min(0.0), (n - 1.0).clamp_min(0.0))
    k1 = torch.minimum(k0 + 1.0, (n - 1.0).clamp_min(0.0))
    ranks = torch.where(both_empty.unsqueeze(1), torch.full_like(k0, -1.0).unsqueeze(1), torch.stack((k0, k1), 1)).to(torch.int32).contiguous()
    roots = ops.surface_select(ma, mb, ranks)[1]
    lo_v, hi_v, t = roots[:, 0], roots[:, 1], vi - lo
    diff = hi_v - lo_v
    pct = torch.where(t >= 0.5, hi_v - diff * (1.0 - t), lo_v + diff * t)
    nsd = torch.where(both_empty, one, (ca[:, 2] + cb[:, 2]).double() / n)      # (one border empty: nothing lies within: 0 / n)
    return SurfaceDistances(dist(hd), dist(pct), dist((mean_ab + mean_ba) / 2.0), nsd, dist(mean_ab), dist(mean_ba), n_a, n_b)


def surface_distances(pr_mask, gt_mask, tolerance=1.0, percentile=95.0):
    """Surface-distance scores of two device masks ((H,W) or (B,H,W), foreground = ``> 0``), per image, as fp64 tensors (0-dim for (H,W)
    inputs) in a ``SurfaceDistances`` tuple.  A mask's border is ``mask & ~binary_erosion(mask, cross, border_value=0)``: its pixels
    with a 4-neighbour that is background or outside the image (the rule of medpy and MONAI).  With d(A->B) the Euclidean distances
    from A's border pixels to the nearest border pixel of B:

      hd             max over both directions
      hd_percentile  ``np.percentile(hstack(d(A->B), d(B->A)), percentile)`` with numpy's default linear interpolation -- medpy's
                     ``hd95``: the percentile of the POOLED distances, NOT the max of the two directions' percentiles
      assd           (mean d(A->B) + mean d(B->A)) / 2; the two means are ``mean_pr_to_gt`` and ``mean_gt_to_pr``
      nsd            surface Dice at ``tolerance``: (#{d(A->B) <= tol} + #{d(B->A) <= tol}) / (n_A + n_B), compared exactly as
                     squared distance <= floor(tol^2)
      n_pr, n_gt     the border pixel counts (int32)

    Both borders empty: distances 0, nsd 1.  Exactly one empty: distances inf, nsd 0 (as ``hausdorff_distance_mask``).  Squared
    distances, counts and the two order statistics are exact integers; sums are fp64 in a fixed order.  1 <= H, W <= 4096."""
    _check_surface_cfg("surface_distances", tolerance, percentile)
    if not (torch.is_tensor(pr_mask) and torch.is_tensor(gt_mask) and pr_mask.is_cuda and gt_mask.is_cuda):
        raise RuntimeError("surface_distances runs on the GPU only; there is no CPU fallback in this package")
    a, batched = _as_masks(pr_mask)
    b, _ = _as_masks(gt_mask)
    if a.shape != b.shape:
        raise ValueError("both masks must have the same shape")
    ops._edt_check("surface_distances", a, torch.uint8)
    out = _surface_of_masks(a, b, tolerance, percentile)
    return out if batched else SurfaceDistances(*(v[0] for v in out))


def _surface_pair(y_pr, y_gt, threshold, what):
    """Two-class logits and a one-hot target, binarised as ``hausdorff`` does: softmax > threshold on channel 1, the target's channel 1."""
    _check_two_class(y_pr, y_gt, what)
    B, _, H, W = y_pr.shape
    yp = torch.empty(B, H, W, dtype=torch.float32, device=y_pr.device)
    ops.softmax2_threshold(y_pr.detach().float().contiguous(), threshold, yp)
    return _as_masks(yp)[0], _as_masks(y_gt.detach()[:, 1])[0]


class _SurfaceMetric(Metric):
    def __init__(self, threshold=0.5, tolerance=1.0, percentile=95.0, **kwargs):
        super().__init__(**kwargs)
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"{self.__name__}: threshold must lie inside (0, 1), got {threshold!r}")
        _check_surface_cfg(self.__name__, tolerance, percentile)
        self.threshold, self.tolerance, self.percentile = float(threshold), tolerance, percentile

    def per_image(self, y_pr, y_gt):
        """SurfaceDistances of (B,) tensors."""
        a, b = _surface_pair(y_pr, y_gt, self.threshold, self.__name__)
        ops._edt_check(self.__name__, a, torch.uint8)
        return _surface_of_masks(a, b, self.tolerance, self.percentile)


class HausdorffDistance95(_SurfaceMetric):
    """The ``percentile``-th (default 95) percentile Hausdorff distance of ``surface_distances`` (medpy's ``hd95``: pooled over both
    directions), fp64 mean over the batch (inf if any image is inf).  Two-class (B,2,H,W) logits and one-hot targets, as ``hausdorff``."""
    __name__ = "hd95"

    def __init__(self, percentile=95.0, **kwargs):
        super().__init__(percentile=percentile, **kwargs)

    def forward(self, y_pr, y_gt):
        return self.per_image(y_pr, y_gt).hd_percentile.mean()


class AverageSurfaceDistance(_SurfaceMetric):
    """The average symmetric surface distance of ``surface_distances``, fp64 mean over the batch."""
    __name__ = "assd"

    def forward(self, y_pr, y_gt):
        return self.per_image(y_pr, y_gt).assd.mean()


class SurfaceDice(_SurfaceMetric):
    """The surface Dice (normalised surface distance) at ``tolerance`` pixels of ``surface_distances``, fp64 mean over the batch."""
    __name__ = "surface_dice"

    def __init__(self, tolerance=1.0, **kwargs):
        super().__init__(tolerance=tolerance, **kwargs)

    def forward(self, y_pr, y_gt):
        return self.per_image(y_pr, y_gt).nsd.mean()


# ---------------------------------------------------------------------------------------------------
# the rest of the reference's loss surface (metrics.py:495-551): L1Loss, MSELoss, BCELoss, BCEWithLogitsLoss (one-channel binary
# heads) on cmu_pointwise_loss_fwd / _bwd; NLLLoss and RobustCrossEntropyLoss (class-index targets) on cmu_index_ce_fwd / _bwd
# (csrc/pointwise_loss.hip)
# ---------------------------------------------------------------------------------------------------
def _check_device(what, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")


def _check_reduction(what, reduction):
    if reduction == "none":
        raise NotImplementedError(f"{what}: reduction 'mean' / 'sum' on the HIP path (the kernels return sums, not per-element values)")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"{what}: {reduction!r} is not a valid value for reduction")
    return reduction


def _float_target(y):
    y = y.detach()
    return (y if y.dtype in (torch.float32, torch.float64) else y.double()).contiguous()


class _PointwiseSumFn(torch.autograd.Function):
    """S = sum_i w_c term_i as a 0-dim fp64 device tensor; the backward kernel reads its incoming gradient from the device."""

    @staticmethod
    def forward(ctx, x, y, kind, chan_w, chan_pw):
        xc = x.detach().contiguous()
        out = torch.empty(1, dtype=torch.float64, device=x.device)
        ws = ops.workspace("cmu_pointwise_loss_ws_bytes", x.device)
        ops.pointwise_loss_fwd(kind, xc, y, chan_w, chan_pw, out, ws)
        ctx.save_for_backward(xc, y, chan_w, chan_pw)
        ctx.kind = kind
        return out[0]

    @staticmethod
    def backward(ctx, g):
        xc, y, chan_w, chan_pw = ctx.saved_tensors
        dx = torch.empty_like(xc)
        ops.pointwise_loss_bwd(ctx.kind, xc, y, chan_w, chan_pw, g.reshape(1).contiguous(), dx)
        return dx, None, None, None, None


def _pointwise(what, kind, reduction, y_pr, y_gt, chan_w=None, chan_pw=None):
    _check_device(what, y_pr, y_gt)
    if y_pr.shape != y_gt.shape:
        raise ValueError(f"{what}: target size {tuple(y_gt.shape)} must be the same as input size {tuple(y_pr.shape)}")
    if y_pr.numel() == 0:
        raise ValueError(f"{what}: empty input")
    s = _PointwiseSumFn.apply(y_pr.float(), _float_target(y_gt), kind, chan_w, chan_pw)
    return s / float(y_pr.numel()) if reduction == "mean" else s


class L1Loss(Loss):
    """nn.L1Loss(reduction) (metrics.py:495) on two tensors of one shape; fp32 or fp64 targets."""

    def __init__(self, reduction="mean", **kwargs):
        super().__init__(**kwargs)
        self.reduction = _check_reduction("L1Loss", reduction)

    def forward(self, y_pr, y_gt):
        return _pointwise("L1Loss", "l1", self.reduction, y_pr, y_gt)


class MSELoss(Loss):
    """nn.MSELoss(reduction) (metrics.py:499)."""

    def __init__(self, reduction="mean", **kwargs):
        super().__init__(**kwargs)
        self.reduction = _check_reduction("MSELoss", reduction)

    def forward(self, y_pr, y_gt):
        return _pointwise("MSELoss", "mse", self.reduction, y_pr, y_gt)


def _channel_weight(what, name, w):
    """None, or the weight as an fp32 vector: one element (a factor on everything) or one per channel, from the shapes that
    broadcast per channel against (B,C,H,W) in torch: (C,1,1) and (1,C,1,1)."""
    if w is None:
        return None
    w = torch.as_tensor(w, dtype=torch.float32).detach().clone()
    per_channel = (w.dim() == 3 and w.shape[1:] == (1, 1)) or (w.dim() == 4 and w.shape[0] == 1 and w.shape[2:] == (1, 1))
    if w.numel() != 1 and not per_channel:
        raise NotImplementedError(f"{what}: {name} of shape {tuple(w.shape)}: one element, (C,1,1) or (1,C,1,1) on the HIP path")
    if w.numel() > ops.PWL_MAX_C:
        raise NotImplementedError(f"{what}: {name} over {w.numel()} channels (at most {ops.PWL_MAX_C})")
    return w.reshape(-1).contiguous()


class _ChannelWeighted(Loss):
    """Shared by the two BCE classes: the per-channel vectors the kernel takes, fitted to the input's channel count."""

    def _vectors(self, what, y_pr):
        for name in ("weight", "pos_weight"):               # moved to the input's device once, as CrossEntropyLoss._weight_on
            v = getattr(self, name, None)
            if v is not None and v.device != y_pr.device:
                setattr(self, name, v.to(y_pr.device))
        vs = [v for v in (self.weight, getattr(self, "pos_weight", None)) if v is not None]
        if not vs:
            return None, None
        C = max(v.numel() for v in vs)
        if C > 1 and (y_pr.dim() != 4 or y_pr.shape[1] != C):
            raise ValueError(f"{what}: weights over {C} channels against an input of shape {tuple(y_pr.shape)}")
        return tuple(None if v is None else (v if v.numel() == C else v.expand(C).contiguous()) for v in (self.weight, getattr(self, "pos_weight", None)))


class BCELoss(_ChannelWeighted):
    """nn.BCELoss(weight, reduction) (metrics.py:546) on probabilities: (B,C,H,W) with 1 <= C <= 8, or any shape without a
    per-channel weight.  A prediction outside [0, 1] gives NaN (torch raises; that would need a host sync)."""

    def __init__(self, weight=None, reduction="mean", **kwargs):
        super().__init__(**kwargs)
        self.register_buffer("weight", _channel_weight("BCELoss", "weight", weight))
        self.reduction = _check_reduction("BCELoss", reduction)

    def forward(self, y_pr, y_gt):
        _check_device("BCELoss", y_pr, y_gt)
        w, _ = self._vectors("BCELoss", y_pr)
        return _pointwise("BCELoss", "bce", self.reduction, y_pr, y_gt, w)


class BCEWithLogitsLoss(_ChannelWeighted):
    """nn.BCEWithLogitsLoss(weight, reduction, pos_weight) (metrics.py:550): the criterion of a one-channel binary head
    (UNet(out_classes=1)); finite for any logit."""

    def __init__(self, weight=None, reduction="mean", pos_weight=None, **kwargs):
        super().__init__(**kwargs)
        self.register_buffer("weight", _channel_weight("BCEWithLogitsLoss", "weight", weight))
        self.register_buffer("pos_weight", _channel_weight("BCEWithLogitsLoss", "pos_weight", pos_weight))
        self.reduction = _check_reduction("BCEWithLogitsLoss", reduction)

    def forward(self, y_pr, y_gt):
        _check_device("BCEWithLogitsLoss", y_pr, y_gt)
        w, pw = self._vectors("BCEWithLogitsLoss", y_pr)
        return _pointwise("BCEWithLogitsLoss", "bce_with_logits", self.reduction, y_pr, y_gt, w, pw)


class _IndexCEFn(torch.autograd.Function):
    """table = [sum w_t (-log p_t) | sum w_t | sum_kept w_c (-log p_c)] (3 fp64); the backward kernel takes the incoming gradients
    of table[0] and table[2] from the device (table[1] does not depend on the input)."""

    @staticmethod
    def forward(ctx, x, target, onehot, log_input, keep, class_w, ignore_index):
        xc = x.detach().contiguous()
        table = torch.empty(3, dtype=torch.float64, device=x.device)
        ws = ops.workspace("cmu_index_ce_ws_bytes", x.device)
        ops.index_ce_fwd(xc, target, onehot, log_input, keep, class_w, ignore_index, table, ws)
        ctx.save_for_backward(xc, target, class_w)
        ctx.cfg = (onehot, log_input, keep, ignore_index)
        return table

    @staticmethod
    def backward(ctx, g):
        xc, target, class_w = ctx.saved_tensors
        onehot, log_input, keep, ignore_index = ctx.cfg
        dx = torch.empty_like(xc)
        ops.index_ce_bwd(xc, target, onehot, log_input, keep, class_w, ignore_index, torch.stack((g[0], g[2])), dx)
        return dx, None, None, None, None, None, None


def _check_index_input(what, y_pr):
    if y_pr.dim() != 4 or not 2 <= y_pr.shape[1] <= ops.SEG_MAX_K:
        raise NotImplementedError(f"{what}: (B,K,H,W) input with 2 <= K <= {ops.SEG_MAX_K} (got shape {tuple(y_pr.shape)})")


class NLLLoss(Loss):
    """metrics.py:523-543: activation -> drop ``ignore_channels`` from prediction and target -> arg-max of the kept one-hot target
    channels -> nn.NLLLoss() (mean over pixels), as one pass: 'logsoftmax' (nn.LogSoftmax()'s implicit dim is 1 for a 4-D input,
    which is required here) takes the log-softmax over all K channels in the kernel, None / 'identity' reads log-probabilities.
    ``threshold`` is stored and unused, as in the reference."""

    def __init__(self, activation=None, ignore_channels=None, threshold=None, **kwargs):
        super().__init__(**kwargs)
        if activation not in (None, "identity", "logsoftmax"):
            raise NotImplementedError(f"NLLLoss: activation 'logsoftmax', 'identity' or None on the HIP path (got {activation!r})")
        _kept(ops.SEG_MAX_K, ignore_channels)
        self.activation, self.threshold = activation, threshold
        self.ignore_channels = None if ignore_channels is None else list(ignore_channels)

    def forward(self, y_pr, y_gt):
        _check_device("NLLLoss", y_pr, y_gt)
        _check_index_input("NLLLoss", y_pr)
        if y_gt.shape != y_pr.shape:
            raise NotImplementedError("NLLLoss: one-hot targets of the prediction's shape")
        keep = _kept(y_pr.shape[1], self.ignore_channels)
        y = y_gt.detach()
        y = (y if y.dtype in (torch.float32, torch.float64) else y.float()).contiguous()
        table = _IndexCEFn.apply(y_pr.float(), y, True, self.activation != "logsoftmax", keep, None, -100)
        return table[0] / float(y_pr.numel() // y_pr.shape[1])


class RobustCrossEntropyLoss(Loss):
    """metrics.py:511-521: nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing) on logits (B,K,H,W) against a label
    map (B,1,H,W) or (B,H,W) of int64 / int32 / uint8 / fp32 / fp64 (truncated as ``.long()`` does; other dtypes are converted).
    A Loss here (it composes with ``+``); the reference's is a bare nn.CrossEntropyLoss.  A label outside [0, K) that is not
    ``ignore_index`` makes the value NaN and gets a zero gradient (torch asserts on the device)."""

    def __init__(self, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0, **kwargs):
        super().__init__(**kwargs)
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).detach().clone().contiguous())
        if self.weight is not None and self.weight.dim() != 1:
            raise ValueError("RobustCrossEntropyLoss: weight is a vector of one value per class")
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"RobustCrossEntropyLoss: label_smoothing must be inside [0, 1], got {label_smoothing}")
        self.reduction = _check_reduction("RobustCrossEntropyLoss", reduction)
        self.ignore_index, self.label_smoothing = int(ignore_index), float(label_smoothing)

    def forward(self, y_pr, y_gt):
        _check_device("RobustCrossEntropyLoss", y_pr, y_gt)
        _check_index_input("RobustCrossEntropyLoss", y_pr)
        B, K, H, W = y_pr.shape
        if y_gt.dim() == 4 and y_gt.shape[1] == 1:
            y_gt = y_gt[:, 0]
        if y_gt.shape != (B, H, W):
            raise NotImplementedError(f"RobustCrossEntropyLoss: a label map (B,1,H,W) or (B,H,W) for input {tuple(y_pr.shape)}, got {tuple(y_gt.shape)}")
        if self.weight is not None and self.weight.shape[0] != K:
            raise ValueError(f"RobustCrossEntropyLoss: {self.weight.shape[0]} class weights for {K} classes")
        if self.weight is not None and self.weight.device != y_pr.device:
            self.weight = self.weight.to(y_pr.device)
        y = y_gt.detach()
        y = (y if y.dtype in ops.ICE_LABEL_KINDS else y.long()).contiguous()
        t = _IndexCEFn.apply(y_pr.float(), y, False, False, None, self.weight, self.ignore_index)
        e = self.label_smoothing
        if self.reduction == "mean":
            return t[0] / t[1] if e == 0.0 else (1.0 - e) * t[0] / t[1] + (e / K) * t[2] / t[1]
        return t[0] if e == 0.0 else (1.0 - e) * t[0] + (e / K) * t[2]


# ---------------------------------------------------------------------------------------------
# Losses for thin, rare foregrounds (no reference counterpart; csrc/map_loss.hip): focal and Tversky against
# class imbalance, the boundary and Hausdorff distance-transform losses on distance maps from the exact transform of csrc/edt.hip
# ---------------------------------------------------------------------------------------------
class _FocalFn(torch.autograd.Function):
    """table = [sum alpha_t (1 - p_t)^gamma (-log p_t) | sum alpha_t | pixels not ignored] (3 fp64); the backward kernel takes the
    incoming gradient of table[0] from the device (the other two do not depend on the input)."""

    @staticmethod
    def forward(ctx, x, target, onehot, class_w, gamma, ignore_index):
        xc = x.detach().contiguous()
        table = torch.empty(3, dtype=torch.float64, device=x.device)
        ops.focal_fwd(xc, target, onehot, class_w, gamma, ignore_index, table)
        ctx.save_for_backward(xc, target, class_w)
        ctx.cfg = (onehot, gamma, ignore_index)
        return table

    @staticmethod
    def backward(ctx, g):
        xc, target, class_w = ctx.saved_tensors
        onehot, gamma, ignore_index = ctx.cfg
        dx = torch.empty_like(xc)
        ops.focal_bwd(xc, target, onehot, class_w, gamma, ignore_index, g[0:1].contiguous(), dx)
        return dx, None, None, None, None, None


class FocalLoss(Loss):
    """Focal loss (Lin et al., 2017) on logits (B,K,H,W), 2 <= K <= 8: -alpha_t (1 - p_t)^gamma log p_t per pixel, against a label map
    ((B,H,W) or (B,1,H,W) of int64 / int32 / uint8 / fp32 / fp64, as ``RobustCrossEntropyLoss`` takes it) or one-hot planes of the
    logits' shape (fp32 / fp64; the arg-max over the channels is the label).  ``alpha``: one weight per class, or None.
    ``reduction``: 'mean' divides the sum by the number of pixels that are not ``ignore_index`` (the paper's and
    segmentation_models.pytorch's convention), 'weighted_mean' by the sum of their alpha_t (torch's weighted cross entropy), 'sum' by
    nothing.  With ``gamma=0`` the values are those of ``RobustCrossEntropyLoss(weight=alpha)``: its 'mean' is 'weighted_mean' here,
    and without ``alpha`` the two means coincide.  A label outside [0, K) that is not ``ignore_index`` makes the value NaN and gets
    a zero gradient."""

    def __init__(self, gamma=2.0, alpha=None, ignore_index=-100, reduction="mean", **kwargs):
        super().__init__(**kwargs)
        if not 0.0 <= float(gamma) <= 1e6:
            raise ValueError(f"FocalLoss: gamma must be a number >= 0, got {gamma}")
        self.register_buffer("alpha", None if alpha is None else torch.as_tensor(alpha, dtype=torch.float32).detach().clone().contiguous())
        if self.alpha is not None and self.alpha.dim() != 1:
            raise ValueError("FocalLoss: alpha is a vector of one value per class")
        if reduction == "none":
            raise NotImplementedError("FocalLoss: reduction 'mean' / 'weighted_mean' / 'sum' on the HIP path (the kernel returns sums)")
        if reduction not in ("mean", "weighted_mean", "sum"):
            raise ValueError(f"FocalLoss: {reduction!r} is not a valid value for reduction")
        self.gamma, self.ignore_index, self.reduction = float(gamma), int(ignore_index), reduction

    def forward(self, y_pr, y_gt):
        _check_device("FocalLoss", y_pr, y_gt)
        _check_index_input("FocalLoss", y_pr)
        B, K, H, W = y_pr.shape
        onehot = y_gt.shape == y_pr.shape
        if not onehot:
            if y_gt.dim() == 4 and y_gt.shape[1] == 1:
                y_gt = y_gt[:, 0]
            if y_gt.shape != (B, H, W):
                raise NotImplementedError(f"FocalLoss: a label map (B,1,H,W) / (B,H,W) or one-hot planes for input {tuple(y_pr.shape)}, got {tuple(y_gt.shape)}")
        if self.alpha is not None and self.alpha.shape[0] != K:
            raise ValueError(f"FocalLoss: {self.alpha.shape[0]} class weights for {K} classes")
        if self.alpha is not None and self.alpha.device != y_pr.device:
            self.alpha = self.alpha.to(y_pr.device)
        y = y_gt.detach()
        if onehot:
            y = (y if y.dtype in ops.ICE_ONEHOT_KINDS else y.float()).contiguous()
        else:
            y = (y if y.dtype in ops.ICE_LABEL_KINDS else y.long()).contiguous()
        t = _FocalFn.apply(y_pr.float(), y, onehot, self.alpha, self.gamma, self.ignore_index)
        return t[0] / t[2] if self.reduction == "mean" else t[0] / t[1] if self.reduction == "weighted_mean" else t[0]


class TverskyLoss(Loss):
    """(1 - TI)^gamma with the Tversky index TI = (tp + eps) / (tp + alpha fp + beta fn + eps) of the softmax probabilities over the
    kept channels pooled (Salehi et al., 2017; gamma != 1: the focal Tversky loss of Abraham & Khan, 2019).  It reads the pair's
    counter table (``seg_table``), so ``TverskyLoss() + CrossEntropyLoss()`` costs one pass.  ``threshold=None`` is differentiable;
    with a threshold the value is detached, as for ``DiceLoss``.  ``alpha = beta = 0.5`` is ``DiceLoss(beta=1)`` up to eps."""

    def __init__(self, alpha=0.5, beta=0.5, gamma=1.0, eps=1e-7, activation="softmax", ignore_channels=None, threshold=None, **kwargs):
        super().__init__(**kwargs)
        _check_seg_cfg("TverskyLoss", activation, threshold, ignore_channels, eps)
        if not (float(alpha) >= 0 and float(beta) >= 0 and float(gamma) > 0):
            raise ValueError(f"TverskyLoss: alpha, beta >= 0 and gamma > 0 (got alpha={alpha}, beta={beta}, gamma={gamma})")
        self.alpha, self.beta, self.gamma, self.eps = float(alpha), float(beta), float(gamma), float(eps)
        self.activation, self.threshold = activation, None if threshold is None else float(threshold)
        self.ignore_channels = None if ignore_channels is None else list(ignore_channels)
        self._reference_cfg = False          # a term of the K-class pass: a combined Loss that holds it never takes the two-class kernel

    def forward(self, y_pr, y_gt):
        tp, spr, sgt = _counters(seg_table(y_pr, y_gt, self.threshold, any_weight=True), self.threshold)
        v = 1.0 - tversky_from_counters(tp, spr, sgt, self.alpha, self.beta, self.eps, self.ignore_channels)
        if self.gamma != 1.0:
            v = v ** self.gamma
        return v if self.threshold is None else v.detach()


def _label_map(what, target, classes):
    """(uint8 label map (B,H,W), K) of a label map ((B,H,W) / (B,1,H,W), any integer or floating dtype; ``classes`` = K is required) or
    of one-hot planes (B,K,H,W) of a floating dtype, whose arg-max over the channels is the label, as the index CE takes it."""
    _check_device(what, target)
    t = target.detach()
    if t.dim() == 4 and t.is_floating_point() and t.shape[1] > 1:
        K = t.shape[1]
        if classes is not None and int(classes) != K:
            raise ValueError(f"{what}: classes={classes} against {K} one-hot planes")
        t = torch.argmax(t, dim=1)
    else:
        if t.dim() == 4 and t.shape[1] == 1:
            t = t[:, 0]
        if t.dim() != 3 or classes is None:
            raise ValueError(f"{what}: a label map (B,H,W) / (B,1,H,W) with classes=K, or one-hot planes (B,K,H,W); got {tuple(target.shape)}, classes={classes}")
        K = int(classes)
    if not 1 <= K <= 255:
        raise ValueError(f"{what}: 1 <= classes <= 255, got {K}")
    return t.to(torch.uint8).contiguous(), K


class _D2Scratch:
    """The int32 scratch of the transforms of one set: g (the column pass), and the squared distances to the set and to its complement."""

    def __init__(self, like):
        self.g, self.to, self.frm = (torch.empty(like.shape, dtype=torch.int32, device=like.device) for _ in range(3))

    def pair(self, src, cls_to, cls_from):
        ops.edt_rows(ops.edt_columns(src, cls_to, g=self.g), out=self.to)
        ops.edt_rows(ops.edt_columns(src, cls_from, g=self.g), out=self.frm)
        return self.to, self.frm


def _signed_maps(lab, K, keep):
    """(B,K,H,W) fp32: plane c of ``keep`` = the signed distance to the boundary of {lab == c}; the other planes are zero."""
    out = torch.zeros((lab.shape[0], K) + tuple(lab.shape[1:]), dtype=torch.float32, device=lab.device)
    s = _D2Scratch(lab)
    for c in keep:
        ops.distance_field(*s.pair(lab, c, -2 - c), out, c, "signed")
    return out


def signed_distance_maps(target, classes=None):
    """(B,K,H,W) fp32 signed distance maps of a target (Kervadec et al.'s ``one_hot2dist``): in plane c, a pixel outside class c
    holds its Euclidean distance to the class, a pixel inside 1 - its distance to the complement; an image in which the class is
    empty or full holds zeros.  ``target``: a label map (B,H,W) / (B,1,H,W) with ``classes`` = K, or one-hot planes (B,K,H,W) of a
    floating dtype (arg-max).  Two exact transforms (``ops.edt_columns`` + ``ops.edt_rows``) and one ``ops.distance_field`` per class;
    H, W <= 4096.  No gradient.  For a dataset whose targets do not change, compute once and pass as ``BoundaryLoss``'s ``maps``."""
    lab, K = _label_map("signed_distance_maps", target, classes)
    return _signed_maps(lab, K, range(K))


def _mask_sets(what, mask, classes):
    """-> (K, sets) with sets(c) = (uint8 map (B,H,W), site rule of class c's set, site rule of its complement): 0/1 uint8 planes
    (B,K,H,W) -- thresholded probabilities, each plane its own set -- or whatever ``_label_map`` takes."""
    if mask.dim() == 4 and mask.dtype == torch.uint8 and mask.shape[1] > 1:
        _check_device(what, mask)
        return mask.shape[1], lambda c: (mask[:, c].contiguous(), -1, 0)
    lab, K = _label_map(what, mask, classes)
    return K, lambda c: (lab, c, -2 - c)


def distance_fields(mask_a, mask_b=None, alpha=2.0, classes=None):
    """(B,K,H,W) fp32: per class the distance to the boundary of its set (to the set outside it, to its complement inside) to the
    power ``alpha`` -- MONAI's ``HausdorffDTLoss.distance_field`` raised -- of ``mask_a``, plus that of ``mask_b`` when given.  A mask:
    a label map with ``classes`` = K, one-hot planes of a floating dtype (arg-max), or 0/1 uint8 planes (B,K,H,W) such as thresholded
    probabilities (each plane its own set).  An image whose set is empty or full adds zeros.  No gradient; H, W <= 4096."""
    if not 0.0 < float(alpha) <= 16.0:
        raise ValueError(f"distance_fields: 0 < alpha <= 16, got {alpha!r}")
    K, sets_a = _mask_sets("distance_fields", mask_a, classes)
    sets_b = None
    if mask_b is not None:
        Kb, sets_b = _mask_sets("distance_fields", mask_b, classes)
        if Kb != K or mask_b.shape[0] != mask_a.shape[0] or mask_b.shape[-2:] != mask_a.shape[-2:]:
            raise ValueError(f"distance_fields: masks of {tuple(mask_a.shape)} and {tuple(mask_b.shape)} do not describe the same classes and pixels")
    B, (H, W) = mask_a.shape[0], mask_a.shape[-2:]
    out = torch.empty((B, K, H, W), dtype=torch.float32, device=mask_a.device)
    sa = sb = None
    for c in range(K):
        src, cls_to, cls_from = sets_a(c)
        sa = sa or _D2Scratch(src)
        pair_b = (None, None)
        if sets_b is not None:
            src_b, to_b, from_b = sets_b(c)
            sb = sb or _D2Scratch(src_b)
            pair_b = sb.pair(src_b, to_b, from_b)
        ops.distance_field(*sa.pair(src, cls_to, cls_from), out, c, "unsigned", alpha, *pair_b)
    return out


class _SoftmaxMapFn(torch.autograd.Function):
    """table (K fp64) = sum Wm_c p_c ('linear') or sum Wm_c (p_c - y_c)^2 ('squared') over the kept classes; the backward kernel takes
    the K incoming gradients from the device.  Wm and y carry no gradient."""

    @staticmethod
    def forward(ctx, logits, wmap, y, keep, kind):
        lg = logits.detach().contiguous()
        table = torch.empty(lg.shape[1], dtype=torch.float64, device=lg.device)
        ops.softmax_map_fwd(lg, wmap, y, keep, kind, table)
        ctx.save_for_backward(lg, wmap, y)
        ctx.cfg = (keep, kind)
        return table

    @staticmethod
    def backward(ctx, g):
        lg, wmap, y = ctx.saved_tensors
        dl = torch.empty_like(lg)
        ops.softmax_map_bwd(lg, wmap, y, ctx.cfg[0], ctx.cfg[1], g.contiguous(), dl)
        return dl, None, None, None, None


def _check_map_loss(what, activation, ignore_channels):
    if activation not in ("softmax", "softmax2d"):
        raise NotImplementedError(f"{what}: activation 'softmax' / 'softmax2d' only on the HIP path (got {activation!r})")
    _kept(ops.SEG_MAX_K, ignore_channels)


def _check_map_input(what, y_pr, y_gt):
    _check_device(what, y_pr, y_gt)
    _check_index_input(what, y_pr)
    if y_pr.shape[2] > ops.EDT_MAX_SIDE or y_pr.shape[3] > ops.EDT_MAX_SIDE:
        raise NotImplementedError(f"{what}: H, W <= {ops.EDT_MAX_SIDE} (the distance transform's limit), got {tuple(y_pr.shape)}")


class BoundaryLoss(Loss):
    """The boundary loss of Kervadec et al. (2019): the mean over B x kept classes x H x W of phi_c p_c, with p the softmax and phi_c
    the signed distance map of class c of the target (``signed_distance_maps``) -- ``einsum(pc, dc).mean()`` over the kept classes.
    The value can be NEGATIVE: phi is negative inside the target, and a perfect prediction sums it there.  ``forward(y_pr, y_gt)``
    builds phi from ``y_gt`` (one-hot planes of the logits' shape, or a label map); ``forward(y_pr, y_gt, maps)`` -- or ``maps=`` at
    construction -- takes a precomputed (B,K,H,W) fp32 map and does not look at ``y_gt``.  The maps carry no gradient."""

    def __init__(self, activation="softmax", ignore_channels=(0,), maps=None, **kwargs):
        super().__init__(**kwargs)
        _check_map_loss("BoundaryLoss", activation, ignore_channels)
        self.activation, self.maps = activation, maps
        self.ignore_channels = None if ignore_channels is None else list(ignore_channels)

    def forward(self, y_pr, y_gt=None, maps=None):
        maps = self.maps if maps is None else maps
        if y_gt is None and maps is None:
            raise ValueError("BoundaryLoss: a target or precomputed maps")
        _check_map_input("BoundaryLoss", y_pr, y_pr if maps is not None else y_gt)
        B, K, H, W = y_pr.shape
        keep = _kept(K, self.ignore_channels)
        if maps is None:
            lab, _ = _label_map("BoundaryLoss", y_gt, K)
            if lab.shape != (B, H, W):
                raise ValueError(f"BoundaryLoss: a target of {tuple(y_gt.shape)} for logits of {tuple(y_pr.shape)}")
            maps = _signed_maps(lab, K, keep)
        elif maps.shape != y_pr.shape or maps.dtype != torch.float32 or maps.device != y_pr.device:
            raise ValueError(f"BoundaryLoss: maps must be a float32 tensor of the logits' shape {tuple(y_pr.shape)} on their device")
        table = _SoftmaxMapFn.apply(y_pr.float(), maps.detach().contiguous(), None, keep, "linear")
        return table.sum() / float(B * len(keep) * H * W)


class HausdorffDTLoss(Loss):
    """The Hausdorff distance-transform loss of Karimi & Salcudean (2019) as MONAI's ``HausdorffDTLoss`` states it: per kept class the
    mean over B x H x W of (p_c - y_c)^2 (f_pred,c^alpha + f_target,c^alpha), averaged over the kept classes.  f is the distance to the
    boundary of a set (``distance_fields``): the target's class, and the DETACHED softmax probability thresholded at ``threshold``
    (``cmu_softmax_planes`` -> ``cmu_threshold_mask`` -> the exact transform, every step on the device).  The gradient reaches the
    logits through (p - y)^2 only.  ``y_gt``: one-hot planes of the logits' shape, fp32 / fp64."""

    def __init__(self, alpha=2.0, activation="softmax", ignore_channels=(0,), threshold=0.5, **kwargs):
        super().__init__(**kwargs)
        _check_map_loss("HausdorffDTLoss", activation, ignore_channels)
        if not 0.0 < float(alpha) <= 16.0:
            raise ValueError(f"HausdorffDTLoss: 0 < alpha <= 16, got {alpha}")
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"HausdorffDTLoss: threshold must be inside (0, 1), got {threshold}")
        self.alpha, self.threshold, self.activation = float(alpha), float(threshold), activation
        self.ignore_channels = None if ignore_channels is None else list(ignore_channels)

    def _fields(self, logits, lab, keep):
        """(B,K,H,W) fp32: f_pred^alpha + f_target^alpha on the kept planes, zero on the others."""
        B, K, H, W = logits.shape
        out = torch.zeros((B, K, H, W), dtype=torch.float32, device=logits.device)
        prob = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=logits.device)
        sp, st = _D2Scratch(lab), _D2Scratch(lab)
        for c in keep:
            ops.softmax_planes(logits, None, [c], None, prob, None)
            ops.threshold_mask(prob, self.threshold, out=mask)
            ops.distance_field(*sp.pair(mask, -1, 0), out, c, "unsigned", self.alpha, *st.pair(lab, c, -2 - c))
        return out

    def forward(self, y_pr, y_gt):
        _check_map_input("HausdorffDTLoss", y_pr, y_gt)
        if y_gt.shape != y_pr.shape:
            raise NotImplementedError("HausdorffDTLoss: one-hot targets of the prediction's shape")
        B, K, H, W = y_pr.shape
        keep = _kept(K, self.ignore_channels)
        y = _float_target(y_gt)
        lg = y_pr.float()
        fields = self._fields(lg.detach().contiguous(), _label_map("HausdorffDTLoss", y, K)[0], keep)
        table = _SoftmaxMapFn.apply(lg, fields, y, keep, "squared")
        return table.sum() / float(B * len(keep) * H * W)


# ---------------------------------------------------------------------------------------------
# The Lovasz-Softmax loss (no reference counterpart; csrc/lovasz.hip on the segmented key sort of csrc/key_sort.hip, DESIGN.md
# section 4.26)
# ---------------------------------------------------------------------------------------------
class _LovaszFn(torch.autograd.Function):
    """The loss as a 0-dim fp64 tensor.  Forward: keys -> sort -> Jaccard gradient, which leaves d loss / d p as a weight map; the
    backward is one call of the map-weighted softmax backward with the incoming gradient in each of its K slots."""

    @staticmethod
    def forward(ctx, x, target, onehot, keep, per_image, classes_all, ignore_index):
        xc = x.detach().contiguous()
        B, K, H, W = xc.shape
        sz = ops.lovasz_sizes(B, K, H, W, keep, per_image)
        keys = torch.empty((sz["rows"], sz["n"]), dtype=torch.int64, device=xc.device)
        counts = torch.empty(sz["counts"], dtype=torch.int64, device=xc.device)
        ops.lovasz_keys(xc, target, onehot, keep, per_image, ignore_index, keys, counts)
        ranked = ops.sort_u64(keys, scratch=keys)                 # (the unsorted keys are not needed again: they are the scratch)
        wmap = torch.empty_like(xc)
        out = torch.empty(sz["out"], dtype=torch.float64, device=xc.device)
        ops.lovasz_grad(ranked, counts, keep, per_image, classes_all, wmap, out)
        ctx.save_for_backward(xc, wmap)
        ctx.keep = keep
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        xc, wmap = ctx.saved_tensors
        dx = torch.empty_like(xc)
        ops.softmax_map_bwd(xc, wmap, None, ctx.keep, "linear", g.reshape(1).expand(xc.shape[1]).contiguous(), dx)
        return dx, None, None, None, None, None, None


class LovaszSoftmaxLoss(Loss):
    """Lovasz-Softmax (Berman et al., 2018), the convex surrogate of the Jaccard index, on logits (B,K,H,W), 2 <= K <= 8, against a
    label map ((B,H,W) or (B,1,H,W) of int64 / int32 / uint8 / fp32 / fp64, as ``FocalLoss`` takes it) or one-hot planes of the
    logits' shape (fp32 / fp64; the arg-max over the channels is the label, and nothing is ignored).  Per class c the errors
    1 - p_c on the class's pixels and p_c elsewhere are sorted in descending order (equal ones by pixel index) and weighted by the
    Jaccard index's gradient along that order.  ``classes``: 'present' averages over the classes that occur in the segment, 'all' over
    all classes, a list of class ids over that list.  ``per_image``: a segment is one image and the images' losses are averaged;
    else the whole batch is one segment.  Pixels labelled ``ignore_index`` take no part.  No class present, or every pixel
    ignored: 0 with a zero gradient.  A label outside [0, K) that is not ``ignore_index`` makes the value NaN and the gradient zero."""

    def __init__(self, classes="present", per_image=False, ignore_index=-100, activation="softmax", **kwargs):
        super().__init__(**kwargs)
        _check_map_loss("LovaszSoftmaxLoss", activation, None)
        if isinstance(classes, str):
            if classes not in ("present", "all"):
                raise ValueError(f"LovaszSoftmaxLoss: classes is 'present', 'all' or a list of class ids, got {classes!r}")
        else:
            classes = sorted(set(int(c) for c in classes))
            if not classes or classes[0] < 0 or classes[-1] >= ops.SEG_MAX_K:
                raise ValueError(f"LovaszSoftmaxLoss: class ids in 0..{ops.SEG_MAX_K - 1}, got {classes}")
        self.classes, self.per_image, self.ignore_index, self.activation = classes, bool(per_image), int(ignore_index), activation

    def forward(self, y_pr, y_gt):
        _check_device("LovaszSoftmaxLoss", y_pr, y_gt)
        _check_index_input("LovaszSoftmaxLoss", y_pr)
        B, K, H, W = y_pr.shape
        onehot = y_gt.shape == y_pr.shape
        if not onehot:
            if y_gt.dim() == 4 and y_gt.shape[1] == 1:
                y_gt = y_gt[:, 0]
            if y_gt.shape != (B, H, W):
                raise NotImplementedError(f"LovaszSoftmaxLoss: a label map (B,1,H,W) / (B,H,W) or one-hot planes for input {tuple(y_pr.shape)}, got {tuple(y_gt.shape)}")
        keep = list(range(K)) if isinstance(self.classes, str) else self.classes
        if keep[-1] >= K:
            raise ValueError(f"LovaszSoftmaxLoss: class {keep[-1]} of {K} classes")
        y = y_gt.detach()
        if onehot:
            y = (y if y.dtype in ops.ICE_ONEHOT_KINDS else y.float()).contiguous()
        else:
            y = (y if y.dtype in ops.ICE_LABEL_KINDS else y.long()).contiguous()
        return _LovaszFn.apply(y_pr.float(), y, onehot, keep, self.per_image, self.classes != "present", self.ignore_index)


# ---------------------------------------------------------------------------------------------
# Choosing the operating point: one histogram pass (csrc/prob_hist.hip), then every threshold j / bins at once (csrc/hist_curves.h)
# ---------------------------------------------------------------------------------------------
class ProbHistogram:
    """``counts`` (Bout,K,2,bins+1) int64: pixels by row (image or pool, class), ground truth and bin; ``conf`` (Bout,K,bins+1) uint64: the
    bin's sum of floor(p * 2**32); ``invalid`` (Bout,K) int32: probabilities that were NaN or outside [0, 1]; ``bins``."""

    def __init__(self, counts, conf, invalid, bins):
        self.counts, self.conf, self.invalid, self.bins = counts, conf, invalid, int(bins)

    def __iter__(self):
        return iter((self.counts, self.conf, self.invalid, self.bins))


_HIST_ACTIVATIONS = ("softmax", "softmax2d", "sigmoid", None)


def prob_histogram(y_pr, y_gt, bins=256, activation="softmax", pooled=True, out=None):
    """The probability histogram of a batch in ONE pass.  ``y_pr`` (B,K,H,W): logits with ``activation`` 'softmax' / 'softmax2d' (K >= 2;
    the probability bits ``DiceMetric(threshold=)`` compares) or 'sigmoid' (K = 1), probability planes with ``None`` (what
    ``UNet.predict_probs``, ``ops.softmax_planes`` or ``Segmenter.segment(prob_class=)`` give; a (B,H,W) tensor is one plane).  ``y_gt``:
    one-hot float32 / float64 planes of y_pr's shape (positive iff > 0.5) or a (B,H,W) uint8 label map (class c positive for plane c; one
    plane: label != 0).  ``bins``: a power of two in 2..1024; bin b holds (b-1)/bins < p <= b/bins, so the pixels above threshold j/bins
    are the bins above j.  ``pooled``: one row set for the batch, else one per image.  ``out``: a ProbHistogram to add into (a whole
    validation set, images of any sizes, pools without a host synchronisation)."""
    if activation not in _HIST_ACTIVATIONS:
        raise ValueError(f"prob_histogram: activation must be one of {_HIST_ACTIVATIONS}, got {activation!r}")
    bins = ops.check_bins("prob_histogram", bins)
    if not (torch.is_tensor(y_pr) and torch.is_tensor(y_gt)):
        raise ValueError("prob_histogram: y_pr and y_gt are tensors")
    if not y_pr.is_cuda or not y_gt.is_cuda:
        raise RuntimeError("prob_histogram: the HIP path needs CUDA/ROCm tensors (no CPU fallback)")
    if y_pr.dim() == 3 and activation is None:
        y_pr = y_pr[:, None]
        if y_gt.dim() == 3 and y_gt.dtype != torch.uint8:
            y_gt = y_gt[:, None]
    if y_pr.dim() != 4 or not 1 <= y_pr.shape[1] <= ops.HIST_MAX_K:
        raise ValueError(f"prob_histogram: y_pr must be (B,K,H,W) with 1 <= K <= {ops.HIST_MAX_K}, got {tuple(y_pr.shape)}")
    B, K, H, W = y_pr.shape
    if activation in ("softmax", "softmax2d") and K < 2:
        raise ValueError("prob_histogram: a softmax needs K >= 2 planes; a one-channel head takes activation='sigmoid'")
    if activation == "sigmoid" and K != 1:
        raise ValueError(f"prob_histogram: activation='sigmoid' is the one-channel head's; got K = {K}")
    if y_gt.dtype == torch.uint8:
        if tuple(y_gt.shape) != (B, H, W):
            raise ValueError(f"prob_histogram: a uint8 label map must be (B,H,W) = {(B, H, W)}, got {tuple(y_gt.shape)}")
    elif y_gt.dtype in (torch.float32, torch.float64):
        if tuple(y_gt.shape) != (B, K, H, W):
            raise ValueError(f"prob_histogram: one-hot targets must have y_pr's shape {(B, K, H, W)}, got {tuple(y_gt.shape)}")
    else:
        raise ValueError(f"prob_histogram: y_gt must be float32 / float64 one-hot planes or a uint8 label map, got {y_gt.dtype}")
    Bout = 1 if pooled else B
    if out is None:
        counts, conf, invalid = ops.hist_buffers(Bout, K, bins, y_pr.device)
        out = ProbHistogram(counts, conf, invalid, bins)
        accumulate = False
    else:
        if not isinstance(out, ProbHistogram) or out.bins != bins or tuple(out.counts.shape) != (Bout, K, 2, bins + 1):
            raise ValueError(f"prob_histogram: out must be a ProbHistogram of {bins} bins with counts {(Bout, K, 2, bins + 1)}")
        accumulate = True
    ops.prob_hist(y_pr.detach().float().contiguous(), y_gt.contiguous(), bins, activation is not None, out.counts, out.conf, out.invalid,
                  pooled=pooled, accumulate=accumulate)
    return out


class ThresholdSweep:
    """Device tensors of ``threshold_sweep``; the leading dimensions are the histogram's (Bout,K).  ``thresholds`` (bins+1,) float64 = j/bins;
    ``tp fp fn tn`` (...,bins+1) int64; ``dice iou precision recall specificity`` (...,bins+1) float64; ``auroc average_precision ece mce``
    (...) float64; ``best_j`` / ``best_value``: the argmax over j = 1..bins-1 of the selected score and its value."""


_CURVE_NAMES = ("dice", "iou", "precision", "recall", "specificity")


def _curves(hist, eps, beta, select):
    if not isinstance(hist, ProbHistogram):
        raise ValueError("expected the ProbHistogram prob_histogram returns")
    return ops.hist_curves(hist.counts, hist.conf, eps=eps, beta=beta, select=select)


def threshold_sweep(hist, eps=1e-7, beta=1.0, score="dice"):
    """Every threshold j / bins of the histogram at once (cmu_hist_curves): the exact confusion counts -- at threshold j/bins the integers
    ``DiceMetric(threshold=j/bins)`` / ``IoU`` count -- the reference's score formulas (metrics.py:135-198) with ``eps`` / ``beta``, and the
    threshold-free AUROC, average precision, expected / maximum calibration error.  The sweep describes the PROBABILITIES; a one-channel
    ``UNet.predict`` compares the logit with log(t / (1 - t)), which can differ from sigmoid > t at a probability on a bin edge."""
    if score not in ops.HIST_SELECT:
        raise ValueError(f"threshold_sweep: score must be one of {sorted(ops.HIST_SELECT)}, got {score!r}")
    cum, scores, summary = _curves(hist, eps, beta, ops.HIST_SELECT[score])
    s = ThresholdSweep()
    s.bins = hist.bins
    s.thresholds = torch.arange(hist.bins + 1, dtype=torch.float64, device=cum.device) / hist.bins
    s.tp, s.fp, s.fn, s.tn = cum.unbind(-2)
    for k, name in enumerate(_CURVE_NAMES):
        setattr(s, name, scores.select(-2, k))
    s.auroc, s.average_precision, s.ece, s.mce, s.best_j, s.best_value = summary.unbind(-1)
    return s


def best_threshold(hist, cls=1, score="dice", beta=1.0, eps=1e-7):
    """(threshold, value): the threshold j / bins, 1 <= j <= bins - 1, that maximises ``score`` ('dice': F-beta, 'iou', 'youden') of class
    ``cls`` on the pooled histogram (row 0), the first one on a tie, and that score -- 0-d float64 device tensors, no host synchronisation."""
    if score not in ops.HIST_SELECT:
        raise ValueError(f"best_threshold: score must be one of {sorted(ops.HIST_SELECT)}, got {score!r}")
    if not isinstance(hist, ProbHistogram) or not 0 <= int(cls) < hist.counts.shape[1]:
        raise ValueError(f"best_threshold: cls {cls!r} outside the histogram's classes")
    _, _, summary = ops.hist_curves(hist.counts[0, int(cls)].contiguous(), hist.conf[0, int(cls)].contiguous(), eps=eps, beta=beta,
                                    select=ops.HIST_SELECT[score])
    return summary[4] / hist.bins, summary[5]


class _HistMetric(Metric):
    """A threshold-free score of class ``cls`` from the batch's pooled probability histogram: a float64 device scalar."""
    _column = 0

    def __init__(self, cls=1, bins=256, activation="softmax", **kwargs):
        super().__init__(**kwargs)
        if activation not in _HIST_ACTIVATIONS:
            raise ValueError(f"{self.__name__}: activation must be one of {_HIST_ACTIVATIONS}, got {activation!r}")
        if isinstance(cls, bool) or int(cls) != cls or not 0 <= int(cls) < ops.HIST_MAX_K:
            raise ValueError(f"{self.__name__}: cls must lie in 0..{ops.HIST_MAX_K - 1}, got {cls!r}")
        self.cls, self.bins, self.activation = int(cls), ops.check_bins(self.__name__, bins), activation

    def forward(self, y_pr, y_gt):
        hist = prob_histogram(y_pr, y_gt, self.bins, self.activation)
        if self.cls >= hist.counts.shape[1]:
            raise ValueError(f"{self.__name__}: cls {self.cls} outside the {hist.counts.shape[1]} classes of the prediction")
        summary = ops.hist_curves(hist.counts[0, self.cls].contiguous(), hist.conf[0, self.cls].contiguous())[2]
        return summary[self._column]


class AUROC(_HistMetric):
    """Area under the ROC curve of class ``cls`` over the batch's pixels (sklearn's roc_auc_score on the bin indices); NaN when a class is empty."""
    __name__ = "auroc"
    _column = 0


class AveragePrecision(_HistMetric):
    """sklearn's average_precision_score of class ``cls`` on the bin indices; NaN without a positive pixel."""
    __name__ = "average_precision"
    _column = 1


class CalibrationError(_HistMetric):
    """Expected calibration error of class ``cls``: sum over the bins of |positives - sum of probabilities| / pixels."""
    __name__ = "ece"
    _column = 2
