"""CPU suite of the element-wise and class-index losses (L1Loss, MSELoss, BCELoss, BCEWithLogitsLoss, NLLLoss,
RobustCrossEntropyLoss of cmunet_amd/metrics.py): names, what the constructors accept and refuse, the C-ABI surface, and the float64
restatement tests/pointwise_loss_ref.py against torch.nn in float64 (values and autograd).  The kernels are pinned on the GPU in
tests/test_gpu_pointwise_losses_fp64.py."""
import itertools

import pytest
import torch
import torch.nn as nn

import pointwise_loss_ref as R

NEW = ("cmu_pointwise_loss_ws_bytes", "cmu_pointwise_loss_fwd", "cmu_pointwise_loss_bwd", "cmu_index_ce_ws_bytes", "cmu_index_ce_fwd",
       "cmu_index_ce_bwd")


def test_names_follow_the_snake_case_rule_and_compose():
    from cmunet_amd import metrics as M
    assert M.L1Loss().__name__ == "l1_loss"
    assert M.MSELoss().__name__ == "mse_loss"
    assert M.BCELoss().__name__ == "bce_loss"
    assert M.BCEWithLogitsLoss().__name__ == "bce_with_logits_loss"
    assert M.NLLLoss(activation="logsoftmax").__name__ == "nll_loss"
    assert M.RobustCrossEntropyLoss().__name__ == "robust_cross_entropy_loss"
    assert M.BCELoss(name="my_bce").__name__ == "my_bce"
    for cls in (M.L1Loss, M.MSELoss, M.BCELoss, M.BCEWithLogitsLoss, M.NLLLoss, M.RobustCrossEntropyLoss):
        assert issubclass(cls, M.Loss)
    dice = M.DiceLoss(activation="softmax", threshold=None)
    assert (dice + 0.5 * M.BCEWithLogitsLoss()).__name__ == "dice_loss + 0.5 * bce_with_logits_loss"
    assert (dice + M.NLLLoss(activation="logsoftmax")).__name__ == "dice_loss + nll_loss"
    assert (2 * (M.RobustCrossEntropyLoss() + M.L1Loss())).__name__ == "2 * (robust_cross_entropy_loss + l1_loss)"
    assert (M.MSELoss() + M.BCELoss()).__name__ == "mse_loss + bce_loss"


def test_constructors_keep_torchs_keywords():
    from cmunet_amd import metrics as M
    assert M.L1Loss(reduction="sum").reduction == "sum" and M.MSELoss().reduction == "mean"
    b = M.BCEWithLogitsLoss(weight=torch.tensor([[[2.0]], [[3.0]]]), pos_weight=torch.tensor([[[[0.5]], [[4.0]]]]), reduction="sum")
    assert b.weight.tolist() == [2.0, 3.0] and b.pos_weight.tolist() == [0.5, 4.0] and b.weight.dtype == torch.float32
    assert M.BCELoss(weight=torch.tensor(2.0, dtype=torch.float64)).weight.tolist() == [2.0]
    assert M.BCELoss(weight=torch.tensor([2.0])).weight.dtype == torch.float32
    n = M.NLLLoss(activation="logsoftmax", ignore_channels=[0], threshold=0.5)
    assert n.threshold == 0.5 and n.ignore_channels == [0]
    assert M.NLLLoss().activation is None and M.NLLLoss(activation="identity").activation == "identity"
    r = M.RobustCrossEntropyLoss(weight=[1.0, 2.0, 0.5], ignore_index=255, reduction="sum", label_smoothing=0.1)
    assert r.weight.tolist() == [1.0, 2.0, 0.5] and r.ignore_index == 255 and r.label_smoothing == 0.1 and r.reduction == "sum"
    assert M.RobustCrossEntropyLoss().ignore_index == -100


def test_constructors_refuse_what_the_kernels_do_not_cover():
    from cmunet_amd import metrics as M
    for cls in (M.L1Loss, M.MSELoss, M.BCELoss, M.BCEWithLogitsLoss, M.RobustCrossEntropyLoss):
        with pytest.raises(NotImplementedError):
            cls(reduction="none")
        with pytest.raises(ValueError):
            cls(reduction="average")
    for shape in ((3,), (2, 3), (3, 1), (1, 3, 1), (3, 4, 4), (2, 3, 1, 1), (1, 3, 2, 2)):
        with pytest.raises(NotImplementedError):
            M.BCELoss(weight=torch.ones(shape))
        with pytest.raises(NotImplementedError):
            M.BCEWithLogitsLoss(weight=torch.ones(shape))
        with pytest.raises(NotImplementedError):
            M.BCEWithLogitsLoss(pos_weight=torch.ones(shape))
    with pytest.raises(NotImplementedError):
        M.BCELoss(weight=torch.ones(9, 1, 1))
    for act in ("softmax", "softmax2d", "sigmoid", "tanh", torch.sigmoid):
        with pytest.raises(NotImplementedError):
            M.NLLLoss(activation=act)
    for ign in ([-1], [8], list(range(8))):
        with pytest.raises(ValueError):
            M.NLLLoss(activation="logsoftmax", ignore_channels=ign)
    with pytest.raises(ValueError):
        M.RobustCrossEntropyLoss(weight=[[1.0, 2.0]])
    for ls in (-0.1, 1.5):
        with pytest.raises(ValueError):
            M.RobustCrossEntropyLoss(label_smoothing=ls)


def test_existing_refusals_are_untouched():
    """The new classes are new names: the softmax-only constructors and the same-shape rule of CrossEntropyLoss stay as they were."""
    from cmunet_amd import metrics as M
    for cls in (M.DiceLoss, M.IoU, M.DiceMetric):
        with pytest.raises(NotImplementedError):
            cls(activation="sigmoid", threshold=0.5, ignore_channels=[0])
    with pytest.raises(NotImplementedError):
        M.soft_cldice(activation="sigmoid")


def test_cpu_tensors_are_refused():
    from cmunet_amd import metrics as M
    x, y = torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4, dtype=torch.float64)
    lab = torch.zeros(2, 4, 4, dtype=torch.int64)
    crit = M.DiceLoss(activation="softmax", threshold=None) + 0.5 * M.BCEWithLogitsLoss()
    for fn, tgt in ((M.L1Loss(), y), (M.MSELoss(), y), (M.BCELoss(), y), (M.BCEWithLogitsLoss(pos_weight=torch.ones(3, 1, 1)), y),
                    (M.NLLLoss(activation="logsoftmax"), y), (M.RobustCrossEntropyLoss(), lab), (crit, y)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, tgt)


def test_header_and_binding_hold_the_new_entry_points():
    import os
    import re
    from cmunet_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "cmunet_hip.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"(?:int64_t|int)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/cmunet_hip.h"
        args = m.group(1).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][1]) == n, name
    from cmunet_amd import ops
    for k, code in ops.PWL_KINDS.items():
        assert re.search(rf"#define CMU_PWL_{k.upper()} {code}\b", src), k
    assert re.search(rf"#define CMU_PWL_MAX_C {ops.PWL_MAX_C}\b", src)
    names = {torch.int64: "LABEL_I64", torch.int32: "LABEL_I32", torch.uint8: "LABEL_U8", torch.float32: "LABEL_F32", torch.float64: "LABEL_F64"}
    for dt, code in ops.ICE_LABEL_KINDS.items():
        assert re.search(rf"#define CMU_ICE_{names[dt]} {code}\b", src), dt
    assert re.search(rf"#define CMU_ICE_ONEHOT_F32 {ops.ICE_ONEHOT_KINDS[torch.float32]}\b", src)
    assert re.search(rf"#define CMU_ICE_ONEHOT_F64 {ops.ICE_ONEHOT_KINDS[torch.float64]}\b", src)


# ---------------------------------------------------------------------------------------------------
# tests/pointwise_loss_ref.py against torch.nn in float64
# ---------------------------------------------------------------------------------------------------
def pointwise_case(kind, C, ydt, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (2, C, 5, 7)
    if kind == "bce":
        x = torch.rand(shape, generator=g)
        y = torch.rand(shape, generator=g, dtype=ydt)
        x.view(-1)[:6] = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])            # the -100 clamp and the 1e-12 clamp
        y.view(-1)[:6] = torch.tensor([0.0, 1.0, 0.3, 0.0, 1.0, 0.3], dtype=ydt)
    elif kind == "bce_with_logits":
        x = torch.randn(shape, generator=g) * 3
        y = (torch.rand(shape, generator=g) > 0.5).to(ydt)
        y.view(-1)[10:20] = torch.rand(10, generator=g, dtype=ydt)
        x.view(-1)[:10] = torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0, 0.0, 30.0, -30.0, 100.0, -100.0])
        y.view(-1)[:10] = torch.tensor([0, 0, 0, 0, 0, 1, 1, 1, 1, 1], dtype=ydt)
    else:
        x = torch.randn(shape, generator=g)
        y = torch.randn(shape, generator=g, dtype=ydt)
        y.view(-1)[:5] = x.view(-1)[:5].to(ydt)                                   # exact ties
    return x, y


@pytest.mark.parametrize("kind,C,ydt", list(itertools.product(R.KINDS, (1, 3), (torch.float32, torch.float64))))
def test_pointwise_ref_is_torch_in_fp64(kind, C, ydt):
    x, y = pointwise_case(kind, C, ydt, 7 * C + len(kind))
    w = torch.tensor([0.5, 2.0, 1.25][:C]) if kind.startswith("bce") else None
    pw = torch.tensor([3.0, 0.25, 1.0][:C]) if kind == "bce_with_logits" else None
    g = 0.37
    r = R.pointwise_ref(kind, x, y, w, pw, g)
    xd = x.double().requires_grad_(True)
    wt = None if w is None else w.double().view(C, 1, 1)
    if kind == "l1":
        fn = nn.L1Loss(reduction="sum")
    elif kind == "mse":
        fn = nn.MSELoss(reduction="sum")
    elif kind == "bce":
        fn = nn.BCELoss(weight=wt, reduction="sum")
    else:
        fn = nn.BCEWithLogitsLoss(weight=wt, pos_weight=pw.double().view(C, 1, 1), reduction="sum")
    want = fn(xd, y.double())
    (g * want).backward()
    assert abs(float(r["S"]) - float(want)) <= 1e-12 * float(r["S_mag"])
    assert float(r["S_mag"]) >= abs(float(r["S"]))
    # torch's own forms cancel where the restatement's do not (sigmoid(x) - y at a saturated logit): its float64 roundoff at the
    # size of its operands, 2^-50 |g w| (1 + pw), is the tolerance next to 1e-12 of the magnitude
    scale = abs(g) * (1.0 if w is None else float(w.max())) * (1.0 + (1.0 if pw is None else float(pw.max())))
    err = (r["dx"] - xd.grad).abs()
    assert bool((err <= 1e-12 * r["dx_mag"] + 2.0 ** -50 * scale).all()), float((err - 1e-12 * r["dx_mag"]).max())
    assert bool((r["dx_mag"] >= r["dx"].abs() * (1 - 1e-12)).all())
    if kind == "l1":
        assert bool((r["dx"].view(-1)[:5] == 0).all()) and bool((r["dx_mag"].view(-1)[:5] == 0).all())
    if kind == "bce_with_logits":
        assert bool(torch.isfinite(r["dx"]).all()) and bool(torch.isfinite(r["S"]))
        # the table's forms, literally
        xx, yy = x.double(), y.double()
        c = 1 + (pw.double().view(1, C, 1, 1) - 1) * yy
        term = (1 - yy) * xx + c * (torch.log1p(torch.exp(-xx.abs())) + (-xx).clamp_min(0))
        assert abs(float((wt * term).sum()) - float(r["S"])) <= 1e-12 * float(r["S_mag"])
        dterm = (1 - yy) - c * torch.sigmoid(-xx)
        assert bool(((g * wt * dterm - r["dx"]).abs() <= 1e-12 * r["dx_mag"] + 2.0 ** -50 * scale).all())


def index_case(K, seed, ignore_frac=0.1):
    g = torch.Generator().manual_seed(seed)
    B, H, W = 2, 6, 5
    x = torch.randn(B, K, H, W, generator=g) * 2
    lab = torch.randint(0, K, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < ignore_frac] = -100
    return x, lab


@pytest.mark.parametrize("K,weighted,eps,reduction", list(itertools.product((2, 3, 8), (False, True), (0.0, 0.1), ("mean", "sum"))))
def test_index_ce_ref_is_torch_cross_entropy_in_fp64(K, weighted, eps, reduction):
    x, lab = index_case(K, 100 + K)
    w = torch.tensor([0.5, 2.0, 1.25, 0.75, 1.5, 1.0, 3.0, 0.25][:K]) if weighted else None
    xd = x.double().requires_grad_(True)
    want = nn.CrossEntropyLoss(weight=None if w is None else w.double(), ignore_index=-100, reduction=reduction, label_smoothing=eps)(xd, lab)
    (0.37 * want).backward()
    r0 = R.index_ce_ref(x, lab, w)
    T = r0["T"].clone().requires_grad_(True)
    v = R.reduce_ce(T, K, reduction, eps)
    assert abs(float(v) - float(want)) <= 1e-12 * float(R.reduce_ce(r0["T_mag"], K, reduction, eps))
    gT, = torch.autograd.grad(0.37 * v, T)
    r = R.index_ce_ref(x, lab, w, g0=float(gT[0]), g2=float(gT[2]))
    assert bool(((r["dx"] - xd.grad).abs() <= 1e-12 * r["dx_mag"]).all())
    assert bool((r["dx"][(lab == -100).unsqueeze(1).expand_as(x)] == 0).all())


def test_index_ce_ref_all_ignored_is_nan_as_in_torch():
    x, lab = index_case(3, 5)
    lab[:] = -100
    T = R.index_ce_ref(x, lab)["T"]
    assert float(T[1]) == 0 and torch.isnan(R.reduce_ce(T, 3, "mean", 0.0))
    assert torch.isnan(nn.CrossEntropyLoss()(x.double(), lab))


def test_index_ce_ref_out_of_range_label():
    x, lab = index_case(3, 6, ignore_frac=0.0)
    lab[1, 2, 3] = 3
    r = R.index_ce_ref(x, lab, torch.tensor([0.5, 2.0, 1.25]), g0=0.4, g2=0.1)
    assert torch.isnan(r["T"][0]) and bool(torch.isfinite(r["T"][1:]).all())
    assert bool((r["dx"][1, :, 2, 3] == 0).all()) and bool(torch.isfinite(r["dx"]).all())
    lab[1, 2, 3] = 0
    r2 = R.index_ce_ref(x, lab, torch.tensor([0.5, 2.0, 1.25]), g0=0.4, g2=0.1)
    mask = torch.ones_like(r["dx"], dtype=torch.bool)
    mask[1, :, 2, 3] = False
    assert torch.equal(r["dx"][mask], r2["dx"][mask])


@pytest.mark.parametrize("activation,ign", [("logsoftmax", None), ("logsoftmax", [0]), (None, [0]), ("identity", [1, 2])])
def test_index_ce_ref_is_the_reference_nll_loss(activation, ign):
    """metrics.py:523-543 restated with torch.nn: activation, drop the ignored channels of both tensors, arg-max of the kept target
    channels, nn.NLLLoss() -- including pixels whose kept target channels are all zero (arg-max 0: the first kept channel)."""
    K = 4
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, K, 6, 5, generator=g)
    x = x if activation == "logsoftmax" else torch.log_softmax(x * 2, 1)
    y = torch.nn.functional.one_hot(torch.randint(0, K, (2, 6, 5), generator=g), K).permute(0, 3, 1, 2).double()
    keep = [c for c in range(K) if c not in (ign or [])]
    xd = x.double().requires_grad_(True)
    pr = torch.log_softmax(xd, 1) if activation == "logsoftmax" else xd
    want = nn.NLLLoss()(pr[:, keep], torch.argmax(y[:, keep], dim=1))
    (0.37 * want).backward()
    lab = R.labels_of(y, True, keep)
    if ign:
        assert bool((y[:, keep].sum(1) == 0).any())
    npix = 2 * 6 * 5
    r = R.index_ce_ref(x, lab, None, -100, activation != "logsoftmax", keep, g0=0.37 / npix)
    assert abs(float(r["T"][0]) / npix - float(want)) <= 1e-12 * float(r["T_mag"][0]) / npix
    assert bool(((r["dx"] - xd.grad).abs() <= 1e-12 * r["dx_mag"]).all())
    if activation != "logsoftmax" and ign:
        assert bool((r["dx"][:, ign] == 0).all())


def test_labels_truncate_as_long_does():
    t = torch.tensor([[[0.0, 1.9, 2.0, -0.5, -100.0, 3.99]]])
    assert R.labels_of(t).tolist() == [[[0, 1, 2, 0, -100, 3]]]
    assert R.labels_of(t.double()).tolist() == t.long().tolist()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument checks return CMU_ERR_ARG (-1) with a message and touch neither the pointers nor a device."""
    import ctypes
    from cmunet_amd import _lib
    l = _lib.lib()
    p = ctypes.c_void_p(4096)                    # never dereferenced: every call below fails its checks first
    assert l.cmu_pointwise_loss_ws_bytes() == 1024 * 8 and l.cmu_index_ce_ws_bytes() == 3 * 1024 * 8
    assert l.cmu_pointwise_loss_fwd(0, p, p, 0, None, None, p, 2, 9, 16, p, None) == -1 and b"1 <= C <= 8" in l.cmu_last_error()
    assert l.cmu_pointwise_loss_fwd(0, p, p, 0, None, None, p, 2, 0, 16, p, None) == -1
    assert l.cmu_pointwise_loss_fwd(4, p, p, 0, None, None, p, 1, 1, 16, p, None) == -1 and b"unknown kind" in l.cmu_last_error()
    assert l.cmu_pointwise_loss_fwd(0, None, p, 0, None, None, p, 1, 1, 16, p, None) == -1
    assert l.cmu_pointwise_loss_bwd(2, p, p, 0, None, p, None, p, 2, 8, 18, None) == -1 and b"BCE_WITH_LOGITS only" in l.cmu_last_error()
    assert l.cmu_pointwise_loss_bwd(3, p, p, 0, None, p, None, None, 2, 8, 18, None) == -1
    for K in (1, 9):
        assert l.cmu_index_ce_fwd(p, p, 0, 0, 1, None, -100, p, 2, K, 4, 4, p, None) == -1 and b"2 <= K <= 8" in l.cmu_last_error()
    for mask in (0, 1 << 3, -1):
        assert l.cmu_index_ce_fwd(p, p, 0, 0, mask, None, -100, p, 2, 3, 4, 4, p, None) == -1 and b"keep_mask" in l.cmu_last_error()
    for kind in (-1, 7):
        assert l.cmu_index_ce_bwd(p, p, kind, 0, 7, None, -100, None, p, 2, 3, 4, 4, None) == -1 and b"unknown target kind" in l.cmu_last_error()
    assert l.cmu_index_ce_bwd(p, p, 0, 0, 7, None, -100, None, None, 2, 3, 4, 4, None) == -1
