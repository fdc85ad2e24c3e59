"""CPU suite of the focal, Tversky, boundary and Hausdorff-DT losses (cmunet_amd/metrics.py, csrc/map_loss.hip): the float64
restatement tests/map_loss_ref.py against torch autograd in float64 on hand-written expressions of the papers' formulas, its two
distance-field modes against scipy.ndimage.distance_transform_edt bit for bit, ``tversky_from_counters`` against the formula in
Python floats, and the argument checks of the new classes that need no GPU.  The kernels are pinned on the GPU in
tests/test_gpu_map_losses_fp64.py, which borrows the hand-written expressions below."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edt_cases
import edt_ref
import map_loss_ref as R

NEW = ("cmu_focal_fwd", "cmu_focal_bwd", "cmu_softmax_map_fwd", "cmu_softmax_map_bwd", "cmu_distance_field")


# ---------------------------------------------------------------------------------------------------
# the papers' formulas, hand-written in torch float64 / numpy + scipy
# ---------------------------------------------------------------------------------------------------
def hand_focal(x64, labels, alpha=None, gamma=2.0, ignore_index=-100, reduction="mean"):
    """-alpha_t (1 - p_t)^gamma log_softmax(x)_t over the pixels that are not ignored (Lin et al., eq. 5)."""
    K = x64.shape[1]
    live = labels != ignore_index
    t = labels.clamp(0, K - 1).unsqueeze(1)
    ls = torch.log_softmax(x64, 1).gather(1, t)[:, 0]
    a = torch.ones(K, dtype=torch.float64) if alpha is None else alpha.double()
    at = a[t[:, 0]]
    per = -at * (1 - ls.exp()) ** gamma * ls
    s = per[live].sum()
    return s / live.sum() if reduction == "mean" else s / at[live].sum() if reduction == "weighted_mean" else s


def hand_boundary(x64, phi, keep):
    """Kervadec et al.: ``einsum("bkwh,bkwh->bkwh", pc, dc).mean()`` over the kept classes."""
    pc, dc = torch.softmax(x64, 1)[:, keep], phi.double()[:, keep]
    return torch.einsum("bkwh,bkwh->bkwh", pc, dc).mean()


def hand_squared(x64, y, w, keep):
    """MONAI's HausdorffDTLoss: per class ((p - y)^2 * distance).mean(), averaged over the kept classes."""
    p = torch.softmax(x64, 1)
    return torch.stack([((p[:, c] - y.double()[:, c]) ** 2 * w.double()[:, c]).mean() for c in keep]).mean()


def hand_tversky(x64, y, alpha, beta, gamma, eps, keep):
    p, yy = torch.softmax(x64, 1)[:, keep], y.double()[:, keep]
    tp = (p * yy).sum()
    ti = (tp + eps) / (tp + alpha * (p.sum() - tp) + beta * (yy.sum() - tp) + eps)
    return (1 - ti) ** gamma


def kervadec_one_hot2dist(pos):
    """One class of one image (Kervadec et al., utils.one_hot2dist): zeros for an empty class, else
    ``distance(neg) * neg - (distance(pos) - 1) * pos``; float64."""
    from scipy.ndimage import distance_transform_edt as distance
    pos = np.asarray(pos, dtype=bool)
    if not pos.any():
        return np.zeros(pos.shape)
    neg = ~pos
    return distance(neg) * neg - (distance(pos) - 1) * pos


def monai_distance_field(fg):
    """One class of one image (MONAI, HausdorffDTLoss.distance_field): zeros for an empty mask, else edt(fg) + edt(bg); float64."""
    from scipy.ndimage import distance_transform_edt as edt
    fg = np.asarray(fg, dtype=bool)
    if not fg.any():
        return np.zeros(fg.shape)
    return edt(fg) + edt(~fg)


def scipy_signed_maps(lab, K, keep):
    """(B,K,H,W) float32 from a (B,H,W) integer label map: Kervadec's map on the kept planes (zeros where the class fills the image:
    this library's rule), zeros elsewhere."""
    lab = np.asarray(lab)
    out = np.zeros((lab.shape[0], K) + lab.shape[1:], np.float32)
    for b in range(lab.shape[0]):
        for c in keep:
            pos = lab[b] == c
            if pos.any() and not pos.all():
                out[b, c] = kervadec_one_hot2dist(pos).astype(np.float32)
    return torch.from_numpy(out)


def scipy_fields(mask, alpha):
    """(...,H,W) bool -> float32 MONAI field to the power alpha per leading index (zeros for an empty or a full mask)."""
    mask = np.asarray(mask, dtype=bool)
    out = np.zeros(mask.shape, np.float32)
    for idx in np.ndindex(*mask.shape[:-2]):
        if mask[idx].any() and not mask[idx].all():
            f = monai_distance_field(mask[idx])
            out[idx] = (f * f if alpha == 2 else f if alpha == 1 else f ** alpha).astype(np.float32)
    return torch.from_numpy(out)


def vessel_batch(K, B=2, H=24, W=40, seed=3):
    """(B,H,W) int64 labels with thin vessel-like classes 1..K-1 on background 0: every class present in every image, none full."""
    lab = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for c in range(1, K):
            m = edt_cases.vessel_like(H, W, strokes=2, steps=30, seed=seed + 17 * b + c)
            lab[b][m != 0] = c
        for c in range(K):
            lab[b, 1 + c, 2] = c                       # (a class a later stroke painted over keeps one pixel)
    return torch.from_numpy(lab)


# ---------------------------------------------------------------------------------------------------
# the restatement against autograd
# ---------------------------------------------------------------------------------------------------
def _case(K, seed=0, B=2, H=7, W=9):
    g = torch.Generator().manual_seed(100 * K + seed)
    x = (torch.randn(B, K, H, W, generator=g) * 2).float()
    lab = torch.randint(0, K, (B, H, W), generator=g)
    return x, lab, g


@pytest.mark.parametrize("K,gamma,weighted", [(2, 0.0, False), (3, 0.5, True), (3, 1.0, False), (5, 2.0, True), (8, 3.5, True)])
def test_focal_ref_against_autograd(K, gamma, weighted):
    x, lab, g = _case(K)
    lab[torch.rand(lab.shape, generator=g) < 0.1] = -100
    alpha = torch.tensor([0.5, 2.0, 1.25, 0.75, 1.5, 1.0, 3.0, 0.25][:K]) if weighted else None
    x64 = x.double().requires_grad_(True)
    want = hand_focal(x64, lab, alpha, gamma, -100, "sum")
    (0.37 * want).backward()
    want = want.detach()
    r = R.focal_ref(x, lab, alpha, gamma, -100, 0.37)
    assert abs(float(r["T"][0]) - float(want)) <= 1e-12 * float(r["T_mag"][0])
    assert float(r["T"][2]) == float((lab != -100).sum())
    a = torch.ones(K, dtype=torch.float64) if alpha is None else alpha.double()
    assert abs(float(r["T"][1]) - float(a[lab[lab != -100]].sum())) <= 1e-12 * float(r["T_mag"][1])
    assert bool(((r["dx"] - x64.grad).abs() <= 1e-11 * r["dx_mag"] + 1e-300).all())
    assert bool(((r["dx_mag"] - r["dx"].abs()).abs() <= 1e-15 * r["dx_mag"]).all())      # no cancellation: the magnitude is |dx| itself
    assert bool((r["dx"][(lab == -100).unsqueeze(1).expand_as(r["dx"])] == 0).all())
    for red in ("mean", "weighted_mean"):
        v = r["T"][0] / (r["T"][2] if red == "mean" else r["T"][1])
        assert abs(float(v) - float(hand_focal(x.double(), lab, alpha, gamma, -100, red))) <= 1e-12 * abs(float(v))


def test_focal_ref_at_saturated_logits_and_bad_labels():
    """Logits of +-100: q underflows (the label is the +100 class) or p_t does (the -100 class); nothing is inf * 0 or NaN.  With
    gamma = 0 the sums are the cross entropy's.  An out-of-range label: NaN sum, zero gradient, counted as not ignored."""
    x = torch.stack([torch.tensor([100.0, -100.0, 0.0]), torch.tensor([-100.0, 100.0, 0.0])]).view(1, 2, 1, 3)
    lab = torch.tensor([[[0, 0, 1]]])
    for gamma in (0.0, 0.5, 1.0, 2.0, 3.5):
        r = R.focal_ref(x, lab, None, gamma, -100, 1.0)
        assert bool(torch.isfinite(r["T"]).all()) and bool(torch.isfinite(r["dx"]).all()) and bool(torch.isfinite(r["lnq"]).all())
        assert abs(float(r["dx"][0, 0, 0, 1]) + 1.0) < 1e-12 and abs(float(r["dx"][0, 1, 0, 1]) - 1.0) < 1e-12      # p_t = e^-200: the CE's gradient
    ce = F.cross_entropy(x.double(), lab, reduction="sum")
    assert abs(float(R.focal_ref(x, lab, None, 0.0)["T"][0]) - float(ce)) <= 1e-12 * float(ce)
    bad = torch.tensor([[[0, 2, -100]]])
    r = R.focal_ref(x, bad, None, 2.0, -100, 1.0)
    assert bool(torch.isnan(r["T"][0])) and float(r["T"][2]) == 2.0 and float(r["T"][1]) == 1.0
    assert bool((r["dx"][0, :, 0, 1:] == 0).all()) and bool(torch.isfinite(r["dx"]).all())


@pytest.mark.parametrize("K,kind,keep", [(2, "linear", [1]), (3, "linear", None), (5, "linear", [1, 3, 4]), (2, "squared", [1]),
                                         (4, "squared", None), (8, "squared", [1, 2, 5, 7])])
def test_softmax_map_ref_against_autograd(K, kind, keep):
    x, lab, g = _case(K, seed=1)
    w = torch.randn(x.shape, generator=g).float() * 3                        # signed, as phi is
    y = F.one_hot(lab, K).permute(0, 3, 1, 2).double()
    kp = list(range(K)) if keep is None else keep
    gv = [0.1 * (c + 1) * (-1) ** c for c in range(K)]
    x64 = x.double().requires_grad_(True)
    p = torch.softmax(x64, 1)
    per = w.double() * (p if kind == "linear" else (p - y) ** 2)
    T = per.sum((0, 2, 3))
    sum(gv[c] * T[c] for c in kp).backward()
    r = R.softmax_map_ref(x, w, y, keep, kind, gv)
    for c in range(K):
        want = float(T[c].detach()) if c in kp else 0.0
        assert abs(float(r["T"][c]) - want) <= 1e-12 * float(r["T_mag"][c]) + 1e-300
    assert bool(((r["dx"] - x64.grad).abs() <= 1e-11 * r["dx_mag"] + 1e-300).all())
    # the losses on top of the sums: the einsum boundary loss, and MONAI's (p - y)^2 w
    N = x.shape[0] * len(kp) * x.shape[2] * x.shape[3]
    hand = hand_boundary(x.double(), w, kp) if kind == "linear" else hand_squared(x.double(), y, w, kp)
    assert abs(float(r["T"].sum() / N) - float(hand)) <= 1e-12 * float(r["T_mag"].sum() / N)
    # None stands for ones / zeros
    r1 = R.softmax_map_ref(x, None, y, keep, kind, None)
    assert bool((r1["dx"] == 0).all()) and abs(float(r1["T"].sum()) - float((per.detach() / w.double()).sum((0, 2, 3))[kp].sum())) < 1e-9


def test_squared_difference_keeps_its_bits_where_float64_softmax_saturates():
    """p_c - y_c as (1 - y) p_c - y sum of the others: at logits (30, 0) against y = (1, 0) the plain difference of float64
    probabilities has lost 1e-3 of its value, the restatement none."""
    x = torch.tensor([30.0, 0.0]).view(1, 2, 1, 1)
    y = torch.tensor([1.0, 0.0]).view(1, 2, 1, 1).double()
    r = R.softmax_map_ref(x, None, y, None, "squared", None)
    d = np.exp(-30.0) / (1 + np.exp(-30.0))
    assert abs(float(r["T"][0]) - d * d) <= 1e-14 * d * d and abs(float(r["T"][1]) - d * d) <= 1e-14 * d * d


# ---------------------------------------------------------------------------------------------------
# the distance fields against scipy, bit for bit
# ---------------------------------------------------------------------------------------------------
def field_masks():
    m = {}
    m["single_pixel"] = np.zeros((9, 13), bool)
    m["single_pixel"][4, 6] = True
    d = np.zeros((11, 11), bool)
    d[np.arange(11), np.arange(11)] = True
    m["diagonal_vessel"] = d
    f = np.zeros((8, 12), bool)
    f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = True
    f[3:5, 3:9] = True
    m["touches_all_borders"] = f
    m["vessel"] = edt_cases.vessel_like(24, 40, strokes=3, steps=40, seed=5) != 0
    m["all_but_one"] = ~m["single_pixel"]
    return m


@pytest.mark.parametrize("name", list(field_masks()))
def test_distance_field_refs_against_scipy(name):
    S = field_masks()[name]
    assert S.any() and not S.all()                                          # the only place scipy defines an answer
    d2_to, d2_from = edt_ref.dist2(S), edt_ref.dist2(~S)
    phi = R.signed_field_ref(d2_to, d2_from)
    assert phi.dtype == np.float32 and np.array_equal(phi, kervadec_one_hot2dist(S).astype(np.float32))
    assert (phi[S] <= 0).all() and (phi[~S] >= 1).all()
    mon = monai_distance_field(S)
    f1, _, d2 = R.unsigned_field_ref(d2_to, d2_from, 1)
    assert f1.dtype == np.float32 and np.array_equal(f1, mon.astype(np.float32))
    f2, _, _ = R.unsigned_field_ref(d2_to, d2_from, 2)
    assert np.array_equal(f2, d2.astype(np.float32)) and np.array_equal(d2, np.maximum(d2_to, d2_from))
    assert np.abs(f2.astype(np.float64) - mon ** 2).max() <= 1e-9 * (mon ** 2).max()      # (scipy's root squared again: not the integer)
    f25, exact, _ = R.unsigned_field_ref(d2_to, d2_from, 2.5)
    assert np.abs(exact - mon ** 2.5).max() <= 1e-12 * (mon ** 2.5).max() and np.array_equal(f25, exact.astype(np.float32))


def test_distance_field_refs_are_zero_for_an_empty_and_a_full_set():
    for S in (np.zeros((5, 7), bool), np.ones((5, 7), bool)):
        d2_to, d2_from = edt_ref.dist2(S), edt_ref.dist2(~S)
        assert (d2_to == -1).all() or (d2_from == -1).all()
        assert not R.signed_field_ref(d2_to, d2_from).any()
        for a in (1, 2, 2.5):
            assert not R.unsigned_field_ref(d2_to, d2_from, a)[0].any()
    assert not kervadec_one_hot2dist(np.zeros((5, 7), bool)).any() and not monai_distance_field(np.zeros((5, 7), bool)).any()


def test_vessel_batch_has_every_class_in_every_image():
    for K in (2, 3, 5):
        lab = vessel_batch(K)
        assert lab.shape == (2, 24, 40) and all(bool((lab[b] == c).any()) for b in range(2) for c in range(K))


# ---------------------------------------------------------------------------------------------------
# tversky_from_counters, names and argument checks
# ---------------------------------------------------------------------------------------------------
def test_tversky_from_counters_against_the_formula():
    from cmunet_amd import metrics as M
    tp, spr, sgt = [3.0, 10.5, 0.25], [4.0, 12.0, 2.0], [5.5, 11.0, 0.5]
    T = [torch.tensor(v, dtype=torch.float64) for v in (tp, spr, sgt)]
    for alpha, beta, eps, ign in ((0.5, 0.5, 1e-7, None), (0.3, 0.7, 1e-5, [0]), (0.7, 0.3, 1.0, [0, 2]), (1.0, 0.0, 1e-7, [1])):
        keep = [c for c in range(3) if c not in (ign or [])]
        t, s, gs = (sum(v[c] for c in keep) for v in (tp, spr, sgt))
        want = (t + eps) / (t + alpha * (s - t) + beta * (gs - t) + eps)
        got = float(M.tversky_from_counters(*T, alpha=alpha, beta=beta, eps=eps, ignore_channels=ign))
        assert abs(got - want) <= 4e-16 * want and abs(R.tversky_ref(tp, spr, sgt, alpha, beta, eps, ign) - want) <= 4e-16 * want
    # alpha = beta = 0.5 is the Dice score with the eps of numerator and denominator halved
    dice = float(M.f_score_from_counters(*T, beta=1.0, eps=2e-7))
    assert abs(float(M.tversky_from_counters(*T, eps=1e-7)) - dice) <= 4e-16
    # differentiable in tp and spr
    tpg = T[0].clone().requires_grad_(True)
    M.tversky_from_counters(tpg, T[1], T[2]).backward()
    assert bool((tpg.grad > 0).all())


def test_names_compose_and_the_abi_declares_the_entries():
    from cmunet_amd import _lib, metrics as M, ops
    assert M.FocalLoss().__name__ == "focal_loss" and M.TverskyLoss().__name__ == "tversky_loss"
    assert M.BoundaryLoss().__name__ == "boundary_loss" and M.HausdorffDTLoss().__name__ == "hausdorff_dt_loss"
    for cls in (M.FocalLoss, M.TverskyLoss, M.BoundaryLoss, M.HausdorffDTLoss):
        assert issubclass(cls, M.Loss)
    crit = M.DiceLoss(activation="softmax") + 0.5 * M.FocalLoss() + 0.01 * M.BoundaryLoss()
    assert crit.__name__ == "dice_loss + 0.5 * focal_loss + 0.01 * boundary_loss"
    assert all(n in _lib.EXPORTS for n in NEW) and not any(n.endswith("_ws_bytes") for n in NEW)
    assert ops.MAP_KINDS == {"linear": 0, "squared": 1} and ops.FIELD_MODES == {"signed": 0, "unsigned": 1} and ops.MAP_LOSS_MAX_BLOCKS == 1024
    D = __import__("ctypes").c_double
    assert _lib._SIGS["cmu_focal_fwd"][1][4] is D and _lib._SIGS["cmu_distance_field"][1][5] is D


def test_constructors_keep_their_configuration_and_refuse_the_rest():
    from cmunet_amd import metrics as M
    f = M.FocalLoss(gamma=1.5, alpha=[0.25, 0.75], ignore_index=255, reduction="weighted_mean")
    assert f.gamma == 1.5 and f.alpha.tolist() == [0.25, 0.75] and f.alpha.dtype == torch.float32 and f.ignore_index == 255
    assert M.FocalLoss().gamma == 2.0 and M.FocalLoss().reduction == "mean" and M.FocalLoss().alpha is None
    with pytest.raises(NotImplementedError):
        M.FocalLoss(reduction="none")
    for bad in (dict(reduction="average"), dict(gamma=-1.0), dict(alpha=[[0.5, 0.5]])):
        with pytest.raises(ValueError):
            M.FocalLoss(**bad)
    t = M.TverskyLoss(alpha=0.3, beta=0.7, gamma=0.75, ignore_channels=[0])
    assert (t.alpha, t.beta, t.gamma, t.eps, t.threshold, t.ignore_channels) == (0.3, 0.7, 0.75, 1e-7, None, [0])
    for bad in (dict(alpha=-0.1), dict(gamma=0.0), dict(eps=0.0), dict(threshold=1.0), dict(ignore_channels=[9])):
        with pytest.raises(ValueError):
            M.TverskyLoss(**bad)
    b, h = M.BoundaryLoss(), M.HausdorffDTLoss()
    assert b.ignore_channels == [0] and b.maps is None and h.ignore_channels == [0] and (h.alpha, h.threshold) == (2.0, 0.5)
    for cls in (M.TverskyLoss, M.BoundaryLoss, M.HausdorffDTLoss):
        assert cls(activation="softmax2d").activation == "softmax2d"
        for act in (None, "sigmoid", "identity"):
            with pytest.raises(NotImplementedError):
                cls(activation=act)
    for bad in (dict(alpha=0.0), dict(alpha=17.0), dict(threshold=0.0), dict(ignore_channels=[-1])):
        with pytest.raises(ValueError):
            M.HausdorffDTLoss(**bad)


def test_new_losses_refuse_cpu_tensors_and_unsupported_shapes():
    from cmunet_amd import metrics as M
    x, y = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4)
    for crit in (M.FocalLoss(), M.TverskyLoss(), M.BoundaryLoss(), M.HausdorffDTLoss()):
        with pytest.raises(RuntimeError, match="GPU|CUDA"):
            crit(x, y)
    for fn in (M.signed_distance_maps, M.distance_fields):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(y)
    with pytest.raises(ValueError):
        M.distance_fields(y, alpha=0.0)
