"""HIP geometry metrics (csrc/geometry.hip, metrics.hausdorff / radius_arteries) against tests/golden/geometry_metrics.npz, which
the reference's own hausdorff_distance_mask / compute_radius_arteries and scikit-image wrote (tests/gen_geometry_metrics.py)."""
import math

import numpy as np
import pytest
import torch

import gen_geometry_metrics as GEN
import geometry_lattice as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return GEN.load(f"{golden_dir}/geometry_metrics.npz")


def _close(got, ref, rel=1e-9):
    got, ref = float(got), float(ref)
    if math.isnan(ref) or math.isinf(ref) or ref == 0.0:
        return (math.isnan(ref) and math.isnan(got)) or got == ref
    return abs(got - ref) <= rel * abs(ref)


def test_skeleton_counts_radius_per_mask(fix):
    from cmunet_amd import metrics as M
    for i, (m, sk) in enumerate(zip(fix["masks"], fix["skeletons"])):
        name = fix["names"][i]
        t = torch.from_numpy(m.astype(np.uint8)).cuda()
        got_sk = M.skeletonize(t).cpu().numpy().astype(bool)
        assert (got_sk == sk).all(), (name, int((got_sk != sk).sum()))
        cnt = M.contour_counts(t).cpu().numpy()
        assert (int(cnt[0]), int(cnt[1])) == (int(fix["n_cross"][i]), int(fix["n_closed"][i])), (name, cnt)
        rad = M.compute_radius_arteries(t).cpu().numpy()
        for g, r in zip(rad, fix["radius"][i]):
            assert _close(g, r), (name, rad, fix["radius"][i])
        assert t.cpu().numpy().astype(bool).tolist() == m.tolist()        # the input is left as it was


def test_hausdorff_per_pair_and_batched(fix):
    from cmunet_amd import metrics as M
    by_shape = {}
    for k, (p, g) in enumerate(fix["pairs"]):
        a = torch.from_numpy(fix["masks"][p].astype(np.float32)).cuda()
        b = torch.from_numpy(fix["masks"][g].astype(np.float32)).cuda()
        got_m = M.hausdorff_distance_mask(a, b)
        got_s = M.hausdorff_distance_mask(a, b, method="standard")
        assert got_m.dtype == torch.float64 and got_m.dim() == 0
        assert _close(got_m, fix["hausdorff"][k][0]), (fix["names"][p], float(got_m), fix["hausdorff"][k][0])
        assert _close(got_s, fix["hausdorff"][k][1]), (fix["names"][p], float(got_s), fix["hausdorff"][k][1])
        by_shape.setdefault(fix["masks"][p].shape, []).append(k)
    ks = by_shape[(256, 256)]
    assert len(ks) >= 2
    a = torch.stack([torch.from_numpy(fix["masks"][fix["pairs"][k][0]]) for k in ks]).cuda()
    b = torch.stack([torch.from_numpy(fix["masks"][fix["pairs"][k][1]]) for k in ks]).cuda()
    got = M.hausdorff_distance_mask(a, b).cpu().numpy()
    for g, k in zip(got, ks):
        assert _close(g, fix["hausdorff"][k][0])
    with pytest.raises(ValueError):
        M.hausdorff_distance_mask(a, b, method="lee")


def _logits_for(masks):
    """Two-channel logits whose softmax thresholds (and argmax) to ``masks``."""
    m = torch.from_numpy(np.stack(masks)).float()
    l1 = torch.where(m > 0, 1.5, -1.5)
    return torch.stack([-l1, l1], 1).contiguous()


def test_metric_classes_on_logits(fix):
    from cmunet_amd import metrics as M
    ks = [k for k, (p, g) in enumerate(fix["pairs"]) if fix["masks"][p].shape == (256, 256)]
    prs = [fix["masks"][fix["pairs"][k][0]] for k in ks]
    gts = [fix["masks"][fix["pairs"][k][1]] for k in ks]
    idx_p = [fix["pairs"][k][0] for k in ks]
    idx_g = [fix["pairs"][k][1] for k in ks]
    y_pr = _logits_for(prs).cuda()
    y_gt = torch.stack([torch.from_numpy(1.0 - np.stack(gts).astype(np.float64)), torch.from_numpy(np.stack(gts).astype(np.float64))], 1).cuda()
    h = M.hausdorff(threshold=0.5, activation="softmax", ignore_channels=[0])
    r = M.radius_arteries()
    assert h.__name__ == "hausdorff" and r.__name__ == "radius_arteries"
    hv = h(y_pr, y_gt)
    ref_h = float(np.mean([fix["hausdorff"][k][0] for k in ks]))
    assert hv.dtype == torch.float64 and _close(hv, ref_h), (float(hv), ref_h)
    rv = r(y_pr, y_gt)
    ref_r = float(np.mean([abs(fix["radius"][p][1] - fix["radius"][g][1]) for p, g in zip(idx_p, idx_g)]))
    assert rv.dtype == torch.float64 and _close(rv, ref_r), (float(rv), ref_r)
    # f32 one-hot targets take the same path
    assert _close(r(y_pr, y_gt.float()), ref_r)
    # one image with an empty prediction against a non-empty target: inf for that image -> the batch value is inf
    y_pr2 = y_pr.clone()
    y_pr2[0, 1] = -5.0
    y_pr2[0, 0] = 5.0
    assert math.isinf(float(h(y_pr2, y_gt)))
    # the driver's configuration only
    with pytest.raises(NotImplementedError):
        M.hausdorff(threshold=0.4, activation="softmax", ignore_channels=[0])


def test_metric_call_has_no_host_sync(fix):
    from cmunet_amd import metrics as M
    y_pr = _logits_for([fix["masks"][0], fix["masks"][1]]).cuda()
    y_gt = torch.stack([1.0 - y_pr[:, 1].gt(0).double(), y_pr[:, 1].gt(0).double()], 1).contiguous()
    h = M.hausdorff(threshold=0.5, activation="softmax", ignore_channels=[0])
    r = M.radius_arteries()
    h(y_pr, y_gt), r(y_pr, y_gt)          # warm-up (library load, allocator)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        hv, rv = h(y_pr, y_gt), r(y_pr, y_gt)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert math.isfinite(float(hv)) and math.isfinite(float(rv))


def test_size_limits_raise(fix):
    from cmunet_amd import metrics as M
    big = torch.zeros(600, 600, device="cuda")
    with pytest.raises(NotImplementedError, match="512"):
        M.hausdorff_distance_mask(big, big)
    with pytest.raises(NotImplementedError, match="512"):
        M.compute_radius_arteries(big)


def test_finetune_with_the_reference_six_metrics():
    """A small finetuning run (the synthetic setup of test_finetune_loop_vs_reference_loop_fixture) with the reference's full
    metric list (train.py:458-465): the log keys are those of the published pickles, the last batch's geometry values equal the CPU
    lattice restatement on the same predictions, and find_best_epochs returns both geometry keys."""
    from cmunet_amd import _lib, metrics as M, model as Mod, ops, train as T
    from oracle import unet as OU
    if not torch.cuda.is_available():
        pytest.skip("no GPU")

    class Rec:
        def __init__(self, metric):
            self.metric, self.last = metric, None

        def wrap(self):
            outer = self

            class _R(type(self.metric)):
                def forward(self, y_pr, y_gt):
                    v = super().forward(y_pr, y_gt)
                    outer.last = (y_pr.detach().clone(), y_gt.detach().clone(), v)
                    return v
            obj = _R.__new__(_R)
            obj.__dict__.update(self.metric.__dict__)
            return obj

    seed = 7
    train_loader, valid_loader = OU.finetune_fixture_data(seed + 1)
    net = Mod.UNet(dtype="f32")
    net.load_state_dict(OU.make_state_dict(base_ch=64, depth=5, seed=seed))
    mk = dict(activation="softmax", threshold=0.5, ignore_channels=[0])
    crit = M.DiceLoss(**mk) + M.CrossEntropyLoss()
    rh, rr = Rec(M.hausdorff(**mk)), Rec(M.radius_arteries())
    mets = [M.DiceLoss(**mk), M.CrossEntropyLoss(), M.IoU(**mk), rh.wrap(), rr.wrap(), M.soft_cldice(**mk)]
    opt = torch.optim.Adam([dict(params=net.parameters(), lr=1e-3)])
    tr = T.TrainEpoch(net, loss=crit, metrics=mets, optimizer=opt, device="cuda", verbose=False)
    va = T.ValidEpoch(net, loss=crit, metrics=mets, device="cuda", verbose=False)
    tl, vl = T.train(net, train_loader, valid_loader, tr, va, True, 2, name=None)
    keys = {"dice_loss + cross_entropy_loss", "dice_loss", "cross_entropy_loss", "iou_loss", "hausdorff", "radius_arteries", "soft_clDice"}
    for logs in tl + vl:
        assert set(logs) == keys, sorted(logs)
    # last batch (validation): the device values against the lattice restatement on the same predictions
    y_pr, y_gt, hv = rh.last
    B, _, H, W = y_pr.shape
    yp = torch.empty(B, H, W, dtype=torch.float32, device=y_pr.device)
    _lib.call("cmu_softmax2_threshold", ops._p(y_pr.float().contiguous()), 0.5, ops._p(yp), B, H, W, ops._stream())
    pr = yp.cpu().numpy() > 0
    gt = y_gt[:, 1].cpu().numpy() > 0
    ref = float(np.mean([L.hausdorff_distance_mask(pr[b], gt[b]) for b in range(B)]))
    assert _close(hv, ref), (float(hv), ref)
    y_pr, y_gt, rv = rr.last
    yn, gn = y_pr.cpu().numpy(), y_gt.cpu().numpy()
    prm, gtm = np.argmax(yn, axis=1).astype(bool), np.argmax(gn, axis=1).astype(bool)
    ref = float(np.mean([abs(L.compute_radius_arteries(prm[b])[1] - L.compute_radius_arteries(gtm[b])[1]) for b in range(B)]))
    assert _close(rv, ref), (float(rv), ref)
    best = T.find_best_epochs(vl, 2, 1e-3, 2, 0.0)
    assert "hausdorff" in best and "radius_arteries" in best
