"""The finetuning training augmentation on the GPU (csrc/ft_augment.hip, cmunet_amd/ft_augment.py) against the numpy restatement
(tests/ft_augment_restate.py), the sampler's laws, determinism, the no-host-sync rule, the albumentations protocol and a short
main_finetuning run through device_finetune_loaders."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ft_augment_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 475


def _data(B, H=480, W=482, seed=0):
    rng = np.random.RandomState(seed)
    img = rng.uniform(-0.2, 1.2, (B, H, W)).astype(np.float32)
    mask = (rng.uniform(size=(B, H, W)) < 0.2).astype(np.uint8)
    return img, mask


def _recs(B, ops, H=480, W=482, seed=1, **fields):
    from cmunet_amd import ft_augment as FA
    rng = np.random.RandomState(seed)
    r = np.zeros(B, FA.REC_DTYPE)
    r["ops"] = ops
    r["y0"] = rng.randint(0, H - S + 1, B)
    r["x0"] = rng.randint(0, W - S + 1, B)
    r["ksize"] = rng.choice([5, 7, 9, 11], B)
    r["sigma"] = rng.uniform(0.5, 1.0, B)
    r["var_noise"] = rng.uniform(10, 50, B)
    r["var_oneof"] = rng.uniform(10, 50, B)
    r["alpha"] = 1 + rng.uniform(-0.2, 0.2, B)
    r["beta"] = rng.uniform(-0.25, 0.25, B)
    r["scale"] = rng.uniform(0.5, 1.0, B)
    r["oneof"] = rng.randint(0, 4, B)
    r["rot_k"] = rng.randint(0, 4, B)
    for k, v in fields.items():
        r[k] = v
    return r


def _aug(**cfg):
    from cmunet_amd import ft_augment as FA
    return FA.DeviceTrainingAugmentation(FA.FinetuneAugmentConfig(**cfg), seed=5)


def _ulp(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


def _run_only(ops, n=3, clip=True, **fields):
    img, mask = _data(n)
    recs = _recs(n, ops, **fields)
    noise = np.random.RandomState(9).standard_normal((2, n, S, S))
    a, m = _aug(clip_float=clip).augment_only(torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV), records=recs,
                                              noise=torch.from_numpy(noise))
    ra, rm = R.augment_batch(img, mask, recs, noise, S, clip)
    return a.cpu().numpy(), m.cpu().numpy(), ra, rm


@pytest.mark.parametrize("case", ["crop", "hflip", "vflip", "rot90", "downscale", "noise", "noise_noclip", "oneof_noise"])
def test_each_exact_transform_alone_is_bit_exact(case):
    ops, fields, clip = {"crop": (0, {}, True), "hflip": (R.OP_ONEOF, {"oneof": 0}, True), "vflip": (R.OP_ONEOF, {"oneof": 1}, True),
                         "rot90": (R.OP_ONEOF, {"oneof": 2, "rot_k": [1, 2, 3]}, True), "downscale": (R.OP_DOWN, {}, True),
                         "noise": (R.OP_NOISE, {}, True), "noise_noclip": (R.OP_NOISE, {}, False),
                         "oneof_noise": (R.OP_ONEOF, {"oneof": 3}, True)}[case]
    a, m, ra, rm = _run_only(ops, clip=clip, **fields)
    assert np.array_equal(a.view(np.int32), ra.view(np.int32)), case
    assert np.array_equal(m, rm), case


def test_brightness_and_blur_alone_within_bound():
    """Stated bounds: brightness / contrast 0 ulp (float32 restated operation for operation); blur <= 1 ulp (float64 taps in the same
    order; the weights' exp may differ from numpy's in the last bit)."""
    a, m, ra, rm = _run_only(R.OP_BC)
    assert _ulp(a, ra) == 0 and np.array_equal(m, rm)
    a, m, ra, rm = _run_only(R.OP_BC, clip=False)
    assert _ulp(a, ra) == 0
    a, m, ra, rm = _run_only(R.OP_BLUR, n=4, ksize=[5, 7, 9, 11])
    assert _ulp(a, ra) <= 1 and np.array_equal(m, rm)


@pytest.mark.parametrize("oneof", [0, 2, 3])
def test_full_chain_matches_restatement_then_segmentation_batch(oneof):
    from cmunet_amd.dataset import DeviceSegmentationBatch
    B = 3
    img, mask = _data(B, seed=oneof)
    recs = _recs(B, R.OP_NOISE | R.OP_BLUR | R.OP_BC | R.OP_DOWN | R.OP_ONEOF, seed=oneof + 2, oneof=oneof, rot_k=[1, 2, 3])
    noise = np.random.RandomState(4).standard_normal((2, B, S, S))
    aug = _aug(clip_float=False)          # (with the clip, the noise saturates the image to {0, 1}: a weaker check)
    gi, go = aug(torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV), records=recs, noise=torch.from_numpy(noise))
    ra, rm = R.augment_batch(img, mask, recs, noise, S, clip=False)
    ri, ro = DeviceSegmentationBatch(256, [0, 1])(torch.from_numpy(ra).to(DEV), torch.from_numpy(rm).to(DEV))
    assert gi.shape == (B, 256, 256) and gi.dtype == torch.float32 and go.shape == (B, 2, 256, 256) and go.dtype == torch.float64
    assert torch.equal(go, ro)
    assert torch.equal(gi.view(torch.int32), ri.view(torch.int32))
    # and the fused resize equals the resize of the device's own pre-resize output, bit for bit
    da, dm = aug.augment_only(torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV), records=recs, noise=torch.from_numpy(noise))
    di, do = DeviceSegmentationBatch(256, [0, 1])(da, dm)
    assert torch.equal(gi.view(torch.int32), di.view(torch.int32)) and torch.equal(go, do)


def test_image_and_mask_follow_the_same_geometry():
    B = 8
    _, mask = _data(B, seed=7)
    recs = _recs(B, R.OP_ONEOF, oneof=[0, 1, 2, 2, 2, 2, 3, 0], rot_k=[0, 0, 0, 1, 2, 3, 0, 0])
    recs["ops"][7] = 0
    a, m = _aug().augment_only(torch.from_numpy(mask.astype(np.float32)).to(DEV), torch.from_numpy(mask).to(DEV), records=recs,
                               noise=torch.zeros(2, B, S, S, dtype=torch.float64))
    assert torch.equal(a, m.float())
    assert not torch.equal(m[0], m[1])


def test_sampler_laws():
    from cmunet_amd import ft_augment as FA
    n = 24000
    aug = FA.DeviceTrainingAugmentation(FA.FinetuneAugmentConfig(), seed=11)
    aug.sample(n, 480, 481)
    r = aug.records()
    ops = r["ops"]

    def binom(k, p):
        return abs(k - n * p) <= 5 * np.sqrt(n * p * (1 - p))
    for bit, p in ((R.OP_NOISE, 0.1), (R.OP_BLUR, 0.2), (R.OP_BC, 0.15), (R.OP_DOWN, 0.25), (R.OP_ONEOF, 0.75)):
        assert binom(int((ops & bit).astype(bool).sum()), p), (bit, int((ops & bit).astype(bool).sum()))
    for c in range(4):
        assert binom(int((r["oneof"] == c).sum()), 0.25) and binom(int((r["rot_k"] == c).sum()), 0.25)
    assert set(np.unique(r["ksize"])) == {5, 7, 9, 11}
    for k, p in ((5, 1 / 7), (7, 2 / 7), (9, 2 / 7), (11, 2 / 7)):
        assert binom(int((r["ksize"] == k).sum()), p), k

    def uniform(x, lo, hi):
        assert x.min() >= lo and x.max() < hi
        assert abs(x.mean() - (lo + hi) / 2) <= 5 * (hi - lo) / np.sqrt(12 * n)
    uniform(r["sigma"], 0.5, 1.0)
    uniform(r["var_noise"], 10, 50)
    uniform(r["var_oneof"], 10, 50)
    uniform(r["alpha"], 0.8, 1.2)
    uniform(r["beta"], -0.25, 0.25)
    uniform(r["scale"], 0.5, 1.0)
    for c in range(6):
        assert binom(int((r["y0"] == c).sum()), 1 / 6)
    for c in range(7):
        assert binom(int((r["x0"] == c).sum()), 1 / 7)
    aug.sample(64, 475, 475)
    r = aug.records()
    assert (r["y0"] == 0).all() and (r["x0"] == 0).all()


def test_device_noise_moments_and_clip():
    from cmunet_amd import ft_augment as FA
    B = 2
    x = torch.full((B, S, S), 0.5, dtype=torch.float32, device=DEV)
    m = torch.zeros(B, S, S, dtype=torch.uint8, device=DEV)
    for ops, field, var in ((R.OP_NOISE, "var_noise", 25.0), (R.OP_ONEOF, "var_oneof", 16.0)):
        recs = _recs(B, ops, H=S, W=S, oneof=3, **{field: var})
        a, _ = _aug(clip_float=False).augment_only(x, m, records=recs)
        d = (a.double() - 0.5).cpu().numpy()
        n = d.size
        assert abs(d.mean()) <= 5 * np.sqrt(var / n), d.mean()
        assert abs(d.var() / var - 1) <= 5 * np.sqrt(2 / n), d.var()
        assert not np.array_equal(d[0], d[1])
        a, _ = _aug(clip_float=True).augment_only(x, m, records=recs)
        assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    # brightness with the clip lands in [0, 1] too; without it a z-scored image keeps its range
    z = torch.from_numpy(np.random.RandomState(0).standard_normal((B, S, S)).astype(np.float32)).to(DEV)
    recs = _recs(B, R.OP_BC, H=S, W=S)
    a, _ = _aug(clip_float=True).augment_only(z, m, records=recs)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    a, _ = _aug(clip_float=False).augment_only(z, m, records=recs)
    assert float(a.min()) < -1.0 and float(a.max()) > 2.0


def test_same_seed_and_offset_same_bits():
    from cmunet_amd import ft_augment as FA
    img, mask = _data(4, seed=3)
    x, y = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    cfg = FA.FinetuneAugmentConfig(p_noise=0.5, p_blur=0.5, p_brightness_contrast=0.5, p_downscale=0.5, clip_float=False)
    a1 = FA.DeviceTrainingAugmentation(cfg, seed=3, offset=10)
    a2 = FA.DeviceTrainingAugmentation(cfg, seed=3, offset=10)
    a3 = FA.DeviceTrainingAugmentation(cfg, seed=3, offset=11)
    i1, o1 = a1(x, y)
    i2, o2 = a2(x, y)
    i3, o3 = a3(x, y)
    assert torch.equal(i1.view(torch.int32), i2.view(torch.int32)) and torch.equal(o1, o2)
    assert np.array_equal(a1.records(), a2.records())
    assert not torch.equal(i1, i3)
    assert a1.offset == 11 and not np.array_equal(a1.records(), a3.records())


def test_no_host_sync_in_sampler_pipeline_and_loader_epoch(tmp_path):
    from cmunet_amd import ft_augment as FA
    paths = _write_split(tmp_path, 5, 480)
    make_loaders = FA.device_finetune_loaders(*paths, [0, 1], seed=1)
    train, _ = make_loaders([0, 1, 2, 3, 4], [0], 2)
    aug = FA.get_training_augmentation(seed=2)
    img, mask = _data(3, seed=5)
    x, y = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        aug.sample(16, 480, 480)
        gi, go = aug(x, y)
        batches = [b for b in train]
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(batches) == 3 and [tuple(b[0].shape) for b in batches] == [(2, 256, 256), (2, 256, 256), (1, 256, 256)]
    assert torch.isfinite(gi).all() and go.sum(1).eq(1).all()


def _write_split(tmp_path, n, side, seed=0):
    rng = np.random.RandomState(seed)
    xs, ys = [], []
    for i in range(n):
        m = (rng.uniform(size=(side, side)) < 0.15).astype(np.uint8)
        a = (rng.standard_normal((side, side)) + 1.5 * m).astype(np.float32)
        xp, yp = str(tmp_path / f"img_{i}.npy"), str(tmp_path / f"msk_{i}.npy")
        np.save(xp, a)
        np.save(yp, m)
        xs.append(xp)
        ys.append(yp)
    return xs, ys


def test_train_loader_visits_every_index_once_per_epoch(tmp_path):
    from cmunet_amd import ft_augment as FA
    from cmunet_amd.dataset import DeviceSegmentationBatch
    xs, ys = _write_split(tmp_path, 5, 476)
    make_loaders = FA.device_finetune_loaders(xs, ys, [0, 1], seed=3)
    ident = lambda a, b: (a, b)                                            # noqa: E731
    train, test = make_loaders([0, 2, 3, 4], [1], 3)
    train.transform = ident
    for _ in range(2):
        seen = torch.cat([a[:, 0, 0] for a, _ in train]).cpu()
        want = torch.stack([make_loaders.images[i, 0, 0] for i in (0, 2, 3, 4)]).cpu()
        assert sorted(seen.tolist()) == sorted(want.tolist())
    (vi, vo), = list(test)
    ri, ro = DeviceSegmentationBatch(256, [0, 1])(make_loaders.images[1:2], make_loaders.masks[1:2])
    assert torch.equal(vi, ri) and torch.equal(vo, ro)
    bad = str(tmp_path / "bad.npy")
    np.save(bad, np.zeros((470, 476), np.float32))
    with pytest.raises(ValueError, match="differ"):
        FA.device_finetune_loaders(xs + [bad], ys + [ys[0]], [0, 1])


def test_albumentations_protocol_through_segmentation_dataset(tmp_path):
    from cmunet_amd import ft_augment as FA
    from cmunet_amd.dataset import SegmentationDataset
    xs, ys = _write_split(tmp_path, 2, 480)
    aug = FA.get_training_augmentation(seed=4)
    out = aug(image=np.load(xs[0]), mask=np.load(ys[0]))
    assert set(out) == {"image", "mask"} and out["image"].shape == (S, S) and out["image"].dtype == np.float32
    assert out["mask"].shape == (S, S) and out["mask"].dtype == np.uint8
    plain = SegmentationDataset(xs, ys, class_values=[0, 1])[0]
    item = SegmentationDataset(xs, ys, class_values=[0, 1], augmentation=aug)[0]
    for a, b in zip(item, plain):
        assert a.shape == b.shape and a.dtype == b.dtype
    assert item[0].shape == (256, 256) and item[0].dtype == np.float32 and item[1].shape == (2, 256, 256) and item[1].dtype == np.float64


def test_short_main_finetuning_through_device_loaders(tmp_path):
    from cmunet_amd import ft_augment as FA, metrics as M, train as T
    xs, ys = _write_split(tmp_path, 6, 480, seed=2)
    args = T.get_args(["-e", "1", "-b", "2", "-l", "1e-3", "-n", "ftaug"])
    args.base_ch, args.depth = 16, 3
    mk = dict(activation="softmax", threshold=0.5, ignore_channels=[0])
    crit = M.DiceLoss(**mk) + M.CrossEntropyLoss()
    mets = [M.DiceLoss(**mk)]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        best, result = T.main_finetuning(args, crit, mets, DEV, [0, 1], xs, ys, make_loaders=FA.device_finetune_loaders(xs, ys, [0, 1], seed=0),
                                         work_dir=str(tmp_path / "wd"), save_best=False)
    assert not [w for w in caught if "train_augmentation" in str(w.message)]
    assert best == [1e-3, 2, 1]
    assert len(result) == 3
    for r in result:
        assert set(r) >= {"epochs", "lr", "batch_size", "runtime", "fold", "train_logs_list", "valid_logs_list"}
        for logs in (r["train_logs_list"][0], r["valid_logs_list"][0]):
            assert set(logs) == {crit.__name__, "dice_loss"} and all(np.isfinite(v) for v in logs.values())


def test_error_paths():
    from cmunet_amd import ft_augment as FA
    aug = FA.get_training_augmentation()
    small = torch.zeros(1, 470, 480, device=DEV)
    m = torch.zeros(1, 470, 480, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="at least 475"):
        aug(small, m)
    with pytest.raises(TypeError, match="uint8 images"):
        aug(torch.zeros(1, 480, 480, dtype=torch.uint8, device=DEV), torch.zeros(1, 480, 480, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="cuda"):
        aug(torch.zeros(1, 480, 480), torch.zeros(1, 480, 480, dtype=torch.uint8))
    with pytest.raises(TypeError, match="uint8 images"):
        aug(image=np.zeros((480, 480), np.uint8), mask=np.zeros((480, 480), np.uint8))
