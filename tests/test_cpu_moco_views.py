"""CPU checks of the MoCo view pipeline's rules (tests/moco_views_restate.py) against torch's own functions, of the host mirror of the
sampler's laws, of the record layout shared with the HIP library and of the configuration's validation."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moco_views_restate as R  # noqa: E402
from cmunet_amd import moco_views as MV  # noqa: E402

BOXES = [(0, 0, 256, 256), (16, 16, 224, 224), (3, 40, 115, 140), (100, 7, 150, 113), (0, 0, 224, 256), (5, 9, 251, 190)]


def _img(seed=0, n=256):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((n, n)).astype(np.float32))


@pytest.mark.parametrize("antialias", [False, True])
def test_explicit_resize_is_interpolate(antialias):
    """Row 2: the index-and-weight statement of the resize equals F.interpolate on the crop -- in float64 to rounding of the sums, in
    float32 (ATen's float32 source coordinates followed operation by operation) to a few ulp of the pixel values."""
    img = _img(1)
    for box in BOXES:
        ref64 = R.resized_crop(img, box, 224, antialias, torch.float64).numpy()
        got64 = R.resized_crop_explicit(img.numpy(), box, 224, antialias, f32=False)
        assert np.abs(got64 - ref64).max() <= 1e-13, (box, np.abs(got64 - ref64).max())
        ref32 = R.resized_crop(img, box, 224, antialias, torch.float32).numpy()
        got32 = R.resized_crop_explicit(img.numpy(), box, 224, antialias, f32=True)
        floor = np.abs(ref32.astype(np.float64) - ref64).max()
        d = np.abs(got32.astype(np.float64) - ref32).max()
        print(f"antialias {antialias} box {box}: |explicit32 - ATen32| {d:.3g}, rounding floor |ATen32 - ATen64| {floor:.3g}")
        assert d <= 4e-6, (box, d)


def test_explicit_blur_is_pad_conv2d():
    """Row 3: reflect padding (2 left / right, 4 top / bottom) and the outer-product kernel; exactly the identity at sigma = 0.1 in y."""
    img = _img(2, 64)
    for sigma in (0.1, 0.7, 2.0):
        ref = R.blur(img, (5, 9), sigma, torch.float64).numpy()
        assert np.abs(R.blur_explicit(img.numpy(), (5, 9), sigma) - ref).max() <= 1e-14
        w = R.gaussian_kernel1d(9, sigma)
        assert w.dtype == torch.float32 and abs(float(w.sum()) - 1) < 1e-6 and torch.equal(w, w.flip(0))
    x = F.pad(img[None, None], [2, 2, 4, 4], mode="reflect")[0, 0]
    assert torch.equal(x[4:-4, 0], img[:, 2]) and torch.equal(x[0, 2:-2], img[4, :])
    assert torch.equal(R.blur(img, (1, 1), 1.0), img)


def test_rotation_statement_on_exact_angles():
    """Multiples of 90 degrees land on integers: the rotation is a permutation of the pixels (counter-clockwise for positive angles), no
    pixel lies in the tie band, and float32 equals float64."""
    img = _img(3)
    assert torch.equal(R.rotate(img, 0.0), img)
    assert torch.equal(R.rotate(img, 90.0), torch.rot90(img, 1))
    assert torch.equal(R.rotate(img, -90.0), torch.rot90(img, -1))
    assert torch.equal(R.rotate(img, 180.0), torch.rot90(img, 2))
    assert torch.equal(R.rotate(img, -180.0), torch.rot90(img, 2))
    for a in (0.0, 90.0, -90.0, 180.0, -180.0, 0.0005):
        assert not R.rotation_tie_band(256, 256, a).any(), a
    assert torch.equal(R.rotate(img, 0.0005), img)


@pytest.mark.parametrize("angle", [12.345, -77.7, 163.2, 30.0, 45.0])
def test_float32_rotation_differs_from_float64_only_inside_the_tie_band(angle):
    img = _img(4)
    a, b = R.rotate(img, angle, torch.float32), R.rotate(img, angle, torch.float64).float()
    band = R.rotation_tie_band(256, 256, angle)
    share = float(band.float().mean())
    print(f"angle {angle}: tie band {100 * share:.3f} %, pixels differing {(a != b).sum().item()}")
    assert share <= 0.01
    assert torch.equal(a[~band], b[~band])


def test_host_mirror_sampler_laws():
    rng = np.random.RandomState(0)
    r = R.sample_records(4000, 256, 256, rng)
    assert (r["height"] >= 1).all() and (r["width"] >= 1).all() and (r["top"] >= 0).all() and (r["left"] >= 0).all()
    assert (r["top"] + r["height"] <= 256).all() and (r["left"] + r["width"] <= 256).all()
    assert (-180 <= r["angle"]).all() and (r["angle"] < 180).all() and (0.1 <= r["sigma"]).all() and (r["sigma"] <= 2.0).all()
    area = r["height"] * r["width"] / 65536.0
    assert 0.19 <= area.min() and area.max() <= 1.0
    for bit in (R.OP_ROTATION, R.OP_BLUR, R.OP_HFLIP, R.OP_VFLIP, R.OP_NOISE):
        assert abs(((r["ops"] & bit) != 0).mean() - 0.5) <= 4 * 0.5 / np.sqrt(4000)
    # the fallback: a scale range that never fits (every attempt wider than the image) gives the centred box with the ratio clamped
    assert R.crop_box(256, 256, rng, scale=(3.0, 4.0)) == (0, 0, 256, 256, True)
    assert R.crop_box(100, 300, rng, scale=(3.0, 4.0)) == (0, 83, 100, 133, True)
    assert R.crop_box(300, 100, rng, scale=(3.0, 4.0)) == (83, 0, 133, 100, True)
    # the law of the box's size is dataset.random_resized_crop_params' (same generator, same draws -> same size; that function draws
    # the column offset first, torchvision the row offset)
    from cmunet_amd.dataset import random_resized_crop_params
    for seed in range(20):
        i, j, h, w, _ = R.crop_box(256, 256, np.random.RandomState(seed))
        assert (w, h) == random_resized_crop_params(256, 256, np.random.RandomState(seed))[2:]


def test_record_dtype_is_the_librarys_layout():
    from cmunet_amd import _lib
    lay = MV.rec_layout()
    names = ["ops", "top", "left", "height", "width", "angle", "sigma"]
    assert lay[0] == MV.REC_DTYPE.itemsize == 40 and len(lay) == 1 + len(names)
    assert [MV.REC_DTYPE.fields[n][1] for n in names] == lay[1:]
    assert _lib.lib().cmu_mocoviews_max_ksize() == MV.MAX_KSIZE
    assert (MV.OP_ROTATION, MV.OP_BLUR, MV.OP_HFLIP, MV.OP_VFLIP, MV.OP_NOISE) == (R.OP_ROTATION, R.OP_BLUR, R.OP_HFLIP, R.OP_VFLIP, R.OP_NOISE)


def test_config_defaults_and_validation():
    c = MV.MocoViewConfig()
    assert (c.p_rotation, c.degrees, c.scale, c.p_blur, c.kernel_size, c.sigma, c.p_hflip, c.p_vflip, c.p_noise) == \
        (0.5, 180.0, (0.2, 1.0), 0.5, (5, 9), (0.1, 2.0), 0.5, 0.5, 0.5)
    assert c.ratio == (0.75, 4.0 / 3.0) and (c.size, c.out, c.antialias) == (256, 224, False)
    assert list(c.params()) == [0.5, 180.0, 0.2, 1.0, 0.75, 4.0 / 3.0, 0.5, 0.1, 2.0, 0.5, 0.5, 0.5]
    with pytest.raises(TypeError, match="unknown setting"):
        MV.MocoViewConfig(p_rotate=0.5)
    # the whole messages (the override and probability helpers are shared with the other sampler configs)
    with pytest.raises(TypeError, match=r"^MocoViewConfig: unknown setting 'p_rotate'$"):
        MV.MocoViewConfig(p_rotate=0.5)
    with pytest.raises(ValueError, match=r"^p_blur = 1\.5 is not a probability$"):
        MV.MocoViewConfig(p_blur=1.5)
    for bad in (dict(p_blur=1.5), dict(kernel_size=(4, 9)), dict(scale=(0.0, 1.0)), dict(sigma=(2.0, 0.1)), dict(ratio=(2.0, 1.0)),
                dict(degrees=-1), dict(out=2), dict(antialias=True, size=512, out=224)):
        with pytest.raises(ValueError):
            MV.MocoViewConfig(**bad)
    with pytest.raises(ValueError, match="LDS halo"):
        MV.MocoViewConfig(kernel_size=(5, 11))
    with pytest.raises(TypeError):
        MV.DeviceMocoViews(config={"p_blur": 1})
    with pytest.raises(ValueError, match="no CPU path"):
        MV.DeviceMocoViews().views(torch.zeros(1, 256, 256))
    with pytest.raises(ValueError, match="list of .npy paths"):
        MV.MoCoDataModule("some/dir")
    with pytest.raises(ValueError, match="cuda device"):
        MV.MoCoDataModule(["a.npy"], device="cpu")
