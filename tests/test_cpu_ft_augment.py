"""CPU checks of the finetuning augmentation's rules (tests/ft_augment_restate.py) and of the record layout shared with the HIP library."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ft_augment_restate as R  # noqa: E402
from cmunet_amd import ft_augment as FA  # noqa: E402


def test_restated_blur_is_scipy_mirror_correlation():
    from scipy import ndimage
    rng = np.random.RandomState(0)
    a = rng.standard_normal((37, 41))
    for k, sigma in ((5, 0.5), (7, 0.8), (11, 1.0), (15, 2.3)):
        w = R.gaussian_weights(k, sigma)
        assert abs(w.sum() - 1.0) < 1e-15 and np.allclose(w, w[::-1], rtol=0, atol=1e-17)
        got = R.blur(a, k, sigma, store=np.float64)
        ref = ndimage.correlate1d(ndimage.correlate1d(a, w, axis=1, mode="mirror"), w, axis=0, mode="mirror")
        assert np.abs(got - ref).max() < 1e-13, (k, sigma)


def test_restated_flips_and_rot90_are_numpys():
    a = np.arange(30).reshape(5, 6)
    assert np.array_equal(R.geometry(a, 0, 0), np.fliplr(a))
    assert np.array_equal(R.geometry(a, 1, 0), np.flipud(a))
    for k in range(4):
        assert np.array_equal(R.geometry(a, 2, k), np.rot90(a, k))
    assert np.array_equal(R.geometry(a, 3, 1), a)


def test_crop_offset_formula():
    assert R.crop_offset(475, 475, 0.999999) == 0
    assert R.crop_offset(480, 475, 0.0) == 0
    assert R.crop_offset(480, 475, 0.999999) == 5
    assert [R.crop_offset(480, 475, u) for u in (0.1, 0.2, 0.5, 0.84)] == [0, 1, 3, 5]


def test_ksize_law():
    counts = {}
    for k in range(5, 12):                       # the uniform integer draw of blur_limit (5, 11)
        ks = R.ksize_from_draw(k, 11)
        counts[ks] = counts.get(ks, 0) + 1
    assert counts == {5: 1, 7: 2, 9: 2, 11: 2}


def test_downscale_index_maps_monotone_and_in_range():
    for n in (16, 100, 475):
        for s in np.linspace(0.5, 1.0, 23):
            idx = R.downscale_index(n, float(s))
            assert idx.shape == (n,) and idx.min() >= 0 and idx.max() <= n - 1
            assert (np.diff(idx) >= 0).all()
            assert idx[0] == 0
    assert np.array_equal(R.downscale_index(475, 1.0), np.arange(475))
    # s = 0.5 on an even side: every source pixel of the even positions, each twice
    assert np.array_equal(R.downscale_index(8, 0.5), [0, 0, 2, 2, 4, 4, 6, 6])


def test_config_defaults_are_the_reference_arguments():
    c = FA.FinetuneAugmentConfig()
    assert c.crop == 475
    assert (c.p_noise, c.var_limit) == (0.1, (10.0, 50.0))
    assert (c.p_blur, c.blur_limit, c.sigma_limit) == (0.2, (5, 11), (0.5, 1.0))
    assert (c.p_brightness_contrast, c.brightness_limit, c.contrast_limit) == (0.15, 0.25, 0.2)
    assert (c.p_downscale, c.scale_limit) == (0.25, (0.5, 1.0))
    assert (c.p_oneof, c.oneof_var_limit) == (0.75, (10.0, 50.0))
    assert c.clip_float is True
    assert list(c.params()) == [0.1, 10, 50, 0.2, 5, 11, 0.5, 1.0, 0.15, -0.25, 0.25, -0.2, 0.2, 0.25, 0.5, 1.0, 0.75, 10, 50]
    c2 = FA.FinetuneAugmentConfig(p_blur=1.0, blur_limit=(3, 7), clip_float=False)
    assert (c2.p_blur, c2.blur_limit, c2.clip_float) == (1.0, (3, 7), False)


def test_config_refusals():
    with pytest.raises(ValueError, match="above 15"):
        FA.FinetuneAugmentConfig(blur_limit=(5, 17))
    with pytest.raises(ValueError, match="odd"):
        FA.FinetuneAugmentConfig(blur_limit=(5, 10))
    with pytest.raises(ValueError, match="probability"):
        FA.FinetuneAugmentConfig(p_noise=1.5)
    with pytest.raises(TypeError, match="unknown"):
        FA.FinetuneAugmentConfig(crop_width=400)
    # the whole messages (the override and probability helpers are shared with the other sampler configs)
    with pytest.raises(TypeError, match=r"^FinetuneAugmentConfig: unknown setting 'crop_width'$"):
        FA.FinetuneAugmentConfig(crop_width=400)
    with pytest.raises(ValueError, match=r"^p_oneof = -0\.25 is not a probability$"):
        FA.FinetuneAugmentConfig(p_oneof=-0.25)


def test_record_dtype_matches_the_c_struct():
    from cmunet_amd import _lib
    l = _lib.lib()
    out = (ctypes.c_int64 * 16)()
    n = l.cmu_ftaug_rec_layout(out, 16)
    assert n == 1 + len(FA.REC_DTYPE.names)
    assert out[0] == FA.REC_DTYPE.itemsize == 72
    assert [out[i + 1] for i in range(n - 1)] == [FA.REC_DTYPE.fields[k][1] for k in FA.REC_DTYPE.names]
    assert l.cmu_ftaug_max_ksize() == FA.MAX_KSIZE


def test_restated_chain_on_a_small_case():
    """The chain's pieces compose as the table says: crop, then the photometric ops, then Downscale, then OneOf."""
    rng = np.random.RandomState(3)
    img = rng.uniform(0, 1, (20, 22)).astype(np.float32)
    mask = (rng.uniform(size=(20, 22)) < 0.3).astype(np.uint8)
    rec = np.zeros((), FA.REC_DTYPE)
    rec["y0"], rec["x0"] = 2, 5
    rec["ops"] = R.OP_ONEOF
    rec["oneof"], rec["rot_k"] = 2, 1
    a, m = R.augment(img, mask, rec, crop=16)
    assert np.array_equal(a, np.rot90(img[2:18, 5:21], 1)) and np.array_equal(m, np.rot90(mask[2:18, 5:21], 1))
    rec["ops"] = R.OP_BC
    rec["alpha"], rec["beta"] = 1.1, 0.05
    a, m = R.augment(img, mask, rec, crop=16)
    ref = np.clip(img[2:18, 5:21] * np.float32(1.1) + np.float32(0.05), 0, 1)
    assert np.array_equal(a, ref) and np.array_equal(m, mask[2:18, 5:21])
