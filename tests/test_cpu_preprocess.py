"""CPU suite for cmunet_amd.preprocess: the float64 restatement the kernels are held to (tests/preprocess_ref.py) is pinned to scipy,
sklearn and numpy's own expressions, and the Python surface is checked for everything that needs no device.  No GPU call anywhere."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as R      # noqa: E402

EPS = 2.0 ** -53


def _img(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return (rng.standard_normal(shape) * 3.0 + 0.5).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# the restatement against the libraries the reference calls
# ---------------------------------------------------------------------------------------------------
def test_reflect_index_is_half_sample_symmetric():
    assert [R.reflect_index(i, 4) for i in range(-9, 13)] == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3]
    assert [R.reflect_index(i, 1) for i in range(-3, 4)] == [0] * 7
    for n in (1, 2, 5, 7):      # the array form the tap loop uses is the scalar rule
        i = np.arange(-3 * n - 2, 3 * n + 3)
        assert R.reflect_index(i, n).tolist() == [R.reflect_index(int(v), n) for v in i]


@pytest.mark.parametrize("shape,radius", [((5, 7), 3.0), ((1, 1), 1.0), ((1, 1), 3.0), ((9, 4), 0.1), ((5, 7), 0.1), ((37, 129), 1.0),
                                          ((23, 31), 2.5), ((20, 17), 10.0), ((12, 70), 16.0)])
def test_gaussian_restatement_matches_scipy(shape, radius):
    """Within a few float64 roundoffs of sum w |x|: both add the same 2 lw + 1 products per axis, in different orders."""
    ndi = pytest.importorskip("scipy.ndimage")
    x = np.random.default_rng(int(radius * 10) + shape[0]).standard_normal(shape)
    want = ndi.gaussian_filter(x, sigma=radius, mode="reflect", truncate=4.0)
    got = R.gaussian(x, radius)
    lw, w = R.gaussian_taps(radius)
    assert lw == int(4.0 * radius + 0.5) and len(w) == 2 * lw + 1
    if lw == 0:
        assert np.array_equal(got, x)
    scale = R.gaussian(np.abs(x), radius)
    # per axis: 2 lw + 1 products and sums in each implementation
    assert (np.abs(got - want) <= 4 * (2 * lw + 2) * EPS * scale + 1e-300).all(), float(np.abs(got - want).max())


def test_gaussian_taps_match_scipy_kernel():
    ndi = pytest.importorskip("scipy.ndimage")
    for radius in (0.3, 1.0, 2.5, 16.0):
        lw, w = R.gaussian_taps(radius)
        imp = np.zeros(4 * lw + 1)
        imp[2 * lw] = 1.0
        k = ndi.gaussian_filter1d(imp, radius, mode="reflect", truncate=4.0)[lw:3 * lw + 1]
        assert np.allclose(k, w, rtol=8 * EPS, atol=0)
        from cmunet_amd import preprocess as P
        assert np.array_equal(P.gaussian_weights(radius), w[lw:])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_row_normalize_restatement_matches_sklearn(dtype):
    skp = pytest.importorskip("sklearn.preprocessing")
    x = _img((13, 29), np.uint8 if dtype == np.uint8 else np.float32, 5).astype(dtype)
    x[4] = 0
    want = skp.normalize(x)
    got = R.row_normalize(x)
    assert (got[4] == 0).all() and (np.asarray(want)[4] == 0).all()
    if dtype == np.float32:      # sklearn keeps float32 input in float32: norm and quotient round there (a few float32 ulps)
        assert want.dtype == np.float32
        assert (np.abs(got - want) <= 4 * R.ulp32(got)).all()
    else:
        assert np.allclose(got, want, rtol=8 * EPS, atol=0)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_standardize_and_minmax_restatements_are_numpys_expressions(dtype):
    x = _img((11, 17), dtype, 3)
    if dtype == np.uint8:
        want = ((x - np.mean(x)) / np.std(x)).astype("float32")      # the reference's line, numpy's own promotion (float64)
    else:
        want = ((x - np.mean(x, dtype=np.float64)) / np.std(x, dtype=np.float64)).astype("float32")      # float64 statistics
        assert ((x - np.mean(x, dtype=np.float64)) / np.std(x, dtype=np.float64)).dtype == np.float64
    assert np.array_equal(R.standardize(x).astype(np.float32), want)
    m, s, lo, hi = R.image_stats(x)
    assert (m, s, lo, hi) == (float(np.mean(x, dtype=np.float64)), float(np.std(x, dtype=np.float64)), float(x.min()), float(x.max()))
    mm = (x - np.min(x)) / (np.max(x) - np.min(x)).astype("float32")      # the reference's line, precedence included
    assert mm.dtype == np.float32 and np.array_equal(R.minmax(x), mm)
    if dtype == np.uint8:      # each step is one IEEE operation: an exact integer difference, one float32 division
        assert np.array_equal(mm, (x.astype(np.int32) - int(x.min())).astype(np.float32) / np.float32(int(x.max()) - int(x.min())))
    else:
        assert np.array_equal(mm, (x - x.min()) / np.float32(x.max() - x.min()))


def test_constant_image_nan_patterns():
    x = np.full((3, 4), 7, dtype=np.uint8)
    assert np.isnan(R.standardize(x)).all() and np.isnan(R.minmax(x)).all()
    y = np.full((3, 4), 2.5, dtype=np.float32)
    assert np.isnan(R.standardize(y)).all() and np.isnan(R.minmax(y)).all()


def test_unsharp_restatement_definition():
    x = _img((9, 12), np.uint8, 1)
    f = x / 255.0
    assert np.array_equal(R.unsharp_mask(x, 0.1, 2.0), np.clip(f, 0, 1))      # lw = 0: the blur is the identity
    assert np.array_equal(R.unsharp_mask(x, 0.1, 2.0, preserve_range=True), x.astype(np.float64))
    y = _img((9, 12), np.float32, 2)      # holds negative values: clipped to [-1, 1]
    r = R.unsharp_mask(y, 1.0, 1.0)
    assert r.min() == -1.0 and r.max() == 1.0
    r0 = R.unsharp_mask(np.abs(y), 1.0, 1.0)
    assert r0.min() >= 0.0 and r0.max() == 1.0
    ndi = pytest.importorskip("scipy.ndimage")
    want = y.astype(np.float64) + (y.astype(np.float64) - ndi.gaussian_filter(y.astype(np.float64), 2.5, mode="reflect", truncate=4.0)) * 1.5
    assert np.allclose(R.unsharp_mask(y, 2.5, 1.5, preserve_range=True), want, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------
REFERENCE_SIGNATURES = {      # data_processing/pre_processing.py: constructor parameters (name, default) after self
    "PreProcessor": [],
    "skly_normalizer": [],
    "Intensity_normalizer": [],
    "MinMax_normalizer": [],
    "Unsharper": [("radius", inspect.Parameter.empty), ("amount", inspect.Parameter.empty), ("preserve_range", inspect.Parameter.empty)],
    "Mask_Integrater": [],
    "Cropper": [("size", 475), ("border_ratio", 0.25), ("thresh", 20)],
    "Pipeline": [("steps", inspect.Parameter.empty)],
}


def test_class_names_and_signatures_are_the_references():
    from cmunet_amd import preprocess as P
    for name, params in REFERENCE_SIGNATURES.items():
        cls = getattr(P, name)
        got = [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
        assert got == params, (name, got)
        assert issubclass(cls, P.PreProcessor)
        for method in ("transform", "fit_transform"):
            assert list(inspect.signature(getattr(cls, method)).parameters) == ["self", "data"], (name, method)
    with pytest.raises(TypeError):
        P.PreProcessor()      # abstract, as in the reference
    for fn, params in (("image_stats", ["x"]), ("standardize", ["x", "mean", "std"]), ("minmax", ["x", "lo", "hi"]), ("row_normalize", ["x"]),
                       ("unsharp_mask", ["x", "radius", "amount", "preserve_range"]), ("center_crop", ["x", "size", "mask"]),
                       ("integrate_masks", ["masks"])):
        assert list(inspect.signature(getattr(P, fn)).parameters) == params, fn
    sig = inspect.signature(P.unsharp_mask).parameters
    assert (sig["radius"].default, sig["amount"].default, sig["preserve_range"].default) == (1.0, 1.0, False)
    assert P.PRE_MAX_RADIUS >= 16


def test_pipeline_builds_steps_like_the_reference():
    from cmunet_amd import preprocess as P
    pipe = P.Pipeline([(P.Cropper, {"size": 64}), (P.Unsharper, {"radius": 2, "amount": 1, "preserve_range": True}), (P.Intensity_normalizer, None)])
    assert [type(f).__name__ for f in pipe.functions] == ["Cropper", "Unsharper", "Intensity_normalizer"]
    assert pipe.functions[0].size == 64 and pipe.functions[1].radius == 2
    assert callable(P.Preprocess(pipe)) and callable(P.Preprocess([(P.MinMax_normalizer, None)]))
    with pytest.raises(ValueError, match="does not act on images"):
        P.Preprocess([(P.Mask_Integrater, None)])


def test_transform_before_fit_transform_raises():
    from cmunet_amd import preprocess as P
    data = {"a": {"raw": np.zeros((4, 4), np.uint8), "labelled": np.zeros((4, 4), np.uint8)}}
    for cls in (P.Intensity_normalizer, P.MinMax_normalizer):
        with pytest.raises(ValueError, match="please call `fit_transform` first"):
            cls().transform(data)
    with pytest.raises(AttributeError):      # the reference's Cropper has no ``aug`` before fit_transform
        P.Cropper().transform(data)


def test_bad_arguments_are_refused_before_any_device_work():
    from cmunet_amd import preprocess as P
    small = np.zeros((10, 20), np.uint8)
    with pytest.raises(ValueError, match="larger than the image"):
        P.center_crop(small, 11)
    with pytest.raises(ValueError, match="larger than the image"):
        P.center_crop(np.zeros((2, 30, 9), np.float32), 10)
    c = P.Cropper(size=16)
    with pytest.raises(ValueError, match="larger than the image"):
        c.fit_transform({"a": {"raw": small, "labelled": small}})
    for radius in (P.PRE_MAX_RADIUS + 0.5, 1000, -1.0, float("nan")):
        with pytest.raises(ValueError, match="PRE_MAX_RADIUS"):
            P.unsharp_mask(small, radius=radius)
        with pytest.raises(ValueError, match="PRE_MAX_RADIUS"):
            P.Unsharper(radius, 1, False)
    assert len(P.gaussian_weights(P.PRE_MAX_RADIUS)) == 4 * P.PRE_MAX_RADIUS + 1
    with pytest.raises(ValueError, match="normalize must be one of"):
        P.from_options(normalize="zscore")


def test_no_cpu_fallback():
    import torch
    from cmunet_amd import preprocess as P
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    x = np.zeros((8, 8), np.uint8)
    for call in (lambda: P.image_stats(x), lambda: P.standardize(x), lambda: P.minmax(x), lambda: P.row_normalize(x),
                 lambda: P.unsharp_mask(x), lambda: P.center_crop(x, 4), lambda: P.integrate_masks([x, x]),
                 lambda: P.Preprocess([(P.MinMax_normalizer, None)])(torch.zeros(1, 8, 8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_command_line_flags_parse_and_default_to_no_preprocessing():
    from cmunet_amd import infer, preprocess as P
    base = ["--model", "m", "--images", "i", "--out", "o"]
    a = infer.build_parser().parse_args(base)
    assert (a.crop, a.unsharp, a.preserve_range, a.normalize) == (None, None, False, "none")
    assert P.from_options(a.crop, a.unsharp, a.preserve_range, a.normalize) is None
    a = infer.build_parser().parse_args(base + ["--crop", "475", "--unsharp", "2.5", "1.5", "--preserve-range", "--normalize", "intensity"])
    assert (a.crop, a.unsharp, a.preserve_range, a.normalize) == (475, [2.5, 1.5], True, "intensity")
    pre = P.from_options(a.crop, a.unsharp, a.preserve_range, a.normalize)
    steps = pre.pipeline.functions
    assert [type(s).__name__ for s in steps] == ["Cropper", "Unsharper", "Intensity_normalizer"]      # crop -> unsharp -> normalise
    assert steps[0].size == 475 and (steps[1].radius, steps[1].amount, steps[1].preserve_range) == (2.5, 1.5, True)
    for name, cls in (("minmax", "MinMax_normalizer"), ("rows", "skly_normalizer")):
        a = infer.build_parser().parse_args(base + ["--normalize", name])
        assert [type(s).__name__ for s in P.from_options(None, None, False, a.normalize).pipeline.functions] == [cls]
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(base + ["--normalize", "zscore"])
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(base + ["--unsharp", "2"])


def test_segmenter_builds_with_and_without_preprocess():
    from cmunet_amd import infer, preprocess as P
    from cmunet_amd.model import UNet
    m = UNet(base_ch=16, depth=3)
    s = infer.Segmenter(m)
    assert s.preprocess is None and s.size == 256 and not s.tiled and not s.post
    assert "preprocess" in inspect.signature(infer.Segmenter.__init__).parameters
    assert inspect.signature(infer.Segmenter.__init__).parameters["preprocess"].default is None
    pre = P.from_options(crop=64)
    assert infer.Segmenter(m, size=None, tile=32, preprocess=pre).preprocess is pre
    with pytest.raises(ValueError, match="callable"):
        infer.Segmenter(m, preprocess="crop")
