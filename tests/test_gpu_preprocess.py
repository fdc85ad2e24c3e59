"""GPU suite for cmunet_amd.preprocess (csrc/preprocess.hip) against the float64 restatement of tests/preprocess_ref.py.

Shapes are the smallest that reach every seam of the kernels: one pixel, sides shorter than the Gaussian's half-width, sides that are no
multiple of a tile, more than one tile along each axis (row pass: 4 rows x 256 columns per workgroup; column pass: 32 rows x 64 columns;
statistics: 1024 pixels per trip of the workgroup, 64 columns per trip of a row's wave).  Each runs as uint8 and as float32; image 1 of a
batch is constant, the float32 images hold negative values.

Bounds (U = 2^-24), all fixed before the kernels ran:
  statistics    uint8 mean / min / max and float32 min / max: the bits of numpy; std: 4 float64 roundoffs (2^-53) relative;
                float32 mean: the summation depth of the workgroup, (ceil(HW / 1024) + 22) roundoffs, plus numpy's pairwise 32, of mean|x|
  standardise, row-normalise: 1 float32 ulp of the float64 value (one final cast; the float64 statistics differ by ~2^-52); the
                constant image's nan pattern is numpy's
  min-max       the bits of numpy's float32 result (nan where numpy has nan)
  unsharp       c U (|f| + |amount| (|f| + sum w |f|)) with c = 2 lw + 12 -- derived in preprocess_ref.unsharp_bound; no element excluded
  crop, integrate, determinism: equality

The worst error / bound per operation is printed, and written to the file CMU_PRE_PARITY_OUT names when that variable is set
(profiles/preprocess_parity.txt holds one such run)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
EPS = 2.0 ** -53
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 37, 129), (2, 70, 300), (1, 130, 66), (4, 64, 64)]
DTYPES = [np.uint8, np.float32]
RADII = [0.1, 1, 2.5, 3, 10, 16]
AMOUNTS = [0, 1, -0.5, 2]
RATIOS = {}


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), float(ratio))


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import preprocess as p
    assert p.PRE_MAX_RADIUS == RADII[-1]
    yield p
    lines = [f"{k}: worst error / bound = {r:.4f}" for k, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    out = os.environ.get("CMU_PRE_PARITY_OUT")
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tests/test_gpu_preprocess.py: worst error against the float64 restatement as a fraction of its bound:\n"
                    "# std: 4 * 2^-53 relative; mean (float32 images): (ceil(HW / 1024) + 54) * 2^-53 * mean|x|; standardize, row_normalize:\n"
                    "# 1 float32 ulp; unsharp: (2 lw + 12) * 2^-24 * (|f| + |amount| (|f| + sum w |f|)), no element excluded.\n"
                    "# uint8 mean / min / max, min-max, crop, integrate and the repeat call are compared bit for bit (not listed).\n")
            f.write("\n".join(lines) + "\n")


_DATA = {}


def data(shape, dtype):
    """The batch of a (shape, dtype), made once: image 1 (where there is one) constant; float32 images hold negative values."""
    key = (shape, np.dtype(dtype).name)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * shape[1] + shape[2] + (7 if dtype == np.uint8 else 0))
        if dtype == np.uint8:
            x = rng.integers(0, 256, size=shape, dtype=np.uint8)
            if shape[0] > 1:
                x[1] = 7
        else:
            x = (rng.standard_normal(shape) * 0.7 + 0.3).astype(np.float32)
            if shape[0] > 1:
                x[1] = 2.5
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def name(dtype):
    return np.dtype(dtype).name


def same_with_nan(got, want):
    return got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_statistics(P, shape, dtype):
    x = data(shape, dtype)
    got = P.image_stats(torch.from_numpy(x.copy())).cpu().numpy()
    assert got.shape == (shape[0], 4) and got.dtype == np.float64
    for b in range(shape[0]):
        mean, std, lo, hi = R.image_stats(x[b])
        assert got[b, 2] == lo and got[b, 3] == hi
        if dtype == np.uint8:
            assert got[b, 0] == mean, (got[b, 0], mean)
        else:
            depth = math.ceil(x[b].size / 1024) + 22 + 32
            bound = depth * EPS * float(np.mean(np.abs(x[b].astype(np.float64))))
            note(f"mean {name(dtype)}", abs(got[b, 0] - mean) / bound)
            assert abs(got[b, 0] - mean) <= bound, (got[b, 0], mean)
        if std == 0.0:
            assert got[b, 1] == 0.0
        else:
            rel = abs(got[b, 1] - std) / std
            print(f"std {shape} {name(dtype)} image {b}: {rel / EPS:.2f} roundoffs")
            note(f"std {name(dtype)}", rel / (4 * EPS))
            assert rel <= 4 * EPS, (got[b, 1], std, rel / EPS)
    single = P.image_stats(torch.from_numpy(x[0].copy())).cpu().numpy()
    assert single.shape == (4,) and np.array_equal(single, got[0], equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_standardize_minmax_rows(P, shape, dtype):
    x = data(shape, dtype)
    xd = torch.from_numpy(x.copy()).to(DEV)
    with np.errstate(all="ignore"):
        z = P.standardize(xd).cpu().numpy()
        mm = P.minmax(xd).cpu().numpy()
        rows = P.row_normalize(xd).cpu().numpy()
        assert z.dtype == mm.dtype == rows.dtype == np.float32 and z.shape == mm.shape == rows.shape == shape
        for b in range(shape[0]):
            want = R.standardize(x[b])
            assert np.array_equal(np.isnan(z[b]), np.isnan(want)) and np.array_equal(np.isinf(z[b]), np.isinf(want))
            if shape[0] > 1 and b == 1:
                assert np.isnan(z[b]).all()      # the constant image: 0 / 0 everywhere, as numpy
            ok = np.isfinite(want)
            err = np.abs(z[b].astype(np.float64) - want)[ok] / R.ulp32(want)[ok]
            if err.size:
                note(f"standardize {name(dtype)}", err.max())
                assert err.max() <= 1.0, err.max()
            assert same_with_nan(mm[b], R.minmax(x[b])), (shape, b)
            wr = R.row_normalize(x[b])
            err = np.abs(rows[b].astype(np.float64) - wr) / R.ulp32(wr)
            note(f"row_normalize {name(dtype)}", err.max())
            assert err.max() <= 1.0, err.max()
        # statistics handed in: one number, and one per image
        m, s = 0.25, 3.0
        z2 = P.standardize(xd, mean=m, std=s).cpu().numpy()
        want = R.standardize(x, m, s)
        assert (np.abs(z2.astype(np.float64) - want) <= R.ulp32(want)).all()
        los = [float(b) for b in range(shape[0])]
        mm2 = P.minmax(xd, lo=los, hi=300.0).cpu().numpy()
        for b in range(shape[0]):
            if dtype == np.uint8:      # an exact integer difference (never wrapped), one float32 division
                ref = (x[b].astype(np.int32) - int(los[b])).astype(np.float32) / np.float32(300 - int(los[b]))
            else:
                ref = (x[b] - np.float32(los[b])) / (np.float32(300.0) - np.float32(los[b]))
            assert same_with_nan(mm2[b], ref)


def test_zero_row_stays_zero(P):
    for dtype in DTYPES:
        x = data((3, 37, 129), dtype).copy()
        x[0, 5] = 0
        x[2, 36] = 0
        got = P.row_normalize(torch.from_numpy(x)).cpu().numpy()
        assert (got[0, 5] == 0).all() and (got[2, 36] == 0).all() and np.isfinite(got).all()
        want = R.row_normalize(x[0])
        assert (np.abs(got[0].astype(np.float64) - want) <= R.ulp32(want)).all()


def check_unsharp(P, x, kind, radii=RADII, amounts=AMOUNTS):
    """Every (radius, preserve_range, amount) on the batch x; the restatement's blur is computed once per (radius, preserve_range)."""
    xd = torch.from_numpy(x.copy()).to(DEV)
    for radius in radii:
        for preserve in (False, True):
            parts = [R.unsharp_parts(x[b], radius, preserve) for b in range(x.shape[0])]
            lw, _ = R.gaussian_taps(radius)
            for amount in amounts:
                got = P.unsharp_mask(xd, radius=radius, amount=amount, preserve_range=preserve).cpu().numpy()
                assert got.dtype == np.float32 and got.shape == x.shape
                for b, (f, blurred, babs) in enumerate(parts):
                    want = f + (f - blurred) * amount
                    if not preserve:
                        want = np.clip(want, -1.0 if (f < 0).any() else 0.0, 1.0)
                    bound = (2 * lw + 12) * U * (np.abs(f) + abs(amount) * (np.abs(f) + babs))
                    err = np.abs(got[b].astype(np.float64) - want)
                    assert (err[bound == 0] == 0).all()      # (where nothing is in reach of the kernel the result is exactly zero)
                    ratio = (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0
                    note(f"unsharp {kind} lw={lw}", ratio)
                    assert (err <= bound).all(), (kind, radius, preserve, amount, b, ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_unsharp_random_images(P, shape, dtype):
    check_unsharp(P, data(shape, dtype), name(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", [(1, 70, 300), (1, 130, 66)], ids=str)
def test_unsharp_unit_impulses_at_tile_seams_and_corners(P, shape, dtype):
    """Impulses on both sides of every seam of the two passes (row pass: rows 4 r, column 256; column pass: rows 32 r, columns 64 c)
    and at the four corners: a wrong halo, a wrong reflection or a misplaced tile shows as a full tap's weight, far above the bound."""
    _, H, W = shape
    ys = sorted({0, H - 1} | {y for s in (4, 32, 64, 96, 128) for y in (s - 1, s) if y < H})
    xs = sorted({0, W - 1} | {v for s in (64, 128, 192, 256) for v in (s - 1, s) if v < W})
    one = 255 if dtype == np.uint8 else 1
    imgs = []
    for k, y in enumerate(ys):      # one image per seam row: its impulses sit on every seam column (alternating, so that both sides differ)
        im = np.zeros((H, W), dtype=dtype)
        for j, v in enumerate(xs):
            if (j + k) % 2 == 0 or v in (0, W - 1):
                im[y, v] = one
        imgs.append(im)
    check_unsharp(P, np.stack(imgs), f"impulses {name(dtype)}", amounts=[1, -0.5])


def test_unsharp_clip_range_is_decided_per_image(P):
    """[-1,1] for the image that holds a negative value, [0,1] for its non-negative neighbours in the same batch."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 37, 129)) * 2.0).astype(np.float32)
    x[1:] = np.abs(x[1:])
    x[2, 0, 0] = 0.0
    got = P.unsharp_mask(torch.from_numpy(x), radius=2.5, amount=2.0).cpu().numpy()
    assert got[0].min() == -1.0 and got[0].max() == 1.0
    assert got[1].min() == 0.0 and got[2].min() == 0.0 and got[1].max() == 1.0
    check_unsharp(P, x, "mixed clip float32", radii=[1, 2.5], amounts=[2, -0.5])
    one_negative = x.copy()
    one_negative[1, 36, 128] = -1e-30      # a single tiny negative value flips that image alone
    got2 = P.unsharp_mask(torch.from_numpy(one_negative), radius=2.5, amount=2.0).cpu().numpy()
    assert got2[1].min() == -1.0 and got2[2].min() == 0.0
    u8 = data((2, 70, 300), np.uint8)
    g8 = P.unsharp_mask(torch.from_numpy(u8.copy()), radius=1, amount=2.0).cpu().numpy()
    assert g8.min() == 0.0 and g8.max() == 1.0
    assert P.unsharp_mask(torch.from_numpy(u8.copy()), radius=1, amount=2.0, preserve_range=True).max().item() > 255.0


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_center_crop_and_integrate_are_exact(P, shape, dtype):
    x = data(shape, dtype)
    B, H, W = shape
    rng = np.random.default_rng(H + W)
    mask = (rng.random(shape) < 0.3).astype(np.uint8) * 255
    for size in sorted({1, min(H, W), max(1, min(H, W) - 1), max(1, min(H, W) // 2)}):
        got, gm = P.center_crop(torch.from_numpy(x.copy()), size, torch.from_numpy(mask))
        assert got.dtype == torch.from_numpy(x.copy()).dtype and gm.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), R.center_crop(x, size), equal_nan=True)
        assert np.array_equal(gm.cpu().numpy(), R.center_crop(mask, size))
        assert np.array_equal(P.center_crop(x[0].copy(), size).cpu().numpy(), R.center_crop(x[0], size), equal_nan=True)
    with pytest.raises(ValueError, match="larger than the image"):
        P.center_crop(torch.from_numpy(x.copy()).to(DEV), min(H, W) + 1)
    stack = (rng.random((B, 3, H, W)) < 0.2).astype(np.uint8) * rng.integers(1, 256, size=(B, 3, H, W), dtype=np.uint8)
    stack[:, :, 0, 0] = [128, 128, 0]      # the reference's uint8 sum wraps to 0 here; any non-zero counts
    got = P.integrate_masks(torch.from_numpy(stack)).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, np.stack([R.integrate_masks(stack[b]) for b in range(B)]))
    assert got[0, 0, 0] == 1
    assert np.array_equal(P.integrate_masks([stack[0, m] for m in range(3)]).cpu().numpy(), R.integrate_masks(stack[0]))
    assert np.array_equal(P.integrate_masks(stack[0, :1]).cpu().numpy(), (stack[0, 0] != 0).astype(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_two_calls_give_equal_bits(P, dtype):
    xd = torch.from_numpy(data((3, 37, 129), dtype).copy()).to(DEV)
    pipe = P.from_options(crop=33, unsharp=(2.5, 1.5), normalize="intensity")
    for fn in (P.image_stats, P.standardize, P.minmax, P.row_normalize, lambda t: P.unsharp_mask(t, 10, 2.0), lambda t: P.center_crop(t, 30), pipe):
        a, b = fn(xd), fn(xd)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_reference_classes_on_dictionaries(P):
    """fit_transform / transform on {key: {"raw", "labelled"}}: per-key statistics, batches grouped by shape and dtype, an unseen key fails."""
    rng = np.random.default_rng(11)
    raw = {"a": rng.integers(0, 256, (20, 30), dtype=np.uint8), "b": rng.integers(0, 256, (20, 30), dtype=np.uint8),
           "c": rng.standard_normal((9, 14)).astype(np.float32)}
    lab = {k: [(rng.random(v.shape) < 0.2).astype(np.uint8), (rng.random(v.shape) < 0.2).astype(np.uint8)] for k, v in raw.items()}
    d = {k: {"raw": raw[k] if k != "b" else torch.from_numpy(raw[k]).to(DEV), "labelled": lab[k]} for k in raw}
    inorm = P.Intensity_normalizer()
    out = inorm.fit_transform(d)
    assert set(out) == set(d) and set(inorm.means) == set(d) == set(inorm.stds)
    for k in raw:
        want = R.standardize(raw[k])
        assert (np.abs(out[k]["raw"].cpu().numpy().astype(np.float64) - want) <= R.ulp32(want)).all()
        assert out[k]["labelled"] is lab[k]
        assert inorm.means[k].item() == R.image_stats(raw[k])[0] or raw[k].dtype != np.uint8
    other = {"a": {"raw": raw["b"], "labelled": lab["b"]}}      # transform reuses the statistics fitted for the key
    want = R.standardize(raw["b"], *R.image_stats(raw["a"])[:2])
    assert (np.abs(inorm.transform(other)["a"]["raw"].cpu().numpy().astype(np.float64) - want) <= R.ulp32(want)).all()
    with pytest.raises(KeyError):
        inorm.transform({"unseen": d["a"]})
    mnorm = P.MinMax_normalizer()
    out = mnorm.fit_transform(d)
    for k in raw:
        assert np.array_equal(out[k]["raw"].cpu().numpy(), R.minmax(raw[k]))
    with pytest.raises(KeyError):
        mnorm.transform({"unseen": d["a"]})
    out = P.skly_normalizer().fit_transform(d)
    assert (np.abs(out["c"]["raw"].cpu().numpy() - R.row_normalize(raw["c"])) <= R.ulp32(R.row_normalize(raw["c"]))).all()
    out = P.Mask_Integrater().fit_transform(d)
    for k in raw:
        assert np.array_equal(out[k]["labelled"].cpu().numpy(), R.integrate_masks(lab[k]))
    pipe = P.Pipeline([(P.Mask_Integrater, None), (P.Cropper, {"size": 8}), (P.Unsharper, {"radius": 1, "amount": 1, "preserve_range": False}),
                       (P.MinMax_normalizer, None)])
    out = pipe.fit_transform(d)
    for k in raw:
        assert tuple(out[k]["raw"].shape) == (8, 8) == tuple(out[k]["labelled"].shape)
        assert np.array_equal(out[k]["labelled"].cpu().numpy(), R.center_crop(R.integrate_masks(lab[k]), 8))
        sharp = R.unsharp_mask(R.center_crop(raw[k], 8), 1, 1).astype(np.float32)
        got = out[k]["raw"].cpu().numpy()
        assert got.min() == 0.0 and got.max() == 1.0 and np.abs(got - R.minmax(sharp)).max() < 1e-4


def small_unet():
    from cmunet_amd.model import UNet
    torch.manual_seed(3)
    net = UNet(base_ch=16, depth=3)
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    return net.to(DEV).eval()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_segmenter_with_preprocess_equals_preprocessing_by_hand(P, dtype):
    """Segmenter(preprocess=P) on raw 70 x 90 images == P applied by hand, then the same Segmenter without it: plain and tiled, masks at
    the cropped 64 x 64 size, equal at every pixel."""
    from cmunet_amd import infer
    net = small_unet()
    rng = np.random.default_rng(2)
    if dtype == np.uint8:
        raw = rng.integers(0, 256, (5, 70, 90), dtype=np.uint8)
    else:
        raw = (rng.standard_normal((5, 70, 90)) * 40 + 90).astype(np.float32)
    pre = P.from_options(crop=64, unsharp=(1.0, 1.0), normalize="intensity")
    by_hand = pre(torch.from_numpy(raw).to(DEV))
    assert by_hand.shape == (5, 64, 64) and by_hand.dtype == torch.float32
    with torch.no_grad():      # centre the two-class head on these images, so that neither class wins everywhere
        lo = net(by_hand)
        net.conv_last.bias[1] -= (lo[:, 1] - lo[:, 0]).median()
    torch.cuda.synchronize()
    for kw in (dict(size=None), dict(size=None, tile=32, stride=16), dict(size=32)):
        with_pre = infer.Segmenter(net, batch=2, preprocess=pre, **kw).segment(list(raw))
        without = infer.Segmenter(net, batch=2, **kw).segment(list(by_hand))
        assert len(with_pre) == len(without) == 5
        share = torch.stack(with_pre).float().mean().item()
        assert 0.02 < share < 0.98, share
        for a, b in zip(with_pre, without):
            assert a.shape == (64, 64) and a.dtype == torch.uint8 and torch.equal(a, b)
    with pytest.raises(ValueError, match="larger than the image"):
        infer.Segmenter(net, preprocess=P.from_options(crop=80)).segment(list(raw))
