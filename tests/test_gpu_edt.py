"""GPU suite for the exact Euclidean distance transform, the disk morphology and the surface-distance scores (csrc/edt.hip,
cmunet_amd/postprocess.py, cmunet_amd/metrics.py) against tests/edt_ref.py.  Squared distances, borders, morphology results, counts,
maxima and selected ranks are integers: those comparisons are exact equality.  The case list (tests/edt_cases.py) holds the smallest
shapes at which the kernels can go wrong, among them one below, at and one above every workgroup span; references are computed once
per case and shared.  Every call is repeated once: the same bits.
The number of integers compared exactly and the worst error / bound of the three fp64 scores is printed, and written to the file
CMU_EDT_PARITY_OUT names when that variable is set (profiles/edt_parity.txt holds one such run)."""
import functools
import os

import numpy as np
import pytest
import torch

import edt_cases as C
import edt_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
EXACT = {}
RATIOS = {}


def _exact(kind, n):
    EXACT[kind] = EXACT.get(kind, 0) + int(n)


def _ratio(kind, err, bound):
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), float(err) / float(bound) if bound > 0 else 0.0)


@pytest.fixture(scope="module", autouse=True)
def _parity_summary():
    yield
    lines = [f"{k}: {n} integers compared, all equal" for k, n in sorted(EXACT.items())]
    lines += [f"{k}: worst error / bound = {r:.4f}" for k, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    out = os.environ.get("CMU_EDT_PARITY_OUT")
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tests/test_gpu_edt.py against tests/edt_ref.py.  Squared distances, morphology maps, borders, counts, maxima and\n"
                    "# selected ranks are compared for equality; hd and nsd as fp64 values for equality.  Bounds of the others: directed means\n"
                    "# and assd (n + 8) * 2^-53 relative, hd_percentile 8 * 2^-53 relative.\n")
            f.write("\n".join(lines) + "\n")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _ref_d2(name, cls, to):
    return R.squared_distance_transform(C.cases()[name], cls, to)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("name", list(C.cases()))
def test_squared_distances_and_roots_are_exact(name):
    from cmunet_amd import postprocess as P
    m = _dev(C.cases()[name])
    for to in ("background", "foreground"):
        want = _ref_d2(name, -1, to)
        d2 = P.squared_distance_transform(m, to=to)
        assert d2.dtype == torch.int32 and d2.shape == m.shape
        assert np.array_equal(d2.cpu().numpy(), want), to
        _exact("squared_distance_transform", want.size)
        assert torch.equal(d2, P.squared_distance_transform(m, to=to))                      # the same bits on a second call
        d = P.distance_transform_edt(m, to=to)
        assert d.dtype == torch.float32 and np.array_equal(_bits(d), R.edt(want).view(np.int32)), to      # bit for bit, inf included
        assert torch.equal(d, P.distance_transform_edt(m, to=to))


def test_degenerate_shapes_and_the_no_site_rule():
    from cmunet_amd import postprocess as P
    one, zero = _dev(C.cases()["1x1_1"]), _dev(C.cases()["1x1_0"])
    assert P.squared_distance_transform(zero, to="foreground").tolist() == [[-1]] and P.squared_distance_transform(zero).tolist() == [[0]]
    assert P.squared_distance_transform(one, to="foreground").tolist() == [[0]] and P.squared_distance_transform(one).tolist() == [[-1]]
    assert P.distance_transform_edt(one).tolist() == [[float("inf")]] and P.distance_transform_edt(zero).tolist() == [[0.0]]
    full, none = _dev(C.cases()["all_sites"]), _dev(C.cases()["no_sites"])
    assert (P.squared_distance_transform(full, to="foreground") == 0).all() and (P.squared_distance_transform(full) == -1).all()
    assert (P.squared_distance_transform(none, to="foreground") == -1).all() and (P.squared_distance_transform(none) == 0).all()
    assert torch.isinf(P.distance_transform_edt(none, to="foreground")).all()
    for name, axis in (("strip_1x37", 1), ("strip_41x1", 0)):      # a strip: the distance along the strip to the nearest site
        m = C.cases()[name]
        pos = np.flatnonzero(m.ravel())
        want = (np.abs(np.arange(m.size)[:, None] - pos[None, :]).min(1) ** 2).reshape(m.shape)
        assert np.array_equal(P.squared_distance_transform(_dev(m), to="foreground").cpu().numpy(), want), name


def test_closed_form_single_sites_sentinel_and_ties():
    from cmunet_amd import postprocess as P
    H, W = C.CORNERS_SHAPE
    yy, xx = np.mgrid[0:H, 0:W]
    for k, (y0, x0) in enumerate(C.CORNER_SITES):
        got = P.squared_distance_transform(_dev(C.cases()[f"one_site_{k}"]), to="foreground").cpu().numpy()
        assert np.array_equal(got, (yy - y0) ** 2 + (xx - x0) ** 2), (y0, x0)
    # a column with sites among columns without: the sentinel of the empty columns must lose against the real column
    yy, xx = np.mgrid[0:20, 0:9]
    got = P.squared_distance_transform(_dev(C.cases()["one_column"]), to="foreground").cpu().numpy()
    assert np.array_equal(got, (xx - 3) ** 2 + np.minimum((yy - 7) ** 2, (yy - 15) ** 2))
    # a band of rows without a site
    band = C.cases()["row_band"]
    got = P.squared_distance_transform(_dev(band), to="foreground").cpu().numpy()
    assert np.array_equal(got, R.dist2_brute(band != 0)) and got[39].min() >= 35 ** 2 and got.max() < 40 ** 2 + 30 ** 2
    # ties: (4,4) lies 3 from two sites; (2,4) lies sqrt(13) from two and 2 from the third
    got = P.squared_distance_transform(_dev(C.cases()["ties"]), to="foreground").cpu().numpy()
    assert got[4, 4] == 9 and got[2, 4] == 4 and got[4, 0] == 1 and got[8, 4] == 25 and np.array_equal(got, got[:, ::-1])
    chk = P.squared_distance_transform(_dev(C.cases()["checker"]), to="foreground").cpu().numpy()
    assert np.array_equal(chk, 1 - C.cases()["checker"].astype(np.int32))


@pytest.mark.parametrize("cls", [-1, 0, 1, 2, -2, -3, -4])
def test_every_site_rule_code_in_both_directions(cls):
    from cmunet_amd import postprocess as P
    m = _dev(C.cases()["labels3"])
    for to in ("background", "foreground"):
        got = P.squared_distance_transform(m, cls=cls, to=to)
        assert np.array_equal(got.cpu().numpy(), _ref_d2("labels3", cls, to)), to
        assert torch.equal(got, P.squared_distance_transform(m, cls=cls, to=to))


def test_batch_of_three_keeps_images_apart():
    from cmunet_amd import postprocess as P
    rnd = C.cases()["rand_33x65_0.02"]
    b = np.stack([np.ones_like(rnd), np.zeros_like(rnd), rnd])
    for to in ("background", "foreground"):
        got = P.squared_distance_transform(_dev(b), to=to).cpu().numpy()
        want = np.stack([R.squared_distance_transform(x, to=to) for x in b])
        assert np.array_equal(got, want) and len({int(w[0, 0] < 0) + 2 * int(w.max() > 0) for w in want}) == 3
    for fn, rf in ((P.binary_closing, R.binary_closing), (P.binary_erosion, R.binary_erosion)):
        assert np.array_equal(fn(_dev(b), 2).cpu().numpy(), np.stack([rf(x, 2) for x in b]))


def test_outputs_do_not_depend_on_what_the_scratch_held():
    """The memory contract without a table entry: every element of every scratch and output tensor is written on every call and nothing
    is read before it is written -- scratch pre-filled with 0xFF bytes and with zeros gives the same bits."""
    from cmunet_amd import _lib, ops
    a, b = C.cases()["blobs"], np.roll(C.cases()["blobs"], 3, 1)
    A, Bm = _dev(np.stack([a, b])), _dev(np.stack([b, np.zeros_like(a)]))
    p, st = ops._p, ops._stream
    runs = []
    for fill in (0xFF, 0x00):
        def buf(shape, dtype):
            t = torch.empty(shape, dtype=dtype, device="cuda")
            t.view(torch.uint8).fill_(fill)
            return t
        g, d2, dist, out8 = buf(A.shape, torch.int32), buf(A.shape, torch.int32), buf(A.shape, torch.float32), buf(A.shape, torch.uint8)
        _lib.call("cmu_edt_columns", p(Bm), -1, 1, p(g), 2, 48, 61, st())
        _lib.call("cmu_edt_rows", p(g), p(d2), p(dist), p(A), p(out8), 0, 5, 1, -1, 2, 48, 61, st())
        border = buf(A.shape, torch.uint8)
        _lib.call("cmu_surface_border", p(A), -1, p(border), 2, 48, 61, st())
        masked, sums, counts = buf(A.shape, torch.int32), buf((2, 2), torch.float64), buf((2, 3), torch.int32)
        _lib.call("cmu_surface_reduce", p(A), -1, p(d2), 4, p(masked), p(sums), p(counts), 2, 48, 61, st())
        vals, roots = buf((2, 2), torch.int32), buf((2, 2), torch.float64)
        ranks = torch.tensor([[0, 40], [5, 10 ** 6]], dtype=torch.int32, device="cuda")
        _lib.call("cmu_surface_select", p(masked), p(masked), p(ranks), 2, p(vals), p(roots), 2, 48, 61, st())
        runs.append([t.cpu().numpy().view(np.uint8) for t in (g, d2, dist, out8, border, masked, sums, counts, vals, roots)])
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    # and the wrappers hand back a caller's scratch tensor, filled
    g = torch.full(A.shape, -1, dtype=torch.int32, device="cuda")
    assert ops.edt_columns(A, g=g) is g and int(g.min()) >= 0 and int(g.max()) <= 16384


def test_sizes_outside_the_supported_range_are_refused():
    from cmunet_amd import _lib, ops, postprocess as P
    with pytest.raises(ValueError, match="4096"):
        P.squared_distance_transform(torch.zeros(1, 4097, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="4096"):
        P.binary_closing(torch.zeros(4097, 1, dtype=torch.uint8, device="cuda"), 1)
    t, g = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda"), torch.zeros(1, 4, 4, dtype=torch.int32, device="cuda")
    for dims in ((1, 4097, 4), (1, 4, 4097), (0, 4, 4), (65536, 4, 4)):      # refused before anything is launched
        with pytest.raises(_lib.CmuError, match="bad args"):
            _lib.call("cmu_edt_columns", ops._p(t), -1, 0, ops._p(g), *dims, ops._stream())
        with pytest.raises(_lib.CmuError, match="bad args"):
            _lib.call("cmu_edt_rows", ops._p(g), ops._p(g), None, None, None, 0, 0, -1, -1, *dims, ops._stream())
    side = torch.ones(1, 1, 4096, dtype=torch.uint8, device="cuda")      # the largest side: the far end of a row, 4095^2
    side[0, 0, 0] = 0
    assert P.squared_distance_transform(side)[0, 0, -1].item() == 4095 ** 2


@pytest.mark.parametrize("radius", C.RADII)
def test_morphology_is_exact(radius):
    from cmunet_amd import postprocess as P
    pairs = ((P.binary_dilation, R.binary_dilation), (P.binary_erosion, R.binary_erosion), (P.binary_opening, R.binary_opening),
             (P.binary_closing, R.binary_closing))
    for name in C.SMALL:
        m = C.cases()[name]
        if m.size > 6000:
            continue
        if name == "labels3":
            m = m * 7                  # values 0, 7, 14: kept pixels keep their value, added ones become 1
        d = _dev(m)
        for fn, rf in pairs:
            got = fn(d, radius)
            assert got.dtype == torch.uint8 and got.data_ptr() != d.data_ptr()
            assert np.array_equal(got.cpu().numpy(), rf(m, radius)), (name, fn.__name__)
            _exact("binary morphology", m.size)
            assert torch.equal(got, fn(d, radius))
    assert torch.equal(P.binary_closing(d, 0), d) and torch.equal(P.binary_dilation(d, 0.5), d)


def test_clean_mask_opens_and_closes_each_class():
    from cmunet_amd import postprocess as P
    g = C.gap_map()
    batch = np.stack([g, g[::-1, ::-1].copy()])
    d = _dev(batch)
    for kw in ({"closing": 1.5, "keep_largest": 1, "num_classes": 3}, {"keep_largest": 1, "num_classes": 3},
               {"opening": 1, "num_classes": 3}, {"opening": 1, "closing": 2.5, "min_size": 3, "fill_holes": True, "num_classes": 3},
               {"closing": 5, "classes": [2], "class_values": [0, 100, 200]}, {"opening": 1.5, "class_values": [9, 8, 7]},
               {"closing": 2, "classes": [1, 2], "keep_largest": 2, "connectivity": 4, "class_values": [0, 1, 2]}):
        got = P.clean_mask(d, **kw)
        want = np.stack([R.clean_mask(x, **kw) for x in batch])
        assert np.array_equal(got.cpu().numpy(), want), kw
        assert torch.equal(got, P.clean_mask(d, **kw))
    joined = P.clean_mask(d[0], closing=1.5, keep_largest=1, num_classes=3).cpu().numpy()
    split = P.clean_mask(d[0], keep_largest=1, num_classes=3).cpu().numpy()
    assert joined[10, 5] == 1 and joined[10, 17] == 1 and joined[10, 25] == 1 and split[10, 5] == 0 and split[10, 25] == 1
    lab = C.cases()["labels3"]
    for r in C.RADII:
        kw = {"opening": r, "closing": r, "num_classes": 3}
        assert np.array_equal(P.clean_mask(_dev(lab), **kw).cpu().numpy(), R.clean_mask(lab, **kw)), r
    assert np.array_equal(P.clean_mask(d, opening=0, closing=0).cpu().numpy(), batch)                  # the defaults: a copy, as before


@pytest.fixture(scope="module")
def tiny_segmenter_setup():
    from cmunet_amd import model as M
    torch.manual_seed(3)
    m = M.UNet(out_classes=2, base_ch=16, depth=3)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.2)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    m = m.cuda().eval()
    imgs = torch.from_numpy(np.random.default_rng(11).random((2, 40, 56)).astype(np.float32))
    with torch.no_grad():      # re-centre the head on these images: an unscaled random head puts nearly every pixel in one class
        flat = m(imgs.cuda()).transpose(0, 1).reshape(2, -1)
        s = 2.0 / flat.std(1).clamp_min(1e-6)
        m.conv_last.weight.mul_(s.view(2, 1, 1, 1))
        m.conv_last.bias.copy_((m.conv_last.bias - flat.median(1).values) * s)
    torch.cuda.synchronize()
    return m, imgs


@pytest.mark.parametrize("mode", ["plain", "tiled"])
def test_segmenter_closes_at_the_image_size(tiny_segmenter_setup, mode):
    from cmunet_amd import postprocess as P
    from cmunet_amd.infer import Segmenter
    model, imgs = tiny_segmenter_setup
    base = {"size": 32, "batch": 2} if mode == "plain" else {"size": None, "tile": 32, "stride": 16, "batch": 3}
    off = Segmenter(model, **base).segment(imgs)
    assert all(torch.equal(a, b) for a, b in zip(off, Segmenter(model, opening=None, closing=None, **base).segment(imgs)))
    raw = [o.cpu().numpy() for o in off]
    assert all(r.shape == (40, 56) for r in raw) and 0 < sum(int(r.sum()) for r in raw) < 2 * 40 * 56
    changed = 0
    for kw in ({"closing": 1.5}, {"opening": 1, "closing": 2}, {"closing": 1.5, "keep_largest": 1, "class_values": [10, 250]}):
        ckw = {"opening": kw.get("opening", 0), "closing": kw.get("closing", 0), "keep_largest": kw.get("keep_largest"),
               "class_values": kw.get("class_values")}
        on = Segmenter(model, **base, **kw).segment(imgs)
        for o, f, r in zip(on, off, raw):
            assert torch.equal(o, P.clean_mask(f, **ckw)), (mode, kw)
            assert np.array_equal(o.cpu().numpy(), R.clean_mask(r, **ckw)), (mode, kw)
            changed += int((o.cpu().numpy() != r).sum())
    assert changed > 0


# ---- surface distances -------------------------------------------------------------------------------------------------------
def _pairs():
    c = C.cases()
    blobs = c["blobs"]
    return {
        "blobs_shift": (blobs, np.roll(blobs, 3, 1)),
        "blobs_rand": (blobs, C._rand(blobs.shape, 0.01, 9)),
        "rand_33x65": (c["rand_33x65_0.5"], c["rand_33x65_0.02"]),
        "hw31x33": (c["hw31x33"], c["hw31x33"][::-1].copy()),
        "hw32x32": (c["hw32x32"], c["hw32x32"].T.copy()),
        "hw25x41": (c["hw25x41"], c["hw25x41"][:, ::-1].copy()),
        "hw33x63": (c["hw33x63"], np.roll(c["hw33x63"], 5, 0)),
        "w257": (c["w257"], np.roll(c["w257"], 40, 1)),
        "vessel_475": (c["vessel_475"], np.roll(c["vessel_475"], (2, -3), (0, 1))),
    }


@functools.lru_cache(maxsize=None)
def _ref_surface(name, tolerance, percentile):
    a, b = _pairs()[name]
    return R.surface_distances(a, b, tolerance, percentile)


def _check_scores(got, want, where):
    """got: SurfaceDistances of Python floats / ints; want: the reference dict."""
    assert (got.n_pr, got.n_gt) == (want["n_pr"], want["n_gt"]), where
    assert got.hd == want["hd"] and got.nsd == want["nsd"], (where, got.hd, want["hd"], got.nsd, want["nsd"])
    for key, n in (("mean_pr_to_gt", want["n_pr"]), ("mean_gt_to_pr", want["n_gt"])):
        g, w = getattr(got, key), want[key]
        print(f"{where} {key}: got {g!r} want {w!r}")
        assert g == w or abs(g - w) <= (n + 8) * U * w, (where, key, g, w)       # any order of n non-negative fp64 terms, a division
        if 0 < w < float("inf"):
            _ratio("directed mean distance", abs(g - w), (n + 8) * U * w)
    n = max(want["n_pr"], want["n_gt"])
    assert got.assd == want["assd"] or abs(got.assd - want["assd"]) <= (n + 8) * U * want["assd"], (where, got.assd, want["assd"])
    g, w = got.hd_percentile, want["hd_percentile"]
    print(f"{where} hd_percentile: got {g!r} want {w!r}")
    assert g == w or abs(g - w) <= 8 * U * w, (where, g, w)      # two exact order statistics, correctly rounded roots, three fp64 operations
    if 0 < w < float("inf"):
        _ratio("hd_percentile", abs(g - w), 8 * U * w)
        _ratio("assd", abs(got.assd - want["assd"]), (n + 8) * U * want["assd"])
    _exact("surface counts, hd, nsd", 4)


@pytest.mark.parametrize("name", list(_pairs()))
def test_surface_scores_borders_and_ranks(name):
    from cmunet_amd import metrics, ops
    a, b = _pairs()[name]
    A, B_ = _dev(a), _dev(b)
    assert np.array_equal(ops.surface_border(A[None]).cpu().numpy()[0], R.border(a)) and np.array_equal(
        ops.surface_border(B_[None]).cpu().numpy()[0], R.border(b))
    for tol, q in ((1.0, 95.0), (2.5, 50.0)) if name != "vessel_475" else ((1.0, 95.0),):
        want = _ref_surface(name, tol, q)
        s = metrics.surface_distances(A, B_, tolerance=tol, percentile=q)
        assert all(v.dim() == 0 and v.is_cuda for v in s) and s.hd.dtype == torch.float64 and s.n_pr.dtype == torch.int32
        _check_scores(type(s)(*(v.item() for v in s)), want, (name, tol, q))
        s2 = metrics.surface_distances(A, B_, tolerance=tol, percentile=q)
        assert all(torch.equal(x, y) for x, y in zip(s, s2))
    # the kernels underneath: masked maps, the integer triple, exact ranks of the pooled squared distances
    want = _ref_surface(name, 1.0, 95.0)
    to_b = ops.edt_rows(ops.edt_columns(B_[None], -1, True), "dist2")
    assert np.array_equal(to_b.cpu().numpy()[0], R.dist2(R.border(b)))
    sums, counts, ma = ops.surface_reduce(A[None], to_b, 1)
    to_a = ops.edt_rows(ops.edt_columns(A[None], -1, True), "dist2")
    _, counts_b, mb = ops.surface_reduce(B_[None], to_a, 1)
    assert np.array_equal(ma.cpu().numpy()[0], np.where(R.border(a), R.dist2(R.border(b)), -2))
    assert counts.cpu().tolist() == [[want["n_pr"], int(want["d2_ab"].max()), int((want["d2_ab"] <= 1).sum())]]
    assert counts_b.cpu().tolist() == [[want["n_gt"], int(want["d2_ba"].max()), int((want["d2_ba"] <= 1).sum())]]
    pooled = np.sort(np.hstack((want["d2_ab"], want["d2_ba"])))
    n = pooled.size
    for k0, k1 in ((0, n - 1), (n // 2, n // 2 + 1), (int(0.95 * (n - 1)), n), (n // 3, -1)):
        ranks = torch.tensor([[k0, k1]], dtype=torch.int32, device="cuda")
        vals, roots = ops.surface_select(ma, mb, ranks)
        exp = [int(pooled[k]) if 0 <= k < n else -1 for k in (k0, k1)]
        assert vals.cpu().tolist() == [exp], (k0, k1)
        _exact("selected ranks", 2)
        assert roots.cpu().tolist() == [[float(np.sqrt(np.float64(v))) if v >= 0 else float("inf") for v in exp]]
    one = ops.surface_select(ma, mb, torch.tensor([[n - 1]], dtype=torch.int32, device="cuda"))[0]
    assert one.cpu().tolist() == [[int(pooled[-1])]]


def test_surface_conventions_and_a_batch_whose_images_differ():
    from cmunet_amd import metrics
    blobs = C.cases()["blobs"]
    z = np.zeros_like(blobs)
    pr = np.stack([blobs, blobs, z, z, blobs, np.roll(blobs, 2, 0)])
    gt = np.stack([np.roll(blobs, 3, 1), z, blobs, z, blobs, C._rand(blobs.shape, 0.01, 9)])
    for tol, q in ((1.0, 95.0), (0.0, 100.0), (3.0, 0.0), (1.5, 37.5)):
        s = metrics.surface_distances(_dev(pr), _dev(gt), tolerance=tol, percentile=q)
        assert all(v.shape == (6,) for v in s)
        for i in range(6):
            want = R.surface_distances(pr[i], gt[i], tol, q)
            _check_scores(type(s)(*(v[i].item() for v in s)), want, (i, tol, q))
    inf = float("inf")
    s = metrics.surface_distances(_dev(pr), _dev(gt))
    assert s.hd.tolist()[1:5] == [inf, inf, 0.0, 0.0] and s.hd_percentile.tolist()[1:5] == [inf, inf, 0.0, 0.0]
    assert s.assd.tolist()[1:5] == [inf, inf, 0.0, 0.0] and s.nsd.tolist()[1:5] == [0.0, 0.0, 1.0, 1.0]
    assert s.n_pr.tolist()[2:4] == [0, 0] and s.n_gt.tolist()[1] == 0 and len(set(s.hd.tolist())) >= 4


def test_metric_classes_are_the_batch_means_of_the_function():
    from cmunet_amd import metrics, ops
    blobs = C.cases()["blobs"]
    gt_mask = np.stack([blobs, np.roll(blobs, 4, 1), blobs[::-1].copy()])
    rng = np.random.default_rng(5)
    logit = (gt_mask * 4.0 - 2.0) + rng.standard_normal(gt_mask.shape) * 1.2       # the target, with errors
    pr = np.stack([-logit / 2, logit / 2], 1).astype(np.float32)
    gt = np.stack([1 - gt_mask, gt_mask], 1).astype(np.float32)
    y_pr, y_gt = _dev(pr), _dev(gt)
    yp = torch.empty(3, 48, 61, dtype=torch.float32, device="cuda")
    ops.softmax2_threshold(y_pr, 0.5, yp)
    for met, field, kw in ((metrics.HausdorffDistance95(), "hd_percentile", {}), (metrics.HausdorffDistance95(percentile=80.0), "hd_percentile", {"percentile": 80.0}),
                           (metrics.AverageSurfaceDistance(), "assd", {}), (metrics.SurfaceDice(2.0), "nsd", {"tolerance": 2.0}),
                           (metrics.SurfaceDice(), "nsd", {})):
        per = getattr(metrics.surface_distances(yp, _dev(gt_mask), **kw), field)
        v = met(y_pr, y_gt)
        assert v.dtype == torch.float64 and v.dim() == 0 and torch.equal(v, per.mean()) and 0 < float(v) < float("inf")
        assert torch.equal(getattr(met.per_image(y_pr, y_gt), field), per)
    # ... and the function's values are the reference's on the masks the metric saw
    s = metrics.surface_distances(yp, _dev(gt_mask))
    for i in range(3):
        _check_scores(type(s)(*(v[i].item() for v in s)), R.surface_distances(yp[i].cpu().numpy() > 0, gt_mask[i]), ("metric", i))
    # usable in an epoch's metric list (train.Epoch.run): moved with .to(), named, called on (y_pred, y), reduced to a 0-dim fp64
    mets = [metrics.HausdorffDistance95(), metrics.AverageSurfaceDistance(), metrics.SurfaceDice()]
    assert [m.__name__ for m in mets] == ["hd95", "assd", "surface_dice"]
    vals = torch.stack([m.to("cuda")(y_pr, y_gt).detach().double().reshape(()) for m in mets])
    assert vals.shape == (3,) and bool(torch.isfinite(vals).all())
