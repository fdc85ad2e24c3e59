"""GPU suite for the connected-component clean-up (cmunet_amd/postprocess.py, csrc/components.hip) against tests/components_ref.py.
Every result is an integer: every comparison is exact equality, no tolerance.  The case list (tests/components_cases.py) holds the
smallest shapes at which a union-find on 32 x 32 tiles can go wrong; references are computed once per case and shared."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import components_cases as C
import components_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(C.cases()))
def test_labels_counts_and_sizes_are_exact(name, connectivity):
    from cmunet_amd import postprocess as P
    mask = C.cases()[name]
    want, wn = C.ref_label(name, connectivity)
    m = _dev(mask)
    lab, cnt = P.label(m, connectivity)
    assert lab.dtype == torch.int32 and cnt.dtype == torch.int32 and lab.shape == m.shape and cnt.dim() == 0
    assert int(cnt) != -1, "a find / union walk overran its trip bound"
    assert int(cnt) == wn
    assert np.array_equal(lab.cpu().numpy(), want)
    sizes = P.component_sizes(lab)
    assert sizes.dtype == torch.int32 and np.array_equal(sizes.cpu().numpy(), R.component_sizes(want))
    lab2, cnt2 = P.label(m, connectivity)                       # reproducibility: the same bits on a second call
    assert torch.equal(lab, lab2) and torch.equal(cnt, cnt2) and torch.equal(sizes, P.component_sizes(lab2))


@pytest.mark.parametrize("name", C.SMALL)
def test_cleanup_steps_are_exact(name):
    from cmunet_amd import postprocess as P
    mask = C.cases()[name]
    m = _dev(mask)
    assert np.array_equal(P.fill_holes(m).cpu().numpy(), R.fill_holes(mask).astype(np.uint8))
    for conn in (4, 8):
        assert np.array_equal(P.remove_small_objects(m, 5, conn).cpu().numpy(), R.remove_small_objects(mask, 5, conn).astype(np.uint8)), conn
        assert np.array_equal(P.keep_largest(m, 2, conn).cpu().numpy(), R.keep_largest(mask, 2, conn).astype(np.uint8)), conn
        got = P.clean_mask(m, min_size=4, keep_largest=3, fill_holes=True, connectivity=conn)
        assert np.array_equal(got.cpu().numpy(), R.clean_mask(mask, min_size=4, keep_largest=3, fill_holes=True, connectivity=conn)), conn
        assert torch.equal(got, P.clean_mask(m, min_size=4, keep_largest=3, fill_holes=True, connectivity=conn))


def test_batch_of_three_keeps_images_apart():
    from cmunet_amd import ops, postprocess as P
    b = C.batch3()
    m = _dev(b)
    for conn in (4, 8):
        want, wn = R.label_batch(b, conn)
        lab, cnt = P.label(m, conn)
        assert cnt.shape == (3,) and np.array_equal(cnt.cpu().numpy(), wn) and len(set(wn.tolist())) == 3
        assert np.array_equal(lab.cpu().numpy(), want)
        sizes = P.component_sizes(lab)
        assert np.array_equal(sizes.cpu().numpy(), np.stack([R.component_sizes(w) for w in want]))
        keep = ops.select_largest(sizes, 8).cpu().numpy()
        assert keep.tolist() == [R.select_largest(R.component_sizes(w), 8) for w in want]
        got = P.clean_mask(m, min_size=3, keep_largest=2, fill_holes=True, connectivity=conn).cpu().numpy()
        assert np.array_equal(got, np.stack([R.clean_mask(x, min_size=3, keep_largest=2, fill_holes=True, connectivity=conn) for x in b]))
    # a class index and a complement label as the non-zero rule does on a 0 / 1 map
    assert torch.equal(P.label(m, 8, cls=1)[0], P.label(m, 8)[0]) and torch.equal(P.label(m, 4, cls=-2)[0], P.label(m, 4)[0])


def test_tie_goes_to_the_smaller_label_and_min_size_boundary():
    from cmunet_amd import ops, postprocess as P
    m = np.zeros((40, 70), np.uint8)
    m[1, 1:5] = 1            # size 4, first pixel at index 71
    m[35, 60:64] = 1         # size 4, in another tile, later in row-major order
    m[20, 30:33] = 1         # size 3
    d = _dev(m)
    lab, _ = P.label(d)
    sizes = P.component_sizes(lab)
    assert ops.select_largest(sizes[None], 4).cpu().tolist() == [[72, 35 * 70 + 61, 20 * 70 + 31, -1]]
    k1 = P.keep_largest(d, 1).cpu().numpy()
    assert k1.sum() == 4 and k1[1, 1:5].all()
    assert np.array_equal(k1, R.keep_largest(m, 1).astype(np.uint8))
    assert P.remove_small_objects(d, 4).cpu().numpy().sum() == 8           # a size equal to min_size stays
    assert P.remove_small_objects(d, 3).cpu().numpy().sum() == 11
    assert P.remove_small_objects(d, 5).cpu().numpy().sum() == 0           # min_size - 1 goes
    assert np.array_equal(P.clean_mask(d).cpu().numpy(), m)                 # nothing asked for: a copy


def test_multi_class_map_and_class_values():
    from cmunet_amd import postprocess as P
    k3 = np.zeros((45, 70), np.uint8)
    k3[2:10, 2:10] = 1
    k3[5, 5] = 0             # a hole of class 1: stays, class 1 is not cleaned
    k3[20:44, 20:60] = 2
    k3[30, 33] = 1           # a class-1 pixel inside class 2, across a tile seam region: a hole of class 2
    k3[31:33, 31:33] = 0     # a background hole of class 2 on the four-tile corner
    k3[0, 69] = 2            # a class-2 speck
    d = _dev(np.stack([k3, k3[::-1].copy()]))
    for kw in ({"classes": [2], "min_size": 2, "fill_holes": True, "class_values": [0, 100, 200]},
               {"classes": [2], "min_size": 2, "fill_holes": True},
               {"min_size": 2, "keep_largest": 1, "num_classes": 3},
               {"fill_holes": True, "connectivity": 4, "class_values": [7, 8, 9]},
               {"class_values": [3, 2, 1]}):
        got = P.clean_mask(d, **kw).cpu().numpy()
        want = np.stack([R.clean_mask(x, **kw) for x in d.cpu().numpy()])
        assert np.array_equal(got, want), kw
    out = P.clean_mask(d[0], classes=[2], min_size=2, fill_holes=True, class_values=[0, 100, 200]).cpu().numpy()
    assert out[0, 69] == 0 and out[30, 33] == 200 and out[31, 31] == 200 and out[5, 5] == 0 and (out[2:5, 2:10] == 100).all()


def test_components_metric_is_the_count_difference():
    from cmunet_amd import metrics
    rng = np.random.default_rng(5)
    pr = rng.standard_normal((3, 2, 70, 45)).astype(np.float32)
    gt_mask = C.batch3()
    gt = np.stack([1 - gt_mask, gt_mask], 1).astype(np.float32)
    for conn in (4, 8):
        cp = R.label_batch((pr[:, 1] > pr[:, 0]).astype(np.uint8), conn)[1]
        ct = R.label_batch(gt_mask, conn)[1]
        met = metrics.components(connectivity=conn)
        per = met.per_image(_dev(pr), _dev(gt)).cpu().numpy()
        assert np.array_equal(per, np.stack([cp, ct], 1))
        v = met(_dev(pr), _dev(gt))
        # the counts above are exact; their fp64 mean over three images depends on the order of the sum and on how the division is
        # done: two roundings of 2^-53 relative each at the most
        want = np.abs(cp.astype(np.float64) - ct).mean()
        assert v.dtype == torch.float64 and v.dim() == 0 and abs(float(v) - want) <= 2 * 2.0 ** -53 * want and want > 0


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
def test_segmenter_cleans_at_the_image_size(tiny_segmenter_setup, mode):
    """Options on = the reference clean-up of what the options-off call returns; options off = the calls of before (same bits as a
    Segmenter built without the new keywords and as UNet.predict + resize)."""
    from cmunet_amd import ops
    from cmunet_amd.infer import Segmenter
    model, imgs = tiny_segmenter_setup
    base = {"size": 32, "batch": 2} if mode == "plain" else {"size": None, "tile": 32, "stride": 16, "batch": 3}
    off = Segmenter(model, **base).segment(imgs)
    off_kw = Segmenter(model, min_size=None, keep_largest=None, fill_holes=False, connectivity=8, **base).segment(imgs)
    assert all(torch.equal(a, b) for a, b in zip(off, off_kw))
    if mode == "plain":       # the parent's sequence, spelled out
        x = ops.resize_bicubic(imgs.cuda().contiguous(), 32, 32)
        parent = ops.resize_nearest(model.predict(x, threshold=0.5), 40, 56)
        assert all(torch.equal(a, b) for a, b in zip(off, parent))
    raw = [o.cpu().numpy() for o in off]
    assert all(r.shape == (40, 56) for r in raw) and 0 < sum(int(r.sum()) for r in raw) < 2 * 40 * 56
    for kw in ({"min_size": 6, "keep_largest": 2, "fill_holes": True}, {"min_size": 3, "connectivity": 4}, {"fill_holes": True}):
        ref_kw = {"min_size": kw.get("min_size") or 0, "keep_largest": kw.get("keep_largest"), "fill_holes": kw.get("fill_holes", False),
                  "connectivity": kw.get("connectivity", 8)}
        on = Segmenter(model, **base, **kw).segment(imgs)
        for o, r in zip(on, raw):
            assert np.array_equal(o.cpu().numpy(), R.clean_mask(r, **ref_kw)), (mode, kw)
        on = Segmenter(model, class_values=[10, 250], **base, **kw).segment(imgs, prob_class=1)      # the table is applied after the clean-up
        plain = Segmenter(model, class_values=[10, 250], **base).segment(imgs, prob_class=1)
        for (o, p), (_, p0), r in zip(on, plain, raw):
            assert np.array_equal(o.cpu().numpy(), R.clean_mask(r, class_values=[10, 250], **ref_kw)), (mode, kw)
            assert torch.equal(p, p0)                                                                 # prob is untouched


def test_cli_cleanup_flags_write_the_reference_cleanup(tiny_segmenter_setup, tmp_path):
    model, imgs = tiny_segmenter_setup
    torch.save(model.state_dict(), tmp_path / "m.pth")
    os.makedirs(tmp_path / "in")
    for i, im in enumerate(imgs):
        np.save(tmp_path / "in" / f"im{i}.npy", im.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    common = [sys.executable, "-m", "cmunet_amd.infer", "--model", str(tmp_path / "m.pth"), "--images", str(tmp_path / "in"), "--size", "32"]
    for out, flags in (("a", []), ("b", ["--min-size", "6", "--keep-largest", "2", "--fill-holes"])):
        r = subprocess.run(common + ["--out", str(tmp_path / out)] + flags, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    for i in range(len(imgs)):
        a, b = np.load(tmp_path / "a" / f"im{i}_mask.npy"), np.load(tmp_path / "b" / f"im{i}_mask.npy")
        assert np.array_equal(b, R.clean_mask(a, min_size=6, keep_largest=2, fill_holes=True))


def test_library_refuses_bad_arguments():
    from cmunet_amd import ops, postprocess as P
    m = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    for fn in (lambda: P.label(m, 6), lambda: P.keep_largest(m, 9), lambda: P.remove_small_objects(m, -1), lambda: ops.label_components(m, 300),
               lambda: ops.label_components(m.int()), lambda: ops.select_largest(m.int(), 0), lambda: P.label(m.float())):
        with pytest.raises(ValueError):
            fn()
