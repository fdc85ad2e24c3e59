"""Host side of tiled prediction (cmunet_amd.infer / ops.TileGrid / UNet.predict_probs) and the numpy restatement the GPU tests use
(tests/tiled_predict_ref.py), checked against numpy's and torch's own padding, flips and transposes.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tiled_predict_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_fold_is_numpy_reflect():
    """Every length 1..7 against every pad width up to more than three periods: pads wider than the image included."""
    rng = np.random.RandomState(0)
    for L in range(1, 8):
        a = rng.rand(L)
        for pad in range(0, 3 * 2 * L + 3):
            want = np.pad(a, (0, pad), mode="reflect")
            got = np.array([a[R.fold(i, L)] for i in range(L + pad)])
            assert np.array_equal(got, want), (L, pad)
    img = rng.rand(3, 5)
    assert np.array_equal(R.canvas(img, 8, 16, "reflect"), np.pad(img, ((0, 5), (0, 11)), mode="reflect"))
    assert np.array_equal(R.canvas(img, 8, 16, "zero"), np.pad(img, ((0, 5), (0, 11))))
    assert np.array_equal(R.canvas(img, 3, 5, "reflect"), img)


def test_restated_views_are_torch_flips_and_transposes():
    a = np.arange(2 * 5 * 5, dtype=np.float32).reshape(2, 5, 5)
    r = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
    for code in range(8):
        t = torch.from_numpy(a)
        if code & 1:
            t = torch.flip(t, dims=[-1])
        if code & 2:
            t = torch.flip(t, dims=[-2])
        if code & 4:
            t = t.transpose(-1, -2)
        assert np.array_equal(R.view(a, code), t.numpy()), code
        assert np.array_equal(R.inverse_view(R.view(a, code), code), a), code
        assert np.array_equal(R.view(R.inverse_view(a, code), code), a), code
        if code < 4:
            assert R.view(r, code).shape == r.shape and np.array_equal(R.inverse_view(R.view(r, code), code), r)
    # the eight views of an asymmetric square are pairwise different: the codes name the whole dihedral group
    views = [R.view(a[0], c).tobytes() for c in range(8)]
    assert len(set(views)) == 8
    # codes 5 and 6 are the two quarter turns
    assert np.array_equal(R.view(a[0], 5), np.rot90(a[0], 1)) or np.array_equal(R.view(a[0], 5), np.rot90(a[0], 3))
    assert np.array_equal(R.view(a[0], 6), np.rot90(a[0], 1)) or np.array_equal(R.view(a[0], 6), np.rot90(a[0], 3))


def test_tile_starts_and_blend_window_values():
    from cmunet_amd import infer
    assert infer.tile_starts(475, 256, 128) == [0, 128, 219]
    assert infer.tile_starts(256, 256, 128) == [0] and infer.tile_starts(11, 16, 8) == [0] and infer.tile_starts(1, 1, 1) == [0]
    assert infer.tile_starts(37, 16, 8) == [0, 8, 16, 21] and infer.tile_starts(29, 16, 12) == [0, 12, 13]
    assert infer.tile_starts(17, 16, 16) == [0, 1]                  # the clamped last tile overlaps its neighbour by T - 1
    assert infer.tile_starts(48, 16, 16) == [0, 16, 32]
    for L in range(1, 60):
        for T in (1, 4, 16):
            for stride in {1, max(1, T // 2), T}:
                s = infer.tile_starts(L, T, stride)
                assert s == R.tile_starts(L, T, stride)
                assert s[0] == 0 and s[-1] + T == max(L, T) and sorted(set(s)) == s
                assert R.uncovered(s, T, L) is None
    for bad in [(0, 4, 2), (8, 0, 1), (8, 4, 0), (8, 4, 5)]:
        with pytest.raises(ValueError):
            infer.tile_starts(*bad)
    u = infer.blend_window(16, "uniform")
    assert u.dtype == torch.float32 and torch.equal(u, torch.ones(16))
    for T in (1, 5, 16, 256):
        g = infer.blend_window(T, "gaussian")
        d = (np.arange(T, dtype=np.float64) - (T - 1) / 2.0) / (T / 8.0)
        want = np.exp(-0.5 * d * d)
        want = (want / want.max()).astype(np.float32)
        assert g.dtype == torch.float32 and np.array_equal(g.numpy(), want) and np.array_equal(want, R.window(T, "gaussian"))
        assert float(g.max()) == 1.0 and float(g.min()) > 0.0 and np.array_equal(want, want[::-1])
    # T = 256: sigma 32, the two centre entries (half a pixel off the centre) are the maximum; the corner to fp32 rounding
    corner = np.exp(-0.5 * (127.5 / 32.0) ** 2) / np.exp(-0.5 * (0.5 / 32.0) ** 2)
    assert abs(float(infer.blend_window(256)[0]) - corner) <= corner * 2.0 ** -24
    with pytest.raises(ValueError):
        infer.blend_window(16, "hann")
    with pytest.raises(ValueError):
        infer.blend_window(0)


def test_tile_grid_checks_coverage_and_codes_on_the_host():
    from cmunet_amd import ops
    g = ops.TileGrid(37, 29, 16, 16, [0, 8, 16, 21], [0, 8, 13], range(8), device="cpu")
    assert (g.ny, g.nx, g.A, g.per_image, g.transposes) == (4, 3, 8, 96, True)
    assert g.tile_codes(2).tolist() == list(range(8)) * 24
    assert ops.uncovered([0, 8, 16, 21], 16, 37) is None and ops.uncovered([0, 17], 16, 33) == 16 and ops.uncovered([1], 16, 17) == 0
    ops.TileGrid(11, 40, 16, 16, [0], [0, 12, 24], device="cpu")                        # H < T: the padded canvas
    bad = {
        "a gap between two tiles": lambda: ops.TileGrid(40, 16, 16, 16, [0, 17], [0], device="cpu"),
        "the last rows uncovered": lambda: ops.TileGrid(40, 16, 16, 16, [0, 16], [0], device="cpu"),
        "the first column uncovered": lambda: ops.TileGrid(16, 17, 16, 16, [0], [1], device="cpu"),
        "a start past the canvas": lambda: ops.TileGrid(16, 16, 16, 16, [0], [0, 1], device="cpu"),
        "a negative start": lambda: ops.TileGrid(16, 16, 16, 16, [-1, 0], [0], device="cpu"),
        "unordered starts": lambda: ops.TileGrid(40, 16, 16, 16, [8, 0, 24], [0], device="cpu"),
        "no starts": lambda: ops.TileGrid(16, 16, 16, 16, [], [0], device="cpu"),
        "code 8": lambda: ops.TileGrid(16, 16, 16, 16, [0], [0], [0, 8], device="cpu"),
        "a repeated code": lambda: ops.TileGrid(16, 16, 16, 16, [0], [0], [1, 1], device="cpu"),
        "no codes": lambda: ops.TileGrid(16, 16, 16, 16, [0], [0], [], device="cpu"),
        "a transposing code on a 5 x 7 tile": lambda: ops.TileGrid(5, 7, 5, 7, [0], [0], [0, 4], device="cpu"),
        "a zero tile": lambda: ops.TileGrid(5, 7, 0, 7, [0], [0], device="cpu"),
    }
    for name, fn in bad.items():
        with pytest.raises(ValueError):
            fn()
            pytest.fail(name)


def test_segmenter_checks_its_new_arguments():
    from cmunet_amd import infer
    from cmunet_amd.model import UNet
    net = UNet(base_ch=4, depth=5)
    s = infer.Segmenter(net, size=None, tile=256)
    assert (s.tile, s.stride, s.window, s.pad, s.codes, s.tiled) == (256, 128, "gaussian", "reflect", None, True)
    assert infer.Segmenter(net, tta="flips").codes == [0, 1, 2, 3] and infer.Segmenter(net, tta="d4").codes == list(range(8))
    assert infer.Segmenter(net, tta=[0, 5]).codes == [0, 5] and infer.Segmenter(net, tile=32, stride=32).stride == 32
    d = infer.Segmenter(net)
    assert (d.tile, d.stride, d.codes, d.tiled) == (None, None, None, False)
    bad = [dict(tile=250), dict(tile=0), dict(tile=-16), dict(stride=8), dict(tile=32, stride=0), dict(tile=32, stride=33),
           dict(tile=32, window="hann"), dict(tile=32, pad="edge"), dict(tta="rot"), dict(tta=[0, 0]), dict(tta=[8]), dict(tta=[])]
    for kw in bad:
        with pytest.raises(ValueError):
            infer.Segmenter(net, **kw)
            pytest.fail(str(kw))
    with pytest.raises(ValueError, match="multiple of 16"):
        infer.Segmenter(net, tile=250)
    with pytest.raises(ValueError, match="prob_class"):
        infer.Segmenter(net, tile=32).segment([torch.zeros(16, 16)], prob_class=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        infer.Segmenter(net, size=None, tile=32).segment([torch.zeros(19, 23)])


def test_predict_probs_has_no_cpu_fallback_and_checks_its_arguments():
    from cmunet_amd.model import UNet
    m = UNet(base_ch=8, depth=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_probs(torch.zeros(1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_probs(torch.zeros(2, 16, 16), codes=[0, 7])
    with pytest.raises(ValueError, match=r"\(B,H,W\)"):
        m.predict_probs(torch.zeros(1, 1, 16, 16))
    for codes in ([0], [0, 1, 2], [0, 8], [-1, 0]):
        with pytest.raises(ValueError, match="codes"):
            m.predict_probs(torch.zeros(2, 16, 16), codes=codes)
    with pytest.raises(ValueError, match="square"):
        m.predict_probs(torch.zeros(2, 16, 24), codes=[0, 4])
    with pytest.raises(ValueError, match="uint8"):
        m.predict_probs(torch.zeros(2, 16, 16), codes=torch.zeros(2, dtype=torch.int32))
    assert m.training      # nothing above flipped the mode


def test_cli_help_lists_the_new_flags():
    r = subprocess.run([sys.executable, "-m", "cmunet_amd.infer", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for flag in ("--tile", "--stride", "--window", "--pad", "--tta", "--size", "--batch", "--threshold"):
        assert flag in r.stdout
    for word in ("gaussian", "uniform", "reflect", "zero", "flips", "d4"):
        assert word in r.stdout


def test_header_binding_and_docs_agree_on_the_new_entry_points():
    from cmunet_amd import _lib
    import test_cpu_abi as abi
    protos = abi.header_prototypes()
    for name, n in (("cmu_extract_tiles", 16), ("cmu_head_probs", 16), ("cmu_blend_tiles", 20)):
        assert protos[name] == n == len(_lib._SIGS[name][1]), name
    abi.test_docs_state_the_header_entry_point_count()
