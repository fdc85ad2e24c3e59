"""Tiled prediction on the GPU: cmu_extract_tiles / cmu_head_probs / cmu_blend_tiles (csrc/tiled_predict.hip), UNet.predict_probs and
the tiled / test-time-augmented Segmenter, against the numpy restatement tests/tiled_predict_ref.py.

1. extract_tiles: a copy, compared bit for bit (both source types, both pad modes, all codes, padded and one-pixel images).
2. head_probs: every plane within 16 U absolute (U = 2^-24: the bound and the constant C_GRAD of tests/test_gpu_predict.py) of the float64
   softmax / sigmoid of the fp32 logits ops.conv1x1_head_fwd writes for the same arguments; for every code the planes are the code-0
   planes moved by the inverse view, bitwise; one case past the kernel's block cap.
3. blend_tiles on exact data (probabilities multiples of 1/8, windows from {1, 1/2, 1/4}: every sum exact in fp32 in any order): labels
   equal to the integer restatement, ties and a pixel on the threshold included, the probability plane equal to float32(num / den).
4. The whole path on a small model against the float64 blend of the fp32 logits model.eval() returns for each tile view: blended
   probability within (16 + 2 n + 4) U (16 U per softmax as in 2, two fp32 sums of n positive terms -- numerator and denominator,
   n = the largest number of (tile, copy) pairs over a pixel, each term's product and add one rounding of a sum that never exceeds
   its final value -- and a division with the window's float32 products: 4 U), labels equal wherever the float64 margin exceeds twice
   that bound, at most 1 % of the pixels excluded; repeatable bits; one whole-image tile == predict_probs.
5. Segmenter / segment_files / the command line against the hand-written composition; the untiled path unchanged; a pending training
   step undisturbed.
6. Argument errors: CmuError / ValueError, nothing launched.

The worst error / bound per kind is printed, and written to the file named by CMU_TILED_PARITY_OUT when that is set
(profiles/tiled_predict_parity.txt holds one such run)."""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tiled_predict_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
C_GRAD = 16
DEV = "cuda"
DTS = ("f32", "f16", "bf16")
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
EPC = {"f32": 4, "f16": 8, "bf16": 8}
LUT = [7, 200, 13, 255, 0, 99, 1, 42]
SENT = 777.0
RATIOS = {}
# the launch geometry of head_probs_kernel, restated: 256 lanes, C / epc lanes per pixel, four pixels per lane group and trip, at most
# 8192 blocks
CAP, LANES, UNROLL = 8192, 256, 4


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), ratio)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    yield o
    lines = [f"{k}: worst error / bound = {r:.4f}" for k, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    out = os.environ.get("CMU_TILED_PARITY_OUT")
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tests/test_gpu_tiled_predict.py: worst absolute error against float64 as a fraction of its bound (U = 2^-24):\n"
                    f"# head_probs planes: {C_GRAD} U; blended probability of the whole path: (16 + 2 n + 4) U, n = (tile, copy) pairs over a\n"
                    "# pixel; 'excluded': share of pixels whose float64 margin is below twice the bound, as a fraction of the 1 % allowed.\n"
                    "# extract_tiles, the inverse views and blend_tiles on exact data are compared bit for bit.\n")
            f.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------------------------------
# 1. extract_tiles
# ---------------------------------------------------------------------------------------------------
EXTRACT_CASES = [        # (H, W), (TH, TW), ystarts, xstarts, codes
    ((11, 40), (16, 16), [0], [0, 12, 24], range(8)),                  # H < T: padded rows
    ((37, 29), (16, 16), [0, 8, 16, 21], [0, 8, 13], range(8)),
    ((5, 7), (5, 7), [0], [0], range(4)),                              # a rectangular tile, TW % 4 != 0: the scalar store path
    ((1, 9), (4, 4), [0], [0, 4, 5], range(8)),                        # a one-pixel-high image: L = 1 under reflect
    ((9, 3), (8, 12), [0, 1], [0], range(4)),                          # W < TW, a pad wider than the image (two folds)
]


@pytest.mark.parametrize("pad", ["zero", "reflect"])
@pytest.mark.parametrize("src_dt", ["f32", "u8"])
def test_extract_tiles_is_bit_exact(ops, src_dt, pad):
    g = torch.Generator().manual_seed(3)
    for (H, W), (TH, TW), ys, xs, codes in EXTRACT_CASES:
        N = 2
        src = torch.randn(N, H, W, generator=g) if src_dt == "f32" else torch.randint(0, 256, (N, H, W), generator=g).to(torch.uint8)
        grid = ops.TileGrid(H, W, TH, TW, ys, xs, list(codes), DEV)
        out = torch.full((N * grid.per_image, TH, TW), SENT, device=DEV)
        ops.extract_tiles(src.to(DEV), grid, pad, out)
        want = R.extract_tiles(src.numpy(), ys, xs, list(codes), TH, TW, pad)
        got = out.cpu().numpy()
        assert not (got == SENT).any(), "an element was not written"
        assert got.dtype == np.float32 and np.array_equal(got, want), (src_dt, pad, (H, W), (TH, TW))
        if pad == "zero" and (H < TH or W < TW):
            assert (want == 0).any()


# ---------------------------------------------------------------------------------------------------
# 2. head_probs
# ---------------------------------------------------------------------------------------------------
def make_act(ops, x, dt, view, scale=None, shift=None):
    """(B,H,W,C) CPU values -> Act on the GPU; ``view``: channels [epc, epc + C) of a buffer 2 epc wider, the rest a sentinel."""
    B, H, W, C = x.shape
    pad = EPC[dt] if view else 0
    buf = torch.full((B, H, W, C + 2 * pad), SENT, dtype=TORCH_DT[dt], device=DEV)
    buf[..., pad:pad + C] = x.to(DEV)
    return ops.Act(buf, pad, C, None if scale is None else scale.to(DEV), None if shift is None else shift.to(DEV))


def probs64(logits):
    l = logits.double()
    return torch.sigmoid(l) if l.shape[1] == 1 else torch.softmax(l, 1)


def run_probs(ops, act, w, b, codes=None, transposes=False):
    K = w.shape[0]
    probs = torch.full((act.B, max(K, 1), act.H, act.W), -1.0, device=DEV)
    ops.head_probs(act, w.to(DEV), b.to(DEV), probs, None if codes is None else torch.tensor(codes, dtype=torch.uint8, device=DEV), transposes)
    return probs


@pytest.mark.parametrize("bias_mode", ["plain", "+100", "-100"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("dt", DTS)
def test_head_probs_vs_fp64_of_the_logits_path(ops, dt, K, bias_mode):
    e = EPC[dt]
    for ci, (C, shape, tf, view) in enumerate(itertools.product((e, 64), [(3, 5, 7), (2, 16, 24)], (False, True), (False, True))):
        g = torch.Generator().manual_seed(7 * K + 100 * ci + len(bias_mode))
        B, H, W = shape
        x = torch.randn(B, H, W, C, generator=g).to(TORCH_DT[dt]).float()
        sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        w, b = torch.randn(K, C, generator=g) / math.sqrt(C), torch.randn(K, generator=g) * 0.2
        if bias_mode != "plain":          # saturated: the probabilities are 0 and 1 to fp32
            b[0] += 100.0 if bias_mode == "+100" else -100.0
            if K > 1:
                b[1] -= 100.0 if bias_mode == "+100" else -100.0
        act = make_act(ops, x, dt, view, sc if tf else None, sh if tf else None)
        logits = torch.empty(B, K, H, W, device=DEV)
        ops.conv1x1_head_fwd(act, w.to(DEV), b.to(DEV), logits)
        if bias_mode != "plain":
            assert float(logits[:, 0].abs().min()) > 90.0
        got = run_probs(ops, act, w, b)
        assert not bool((got == -1.0).any()), "an element was not written"
        err = (got.double() - probs64(logits)).abs().max().item()
        note(f"head_probs K={K} {bias_mode}", err / (C_GRAD * U))
        assert err <= C_GRAD * U, (dt, C, K, shape, tf, view, err / U)
        # the same arithmetic as the label head's one probability, not a second version of it: bitwise
        labels = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
        for pc in range(max(K, 1)):
            one = torch.full((B, H, W), -1.0, device=DEV)
            ops.head_predict(act, w.to(DEV), b.to(DEV), labels, one, pc)
            assert torch.equal(got[:, pc], one), (dt, C, K, shape, tf, view, pc)
        if K > 1:       # the planes of one pixel sum to one within their own bounds
            assert float((got.double().sum(1) - 1.0).abs().max()) <= K * C_GRAD * U


@pytest.mark.parametrize("dt", DTS)
def test_head_probs_stores_the_inverse_view_bitwise(ops, dt):
    e = EPC[dt]
    g = torch.Generator().manual_seed(21)
    for (H, W), codes, C, K in [((8, 8), list(range(8)), e, 3), ((8, 8), list(range(8)), 64, 2), ((8, 8), [7, 6, 5, 4, 3, 2, 1, 0], 4 * e, 1),
                                ((5, 7), [0, 1, 2, 3], e, 8), ((5, 7), [3, 2, 1, 0], 64, 2)]:
        B = len(codes)
        x = torch.randn(B, H, W, C, generator=g).to(TORCH_DT[dt]).float()
        sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        w, b = torch.randn(K, C, generator=g) / math.sqrt(C), torch.randn(K, generator=g) * 0.2
        act = make_act(ops, x, dt, True, sc, sh)
        base = run_probs(ops, act, w, b).cpu().numpy()
        assert np.array_equal(base, run_probs(ops, act, w, b, [0] * B).cpu().numpy())
        got = run_probs(ops, act, w, b, codes, transposes=any(c & 4 for c in codes)).cpu().numpy()
        assert not (got == -1.0).any()
        for t, code in enumerate(codes):
            assert np.array_equal(got[t], R.inverse_view(base[t], code)), (dt, (H, W), code)
        assert any(not np.array_equal(got[t], base[t]) for t, code in enumerate(codes) if code)


def test_head_probs_past_the_block_cap(ops):
    """More pixels than one full grid covers at the smallest channel count (one 16-byte chunk per pixel: 256 pixels x 4 per block
    and trip, 8192 blocks = 8,388,608 pixels): 2897 x 2897 = 8,392,609, so blocks 0..3 take a second trip and the last lane group of
    the tensor holds one pixel.  Both flips: a slip in the second trip's indices moves planes."""
    dt, K, S = "f32", 2, 2897
    C = EPC[dt]
    assert S * S > CAP * (LANES // 1) * UNROLL and (S * S) % UNROLL == 1
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, S, S, C, generator=g)
    w, b = torch.randn(K, C, generator=g) / math.sqrt(C), torch.randn(K, generator=g) * 0.2
    act = make_act(ops, x, dt, False)
    logits = torch.empty(1, K, S, S, device=DEV)
    ops.conv1x1_head_fwd(act, w.to(DEV), b.to(DEV), logits)
    got = run_probs(ops, act, w, b, [3])
    want = torch.flip(probs64(logits), dims=[-1, -2])
    err = (got.double() - want).abs().max().item()
    note("head_probs past the block cap", err / (C_GRAD * U))
    assert err <= C_GRAD * U, err / U


# ---------------------------------------------------------------------------------------------------
# 3. blend_tiles on exact data
# ---------------------------------------------------------------------------------------------------
BLEND_GRIDS = [        # N, (H, W), (TH, TW), ystarts, xstarts, A
    (1, (37, 29), (16, 16), [0, 13, 21], [0, 13], 4),                   # ny x nx x A = 3 x 2 x 4
    (1, (11, 40), (16, 16), [0], [0, 12, 24], 1),                       # 1 x 3 x 1, padded rows never read
    (2, (17, 16), (16, 16), [0, 1], [0], 2),                            # the clamped last tile overlaps its neighbour by T - 1
    (3, (20, 23), (8, 12), [0, 4, 8, 12], [0, 6, 11], 3),               # N = 3 images, a rectangular tile
]


def exact_window(g, T):
    return torch.tensor([1.0, 0.5, 0.25])[torch.randint(0, 3, (T,), generator=g)]


def run_blend(ops, probs, N, H, W, TH, TW, ys, xs, A, wy, wx, lut, pc, thr):
    KP = probs.shape[1]
    grid = ops.TileGrid(H, W, TH, TW, ys, xs, list(range(A)), DEV)
    labels = torch.full((N, H, W), 251, dtype=torch.uint8, device=DEV)
    prob = torch.full((N, H, W), -1.0, device=DEV)
    lut_t = torch.tensor(LUT[:max(KP, 2)], dtype=torch.uint8, device=DEV) if lut else None
    ops.blend_tiles(probs.to(DEV).contiguous(), grid, wy.to(DEV), wx.to(DEV), labels, prob, pc, thr, lut_t)
    return labels.cpu().numpy(), prob.cpu().numpy()


def check_blend(ops, probs, N, H, W, TH, TW, ys, xs, A, wy, wx, lut, tag):
    """probs: (n, K', TH, TW) float32 multiples of 1/8; windows from {1, 1/2, 1/4}: num in units of 1/128, exactly, as integers."""
    KP = probs.shape[1]
    num, den = R.blend(probs.numpy(), N, H, W, ys, xs, A, wy.numpy(), wx.numpy())
    n128, d16 = np.rint(num * 128).astype(np.int64), np.rint(den * 16).astype(np.int64)
    assert np.array_equal(n128 / 128.0, num) and np.array_equal(d16 / 16.0, den) and d16.min() > 0
    vals = np.array(LUT[:max(KP, 2)] if lut else list(range(max(KP, 2))), np.uint8)
    for pc in sorted({0, KP - 1}):
        thr = 0.5
        if KP == 1:      # the blended probability of one of the pixels, exactly: that pixel sits on the threshold -> label 0
            q = np.float32(num[0, 0, H // 2, W // 2] / den[0, H // 2, W // 2])
            thr = float(q)
            want = vals[((num[:, 0] / den).astype(np.float32) > np.float32(thr)).astype(np.int64)]
            assert want[0, H // 2, W // 2] == vals[0]
        else:
            want = vals[np.argmax(n128, axis=1)]      # integers: the first maximum
        got, prob = run_blend(ops, probs, N, H, W, TH, TW, ys, xs, A, wy, wx, lut, pc, thr)
        assert np.array_equal(got, want), (tag, KP, pc)
        assert np.array_equal(prob, (num[:, pc] / den).astype(np.float32)), (tag, KP, pc)
    return n128


@pytest.mark.parametrize("KP", [1, 2, 3, 8])
def test_blend_tiles_exact_random_eighths(ops, KP):
    g = torch.Generator().manual_seed(40 + KP)
    ties = 0
    for gi, (N, (H, W), (TH, TW), ys, xs, A) in enumerate(BLEND_GRIDS):
        n = N * len(ys) * len(xs) * A
        probs = torch.randint(0, 9, (n, KP, TH, TW), generator=g).float() / 8.0
        if KP > 1:      # built-in ties: classes 0 and 1 equal on half of every tile, and the largest there
            probs[:, 1, :, : TW // 2] = probs[:, 0, :, : TW // 2] = 1.0
        wy, wx = exact_window(g, TH), exact_window(g, TW)
        n128 = check_blend(ops, probs, N, H, W, TH, TW, ys, xs, A, wy, wx, lut=bool(gi % 2), tag=gi)
        if KP > 1:
            ties += int(((n128 == n128.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert KP == 1 or ties > 0, "the tie cases hold no tie"


@pytest.mark.parametrize("KP", [2, 3, 8])
def test_blend_tiles_reads_the_right_pixel_of_the_right_tile(ops, KP):
    """The canvas coordinate is in the data: every tile's planes are one-hot in hash(img, y, x) % K' of the CANVAS pixel they lie on,
    so the blend must give that class back at every pixel; a slip in an offset, a start or a tile index changes labels."""
    g = torch.Generator().manual_seed(50 + KP)
    for gi, (N, (H, W), (TH, TW), ys, xs, A) in enumerate(BLEND_GRIDS):
        Hp, Wp = max(H, TH), max(W, TW)
        yy, xx = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
        n = N * len(ys) * len(xs) * A
        probs = np.zeros((n, KP, TH, TW), np.float32)
        want = np.zeros((N, H, W), np.uint8)
        for img in range(N):
            cls = ((yy * 7919 + xx * 104729 + img * 31 + (yy * xx) % 13) % KP)
            want[img] = cls[:H, :W]
            for iy, y0 in enumerate(ys):
                for ix, x0 in enumerate(xs):
                    for a in range(A):
                        t = ((img * len(ys) + iy) * len(xs) + ix) * A + a
                        c = cls[y0:y0 + TH, x0:x0 + TW]
                        probs[t] = (np.arange(KP)[:, None, None] == c[None]).astype(np.float32)
        wy, wx = exact_window(g, TH), exact_window(g, TW)
        got, prob = run_blend(ops, torch.from_numpy(probs), N, H, W, TH, TW, ys, xs, A, wy, wx, False, KP - 1, 0.5)
        assert np.array_equal(got, want), gi
        assert np.array_equal(prob, (want == KP - 1).astype(np.float32)), gi
        assert len(np.unique(want)) == KP


# ---------------------------------------------------------------------------------------------------
# 4. the whole path on a small model
# ---------------------------------------------------------------------------------------------------
IMAGES = [(37, 29), (11, 40)]
T = 16
BATCH = 32


def small_net(K, dt, seed=0):
    """UNet(base 8, depth 3) in eval mode with random BatchNorm statistics and affine parameters."""
    from cmunet_amd.model import UNet
    torch.manual_seed(100 * seed + K)
    net = UNet(out_classes=K, base_ch=8, depth=3, dtype=dt)
    g = torch.Generator().manual_seed(seed + 17 * K)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    return net.to(DEV).eval()


def eval_logits(net, tiles):
    """fp32 logits of model.eval() for a stack of tile views, in the network batches the Segmenter uses."""
    out = []
    with torch.no_grad():
        for c0 in range(0, tiles.shape[0], BATCH):
            out.append(net(tiles[c0:c0 + BATCH].contiguous()))
    return torch.cat(out)


def spread_the_head(net, images, K):
    """Rescale and re-centre the head on the tests' own tiles so that no class wins everywhere: unit spread per class, medians
    aligned (an unscaled random head puts nearly every pixel in one class)."""
    views = []
    for im in images:
        H, W = im.shape
        ys, xs = R.tile_starts(H, T, 8), R.tile_starts(W, T, 8)
        views.append(R.extract_tiles(im.numpy()[None], ys, xs, [0], T, T, "reflect"))
    lo = eval_logits(net, torch.from_numpy(np.concatenate(views)).to(DEV))
    flat = lo.transpose(0, 1).reshape(K, -1)
    with torch.no_grad():
        s = 2.0 / flat.std(1).clamp_min(1e-6)
        net.conv_last.weight.mul_(s.view(K, 1, 1, 1))
        net.conv_last.bias.copy_((net.conv_last.bias - flat.median(1).values) * s)
    torch.cuda.synchronize()


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("dt", DTS)
def test_whole_path_vs_fp64_blend_of_the_eval_logits(ops, dt, K):
    from cmunet_amd import infer
    net = small_net(K, dt)
    g = torch.Generator().manual_seed(9)
    images = [torch.randn(*s, generator=g) for s in IMAGES]
    spread_the_head(net, images, K)
    KP = max(K, 1)
    worst, worst_excl = 0.0, 0.0
    shares = np.zeros(max(K, 2))
    for im, stride, kind, tta in itertools.product(images, (8, 12), ("uniform", "gaussian"), (None, "d4")):
        H, W = im.shape
        codes = list(range(8)) if tta else [0]
        ys, xs = R.tile_starts(H, T, stride), R.tile_starts(W, T, stride)
        num, den = R.pipeline(im.numpy()[None], lambda t: eval_logits(net, torch.from_numpy(t).to(DEV)).cpu().numpy(), T, T, ys, xs,
                              codes, kind, "reflect")
        p64 = num[0] / den[0]
        n = R.cover_count(H, W, ys, xs, len(codes), T, T)
        assert n <= 72
        bound = (16 + 2 * n + 4) * U
        seg = infer.Segmenter(net, size=None, batch=BATCH, tile=T, stride=stride, window=kind, pad="reflect", tta=tta)
        got = [seg.segment([im], prob_class=k)[0] for k in range(KP)]
        again = seg.segment([im], prob_class=KP - 1)[0]
        assert torch.equal(again[0], got[KP - 1][0]) and torch.equal(again[1], got[KP - 1][1]), "two calls differ"
        for k in range(KP):
            mask, prob = got[k]
            assert tuple(mask.shape) == (H, W) == tuple(prob.shape) and mask.dtype == torch.uint8 and prob.dtype == torch.float32
            assert torch.equal(mask, got[0][0])
            err = np.abs(prob.double().cpu().numpy() - p64[k]).max()
            worst = max(worst, err / bound)
            assert err <= bound, (dt, K, (H, W), stride, kind, tta, k, err / U, n)
        if K == 1:
            want, margin = (p64[0] > 0.5).astype(np.uint8), np.abs(p64[0] - 0.5)
        else:
            srt = np.sort(p64, axis=0)
            want, margin = np.argmax(p64, axis=0).astype(np.uint8), srt[-1] - srt[-2]
        sure = margin > 2 * bound
        excl = 1.0 - sure.mean()
        worst_excl = max(worst_excl, excl)
        assert excl <= 0.01, (dt, K, (H, W), stride, kind, tta, excl)
        assert np.array_equal(got[0][0].cpu().numpy()[sure], want[sure]), (dt, K, (H, W), stride, kind, tta)
        shares += np.bincount(want.reshape(-1), minlength=max(K, 2)) / want.size
    shares /= len(IMAGES) * 2 * 2 * 2
    assert shares.min() >= 0.05, f"a class holds under 5 % of the pixels: {shares}"
    note(f"whole path {dt} K={K}: blended probability", worst)
    note(f"whole path {dt} K={K}: excluded share / 1 %", worst_excl / 0.01)


@pytest.mark.parametrize("K", [1, 3])
def test_one_whole_image_tile_is_predict_probs(ops, K):
    from cmunet_amd import infer
    net = small_net(K, "f16", seed=2)
    g = torch.Generator().manual_seed(4)
    im = torch.randn(16, 24, generator=g)
    probs = net.predict_probs(im.to(DEV)[None])
    assert tuple(probs.shape) == (1, max(K, 1), 16, 24)
    with torch.no_grad():
        want = probs64(net(im.to(DEV)[None]))
    assert float((probs.double() - want).abs().max()) <= C_GRAD * U
    im2 = torch.randn(16, 16, generator=g)
    p2 = net.predict_probs(im2.to(DEV)[None])
    seg = infer.Segmenter(net, size=None, tile=16, window="uniform")
    for k in range(max(K, 1)):
        assert torch.equal(seg.segment([im2], prob_class=k)[0][1], p2[0, k])
    # predict_probs in an augmented view: the planes come back in the image's frame
    views = torch.from_numpy(np.stack([R.view(im2.numpy(), c).copy() for c in range(8)])).to(DEV)
    back = net.predict_probs(views, codes=list(range(8)))
    plain = net.predict_probs(views)
    for c in range(8):
        assert np.array_equal(back[c].cpu().numpy(), R.inverse_view(plain[c].cpu().numpy(), c)), c
    # tta without tile: every image one tile of its own size; transposing codes need a square image
    assert len(infer.Segmenter(net, size=None, tta="flips").segment([im])) == 1
    with pytest.raises(ValueError, match="square"):
        infer.Segmenter(net, size=None, tta="d4").segment([im])


# ---------------------------------------------------------------------------------------------------
# 5. Segmenter, segment_files, the command line
# ---------------------------------------------------------------------------------------------------
def compose(ops, net, src, size, tile, stride, kind, pad, codes, lut, threshold=0.5):
    """The tiled Segmenter chunk written out with the three ops: src (1,H,W) on the device -> mask (H,W)."""
    from cmunet_amd import infer
    H, W = src.shape[1:]
    x = src if size is None else ops.resize_bicubic(src, size, size)
    h, w = x.shape[1:]
    grid = ops.TileGrid(h, w, tile, tile, infer.tile_starts(h, tile, stride), infer.tile_starts(w, tile, stride), codes or [0], DEV)
    tiles = ops.extract_tiles(x.contiguous(), grid, pad)
    K = net.conv_last.weight.shape[0]
    probs = torch.empty(tiles.shape[0], max(K, 1), tile, tile, device=DEV)
    tc = grid.tile_codes(1)
    for c0 in range(0, tiles.shape[0], BATCH):
        probs[c0:c0 + BATCH] = net.predict_probs(tiles[c0:c0 + BATCH], tc[c0:c0 + BATCH] if codes else None)
    labels = torch.empty(1, h, w, dtype=torch.uint8, device=DEV)
    ops.blend_tiles(probs, grid, infer.blend_window(tile, kind).to(DEV), infer.blend_window(tile, kind).to(DEV), labels, None, 0, threshold, lut)
    return (labels if (h, w) == (H, W) else ops.resize_nearest(labels, H, W))[0]


def test_segmenter_tiled_against_the_composition_files_and_cli(ops, tmp_path):
    from cmunet_amd import infer
    net = small_net(2, "f32", seed=5)
    g = torch.Generator().manual_seed(2)
    images = [torch.randn(59, 59, generator=g), torch.randn(37, 29, generator=g), (torch.rand(59, 59, generator=g) * 255.0).to(torch.uint8),
              torch.randn(11, 40, generator=g).numpy(), torch.randn(37, 29, generator=g).to(DEV)]
    spread_the_head(net, images[:2], 2)
    assert 59 % 4, "the stand-in for 475: not a multiple of 2**(depth-1)"
    vals = [0, 255]
    lut = torch.tensor(vals, dtype=torch.uint8, device=DEV)
    kw = dict(size=None, batch=BATCH, class_values=vals, tile=T, stride=8, window="gaussian", pad="reflect", tta="d4")
    seg = infer.Segmenter(net, **kw)
    masks = seg.segment(images)
    assert len(masks) == len(images)
    for im, m in zip(images, masks):
        src = (im if torch.is_tensor(im) else torch.from_numpy(im)).to(DEV)[None].contiguous()
        assert m.is_cuda and m.dtype == torch.uint8 and tuple(m.shape) == tuple(src.shape[1:])
        assert torch.equal(m, compose(ops, net, src, None, T, 8, "gaussian", "reflect", list(range(8)), lut))
    assert any(0 < int((m == 255).sum()) < m.numel() for m in masks)
    # resize first, then tile; zero padding; no augmentation; a small probability budget changes nothing (groups of one image)
    seg2 = infer.Segmenter(net, size=24, batch=5, class_values=vals, tile=T, stride=12, window="uniform", pad="zero")
    m2 = seg2.segment(images[:3])
    for im, m in zip(images[:3], m2):
        src = im.to(DEV)[None].contiguous()
        assert torch.equal(m, compose(ops, net, src, 24, T, 12, "uniform", "zero", None, lut))
    old = infer.PROB_BUDGET_BYTES
    try:
        infer.PROB_BUDGET_BYTES = 1
        small = infer.Segmenter(net, **kw).segment(images)
    finally:
        infer.PROB_BUDGET_BYTES = old
    assert all(torch.equal(a, b) for a, b in zip(small, masks))
    pairs = seg2.segment(images[:2], prob_class=1)
    assert tuple(pairs[0][1].shape) == (24, 24) and tuple(pairs[0][0].shape) == (59, 59) and torch.equal(pairs[0][0], m2[0])
    # files and the command line (a fresh process)
    paths = []
    for i, im in enumerate(images):
        p = tmp_path / f"img{i}.npy"
        np.save(p, im.cpu().numpy() if torch.is_tensor(im) else im)
        paths.append(str(p))
    written = infer.segment_files(net, paths, str(tmp_path / "out"), **kw)
    assert [os.path.basename(w) for w in written] == [f"img{i}_mask.npy" for i in range(len(images))]
    for w, m in zip(written, masks):
        assert np.array_equal(np.load(w), m.cpu().numpy())
    torch.save(net.state_dict(), tmp_path / "state.pth")
    r = subprocess.run([sys.executable, "-m", "cmunet_amd.infer", "--model", str(tmp_path / "state.pth"), "--images", str(tmp_path),
                        "--out", str(tmp_path / "cli"), "--tile", str(T), "--stride", "8", "--tta", "d4", "--batch", str(BATCH)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = infer.Segmenter(net, size=None, batch=BATCH, tile=T, stride=8, tta="d4").segment(images)
    for i, m in enumerate(plain):      # --tile without --size: native resolution
        assert np.array_equal(np.load(tmp_path / "cli" / f"img{i}_mask.npy"), m.cpu().numpy())


def test_untiled_segmenter_is_unchanged(ops):
    from cmunet_amd import infer
    net = small_net(2, "f16", seed=6)
    g = torch.Generator().manual_seed(8)
    images = [torch.randn(37, 53, generator=g), (torch.rand(40, 64, generator=g) * 255.0).to(torch.uint8)]
    spread_the_head(net, [images[0]], 2)
    lut = torch.tensor([3, 9], dtype=torch.uint8, device=DEV)
    seg = infer.Segmenter(net, size=32, batch=2, class_values=[3, 9])
    assert not seg.tiled
    for im, m in zip(images, seg.segment(images)):
        src = im.to(DEV)[None].contiguous()
        x = ops.resize_bicubic(src, 32, 32).float()
        lab = net.predict(x, threshold=0.5, class_values=lut)
        assert torch.equal(m, ops.resize_nearest(lab, *src.shape[1:])[0])
    (mask, prob), = seg.segment(images[:1], prob_class=1)
    x = ops.resize_bicubic(images[0].to(DEV)[None].contiguous(), 32, 32)
    lab, p = net.predict(x, prob_class=1, class_values=lut)
    assert torch.equal(prob, p[0]) and torch.equal(mask, ops.resize_nearest(lab, 37, 53)[0])
    with pytest.raises(ValueError):
        infer.Segmenter(net, size=None).segment([images[0]])       # without tile, native sizes still need multiples of 4


@pytest.mark.parametrize("dt", DTS)
def test_tiled_call_between_forward_and_backward_leaves_the_step_alone(ops, dt):
    from cmunet_amd import infer
    from cmunet_amd.model import UNet
    torch.manual_seed(3)
    net = UNet(out_classes=2, base_ch=8, depth=3, dtype=dt).to(DEV).train()
    saved = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    xa, im = torch.randn(BATCH, T, T, generator=g).to(DEV), torch.randn(37, 29, generator=g)
    seg = infer.Segmenter(net, size=None, batch=BATCH, tile=T, stride=8, tta="flips")      # network calls of xa's own shape

    def step(with_call):
        net.load_state_dict(saved)
        net.train()
        net.zero_grad(set_to_none=True)
        logits = net(xa)
        if with_call:
            seg.segment([im], prob_class=1)
            assert net.training
        (logits * torch.linspace(-1, 1, logits.numel(), device=DEV).view_as(logits)).sum().backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in net.named_parameters()}, {k: v.clone() for k, v in net.state_dict().items()}

    g0, s0 = step(False)
    g1, s1 = step(True)
    assert all(v.abs().max() > 0 for n, v in g0.items() if n.endswith("weight"))
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


# ---------------------------------------------------------------------------------------------------
# 6. argument errors: nothing launched
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_bad_arguments_raise_and_launch_nothing(ops, dt):
    from cmunet_amd._lib import CmuError, call
    e = EPC[dt]
    C = 4 * e
    z = lambda *s: torch.zeros(*s, device=DEV)
    buf = torch.zeros(2, 4, 6, C + e, dtype=TORCH_DT[dt], device=DEV)
    good = ops.Act(buf, 0, C)
    probs = torch.full((2, 2, 4, 6), -1.0, device=DEV)
    codes = torch.zeros(2, dtype=torch.uint8, device=DEV)
    grid = ops.TileGrid(4, 6, 4, 6, [0], [0], [0, 1], DEV)
    src = z(1, 4, 6)
    tiles = torch.full((2, 4, 6), -1.0, device=DEV)
    labels = torch.full((1, 4, 6), 251, dtype=torch.uint8, device=DEV)
    prob = torch.full((1, 4, 6), -1.0, device=DEV)
    ones = lambda n: torch.ones(n, device=DEV)
    p = ops._p
    st = ops._stream()
    cases = {
        "head_probs: K = 9": (CmuError, lambda: ops.head_probs(good, z(9, C), z(9), torch.full((2, 9, 4, 6), -1.0, device=DEV))),
        "head_probs: misaligned x": (CmuError, lambda: ops.head_probs(ops.Act(buf, 1, C), z(2, C), z(2), probs)),
        "head_probs: scale without shift": (CmuError, lambda: ops.head_probs(ops.Act(buf, 0, C, z(C) + 1, None), z(2, C), z(2), probs)),
        "head_probs: chunk count not a power of two": (CmuError, lambda: ops.head_probs(ops.Act(z(2, 4, 6, 3 * e).to(TORCH_DT[dt]), 0, 3 * e),
                                                                                      z(2, 3 * e), z(2), probs)),
        "head_probs: transposing codes on 4 x 6": (ValueError, lambda: ops.head_probs(good, z(2, C), z(2), probs, codes, True)),
        "head_probs: the same, at the C-ABI": (CmuError, lambda: call("cmu_head_probs", good.ptr(), good.ld, None, None, p(z(2, C)), p(z(2)),
                                                                     p(codes), 1, p(probs), 2, 4, 6, C, 2, good.dt, st)),
        "head_probs: allow_transpose without codes": (CmuError, lambda: call("cmu_head_probs", good.ptr(), good.ld, None, None, p(z(2, C)),
                                                                            p(z(2)), None, 1, p(probs), 2, 4, 4, C, 2, good.dt, st)),
        "extract_tiles: pad mode": (ValueError, lambda: ops.extract_tiles(src, grid, "edge", tiles)),
        "extract_tiles: int32 source": (ValueError, lambda: ops.extract_tiles(src.int(), grid, "zero", tiles)),
        "extract_tiles: pad_mode 2 at the C-ABI": (CmuError, lambda: call("cmu_extract_tiles", p(src), 0, 1, 4, 6, p(grid.ys_dev), 1, p(grid.xs_dev),
                                                                         1, p(grid.codes_dev), 2, 4, 6, 2, p(tiles), st)),
        "extract_tiles: two copies without codes": (CmuError, lambda: call("cmu_extract_tiles", p(src), 0, 1, 4, 6, p(grid.ys_dev), 1,
                                                                          p(grid.xs_dev), 1, None, 2, 4, 6, 0, p(tiles), st)),
        "extract_tiles: no tiles": (CmuError, lambda: call("cmu_extract_tiles", p(src), 0, 1, 4, 6, p(grid.ys_dev), 0, p(grid.xs_dev), 1,
                                                          p(grid.codes_dev), 2, 4, 6, 0, p(tiles), st)),
        "blend_tiles: prob_class = K": (CmuError, lambda: ops.blend_tiles(probs, grid, ones(4), ones(6), labels, prob, 2)),
        "blend_tiles: prob_class < 0": (CmuError, lambda: ops.blend_tiles(probs, grid, ones(4), ones(6), labels, prob, -1)),
        "blend_tiles: K = 9": (CmuError, lambda: ops.blend_tiles(torch.full((2, 9, 4, 6), -1.0, device=DEV), grid, ones(4), ones(6), labels, prob)),
        "blend_tiles: no window": (CmuError, lambda: call("cmu_blend_tiles", p(probs), 1, 4, 6, p(grid.ys_dev), 1, p(grid.xs_dev), 1, 2, 4, 6, 2,
                                                         None, p(ones(6)), 0.5, None, p(labels), p(prob), 0, st)),
        "an uncovered pixel": (ValueError, lambda: ops.TileGrid(9, 6, 4, 6, [0, 5], [0], [0], DEV)),
    }
    for name, (exc, fn) in cases.items():
        with pytest.raises(exc):
            fn()
            pytest.fail(name)
        torch.cuda.synchronize()
        assert bool((probs == -1.0).all()) and bool((tiles == -1.0).all()) and bool((labels == 251).all()) and bool((prob == -1.0).all()), name
    # the same arguments, valid: they do launch
    ops.extract_tiles(src, grid, "zero", tiles)
    ops.head_probs(good, z(2, C), z(2), probs, codes)
    ops.blend_tiles(probs, grid, ones(4), ones(6), labels, prob, 1)
    torch.cuda.synchronize()
    assert bool((tiles == 0).all()) and bool((probs == 0.5).all()) and bool((labels == 0).all()) and bool((prob == 0.5).all())
