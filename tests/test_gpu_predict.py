"""The fused prediction head (cmu_head_predict, csrc/predict.hip), UNet.predict and cmunet_amd.infer on the GPU.

1. Exact integer data at the ops level against numpy int64: no tolerance.  Activations are integers in [-4, 4] (exact in bf16), scales
   from {0.5, 1, 2}, integer shifts, integer weights in [-3, 3], integer biases: every logit is an exact multiple of 1/2 far below
   2^24 in any summation order, so the label is decided by integer arithmetic (computed here in units of 1/2).
2. Seeded float data at the ops level: labels == argmax of the logits ops.conv1x1_head_fwd writes for the same arguments (the kernel
   restates that head's arithmetic bit for bit), one-channel labels == logits > float32(log(t / (1 - t))), and the probability within
   16 U absolute (U = 2^-24; the project's constant C_GRAD = 16 of tests/test_gpu_pointwise_losses_fp64.py, which books "an fp32 exp,
   a sum of K <= 8 terms and a division" at under 12 U) of the float64 softmax / sigmoid of those fp32 logits; with the maximum
   subtracted every term is at most 1 and carries a few U whatever the logit range (logits of +-100 included).
3. Model level: UNet.predict against net.eval()(x).argmax(1), in both modes, the state untouched, a training step undisturbed.
4. Segmenter / segment_files / load_segmentation_model against the hand-written composition of the existing ops.
5. Argument errors: CmuError, nothing launched.

The worst probability error / bound is printed, and written to the file named by CMU_PREDICT_PARITY_OUT when that is set
(profiles/predict_parity.txt holds one such run)."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_GRAD = 16
DEV = "cuda"
DTS = ("f32", "f16", "bf16")
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
EPC = {"f32": 4, "f16": 8, "bf16": 8}
LUT = [7, 200, 13, 255, 0, 99, 1, 42]
SENT = 777.0
RATIOS = {}
# the launch geometry of csrc/predict.hip, restated: 256 lanes, C / epc lanes per pixel, four consecutive pixels per lane group and trip,
# at most 8192 blocks
CAP, LANES, UNROLL = 8192, 256, 4


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), ratio)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    yield o
    lines = [f"{k}: worst |prob - fp64| / ({C_GRAD} U) = {r:.4f}" for k, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    out = os.environ.get("CMU_PREDICT_PARITY_OUT")
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tests/test_gpu_predict.py: worst absolute error of the probability cmu_head_predict / UNet.predict writes against the\n"
                    f"# float64 softmax / sigmoid of the fp32 logits, as a fraction of the bound {C_GRAD} U (U = 2^-24); labels are compared exactly\n")
            f.write("\n".join(lines) + "\n")


def make_act(ops, x, dt, view, scale=None, shift=None):
    """(B,H,W,C) CPU values -> Act on the GPU; ``view``: channels [epc, epc + C) of a buffer 2 epc wider, the rest a sentinel."""
    B, H, W, C = x.shape
    pad = EPC[dt] if view else 0
    buf = torch.full((B, H, W, C + 2 * pad), SENT, dtype=TORCH_DT[dt], device=DEV)
    buf[..., pad:pad + C] = x.to(DEV)
    return ops.Act(buf, pad, C, None if scale is None else scale.to(DEV), None if shift is None else shift.to(DEV))


def run_predict(ops, act, w, b, K, lut, prob_class=None, thr=0.0):
    labels = torch.full((act.B, act.H, act.W), 251, dtype=torch.uint8, device=DEV)
    prob = torch.full((act.B, act.H, act.W), -1.0, device=DEV) if prob_class is not None else None
    lut_t = torch.tensor(LUT[:max(K, 2)], dtype=torch.uint8, device=DEV) if lut else None
    ops.head_predict(act, w.to(DEV), b.to(DEV), labels, prob, prob_class or 0, thr, lut_t)
    return labels.cpu(), None if prob is None else prob.cpu()


# ---------------------------------------------------------------------------------------------------
# 1. exact integer data
# ---------------------------------------------------------------------------------------------------
def int_case(g, shape, C, K, mode):
    B, H, W = shape
    x = torch.randint(-4, 5, (B, H, W, C), generator=g, dtype=torch.int8)
    sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    sh = torch.randint(-2, 3, (C,), generator=g).float()
    w = torch.randint(-3, 4, (K, C), generator=g).float()
    b = torch.randint(-5, 6, (K,), generator=g).float()
    if mode == "dup":            # two identical rows with equal biases: wherever they hold the maximum, the smaller index wins
        w[1], b[1] = w[0], b[0]
    elif mode == "zero":         # every logit equal: label 0 everywhere
        w.zero_()
        b.fill_(3.0)
    return x, sc, sh, w, b


def int_logits2(x, sc, sh, w, b, tf):
    """The logits in units of 1/2, in int64 (in slabs of pixels: the largest case holds 67 M activations)."""
    xi = x.numpy().reshape(-1, x.shape[-1])
    s2, h2 = (2 * sc.numpy()).astype(np.int64), 2 * sh.numpy().astype(np.int64)
    wt, b2 = w.numpy().astype(np.int64).T.copy(), 2 * b.numpy().astype(np.int64)
    out = np.empty((xi.shape[0], w.shape[0]), np.int64)
    for i in range(0, xi.shape[0], 1 << 15):
        blk = xi[i:i + (1 << 15)].astype(np.int64)
        out[i:i + (1 << 15)] = (np.maximum(blk * s2 + h2, 0) if tf else 2 * blk) @ wt + b2
    return out


def check_int_case(ops, dt, shape, C, K, mode, tf, lut, view, seed):
    g = torch.Generator().manual_seed(seed)
    x, sc, sh, w, b = int_case(g, shape, C, K, mode)
    l2 = int_logits2(x, sc, sh, w, b, tf)
    vals = np.array(LUT[:max(K, 2)] if lut else list(range(max(K, 2))), np.uint8)
    thr = 0.0
    if K == 1:
        thr = float(l2[l2.shape[0] // 2, 0]) / 2.0     # the logit of one of the pixels: that pixel sits exactly on the threshold
        assert (l2[:, 0] == 2 * thr).any()
        want = vals[(l2[:, 0] > 2 * thr).astype(np.int64)]
    else:
        want = vals[np.argmax(l2, axis=1)]          # numpy: the first maximum
        if mode != "rand":
            assert ((l2 == l2.max(axis=1, keepdims=True)).sum(axis=1) > 1).any(), "the tie case holds no tie"
        if mode == "zero":
            assert (want == vals[0]).all()
    act = make_act(ops, x, dt, view, sc if tf else None, sh if tf else None)
    got, _ = run_predict(ops, act, w, b, K, lut, thr=thr)
    assert np.array_equal(got.numpy().reshape(-1), want), (dt, shape, C, K, mode, tf, lut, view)


@pytest.mark.parametrize("nchunk", [1, "c16", "c64", 64])
@pytest.mark.parametrize("dt", DTS)
def test_exact_integer_labels(ops, dt, nchunk):
    e = EPC[dt]
    C = {1: e, "c16": 16, "c64": 64, 64: 64 * e}[nchunk]
    n = 0
    for shape, K, tf, lut, view in itertools.product([(1, 1, 1), (3, 5, 7), (2, 16, 24)], (1, 2, 3, 8), (False, True), (False, True),
                                                     (False, True)):
        for mode in (("rand",) if K == 1 else ("rand", "dup", "zero")):
            if mode != "rand" and (shape == (1, 1, 1) or view):       # the tie cases once per (K, transform, lut) on the two larger shapes
                continue
            n += 1
            check_int_case(ops, dt, shape, C, K, mode, tf, lut, view, 1000 * n + C)
    assert n == 3 * 4 * 8 + 2 * 3 * 2 * 4


@pytest.mark.parametrize("dt", DTS)
def test_exact_integer_labels_past_the_grid_cap(ops, dt):
    """More pixels than one full grid covers: 8192 blocks x (256 / nchunk) lane groups x 4 pixels.  The bytes of such a tensor are the
    same at every channel count (8192 x 256 lanes x 4 x 16 bytes = 134 MB); at 64 lanes per pixel it has the fewest pixels (131,072),
    the cheapest reference.  363 x 363 = 131,769: blocks 0..43 take a second trip, the last lane group of the tensor holds one pixel."""
    C = 64 * EPC[dt]
    shape = (1, 363, 363)
    assert shape[1] * shape[2] > CAP * (LANES // 64) * UNROLL and (shape[1] * shape[2]) % UNROLL == 1
    check_int_case(ops, dt, shape, C, 3, "rand", True, True, False, 99)


# ---------------------------------------------------------------------------------------------------
# 2. seeded float data: the logits path of the same arguments, and the probability against float64
# ---------------------------------------------------------------------------------------------------
def prob_ref(logits64, K, pc):
    if K == 1:
        return torch.sigmoid(logits64[:, 0])
    return torch.softmax(logits64, 1)[:, pc]


@pytest.mark.parametrize("bias_mode", ["plain", "+100", "-100"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("dt", DTS)
def test_labels_equal_the_logits_path_and_probability_vs_fp64(ops, dt, K, bias_mode):
    e = EPC[dt]
    for ci, (C, shape, tf, view) in enumerate(itertools.product((e, 16, 64), [(3, 5, 7), (2, 16, 24)], (False, True), (False, True))):
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
        logits = logits.cpu()
        if bias_mode != "plain":
            assert logits[:, 0].abs().min() > 90.0
        l64 = logits.double()
        if K == 1:
            for t in (0.5, 0.3):
                thr = np.float32(math.log(t / (1.0 - t)))
                got, prob = run_predict(ops, act, w, b, K, False, prob_class=0, thr=float(thr))
                assert torch.equal(got, (logits[:, 0] > float(thr)).to(torch.uint8)), (dt, C, shape, tf, view, t)
            classes = (0,)
        else:
            classes = (0, K - 1) if K > 2 else (0, 1)
        for pc in classes:
            got, prob = run_predict(ops, act, w, b, K, False, prob_class=pc)
            if K > 1:
                assert torch.equal(got, logits.argmax(1).to(torch.uint8)), (dt, C, shape, tf, view)
            err = (prob.double() - prob_ref(l64, K, pc)).abs().max().item()
            note(f"ops K={K} {bias_mode}", err / (C_GRAD * U))
            assert err <= C_GRAD * U, (dt, C, K, shape, tf, view, pc, err / U)


# ---------------------------------------------------------------------------------------------------
# 3. model level
# ---------------------------------------------------------------------------------------------------
def trained_net(K, dt, seed=0):
    """UNet(base 16, depth 3) after two training steps: running statistics and counters are no longer their initial values."""
    from cmunet_amd.model import UNet
    torch.manual_seed(seed + K)
    net = UNet(out_classes=K, base_ch=16, depth=3, dtype=dt).to(DEV).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    for i in range(2):
        x = torch.randn(2, 32, 32, device=DEV) * (1.0 + i) + 0.5
        opt.zero_grad()
        net(x).square().mean().backward()
        opt.step()
    # centre every class's logits on a probe input (a shift of the head's bias), so that no class wins every pixel of the tests' inputs
    with torch.no_grad():
        net.eval()
        lo = net(torch.randn(2, 32, 32, device=DEV))
        net.conv_last.bias -= lo.transpose(0, 1).reshape(K, -1).median(1).values
        net.train()
    torch.cuda.synchronize()
    return net


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("dt", DTS)
def test_unet_predict(ops, dt, K):
    net = trained_net(K, dt)
    assert int(net.double_conv.double_conv[1].num_batches_tracked) == 2
    before = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    for shape in [(3, 32, 48), (2, 64, 64)]:
        x = torch.randn(*shape, generator=g).to(DEV)
        net.eval()
        with torch.no_grad():
            logits = net(x)
        # one channel: a probability threshold near the median pixel's, so that both labels occur
        t = min(max(float(torch.sigmoid(logits.median())), 0.05), 0.95) if K == 1 else 0.5
        thr = float(np.float32(math.log(t / (1.0 - t))))
        net.train()
        p_train = net.predict(x, threshold=t)
        assert net.training and p_train.dtype == torch.uint8 and tuple(p_train.shape) == shape
        net.eval()
        p_eval, prob = net.predict(x, threshold=t, prob_class=K - 1)
        assert not net.training
        want = (logits[:, 0] > thr).to(torch.uint8) if K == 1 else logits.argmax(1).to(torch.uint8)
        assert torch.equal(p_eval, want) and torch.equal(p_train, want)
        assert want.unique().numel() > 1, "a constant mask checks nothing"
        err = (prob.double().cpu() - prob_ref(logits.double().cpu(), K, K - 1)).abs().max().item()
        note(f"model K={K}", err / (C_GRAD * U))
        assert err <= C_GRAD * U, err / U
        vals = LUT[:max(K, 2)]
        assert torch.equal(net.predict(x, threshold=t, class_values=vals), torch.tensor(vals, dtype=torch.uint8, device=DEV)[want.long()])
    after = net.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v) and after[k].dtype == v.dtype, k


@pytest.mark.parametrize("dt", DTS)
def test_predict_between_forward_and_backward_leaves_the_step_alone(ops, dt):
    net = trained_net(2, dt, seed=3)
    saved = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    xa, xb = torch.randn(2, 32, 32, generator=g).to(DEV), torch.randn(2, 32, 32, generator=g).to(DEV)

    def step(with_predict):
        net.load_state_dict(saved)
        net.train()
        net.zero_grad(set_to_none=True)
        logits = net(xa)
        if with_predict:
            net.predict(xb)           # same shape as the pending forward: the shape whose concat buffers that forward still holds
            net.predict(xa[:1])
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
# 4. Segmenter, segment_files, load_segmentation_model
# ---------------------------------------------------------------------------------------------------
def test_segmenter_and_files(ops, tmp_path):
    from cmunet_amd import infer
    net = trained_net(2, "f32", seed=7).eval()
    g = torch.Generator().manual_seed(2)
    images = [torch.randn(37, 53, generator=g), torch.randn(64, 40, generator=g),
              (torch.rand(37, 53, generator=g) * 255.0).to(torch.uint8), torch.randn(37, 53, generator=g).numpy(),
              torch.randn(64, 40, generator=g).to(DEV)]
    vals = [0, 255]
    seg = infer.Segmenter(net, size=32, batch=2, class_values=vals)
    masks = seg.segment(images)
    assert len(masks) == len(images)
    lut = torch.tensor(vals, dtype=torch.uint8, device=DEV)
    for im, m in zip(images, masks):
        src = (im if torch.is_tensor(im) else torch.from_numpy(im)).to(DEV)[None].contiguous()
        x = ops.resize_bicubic(src, 32, 32).float()
        with torch.no_grad():
            lab = lut[net(x).argmax(1)]
        want = ops.resize_nearest(lab.contiguous(), *src.shape[1:])[0]
        assert m.is_cuda and m.dtype == torch.uint8 and tuple(m.shape) == tuple(src.shape[1:])
        assert torch.equal(m, want)
    assert any(0 < int((m == 255).sum()) < m.numel() for m in masks)
    # a batched tensor input gives the same masks; native resolution needs multiples of 2**(depth-1)
    stacked = torch.stack([images[0], torch.from_numpy(images[3])])
    for m, i in zip(seg.segment(stacked), (0, 3)):
        assert torch.equal(m, masks[i])
    with pytest.raises(ValueError):
        infer.Segmenter(net, size=None).segment([images[0]])
    nat = infer.Segmenter(net, size=None).segment([images[1]])[0]
    assert torch.equal(nat, net.predict(images[1].to(DEV)[None])[0])
    # files
    paths = []
    for i, im in enumerate(images):
        p = tmp_path / f"img{i}.npy"
        np.save(p, im.cpu().numpy() if torch.is_tensor(im) else im)
        paths.append(str(p))
    written = infer.segment_files(net, paths, str(tmp_path / "out"), size=32, batch=2, class_values=vals)
    assert [os.path.basename(w) for w in written] == [f"img{i}_mask.npy" for i in range(len(images))]
    for w, m in zip(written, masks):
        assert np.array_equal(np.load(w), m.cpu().numpy())
    # both checkpoint forms round-trip to the same predictions
    torch.save(net, tmp_path / "best_model.pth")
    torch.save(net.state_dict(), tmp_path / "state.pth")
    x = torch.randn(2, 32, 32, generator=g).to(DEV)
    want = net.predict(x)
    for src in (str(tmp_path / "best_model.pth"), str(tmp_path / "state.pth"), net.state_dict()):
        m2 = infer.load_segmentation_model(src)
        assert not m2.training and torch.equal(m2.predict(x), want)


# ---------------------------------------------------------------------------------------------------
# 5. argument errors: CmuError, nothing launched
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_bad_arguments_raise_and_launch_nothing(ops, dt):
    from cmunet_amd._lib import CmuError
    e = EPC[dt]
    C = 4 * e
    z = lambda *s: torch.zeros(*s, device=DEV)
    buf = torch.zeros(1, 4, 4, C + e, dtype=TORCH_DT[dt], device=DEV)
    labels = torch.full((1, 4, 4), 251, dtype=torch.uint8, device=DEV)
    prob = torch.full((1, 4, 4), -1.0, device=DEV)
    good = ops.Act(buf, 0, C)
    cases = {
        "K = 9": lambda: ops.head_predict(good, z(9, C), z(9), labels),
        "misaligned x": lambda: ops.head_predict(ops.Act(buf, 1, C), z(2, C), z(2), labels),
        "prob_class = K": lambda: ops.head_predict(good, z(2, C), z(2), labels, prob, 2),
        "prob_class < 0": lambda: ops.head_predict(good, z(2, C), z(2), labels, prob, -1),
        "prob_class = 1 on one channel": lambda: ops.head_predict(good, z(1, C), z(1), labels, prob, 1),
        "scale without shift": lambda: ops.head_predict(ops.Act(buf, 0, C, z(C) + 1, None), z(2, C), z(2), labels),
        "shift without scale": lambda: ops.head_predict(ops.Act(buf, 0, C, None, z(C)), z(2, C), z(2), labels),
        "chunk count not a power of two": lambda: ops.head_predict(ops.Act(z(1, 4, 4, 3 * e).to(TORCH_DT[dt]), 0, 3 * e), z(2, 3 * e), z(2), labels),
    }
    for name, fn in cases.items():
        with pytest.raises(CmuError):
            fn()
        torch.cuda.synchronize()
        assert bool((labels == 251).all()) and bool((prob == -1.0).all()), name
    ops.head_predict(good, z(2, C), z(2), labels, prob, 1)      # the same arguments, valid: it does launch
    torch.cuda.synchronize()
    assert bool((labels == 0).all()) and bool((prob == 0.5).all())
