"""GPU suite for the probability histogram, its curves, the threshold mask and their Python surface (csrc/prob_hist.hip, csrc/hist_curves.h,
cmunet_amd/metrics.py, cmunet_amd/infer.py) against tests/prob_hist_ref.py.  Histograms, cumulative counts, masks and best_j are integers: those
comparisons are exact equality, and every call is made twice to show the same bits.  Shapes are the smallest at which the kernel can go wrong:
one below, at and above the pixels a workgroup takes per trip (1024 lanes x 4 / 2 / 1 pixels), more work than the 256-workgroup cap covers in
one trip, odd H*W, H*W % 4 == 2, a slice that breaks the 16-byte alignment, and the bin counts at which the classes are taken in groups.
Bounds: scores 4 * 2^-53 relative to the same formula in Python floats; AUROC / AP / ECE / MCE (NB + 8) * 2^-53 relative to the exact
rationals (their terms are non-negative).  The worst error / bound per quantity and the number of integers compared are printed, and written to
the file CMU_PROB_HIST_PARITY_OUT names when that variable is set (profiles/prob_hist_parity.txt holds one such run)."""
import functools
import os

import numpy as np
import pytest
import torch

import prob_hist_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
EXACT, RATIOS = {}, {}


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
    out = os.environ.get("CMU_PROB_HIST_PARITY_OUT")
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tests/test_gpu_prob_hist.py against tests/prob_hist_ref.py.  Histogram counts, fixed-point sums, invalid counters, cumulative\n"
                    "# counts, masks and best_j are compared for equality.  Bounds of the others: scores 4 * 2^-53 relative to the Python-float\n"
                    "# formula; AUROC, average precision, ECE and MCE (NB + 8) * 2^-53 relative to the exact rationals.\n")
            f.write("\n".join(lines) + "\n")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _conf_ints(conf):
    return conf.view(torch.int64).cpu().numpy().view(np.uint64).astype(object)


def _hist(src, tgt, NB, from_logits=False, pooled=True):
    """cmu_prob_hist twice into fresh buffers (the second time pre-filled with 0xFF bytes): the same bits; numpy results."""
    from cmunet_amd import ops
    B, K = src.shape[:2]
    Bout = 1 if pooled else B
    a = ops.hist_buffers(Bout, K, NB, src.device)
    ops.prob_hist(src, tgt, NB, from_logits, *a, pooled=pooled)
    b = [torch.full_like(t.view(torch.int64) if t.dtype == torch.uint64 else t, -1) for t in a]
    b[1] = b[1].view(torch.uint64)
    ops.prob_hist(src, tgt, NB, from_logits, *b, pooled=pooled)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.uint64 else x, y.view(torch.int64) if y.dtype == torch.uint64 else y)
    return a[0].cpu().numpy(), _conf_ints(a[1]), a[2].cpu().numpy()


def _onehot(lab, K, dtype):
    return np.stack([(lab == c) for c in range(K)], axis=1).astype(dtype)


def _target(rng, shape, kind):
    """(numpy target for the reference, the same on the device): 'f32' / 'f64' one-hot planes, 'u8' a label map with labels >= K mixed in."""
    B, K, H, W = shape
    lab = rng.integers(0, K + 2 if kind == "u8" and K > 1 else max(K, 2), (B, H, W)).astype(np.uint8)
    if kind == "u8":
        return lab, _dev(lab)
    y = _onehot(lab, K, np.float32 if kind == "f32" else np.float64) if K > 1 else (lab != 0)[:, None].astype(np.float32 if kind == "f32" else np.float64)
    return y, _dev(y)


def _compare(p, src, tgt_np, tgt, NB, tag):
    """Pooled and per-image histograms of probability planes against the reference; the pool is the sum of the images' rows."""
    want = R.histogram(p, tgt_np, NB, pooled=True)
    got = _hist(src, tgt, NB, pooled=True)
    for w, g, name in zip(want, got, ("counts", "conf", "invalid")):
        assert np.array_equal(np.asarray(g, object), np.asarray(w, object)), (tag, name)
        _exact("histogram " + name, np.asarray(w).size)
    assert got[0].sum() == p.size
    if p.shape[0] > 1:
        per = _hist(src, tgt, NB, pooled=False)
        wper = R.histogram(p, tgt_np, NB, pooled=False)
        for w, g, name in zip(wper, per, ("counts", "conf", "invalid")):
            assert np.array_equal(np.asarray(g, object), np.asarray(w, object)), (tag, name, "per image")
            assert np.array_equal(np.asarray(g, object).sum(0, keepdims=True), np.asarray(got[("counts", "conf", "invalid").index(name)], object))
            _exact("histogram " + name, np.asarray(w).size)
    return got


# (shape, bins, target kind).  The smallest shapes, odd H*W, H*W % 4 == 2 on the 8-byte path (16 x 18, K = 8) and on the 16-byte one (9 x 10,
# K = 3: it takes the one-pixel path); 4092 / 4096 / 4100 pixels around one trip of the 16-byte path (K <= 4), 2046 / 2048 / 2050 around the
# 8-byte path (K > 4), 1023 / 1025 around the one-pixel path (1024 itself: the misaligned slice below); 513 x 513 > 256 x 1024 one-pixel
# lanes and 1024 x 1028 > 256 x 1024 x 4: more than the workgroup cap covers in one trip; 1024 bins with 8 / 4 classes and 512 bins with
# 8: the classes taken in groups (3 + 3 + 2, 3 + 1, 7 + 1)
SHAPES = [((1, 2, 1, 1), 2, "f32"), ((3, 2, 5, 7), 16, "f64"), ((1, 8, 16, 18), 1024, "u8"), ((2, 3, 8, 8), 256, "f32"),
          ((2, 2, 32, 32), 256, "u8"), ((2, 4, 64, 64), 1024, "f64"), ((1, 2, 62, 66), 16, "f64"), ((1, 2, 64, 64), 256, "f32"),
          ((1, 2, 50, 82), 256, "u8"), ((1, 8, 31, 66), 512, "f32"), ((1, 8, 32, 64), 256, "f64"), ((1, 8, 25, 82), 16, "u8"),
          ((1, 2, 31, 33), 256, "f64"), ((1, 2, 25, 41), 2, "u8"), ((1, 1, 33, 31), 16, "u8"), ((2, 1, 16, 16), 256, "f32"),
          ((1, 2, 513, 513), 256, "u8"), ((1, 2, 1024, 1028), 16, "u8"), ((2, 3, 9, 10), 16, "f64")]


@pytest.mark.parametrize("shape,NB,kind", SHAPES, ids=[f"{'x'.join(map(str, s))}-{nb}-{k}" for s, nb, k in SHAPES])
def test_histogram_of_probability_planes(shape, NB, kind):
    rng = np.random.default_rng(sum(shape) + NB)
    p = rng.random(shape, dtype=np.float32)
    tgt_np, tgt = _target(rng, shape, kind)
    _compare(p, _dev(p), tgt_np, tgt, NB, (shape, NB, kind))


@pytest.mark.parametrize("kind", ["f32", "f64", "u8"])
def test_misaligned_source_takes_the_one_pixel_path(kind):
    rng = np.random.default_rng(3)
    shape = (2, 2, 32, 32)
    flat = rng.random(int(np.prod(shape)) + 1, dtype=np.float32)
    src = _dev(flat)[1:].view(shape)      # one element past a 16-byte boundary
    assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    tgt_np, tgt = _target(rng, shape, kind)
    _compare(flat[1:].reshape(shape), src, tgt_np, tgt, 256, ("misaligned", kind))
    if kind == "u8":      # ... and a label map one byte past its alignment
        lab = _dev(np.concatenate([[0], tgt_np.ravel()]).astype(np.uint8))[1:].view(tgt_np.shape)
        _compare(flat[1:].reshape(shape), _dev(flat[1:].reshape(shape)), tgt_np, lab, 256, ("misaligned labels",))


def _contents(rng, name, n, NB):
    if name == "uniform":
        return rng.random(n, dtype=np.float32)
    if name == "zeros":
        return np.zeros(n, np.float32)
    if name == "ones":
        return np.ones(n, np.float32)
    edges = (np.arange(n) % (NB + 1)).astype(np.float32) / np.float32(NB)      # every j / NB, each many times
    if name == "edges":
        return edges
    if name == "edges_up":
        return np.nextafter(edges, np.float32(2)).astype(np.float32)
    if name == "edges_down":
        return np.nextafter(edges, np.float32(-1)).astype(np.float32)      # (below 0: one invalid value per cycle, clamped to bin 0)
    if name == "skewed":      # 95 % of the pixels in (0, 1 / NB]: the contention case
        p = rng.random(n, dtype=np.float32)
        low = rng.random(n) < 0.95
        p[low] = np.maximum(p[low] / np.float32(NB), np.float32(1e-30))
        return p
    assert name == "invalid"
    p = rng.random(n, dtype=np.float32)
    bad = np.array([np.nan, -0.0, -1e-3, 1 + 1e-3, np.inf, -np.inf], np.float32)
    at = rng.choice(n, n // 5, replace=False)
    p[at] = bad[np.arange(at.size) % bad.size]
    return p


CONTENTS = ("uniform", "zeros", "ones", "edges", "edges_up", "edges_down", "skewed", "invalid")


@functools.lru_cache(maxsize=None)
def _content_case(NB, name):
    """(p, counts, conf, invalid) of the pooled histogram of one content, checked against the reference once and shared with the curves' test."""
    rng = np.random.default_rng(NB + len(name))
    shape = (2, 2, 48, 44)      # 2112 pixels a plane: two cycles of the 1025 edges of NB = 1024
    p = _contents(rng, name, int(np.prod(shape)), NB).reshape(shape)
    lab = (rng.random((2, 48, 44)) < 0.05 + 0.9 * np.nan_to_num(np.clip(p[:, 1], 0, 1))).astype(np.uint8)
    return (p,) + _compare(p, _dev(p), lab, _dev(lab), NB, (NB, name))


@pytest.mark.parametrize("NB", [2, 16, 256, 1024])
@pytest.mark.parametrize("name", CONTENTS)
def test_bins_and_probability_contents(NB, name):
    p, counts, conf, invalid = _content_case(NB, name)
    with np.errstate(invalid="ignore"):
        assert invalid.sum() == int((~((p >= 0) & (p <= 1))).sum())
    if name in ("uniform", "zeros", "ones", "edges", "skewed"):
        assert invalid.sum() == 0
    if name == "invalid":
        assert invalid.sum() > 0
    if name == "skewed":
        assert counts[0, :, :, 1].sum() > 0.9 * p.size


def test_targets_all_negative_all_positive_and_labels_past_k():
    from cmunet_amd import ops
    rng = np.random.default_rng(8)
    shape = (2, 3, 16, 20)
    p = rng.random(shape, dtype=np.float32)
    for lab_value, pos_class in ((0, 0), (2, 2), (3, None), (200, None)):      # labels >= K are negative for every class
        lab = np.full((2, 16, 20), lab_value, np.uint8)
        counts, conf, _ = _compare(p, _dev(p), lab, _dev(lab), 16, ("constant label", lab_value))
        for c in range(3):
            assert counts[0, c, 1].sum() == (p[:, c].size if c == pos_class else 0)
        _, _, summary = ops.hist_curves(_dev(counts), _dev(np.asarray(conf, np.uint64).view(np.int64)).view(torch.uint64))
        s = summary.cpu().numpy()[0]
        for c in range(3):      # AUROC needs both classes, average precision a positive; the calibration error neither
            assert np.isnan(s[c, 0]) and (np.isnan(s[c, 1]) if c != pos_class else s[c, 1] == 1.0) and np.isfinite(s[c, 2])
    for dtype in (np.float32, np.float64):
        for fill in (0.0, 1.0):
            y = np.full(shape, fill, dtype)
            counts, _, _ = _compare(p, _dev(p), y, _dev(y), 16, ("constant planes", fill))
            assert counts[0, :, int(fill)].sum() == p.size


def test_accumulate_adds_and_overwrite_ignores_what_the_buffers_held():
    from cmunet_amd import ops
    rng = np.random.default_rng(12)
    NB = 256
    parts = []
    for shape in ((2, 2, 20, 24), (1, 2, 33, 47), (3, 2, 8, 8)):      # a validation set of mixed sizes pools into one histogram
        p = rng.random(shape, dtype=np.float32)
        p[0, 0, 0, 0] = np.nan
        lab = rng.integers(0, 2, (shape[0],) + shape[2:]).astype(np.uint8)
        parts.append((p, lab))
    buf = ops.hist_buffers(1, 2, NB, "cuda")
    for t in buf:
        (t.view(torch.int64) if t.dtype == torch.uint64 else t).fill_(-1)      # accumulate = 0 on 0xFF bytes: the same result
    for k, (p, lab) in enumerate(parts):
        ops.prob_hist(_dev(p), _dev(lab), NB, False, *buf, pooled=True, accumulate=k > 0)
    want = [R.histogram(p, lab, NB) for p, lab in parts]
    assert np.array_equal(buf[0].cpu().numpy(), sum(w[0] for w in want))
    assert np.array_equal(_conf_ints(buf[1]), sum(w[1] for w in want))
    assert np.array_equal(buf[2].cpu().numpy(), sum(w[2] for w in want)) and int(buf[2].sum()) == 3 * 1
    _exact("histogram counts", buf[0].numel())
    # the same through the public function: out= accumulates
    from cmunet_amd import metrics
    h = None
    for p, lab in parts:
        h = metrics.prob_histogram(_dev(p), _dev(lab), NB, None, out=h)
    assert torch.equal(h.counts, buf[0]) and torch.equal(h.conf.view(torch.int64), buf[1].view(torch.int64)) and torch.equal(h.invalid, buf[2])


@pytest.mark.parametrize("K,scale", [(2, 3.0), (3, 3.0), (8, 3.0), (2, 100.0), (4, 100.0)])
def test_logit_histogram_counts_are_seg_stats_counters_at_every_checked_threshold(K, scale):
    """The test that the softmax bits are shared: tp, tp + fp and tp + fn of the histogram at j equal the thresholded counters and sgt that
    cmu_seg_stats_fwd counts with its own comparison p > j / NB on the same logits -- integer-valued doubles, compared for equality."""
    from cmunet_amd import metrics, ops
    g = torch.Generator().manual_seed(K + int(scale))
    B, H, W = 2, 24, 36
    if scale == 100.0:
        logits = (torch.randint(0, 2, (B, K, H, W), generator=g).float() * 2 - 1) * 100.0
    else:
        logits = torch.randn(B, K, H, W, generator=g) * scale
    lab = torch.randint(0, K, (B, H, W), generator=g)
    y = torch.nn.functional.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().double()
    logits, y = logits.cuda(), y.cuda()
    for NB in (16, 256):
        hist = metrics.prob_histogram(logits, y, bins=NB, activation="softmax")
        again = metrics.prob_histogram(logits, lab.to(torch.uint8).cuda(), bins=NB, activation="softmax2d")
        assert torch.equal(hist.counts, again.counts) and torch.equal(hist.conf.view(torch.int64), again.conf.view(torch.int64))
        assert int(hist.invalid.sum()) == 0 and int(hist.counts.sum()) == K * B * H * W
        cum = ops.hist_curves(hist.counts, hist.conf)[0].cpu().numpy()[0]      # (K,4,NB+1)
        for j in (1, NB // 4, NB // 2, NB - 1):
            metrics.clear_seg_cache()
            table = metrics.seg_table(logits, y, threshold=j / NB)
            tp, spr, sgt = (t.cpu().numpy() for t in metrics._counters(table, j / NB))
            assert np.array_equal(cum[:, 0, j].astype(np.float64), tp), (K, scale, NB, j)
            assert np.array_equal((cum[:, 0, j] + cum[:, 1, j]).astype(np.float64), spr), (K, scale, NB, j)
            assert np.array_equal((cum[:, 0, j] + cum[:, 2, j]).astype(np.float64), sgt), (K, scale, NB, j)
            _exact("logit histogram against cmu_seg_stats_fwd", 3 * K)


@pytest.mark.parametrize("NB", [16, 1024])
def test_sigmoid_histogram_of_a_one_channel_head(NB):
    """Logits built in float64 from probabilities (b + 0.5 +- 0.3) / NB: none within 1e-4 of a bin edge, so the float32 sigmoid and a float64
    one fall into the same bin at every pixel -- equality, no pixel left out."""
    from cmunet_amd import metrics
    rng = np.random.default_rng(NB)
    shape = (2, 1, 32, 36)
    b = rng.integers(0, NB, shape)
    p = (b + 0.5 + rng.uniform(-0.3, 0.3, shape)) / NB
    logits = np.log(p / (1.0 - p)).astype(np.float32)
    p64 = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    assert np.abs(p64 * NB - np.round(p64 * NB)).min() > 1e-4 * NB
    y = (rng.random(shape) < p).astype(np.float32)
    want = np.zeros((1, 1, 2, NB + 1), np.int64)
    np.add.at(want, (0, 0, y.astype(np.int64).ravel(), np.ceil(p64 * NB).astype(np.int64).ravel()), 1)
    for tgt in (_dev(y), _dev(y.astype(np.float64)), _dev((y[:, 0] * 7).astype(np.uint8))):      # one plane: label != 0
        for _ in range(2):
            h = metrics.prob_histogram(_dev(logits), tgt, bins=NB, activation="sigmoid")
            assert np.array_equal(h.counts.cpu().numpy(), want) and int(h.invalid.sum()) == 0
            _exact("sigmoid histogram counts", want.size)


def _check_curves(counts, conf, eps, beta, select):
    """cmu_hist_curves of (rows...,2,NB+1) numpy counts (+ conf as Python ints) against the reference, row by row; twice: the same bits."""
    from cmunet_amd import ops
    NB = counts.shape[-1] - 1
    c = _dev(counts)
    f = _dev(np.asarray(conf, np.uint64).view(np.int64)).view(torch.uint64)
    a = ops.hist_curves(c, f, eps=eps, beta=beta, select=select)
    b = ops.hist_curves(c, f, eps=eps, beta=beta, select=select)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    cum, scores, summary = (t.cpu().numpy() for t in a)
    rows = counts.reshape(-1, 2, NB + 1)
    for r in range(rows.shape[0]):
        want = R.cum_counts(rows[r])
        got = cum.reshape(-1, 4, NB + 1)[r]
        assert np.array_equal(got, want)
        _exact("cumulative counts", want.size)
        ws = R.scores(want, eps, beta)
        gs = scores.reshape(-1, 5, NB + 1)[r]
        assert np.all(np.abs(gs - ws) <= 4 * U * np.abs(ws))
        _ratio("scores", np.max(np.abs(gs - ws) / np.abs(ws)), 4 * U)
        sm = summary.reshape(-1, 6)[r]
        exact = R.summary_exact(rows[r], conf.reshape(-1, NB + 1)[r])
        for name, g, ex in zip(("auroc", "average precision", "ece", "mce"), sm[:4], exact):
            if ex is None:
                assert np.isnan(g), name
            else:
                assert abs(g - float(ex)) <= (NB + 8) * U * float(ex), (name, g, float(ex))
                if ex:
                    _ratio(name, abs(g - float(ex)) / float(ex), (NB + 8) * U)
        bj, bs = R.best(want, select, eps, beta)
        assert sm[4] == bj and (sm[5] == bs or (np.isnan(sm[5]) and np.isnan(bs))), (sm[4:], bj, bs)
        _exact("best_j", 1)
    return summary


@pytest.mark.parametrize("NB", [2, 16, 256, 1024])
def test_curves_of_the_histograms_above(NB):
    k = 0
    for name in CONTENTS:
        _, counts, conf, _ = _content_case(NB, name)
        eps, beta, select = ((1e-7, 1.0, 0), (1e-5, 2.0, 1), (1e-7, 0.5, 2))[k % 3]
        k += 1
        _check_curves(counts, conf, eps, beta, select)


def test_best_threshold_ties_empty_classes_and_two_bins():
    from cmunet_amd import metrics, ops
    row = np.zeros((1, 2, 9), np.int64)      # positives in bin 8, negatives in bin 1: every j in 1..7 separates them: the first one wins
    row[0, 1, 8], row[0, 0, 1] = 5, 7
    conf = np.zeros((1, 9), object)
    for select in (0, 1, 2):
        assert _check_curves(row, conf, 1e-7, 1.0, select)[0, 4] == 1
    row[0, 0, 3] = 2
    for select in (0, 1, 2):
        assert _check_curves(row, conf, 1e-7, 1.0, select)[0, 4] == 3
    two = np.array([[[3, 1, 0], [0, 1, 2]]], np.int64)      # NB = 2 leaves j = 1 only
    assert _check_curves(two, np.zeros((1, 3), object), 1e-7, 1.0, 0)[0, 4] == 1
    nopos = np.zeros((1, 2, 17), np.int64)
    nopos[0, 0, 3:9] = 4
    s = _check_curves(nopos, np.zeros((1, 17), object), 1e-7, 1.0, 2)[0]
    assert np.isnan(s[0]) and np.isnan(s[1]) and s[4] == 1 and np.isnan(s[5])      # Youden's J of an empty class is NaN at every j
    empty = _check_curves(np.zeros((1, 2, 17), np.int64), np.zeros((1, 17), object), 1e-7, 1.0, 0)[0]
    assert np.isnan(empty[:4]).all()
    # the public sweep and best_threshold: device tensors, the same numbers
    h = metrics.ProbHistogram(_dev(np.stack([row, row])[None, :, 0]), _dev(np.zeros((1, 2, 9), np.int64)).view(torch.uint64), torch.zeros(1, 2, dtype=torch.int32).cuda(), 8)
    thr, val = metrics.best_threshold(h, cls=1, score="youden")
    assert thr.is_cuda and thr.dtype == torch.float64 and float(thr) == 3 / 8 and float(val) == 1.0
    sw = metrics.threshold_sweep(h)
    assert sw.thresholds.tolist() == [j / 8 for j in range(9)] and sw.tp.shape == (1, 2, 9) and sw.dice.shape == (1, 2, 9)
    assert sw.tp[0, 1].tolist() == [5] * 8 + [0] and sw.fp[0, 1].tolist() == [9, 2, 2, 0, 0, 0, 0, 0, 0] and float(sw.auroc[0, 1]) == 1.0


SIZES = [(1, 1, 1), (1, 5, 7), (2, 16, 18), (3, 16, 16), (2, 33, 47), (1, 64, 64), (4, 250, 260)]


@pytest.mark.parametrize("shape", SIZES, ids=["x".join(map(str, s)) for s in SIZES])
def test_threshold_mask_is_exact(shape):
    from cmunet_amd import ops
    rng = np.random.default_rng(sum(shape))
    n = int(np.prod(shape))
    flat = rng.random(n + 1, dtype=np.float32)
    flat[rng.choice(n + 1, max(1, n // 7), replace=False)] = np.float32(0.375)      # ties with the threshold: not above it
    flat[rng.choice(n + 1, max(1, n // 9), replace=False)] = np.nan
    for off in (0, 1):      # off = 1: one element past the 16-byte alignment
        p = flat[off:off + n].reshape(shape)
        t = _dev(flat)[off:off + n].view(shape)
        for thr, vp, vn in ((0.375, 1, 0), (0.5, 255, 7)):
            with np.errstate(invalid="ignore"):
                want = np.where(p > np.float32(thr), vp, vn).astype(np.uint8)
            got = ops.threshold_mask(t, thr, vp, vn)
            assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, ops.threshold_mask(t, thr, vp, vn))
            _exact("threshold mask", n)
    out = torch.empty(shape, dtype=torch.uint8, device="cuda")
    assert ops.threshold_mask(_dev(flat)[:n].view(shape), 0.5, 3, 2, out=out) is out


@pytest.fixture(scope="module")
def tiny_two_class_setup():
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
    rng = np.random.default_rng(11)
    imgs = [rng.random((40, 56)).astype(np.float32), rng.random((40, 56)).astype(np.float32), rng.random((33, 47)).astype(np.float32)]
    with torch.no_grad():      # re-centre the head on these images: an unscaled random head puts nearly every pixel in one class
        flat = m(torch.from_numpy(np.stack(imgs[:2])).cuda()).transpose(0, 1).reshape(2, -1)
        s = 2.0 / flat.std(1).clamp_min(1e-6)
        m.conv_last.weight.mul_(s.view(2, 1, 1, 1))
        m.conv_last.bias.copy_((m.conv_last.bias - flat.median(1).values) * s)
    torch.cuda.synchronize()
    masks = [(rng.random(im.shape) < 0.3).astype(np.uint8) for im in imgs]
    return m, imgs, masks


MODES = {"plain": {"size": 48, "batch": 2}, "tiled": {"size": None, "tile": 16, "stride": 8, "tta": "flips", "batch": 5}}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_segmenter_threshold_class(tiny_two_class_setup, mode):
    from cmunet_amd import ops
    from cmunet_amd.infer import Segmenter
    model, imgs, _ = tiny_two_class_setup
    base = MODES[mode]
    off = Segmenter(model, **base).segment(imgs)
    assert all(torch.equal(a, b) for a, b in zip(off, Segmenter(model, threshold_class=None, **base).segment(imgs)))      # byte for byte
    probs = Segmenter(model, **base).segment(imgs, prob_class=1)
    differs = 0
    for t, values in ((0.5, None), (0.3125, None), (0.71, [10, 250])):
        on = Segmenter(model, threshold=t, threshold_class=1, class_values=values, **base).segment(imgs)
        both = Segmenter(model, threshold=t, threshold_class=1, class_values=values, **base).segment(imgs, prob_class=1)
        v = values or [0, 1]
        for im, o, (o2, p2), (argmax, p) in zip(imgs, on, both, probs):
            want = torch.where(p > t, v[1], v[0]).to(torch.uint8)
            if tuple(want.shape) != im.shape:      # the mask is resized back as the masks are
                want = ops.resize_nearest(want[None].contiguous(), *im.shape)[0]
            assert o.shape == im.shape and torch.equal(o, want) and torch.equal(o2, want) and torch.equal(p2, p), (mode, t)
            _exact("segmenter masks", want.numel())
            differs += int((o != (argmax if values is None else argmax * 240 + 10)).sum())
    assert differs > 0      # a threshold away from 0.5 is not the argmax
    cleaned = Segmenter(model, threshold=0.3125, threshold_class=1, min_size=4, class_values=[10, 250], **base).segment(imgs)
    assert all(set(np.unique(c.cpu().numpy())) <= {10, 250} for c in cleaned)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_calibrate_threshold_is_best_threshold_of_the_hand_built_histogram(tiny_two_class_setup, mode):
    from cmunet_amd import metrics, ops
    from cmunet_amd.infer import Segmenter, calibrate_threshold
    model, imgs, masks = tiny_two_class_setup
    seg = Segmenter(model, **MODES[mode])
    for score in ("dice", "iou", "youden"):
        thr, sweep = calibrate_threshold(seg, imgs, masks, cls=1, bins=64, score=score)
        hist = None
        for (_, p), m in zip(seg.segment(imgs, prob_class=1), masks):
            y = _dev(m)[None]
            if tuple(y.shape[1:]) != tuple(p.shape):
                y = ops.resize_nearest(y, *p.shape)
            hist = metrics.prob_histogram(p[None].contiguous(), y, 64, None, out=hist)
        want, value = metrics.best_threshold(hist, 0, score)
        assert isinstance(thr, float) and thr == float(want) and 0.0 < thr < 1.0 and thr * 64 == int(thr * 64)
        assert float(sweep.best_value[0, 0]) == float(value) and int(sweep.tp[0, 0, 0] + sweep.fn[0, 0, 0]) == int(hist.counts[0, 0, 1].sum())
        Segmenter(model, threshold=thr, threshold_class=1, **MODES[mode])      # valid as a Segmenter threshold


def test_metric_classes_in_a_valid_epoch():
    from cmunet_amd import metrics as M, model as Mod, train as T
    torch.manual_seed(11)
    net = Mod.UNet(out_classes=2, base_ch=16, depth=3, dtype="f32")
    loader = []
    for seed in (21, 22):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(2, 32, 32, generator=g)
        y = torch.nn.functional.one_hot(torch.randint(0, 2, (2, 32, 32), generator=g), 2).permute(0, 3, 1, 2).contiguous().double()
        loader.append((x, y))
    mets = [M.AUROC(), M.AveragePrecision(bins=64), M.CalibrationError(cls=0)]
    crit = M.DiceLoss(threshold=None, activation="softmax", ignore_channels=[0]) + M.CrossEntropyLoss()
    va = T.ValidEpoch(net, loss=crit, metrics=mets, device="cuda", verbose=False)
    logs = va.run(loader)
    assert {"auroc", "average_precision", "ece"} <= set(logs)
    want = {"auroc": [], "average_precision": [], "ece": []}
    net.eval()
    for x, y in loader:
        with torch.no_grad():
            logits = net(x.cuda())
        for name, bins, cls, col in (("auroc", 256, 1, 0), ("average_precision", 64, 1, 1), ("ece", 256, 0, 2)):
            h = M.prob_histogram(logits, y.cuda(), bins=bins)
            ex = R.summary_exact(h.counts[0, cls].cpu().numpy(), _conf_ints(h.conf)[0, cls])[col]
            want[name].append(float(ex))
    for name, vals in want.items():
        ref = sum(vals) / len(vals)
        assert abs(logs[name] - ref) <= (256 + 10) * U * ref, (name, logs[name], ref)
        _ratio("epoch " + name, abs(logs[name] - ref) / ref, (256 + 10) * U)
    assert 0.0 < logs["auroc"] < 1.0 and 0.0 < logs["ece"] < 1.0
