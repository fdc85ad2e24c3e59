"""CPU suite for the probability histogram and its curves (no GPU call anywhere):
  * tests/prob_hist_ref.py, the reference of the GPU suite, is pinned to brute-force (p > j / NB) & y counts at every j and to scikit-learn's
    roc_auc_score / average_precision_score on the bin indices (ties, p == 0, p == 1 and values on bin edges included);
  * csrc/hist_curves.h -- the very code cmu_hist_curves calls -- is built into a stand-alone host program (tools/hist_curves_host_check.cpp)
    with the host sanitizers, run directly, and compared with the reference;
  * the three entry points' prototypes in the header and the binding, and the Python-side refusals."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import prob_hist_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _skewed(rng, n, NB):
    """Probabilities with ties at 0, at 1 and on bin edges, most of them in the lowest bins; targets correlated with them."""
    p = (rng.random(n) ** 4).astype(np.float32)
    k = n // 8
    p[:k] = 0
    p[k:2 * k] = 1
    p[2 * k:3 * k] = (rng.integers(0, NB + 1, k) / NB).astype(np.float32)
    p[3 * k:4 * k] = np.nextafter((rng.integers(1, NB, k) / NB).astype(np.float32), np.float32(rng.choice([0, 2])))
    y = (rng.random(n) < 0.1 + 0.8 * p).astype(np.uint8)
    perm = rng.permutation(n)
    return p[perm], y[perm]


@pytest.mark.parametrize("NB", [2, 16, 256, 1024])
def test_suffix_counts_are_the_brute_force_threshold_counts(NB):
    rng = np.random.default_rng(NB)
    p, y = _skewed(rng, 4096, NB)
    counts, conf, invalid = R.histogram(p.reshape(1, 1, 64, 64), y.reshape(1, 64, 64), NB)
    assert invalid.sum() == 0 and counts.sum() == p.size
    cum = R.cum_counts(counts[0, 0])
    for j in range(NB + 1):
        pred = p > np.float32(j / NB)      # the reference's _threshold: j / NB is exact in float32
        want = [(pred & (y == 1)).sum(), (pred & (y == 0)).sum(), (~pred & (y == 1)).sum(), (~pred & (y == 0)).sum()]
        assert list(cum[:, j]) == want, (NB, j)
    assert int(sum(conf[0, 0])) == sum(int(np.floor(float(v) * 2.0 ** 32)) for v in p)


def test_bin_rule_edges_and_clamps():
    NB = 16
    edge = np.arange(NB + 1, dtype=np.float32) / NB
    assert list(R.bins_of(edge, NB)) == list(range(NB + 1))
    assert list(R.bins_of(np.nextafter(edge[:-1], np.float32(2)), NB)) == list(range(1, NB + 1))
    assert list(R.bins_of(np.nextafter(edge[1:], np.float32(0)), NB)) == list(range(1, NB + 1))
    q, bad = R.clamp(np.array([np.nan, -0.0, -1e-3, 1 + 1e-3, np.inf, -np.inf, 0.5], np.float32))
    assert list(q) == [0, 0, 0, 1, 1, 0, 0.5] and list(bad) == [True, False, True, True, True, True, False]
    lab = np.array([[[0, 1, 2, 7]]], np.uint8)
    assert R.positives(lab, 3)[0, :, 0].tolist() == [[True, False, False, False], [False, True, False, False], [False, False, True, False]]
    assert R.positives(lab, 1)[0, 0, 0].tolist() == [False, True, True, True]


@pytest.mark.parametrize("NB", [2, 16, 256])
def test_auroc_and_average_precision_are_scikit_learns_on_the_bin_indices(NB):
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(100 + NB)
    p, y = _skewed(rng, 5000, NB)
    counts, conf, _ = R.histogram(p.reshape(1, 1, 50, 100), y.reshape(1, 50, 100), NB)
    auc, ap, ece, mce = R.summary_exact(counts[0, 0], conf[0, 0])
    b = R.bins_of(p, NB)
    assert abs(float(auc) - metrics.roc_auc_score(y, b)) <= 1e-12
    assert abs(float(ap) - metrics.average_precision_score(y, b)) <= 1e-12
    # the calibration error against its definition on the raw probabilities (float64 sums of float32 values)
    gaps = [abs((y[b == k] == 1).sum() - p[b == k].astype(np.float64).sum()) for k in range(NB + 1)]
    assert abs(float(ece) - sum(gaps) / p.size) <= 1e-9
    assert 0 <= float(ece) <= float(mce) <= 1


def test_auroc_is_the_pairwise_statistic_and_the_empty_class_rules():
    rng = np.random.default_rng(5)
    p, y = _skewed(rng, 600, 16)
    counts, conf, _ = R.histogram(p.reshape(1, 1, 20, 30), y.reshape(1, 20, 30), 16)
    b = R.bins_of(p, 16)
    pos, neg = b[y == 1], b[y == 0]
    pairs = (pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()
    assert float(R.summary_exact(counts[0, 0])[0]) == pytest.approx(pairs / (pos.size * neg.size), abs=1e-14)
    none, _, _ = R.histogram(p.reshape(1, 1, 20, 30), np.zeros((1, 20, 30), np.uint8), 16)
    assert R.summary_exact(none[0, 0])[:2] == (None, None)
    every, _, _ = R.histogram(p.reshape(1, 1, 20, 30), np.ones((1, 20, 30), np.uint8), 16)
    auc, ap, _, _ = R.summary_exact(every[0, 0])
    assert auc is None and ap == 1


def test_best_threshold_takes_the_first_maximum():
    row = np.zeros((2, 9), np.int64)      # positives in bin 8 only, negatives in bin 1 only: every j = 1..7 separates them perfectly
    row[1, 8], row[0, 1] = 5, 7
    cum = R.cum_counts(row)
    for select in (0, 1, 2):
        assert R.best(cum, select) [0] == 1
    row[0, 3] = 2      # two negatives in bin 3: j = 3 is the first threshold above them
    assert [R.best(R.cum_counts(row), s)[0] for s in (0, 1, 2)] == [3, 3, 3]
    two = np.array([[3, 1, 0], [0, 1, 2]], np.int64)
    assert R.best(R.cum_counts(two), 0)[0] == 1      # NB = 2 leaves j = 1 only


def _compiler():
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if shutil.which("g++"):
        return ["g++"] + flags
    if shutil.which("hipcc"):
        return ["hipcc", "-x", "c++"] + flags
    return None


def test_host_program_runs_the_kernels_arithmetic_clean(tmp_path):
    """tools/hist_curves_host_check.cpp runs hist_curves.h's chunked scan, scores and summaries under AddressSanitizer + UBSan on rows with
    ties, empty classes and every chunking from 1 to more chunks than bins; its outputs are compared with tests/prob_hist_ref.py."""
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "hist_curves_host_check")
    r = subprocess.run(cc + [os.path.join(ROOT, "tools", "hist_curves_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(9)
    jobs = []
    for NB, select, nchunks, kind in ((2, 0, 1, "mix"), (2, 2, 256, "mix"), (16, 1, 3, "mix"), (16, 2, 17, "nopos"), (16, 0, 256, "noneg"),
                                      (256, 0, 256, "mix"), (256, 2, 7, "mix"), (1024, 1, 256, "mix"), (1024, 0, 2000, "empty")):
        p, y = _skewed(rng, 3000, NB)
        y = {"mix": y, "nopos": np.zeros_like(y), "noneg": np.ones_like(y), "empty": y}[kind]
        counts, conf, _ = R.histogram(p.reshape(1, 1, 30, 100), y.reshape(1, 30, 100), NB)
        if kind == "empty":
            counts[:], conf[:] = 0, 0
        jobs.append((NB, select, nchunks, 1e-7 if select else 1e-5, 1.0 if select else 2.0, counts[0, 0], conf[0, 0]))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(jobs)).tobytes())
        for NB, select, nchunks, eps, beta, counts, conf in jobs:
            f.write(np.asarray([NB, select, nchunks], np.int32).tobytes())
            f.write(np.asarray([eps, beta], np.float64).tobytes())
            f.write(np.ascontiguousarray(counts, np.int64).tobytes())
            f.write(np.asarray([int(v) for v in conf], np.uint64).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(dst, np.uint8)
    o = 0
    for NB, select, nchunks, eps, beta, counts, conf in jobs:
        n = NB + 1
        cum = raw[o:o + 32 * n].view(np.int64).reshape(4, n)
        sc = raw[o + 32 * n:o + 72 * n].view(np.float64).reshape(5, n)
        sm = raw[o + 72 * n:o + 72 * n + 48].view(np.float64)
        o += 72 * n + 48
        want = R.cum_counts(counts)
        assert np.array_equal(cum, want)
        assert np.array_equal(sc, R.scores(want, eps, beta))      # the same expressions in the same order: the same bits
        exact = R.summary_exact(counts, conf)
        for got, ex in zip(sm[:4], exact):
            if ex is None:
                assert np.isnan(got)
            else:
                assert abs(got - float(ex)) <= (NB + 8) * U * float(ex)
        bj, bs = R.best(want, select, eps, beta)
        assert sm[4] == bj and (sm[5] == bs or (np.isnan(sm[5]) and np.isnan(bs)))
    assert o == raw.size


def test_header_and_binding_declare_the_three_entry_points():
    from cmunet_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "cmunet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, arity in (("cmu_prob_hist", 15), ("cmu_hist_curves", 11), ("cmu_threshold_mask", 7)):
        m = re.search(r"int\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(_lib._SIGS[name][1]), name
        assert name in _lib.EXPORTS
    assert ops.HIST_MAX_BINS == 1024 and "#define CMU_HIST_MAX_BINS 1024" in src
    assert not any(n.endswith("_ws_bytes") and "hist" in n for n in _lib.EXPORTS)


def test_python_side_refusals():
    import torch
    from cmunet_amd import metrics, ops
    z = torch.zeros(1, 2, 4, 4)
    y = torch.zeros(1, 2, 4, 4)
    for bins in (0, 1, 3, 2048):
        with pytest.raises(ValueError, match="bins must be a power of two"):
            metrics.prob_histogram(z, y, bins=bins)
        with pytest.raises(ValueError, match="bins must be a power of two"):
            metrics.AUROC(bins=bins)
    with pytest.raises(ValueError, match="1 <= K <= 8"):
        metrics.prob_histogram(_FakeCuda(1, 9, 4, 4), _FakeCuda(1, 9, 4, 4))
    for fn in (lambda: metrics.prob_histogram(z, y), lambda: ops.prob_hist(z, y, 16, True, *[torch.zeros(1)] * 3),
               lambda: ops.hist_curves(torch.zeros(1, 2, 17, dtype=torch.int64)), lambda: ops.threshold_mask(z, 0.5),
               lambda: metrics.AUROC()(z, y), lambda: metrics.AveragePrecision()(z, y), lambda: metrics.CalibrationError()(z, y)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    with pytest.raises(ValueError, match="activation"):
        metrics.prob_histogram(z, y, activation="tanh")
    with pytest.raises(ValueError, match="activation"):
        metrics.CalibrationError(activation="tanh")
    with pytest.raises(ValueError, match="score"):
        metrics.best_threshold(None, score="f2")
    assert (metrics.AUROC().__name__, metrics.AveragePrecision().__name__, metrics.CalibrationError().__name__) == ("auroc", "average_precision", "ece")


class _FakeCuda:
    """A stand-in that passes the device check, so that the SHAPE refusals behind it are reached without a GPU."""

    def __new__(cls, *shape):
        import torch

        class T(torch.Tensor):
            @property
            def is_cuda(self):
                return True
        return torch.zeros(*shape).as_subclass(T)


def test_shape_mismatches_are_refused_before_any_launch():
    import torch
    from cmunet_amd import metrics
    with pytest.raises(ValueError, match="one-hot targets must have y_pr's shape"):
        metrics.prob_histogram(_FakeCuda(1, 2, 4, 4), _FakeCuda(1, 2, 4, 5))
    with pytest.raises(ValueError, match="uint8 label map must be"):
        metrics.prob_histogram(_FakeCuda(1, 2, 4, 4), _FakeCuda(1, 4, 5).to(torch.uint8).as_subclass(type(_FakeCuda(1))))
    with pytest.raises(ValueError, match="1 <= K <= 8"):
        metrics.prob_histogram(_FakeCuda(1, 9, 4, 4), _FakeCuda(1, 9, 4, 4))
    with pytest.raises(ValueError, match="softmax needs K >= 2"):
        metrics.prob_histogram(_FakeCuda(1, 1, 4, 4), _FakeCuda(1, 1, 4, 4))
    with pytest.raises(ValueError, match="one-channel head's"):
        metrics.prob_histogram(_FakeCuda(1, 2, 4, 4), _FakeCuda(1, 2, 4, 4), activation="sigmoid")
    with pytest.raises(ValueError, match="y_gt must be"):
        metrics.prob_histogram(_FakeCuda(1, 2, 4, 4), _FakeCuda(1, 2, 4, 4).to(torch.int32).as_subclass(type(_FakeCuda(1))))


def test_threshold_class_refusals_and_cli_flag(tmp_path):
    from cmunet_amd import infer, model as M
    two, one = M.UNet(base_ch=16, depth=3, out_classes=2), M.UNet(base_ch=16, depth=3, out_classes=1)
    assert infer.Segmenter(two).threshold_class is None and infer.Segmenter(two, threshold_class=1).threshold_class == 1
    with pytest.raises(ValueError, match="one-channel head"):
        infer.Segmenter(one, threshold_class=1)
    for c in (0, 2, -1, 1.5, True):
        with pytest.raises(ValueError, match="threshold_class must lie in 1..1"):
            infer.Segmenter(two, threshold_class=c)
    three = M.UNet(base_ch=16, depth=3, out_classes=3)
    with pytest.raises(ValueError, match="is not the threshold_class 2"):
        infer.Segmenter(three, threshold_class=2).segment([np.zeros((8, 8), np.float32)], prob_class=1)
    base = ["--model", str(tmp_path / "none.pth"), "--images", str(tmp_path), "--out", str(tmp_path / "o")]
    assert infer.build_parser().parse_args(base + ["--threshold-class", "1"]).threshold_class == 1
    assert infer.build_parser().parse_args(base).threshold_class is None
    with pytest.raises(ValueError, match="images for"):
        infer.calibrate_threshold(infer.Segmenter(two), [], [])
