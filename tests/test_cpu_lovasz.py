"""CPU suite for the Lovasz-Softmax loss and the key sort under it:
  * tests/lovasz_ref.py (the float64 reference of tests/test_gpu_lovasz.py) is pinned by the extension property on every binary error
    vector for n <= 7, the G = 0 and all-ignored cases, ties going to the lower index, the classes / per_image averaging written out by
    hand, and autograd against finite differences;
  * the closed form of the Jaccard gradient that csrc/lovasz.hip evaluates equals the definition, in exact rational arithmetic;
  * the tile sort and the merge passes of csrc/key_sort.h -- the very functions the kernels call -- built into a stand-alone host
    program (tools/sort_host_check.cpp) with the host sanitizers and run over the cases of the GPU sort test against numpy.sort;
  * the class's argument checks, without a GPU."""
import itertools
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import lovasz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extension_property_on_every_binary_error_vector():
    """On errors in {0, 1} the loss is the Jaccard loss of the mispredicted set M = {e = 1}: 1 - (G - |M & fg|) / (G + |M & bg|)."""
    for n in range(1, 8):
        for fg in itertools.product((0, 1), repeat=n):
            fg = np.array(fg)
            G = int(fg.sum())
            for e in itertools.product((0.0, 1.0), repeat=n):
                e = np.array(e)
                loss, _, g = R.class_loss(e, fg)
                mf, mb = int(((e == 1) & (fg == 1)).sum()), int(((e == 1) & (fg == 0)).sum())
                want = 0.0 if G + mb == 0 else 1.0 - (G - mf) / (G + mb)
                assert abs(loss - want) <= 1e-15, (fg, e, loss, want)
                assert (g >= -1e-16).all() and g.sum() <= 1 + 1e-15


def test_closed_form_of_the_gradient_is_the_definition():
    rng = np.random.default_rng(3)
    rows = [np.array(f) for n in range(1, 7) for f in itertools.product((0, 1), repeat=n)]
    rows += [rng.integers(0, 2, 200), np.zeros(50, np.int64), np.ones(50, np.int64), (rng.random(3000) < 0.02).astype(np.int64)]
    for fg in rows:
        G, F, exact, Jp = int(fg.sum()), 0, [], Fraction(0)
        for r, f in enumerate(fg, 1):
            F += int(f)
            J = 1 - Fraction(G - F, G + r - F)
            exact.append(J - Jp)
            Jp = J
        exact = np.array([float(v) for v in exact])
        closed, diff = R.jaccard_grad_closed(fg), R.jaccard_grad(fg)
        assert (np.abs(closed - exact) <= 4 * 2.0 ** -53 * exact).all()           # three roundings, no cancellation
        assert (np.abs(diff - exact) <= 4 * 2.0 ** -53).all()                      # two quotients near 1 and their difference
        assert (exact >= 0).all() and exact.sum() <= 1 + 1e-12
        if G == 0:
            assert closed[0] == 1.0 and not closed[1:].any()


def test_absent_class_and_all_ignored():
    x = torch.randn(1, 3, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    lab = torch.randint(0, 2, (1, 4, 5), generator=torch.Generator().manual_seed(1))          # class 2 absent
    p = torch.softmax(x, 1)
    present, ip = R.lovasz_softmax(x, lab, "present")
    every, ia = R.lovasz_softmax(x, lab, "all")
    assert ip["L_sc"][0, 2] == 0.0 and ip["coef"][0] == 0.5 and ia["coef"][0] == 1.0 / 3
    assert abs(ia["L_sc"][0, 2] - float(p[0, 2].max())) <= 1e-15                                # G = 0: its largest error
    assert ia["g"][(0, 2)][0] == 1.0 and not ia["g"][(0, 2)][1:].any()
    assert abs(float(every) - (ia["L_sc"][0].sum() / 3)) <= 1e-15 and abs(float(present) - ip["L_sc"][0, :2].sum() / 2) <= 1e-15
    only2, i2 = R.lovasz_softmax(x, lab, [2])
    assert abs(float(only2) - float(p[0, 2].max())) <= 1e-15 and i2["coef"][0] == 1.0
    # every pixel ignored (then no class is present either): 0, with a zero gradient
    xr = x.clone().requires_grad_(True)
    for classes, labels, ign in (("present", torch.full((1, 4, 5), -100), -100), ("all", torch.full((1, 4, 5), -100), -100),
                                 ("present", torch.full((1, 4, 5), 1), 1), ([0, 2], torch.full((1, 4, 5), 7), 7)):
        v, _ = R.lovasz_softmax(xr, labels, classes, ignore_index=ign)
        (gr,) = torch.autograd.grad(v, xr)
        assert float(v.detach()) == 0.0 and not gr.any()
    bad = lab.clone()
    bad[0, 0, 0] = 3
    assert np.isnan(float(R.lovasz_softmax(x, bad)[0]))


def test_ties_go_to_the_lower_index():
    e = np.array([0.25, 0.5, 0.25, 0.5, 0.25, 0.0, 0.5])
    assert list(R.error_order(e)) == [1, 3, 6, 0, 2, 4, 5]
    assert list(R.error_order(np.full(9, 0.3))) == list(range(9))
    x = torch.zeros(2, 2, 3, 3, dtype=torch.float64)                                         # constant logits: every error is 0.5
    lab = torch.tensor([[[0, 1, 1], [1, 0, 0], [0, 0, 1]], [[1, 1, 1], [0, 0, 0], [1, 0, 1]]])
    _, info = R.lovasz_softmax(x, lab, "all")
    assert list(info["orders"][(0, 1)]) == list(range(18))
    _, info = R.lovasz_softmax(x, lab, "all", per_image=True)
    assert list(info["orders"][(1, 0)]) == list(range(9))


def hand_class_loss(e, fg):
    idx = sorted(range(len(e)), key=lambda i: (-e[i], i))
    G, F, Jp, total = sum(fg), 0, 0.0, 0.0
    for r, i in enumerate(idx, 1):
        F += fg[i]
        J = 1.0 - (G - F) / (G + r - F)
        total += e[i] * (J - Jp)
        Jp = J
    return total


def test_averaging_over_classes_and_images_by_hand():
    """Two images, three classes; class 2 occurs in image 0 only, pixel (1, 1, 1) is ignored."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 2, 3, dtype=torch.float64, generator=g)
    lab = torch.tensor([[[0, 1, 2], [2, 0, 1]], [[1, 0, 0], [0, -100, 1]]])
    p = torch.softmax(x, 1).numpy()

    def rows(images):
        out = {}
        for c in range(3):
            e, fg = [], []
            for b in images:
                for h in range(2):
                    for w in range(3):
                        if int(lab[b, h, w]) == -100:
                            continue
                        f = int(lab[b, h, w]) == c
                        e.append(1 - p[b, c, h, w] if f else p[b, c, h, w])
                        fg.append(int(f))
            out[c] = (hand_class_loss(e, fg), sum(fg))
        return out

    whole, img = rows([0, 1]), [rows([0]), rows([1])]
    cases = {
        ("present", False): sum(whole[c][0] for c in range(3)) / 3,
        ("all", False): sum(whole[c][0] for c in range(3)) / 3,
        ("present", True): (sum(img[0][c][0] for c in range(3)) / 3 + sum(img[1][c][0] for c in (0, 1)) / 2) / 2,
        ("all", True): (sum(img[0][c][0] for c in range(3)) / 3 + sum(img[1][c][0] for c in range(3)) / 3) / 2,
        ((1, 2), True): (sum(img[0][c][0] for c in (1, 2)) / 2 + sum(img[1][c][0] for c in (1, 2)) / 2) / 2,
        ((0,), False): whole[0][0],
    }
    assert img[1][2][1] == 0 and img[1][2][0] > 0                       # absent from image 1: its largest error counts under 'all'
    for (classes, per_image), want in cases.items():
        got, info = R.lovasz_softmax(x, lab, classes if isinstance(classes, str) else list(classes), per_image)
        assert abs(float(got) - want) <= 1e-15, (classes, per_image, float(got), want)
        assert abs(float((info["coef"] * info["L_s"]).sum()) - want) <= 1e-15
    assert R.lovasz_softmax(x, lab, "present", True)[1]["counts"].tolist() == [[6, 2, 2, 2], [5, 3, 2, 0]]


def test_autograd_against_finite_differences_away_from_ties():
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(2, 3, 3, 4, dtype=torch.float64, generator=g) * 1.5).requires_grad_(True)
    lab = torch.randint(0, 3, (2, 3, 4), generator=g)
    lab[1, 2, 3] = -100
    for classes, per_image in (("present", False), ("all", True), ([0, 2], False)):
        v, info = R.lovasz_softmax(x, lab, classes, per_image)
        gaps = [np.abs(np.diff(e)).min() for e in info["e"].values() if e.size > 1]
        assert min(gaps) > 1e-5                                            # no two errors within reach of the step below
        (grad,) = torch.autograd.grad(v, x)
        # the same value with the order held fixed is what is differentiated
        v2, _ = R.lovasz_softmax(x, lab, classes, per_image, orders=info["orders"])
        assert float(v2.detach()) == float(v.detach())
        h = 1e-7
        flat = x.detach().clone().reshape(-1)
        for i in range(0, flat.numel(), 5):
            xp, xm = flat.clone(), flat.clone()
            xp[i] += h
            xm[i] -= h
            fd = (float(R.lovasz_softmax(xp.view_as(x), lab, classes, per_image)[0]) - float(R.lovasz_softmax(xm.view_as(x), lab, classes, per_image)[0])) / (2 * h)
            assert abs(fd - float(grad.reshape(-1)[i])) <= 1e-7, (classes, per_image, i, fd, float(grad.reshape(-1)[i]))


def test_perturbing_the_errors_moves_a_class_loss_by_no_more():
    rng = np.random.default_rng(9)
    worst = 0.0
    for _ in range(300):
        n = int(rng.integers(1, 40))
        e, fg = rng.random(n), rng.integers(0, 2, n)
        d = 1e-3
        e2 = np.clip(e + rng.uniform(-d, d, n), 0, 1)
        worst = max(worst, abs(R.class_loss(e, fg)[0] - R.class_loss(e2, fg)[0]) / d)
    assert worst <= 1.0


def _compiler():
    if shutil.which("g++"):
        return ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if shutil.which("hipcc"):
        return ["hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    return None


def header_tile():
    import re
    h = open(os.path.join(ROOT, "cmunet_amd", "csrc", "key_sort.h")).read()
    return int(re.search(r"constexpr int CMU_KS_TILE = (\d+);", h).group(1))


def test_host_program_sorts_the_gpu_tests_cases_clean(tmp_path):
    """tools/sort_host_check.cpp runs the tile sort and the merge passes of csrc/key_sort.h serially under AddressSanitizer + UBSan
    over the cases of the GPU sort test; its output is numpy.sort's, segment by segment."""
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "sort_host_check")
    r = subprocess.run(cc + [os.path.join(ROOT, "tools", "sort_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    T = header_tile()
    cases = R.sort_cases(T)
    assert len(cases) == 70 and max(n for _, _, n in cases) == 5 * T + 7
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    data = [R.sort_keys(kind, S, n) for kind, S, n in cases]
    with open(src, "wb") as f:
        f.write(np.int64(len(cases)).tobytes())
        for (kind, S, n), k in zip(cases, data):
            assert k.shape == (S, n) and k.dtype == np.uint64
            f.write(np.asarray([S, n], np.int64).tobytes())
            f.write(np.ascontiguousarray(k).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(dst, np.uint64)
    o = 0
    for (kind, S, n), k in zip(cases, data):
        got = raw[o:o + S * n].reshape(S, n)
        o += S * n
        assert np.array_equal(got, np.sort(k, axis=1)), (kind, S, n)
    assert o == raw.size


def test_sort_case_data_is_what_it_says():
    T = header_tile()
    for kind in R.SORT_DATA:
        k = R.sort_keys(kind, 3, 2 * T + 3)
        assert all(np.unique(row).size == row.size for row in k), kind                     # distinct keys: the order is the keys' alone
    assert np.unique(R.sort_keys("shared_high", 1, 100) >> np.uint64(32)).size == 1
    assert np.unique(R.sort_keys("four_high", 1, 1000) >> np.uint64(32)).size == 4
    a, d = R.sort_keys("ascending", 1, 100)[0], R.sort_keys("descending", 1, 100)[0]
    assert (np.diff(a.astype(np.float64)) > 0).all() and (np.diff(d.astype(np.float64)) < 0).all()


def test_class_checks_its_arguments_without_a_gpu():
    from cmunet_amd import metrics as M, ops
    for act in ("sigmoid", None, "identity"):
        with pytest.raises(NotImplementedError, match="LovaszSoftmaxLoss: activation 'softmax' / 'softmax2d' only on the HIP path"):
            M.LovaszSoftmaxLoss(activation=act)
    for classes in ("some", [], [8], [-1]):
        with pytest.raises(ValueError, match="LovaszSoftmaxLoss"):
            M.LovaszSoftmaxLoss(classes=classes)
    crit = M.LovaszSoftmaxLoss()
    assert (crit.classes, crit.per_image, crit.ignore_index, crit.__name__) == ("present", False, -100, "lovasz_softmax_loss")
    assert M.LovaszSoftmaxLoss(classes=(2, 1, 2)).classes == [1, 2]
    assert (M.DiceLoss(activation="softmax") + 0.5 * M.LovaszSoftmaxLoss()).__name__ == "dice_loss + 0.5 * lovasz_softmax_loss"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sort_u64(torch.zeros(1, 4, dtype=torch.int64))
    sz = ops.lovasz_sizes(2, 3, 91, 91, [1, 2], True)
    assert sz["S"] == 2 and sz["n"] == 8281 and sz["rows"] == 4 and sz["counts"] == 9 and sz["out"] == 11
