"""CPU suite of the differentiable soft-clDice: the restatements of tests/cldice_grad_restate.py against the reference's own
fp64 autograd (tests/golden/cldice_grad.npz, written by tests/gen_cldice_grad.py) and against each other, and the constructor of
``cmunet_amd.metrics.soft_cldice``.  The HIP kernels are held to these restatements in tests/test_gpu_cldice_grad_fp64.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cldice_grad_restate as R  # noqa: E402
import gen_cldice_grad as G  # noqa: E402

ROWS = G.load()


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_autograd_restatement_reproduces_the_reference(row):
    """softmax -> kept channels -> oracle.losses.soft_skel -> clDice in fp64: the reference's loss and gradient to 1e-12."""
    key, K, ign, eb, regime, lg, y, loss, dl = row
    x = torch.from_numpy(lg).requires_grad_(True)
    L = R.cldice(x, torch.from_numpy(y), ign, eb)
    L.backward()
    assert abs(L.item() - loss) <= 1e-12, (key, L.item(), loss)
    assert np.abs(x.grad.numpy() - dl).max() <= 1e-12, key
    if regime == "sat":          # the plateaus the fixture promises
        p = torch.softmax(torch.from_numpy(lg), 1)
        assert float(((p == 0) | (p == 1)).double().mean()) >= 0.2


def test_fixture_covers_the_cases_of_the_issue():
    got = {(K, None if ign is None else tuple(ign), eb, regime) for _, K, ign, eb, regime, *_ in ROWS}
    want = {(2, (0,), False), (3, None, False), (3, (0,), False), (4, None, True), (4, (1,), True)}
    assert got == {c + (r,) for c in want for r in ("soft", "sat")}
    assert all(r[5].shape[0] == 2 and r[5].shape[2:] == (12, 20) for r in ROWS)


SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 2, 2), (2, 3, 3), (2, 17, 33)]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_explicit_gather_form_equals_autograd(kind, shape):
    """The reverse sweep written as a gather with the tie rules spelled out equals fp64 autograd of the pooling chain to
    1e-14 max|g|, for num_iter 0, 1, 3, 10 and upstream gradients of mixed, positive and negative sign."""
    img = R.tie_planes(kind, shape, seed=1).astype(np.float64)
    if kind == "saturated" and img.size >= 9:
        assert np.mean((img == 0) | (img == 1)) >= 0.2
    for num_iter in (0, 1, 3, 10):
        for sign in (0, 1, -1):
            g = R.upstream(shape, num_iter, sign).astype(np.float64)
            want, sk = R.skel_grad_autograd(img, g, num_iter)
            got = R.skel_grad_explicit(img, g, num_iter)
            assert np.array_equal(R.skel_forward(img, num_iter)[1][-1], sk), (kind, shape, num_iter)
            assert np.abs(got - want).max() <= 1e-14 * max(np.abs(want).max(), 1e-300), (kind, shape, num_iter, sign)


def test_tie_rules_on_the_cases_the_issue_names():
    """One erode, one dilate, by hand: a strict centre minimum takes the whole gradient; a flat 3x3 of ones gives half to the top and
    half to the left neighbour; a flat corner keeps 1.0; the dilate's gradient goes to the first maximum in row-major order."""
    one = np.zeros((1, 3, 3))
    one[0, 1, 1] = 1.0                                     # upstream gradient at the centre only
    strict = np.ones((1, 3, 3))
    strict[0, 1, 1] = 0.5
    assert np.array_equal(R._erode_gather(one, strict), one)
    flat = R._erode_gather(one, np.ones((1, 3, 3)))
    assert flat[0, 0, 1] == 0.5 and flat[0, 1, 0] == 0.5 and flat.sum() == 1.0
    corner = np.zeros((1, 3, 3))
    corner[0, 0, 0] = 1.0
    assert np.array_equal(R._erode_gather(corner, np.ones((1, 3, 3))), corner)
    d = R._dilate_gather(one, np.ones((1, 3, 3)))
    assert d[0, 0, 0] == 1.0 and d.sum() == 1.0
    d = R._dilate_gather(corner, np.ones((1, 3, 3)))       # the corner's window starts at itself: padding never wins
    assert d[0, 0, 0] == 1.0 and d.sum() == 1.0


def test_constructor_and_cpu_refusal():
    from cmunet_amd import metrics as M
    for kw in (dict(threshold=None, activation="softmax"), dict(threshold=None, activation="softmax2d", ignore_channels=[0]),
               dict(threshold=None, activation="softmax", ignore_channels=[1], exclude_background=True, smooth=0.5),
               dict(threshold=0.3, activation="softmax", ignore_channels=[0, 2]), dict(threshold=0.5, activation="softmax", exclude_background=True),
               dict(threshold=0.5, activation="softmax", ignore_channels=[0], iter_=7)):
        m = M.soft_cldice(**kw)
        assert m.__name__ == "soft_clDice" and m.num_iter == 10
    for act in (None, "sigmoid", "identity"):
        with pytest.raises(NotImplementedError):
            M.soft_cldice(threshold=None, activation=act)
    for ign in ([-1], [M.ops.SEG_MAX_K], list(range(M.ops.SEG_MAX_K))):
        with pytest.raises(ValueError):
            M.soft_cldice(threshold=None, activation="softmax", ignore_channels=ign)
    with pytest.raises(ValueError):
        M.soft_cldice(threshold=None, activation="softmax", smooth=0.0)
    m = M.soft_cldice(threshold=None, activation="softmax", ignore_channels=[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 4, 4, requires_grad=True), torch.zeros(1, 3, 4, 4))
    crit = M.DiceLoss(activation="softmax", threshold=None, ignore_channels=[0]) + M.CrossEntropyLoss() + 0.5 * m
    assert crit.__name__ == "dice_loss + cross_entropy_loss + 0.5 * soft_clDice"
    assert isinstance(crit, M.Loss)
