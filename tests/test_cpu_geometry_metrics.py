"""CPU checks of the geometry metrics: the lattice formulation (tests/geometry_lattice.py) reproduces what the reference's
hausdorff_distance_mask / compute_radius_arteries and scikit-image recorded in tests/golden/geometry_metrics.npz; the metric
classes' names and configuration checks; find_best_epochs' hausdorff fallback and the meter rules of the new log columns."""
import math

import numpy as np
import pytest

import gen_geometry_metrics as GEN
import geometry_lattice as L


@pytest.fixture(scope="module")
def fix(golden_dir):
    return GEN.load(f"{golden_dir}/geometry_metrics.npz")


def test_fixture_records_versions_and_cases(fix):
    assert any(v.startswith("scikit-image") for v in fix["versions"])
    shapes = {m.shape for m in fix["masks"]}
    assert (256, 256) in shapes and (512, 512) in shapes and (96, 160) in shapes
    assert len(fix["pairs"]) >= 6 and np.isinf(fix["hausdorff"]).any() and (fix["hausdorff"] == 0).any()


def test_lattice_counts_and_skeletons_match_fixture(fix):
    for i, (m, sk) in enumerate(zip(fix["masks"], fix["skeletons"])):
        assert L.counts(m) == (int(fix["n_cross"][i]), int(fix["n_closed"][i])), fix["names"][i]
        assert (L.skeletonize(m) == sk).all(), fix["names"][i]


def _close(got, ref, rel=1e-12):
    if math.isnan(ref) or math.isinf(ref) or ref == 0.0:
        return (math.isnan(ref) and math.isnan(got)) or got == ref
    return abs(got - ref) <= rel * abs(ref)


def test_lattice_radius_matches_fixture(fix):
    for i, m in enumerate(fix["masks"]):
        got = L.compute_radius_arteries(m)
        assert all(_close(g, float(r)) for g, r in zip(got, fix["radius"][i])), (fix["names"][i], got, fix["radius"][i])


def test_lattice_hausdorff_matches_fixture(fix):
    for k, (p, g) in enumerate(fix["pairs"]):
        if fix["masks"][p].size > 256 * 256:
            continue          # (the 512^2 pair: the numpy restatement's row minimum is O(n * W); covered on the GPU)
        a, b = fix["masks"][p], fix["masks"][g]
        assert _close(L.hausdorff_distance_mask(a, b), float(fix["hausdorff"][k][0])), fix["names"][p]
        assert _close(L.hausdorff_distance_mask(a, b, "standard"), float(fix["hausdorff"][k][1])), fix["names"][p]


def test_repeat_rule_matters_for_modified_hausdorff(fix):
    """Without the repeated points the modified distance of a noisy pair moves: the weights are part of the contract."""
    k = next(k for k, (p, g) in enumerate(fix["pairs"]) if fix["names"][p] == "noise0.1_64")
    p, g = fix["pairs"][k]
    assert int(fix["n_closed"][p]) > 0
    wa, wb = L.lattice_weights(fix["masks"][p]), L.lattice_weights(fix["masks"][g])
    bi, bj = np.nonzero(wb)
    d = np.sqrt(L.sq_dist_at(wa > 0, bi, bj).astype(np.float64)) / 2
    weighted = (d * wb[bi, bj]).sum() / wb[bi, bj].sum()
    assert abs(weighted - d.mean()) > 1e-6


def test_metric_names_and_unsupported_configurations():
    from cmunet_amd import metrics as M
    mk = dict(activation="softmax", threshold=0.5, ignore_channels=[0])
    assert M.hausdorff(**mk).__name__ == "hausdorff"
    assert M.radius_arteries().__name__ == "radius_arteries"
    for bad in (dict(mk, activation="sigmoid"), dict(mk, threshold=0.3), dict(mk, ignore_channels=None)):
        with pytest.raises(NotImplementedError):
            M.hausdorff(**bad)
    import torch
    with pytest.raises(RuntimeError):
        M.hausdorff(**mk)(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8))        # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        M.radius_arteries()(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8))
    with pytest.raises(ValueError):
        M.hausdorff_distance_mask(torch.zeros(8, 8), torch.zeros(8, 8), method="lee")


def _logs(dice, haus):
    return [{"dice_loss + cross_entropy_loss": d, "dice_loss": d, "hausdorff": h, "radius_arteries": 1.0} for d, h in zip(dice, haus)]


def _reference_find_best_haus(valid_logs, metric):
    """utils.py:26-45, restated (best epoch by strict <, then the hausdorff fallback); best_result 0 allowed."""
    best_valid, best = valid_logs[0][metric], 0
    for i, r in enumerate(valid_logs):
        if r[metric] < best_valid:
            best_valid, best = r[metric], i
    h = valid_logs[best]["hausdorff"]
    if h == np.inf or np.isnan(h):
        h = None
        for i in range(best - 1, -1, -1):
            if valid_logs[i]["hausdorff"] != np.inf and not np.isnan(valid_logs[i]["hausdorff"]):
                h = valid_logs[i]["hausdorff"]
                break
    return best, h


@pytest.mark.parametrize("dice,haus,want", [
    ([0.9, 0.5, 0.7], [3.0, 2.0, 1.0], 2.0),                    # finite best epoch
    ([0.9, 0.8, 0.5], [4.0, 3.0, np.inf], 3.0),                 # inf best epoch -> last finite earlier one
    ([0.9, 0.8, 0.5], [4.0, np.nan, np.nan], 4.0),              # nan best, nan before it -> further back
    ([0.9, 0.8, 0.5], [np.inf, np.nan, np.inf], None),          # nothing finite
])
def test_find_best_epochs_hausdorff_fallback(dice, haus, want):
    from cmunet_amd import train as T
    logs = _logs(dice, haus)
    out = T.find_best_epochs(logs, 3, 1e-3, 2, 1.0)
    best, ref = _reference_find_best_haus(logs, "dice_loss + cross_entropy_loss")
    assert out["hausdorff"] == want == ref
    assert out["dice_loss"] == dice[best] and out["radius_arteries"] == 1.0


def test_find_best_epochs_without_hausdorff_unchanged():
    from cmunet_amd import train as T
    logs = [{"dice_loss": d, "iou_loss": 0.1 * i} for i, d in enumerate([0.5, 0.3, 0.4])]
    out = T.find_best_epochs(logs, 3, 1e-3, 2, 1.0)
    assert "hausdorff" not in out and out["dice_loss"] == 0.3 and out["iou_loss"] == 0.1


def _meter(values):
    """Finetuning/train.py:43-80 AverageValueMeter, restated: the mean after add(v) for each v."""
    n, mean, mean_old = 0, np.nan, 0.0
    with np.errstate(invalid="ignore"):
        for v in values:
            v = np.float64(v)
            n += 1
            if n == 1:
                mean = 0.0 + v
                mean_old = mean
            else:
                mean = mean_old + (v - 1 * mean_old) / float(n)
                mean_old = mean
    return float(mean)


@pytest.mark.parametrize("col", [[np.inf], [2.5, np.inf], [np.inf, 2.5], [2.5, np.inf, 3.5], [1.1, 2.2, 3.3, 0.7]])
def test_epoch_means_meter_columns(col):
    from cmunet_amd import train as T
    names = ["dice_loss + cross_entropy_loss", "dice_loss", "hausdorff", "radius_arteries"]
    rs = np.random.RandomState(len(col))
    finite = rs.rand(len(col), 2)
    table = np.concatenate([finite, np.array(col)[:, None], np.array(col)[::-1, None]], 1)
    got = T._epoch_means(table, names)
    for c in (2, 3):
        ref = _meter(table[:, c])
        assert (math.isnan(ref) and math.isnan(got[c])) or got[c] == ref, (c, got[c], ref)
    # the other columns keep the plain mean, bit for bit (and the call without names is today's)
    plain = T._epoch_means(table)
    assert got[0] == plain[0] == finite[:, 0].sum() / len(col) and got[1] == plain[1]
    if len(col) == 2 and np.isinf(col[1]):
        assert math.isinf(got[2])          # an inf as the epoch's last value stays inf
    if len(col) >= 2 and np.isinf(col[0]):
        assert math.isnan(got[2])          # inf followed by a batch -> nan
