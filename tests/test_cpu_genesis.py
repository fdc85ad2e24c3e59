"""CPU checks of the Models Genesis / MAE baseline: the host replay of the reference's random stream (cmunet_amd.genesis.replay_records)
fed to a numpy restatement of the per-record apply semantics (tests/genesis_restate.py) reproduces the reference's own generate_pair /
generate_pair_mae batches recorded in tests/golden/genesis_pairs.npz; StepLR's closed form; the checkpoint and losses layouts."""
import os
import pickle
import random

import numpy as np
import pytest
import torch

import gen_genesis_pairs as GEN
import genesis_restate as R
from cmunet_amd import genesis as G


@pytest.fixture(scope="module")
def fix(golden_dir):
    return GEN.load(os.path.join(golden_dir, "genesis_pairs.npz"))[0]


def config_of(case):
    cfg = G.GenesisConfig(model=case["model"])
    for k, v in case["rates"].items():
        setattr(cfg, k, v)
    return cfg


def replay(case):
    cfg = config_of(case)
    return G.replay_records(case["N"], case["B"], case["H"], case["H"], cfg, random.Random(case["seed"]),
                            np.random.RandomState(case["seed"]))


def ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def test_fixture_covers_every_transform(fix):
    assert {"flip", "local", "nonlinear", "inpaint", "outpaint", "genesis64", "genesis128", "genesis256", "mae256"} <= set(fix)
    rep = replay(fix["nonlinear"])
    branches = {bool(f & G.GF_SORTY) for f in rep["recs"]["flags"]}
    assert branches == {True, False}, "the nonlinear case should take both sort branches"
    assert all(int(r["nrect"]) >= 1 for r in replay(fix["inpaint"])["recs"])


@pytest.mark.parametrize("name", ["flip", "local", "nonlinear", "inpaint", "outpaint", "genesis64", "genesis128", "genesis256"])
def test_replay_and_restatement_reproduce_reference(fix, name):
    case = fix[name]
    src = GEN.inputs(case["H"], case["N"], case["seed"])
    rep = replay(case)
    x, y = R.apply_genesis(src, rep["recs"], rep["blocks"], rep["perms"], rep["noise"])
    flips = np.array([int(f) & 3 for f in rep["recs"]["flags"]], np.uint8)
    assert (flips == case["flips"]).all()
    assert x.shape == case["x"].shape
    assert (x.view(np.int32) == case["x"].view(np.int32)).all(), f"{name}: {int((x != case['x']).sum())} pixels differ"


def test_mae_replay_reproduces_reference(fix):
    case = fix["mae256"]
    src = GEN.inputs(case["H"], case["N"], case["seed"])
    rep = replay(case)
    x, _ = R.apply_mae(src, rep["recs"], rep["mask"])
    assert int(rep["mask"].sum()) == 128 * 256
    assert (x.view(np.int32) == case["x"].view(np.int32)).all()


def test_bezier_kernel_order_agrees_with_reference_order():
    """The kernel's evaluation order against bezier_curve's (np.dot over the four Bernstein rows), per element, within
    16 * 2^-53 * max|P_i|: each Bernstein term carries at most 4 roundings (the power included), its product with P_i and the three
    additions at most 4 more, against terms that sum to at most max|P_i| -- 8 u per evaluation, and two evaluations are compared."""
    for group, name, mn, mx, bez, _, _ in R.BEZIER_CASES:
        cx, cy = R.controls(mn, mx, bez)
        rx, ry = R.bezier([[cx[i], cy[i]] for i in range(4)])
        for P, ref in ((cx, rx), (cy, ry)):
            bound = 16 * 2.0 ** -53 * np.abs(P).max()
            err = np.abs(R.bezier_kernel_order(P) - ref).max()
            assert err <= bound, (group, name, err / bound)


def test_controls_round_in_float32():
    cx, cy = R.controls(np.float32(-1.7), np.float32(2.9), (0.3, 0.6, 0.2, 0.9))
    d = np.float32(np.float32(2.9) - np.float32(-1.7))
    assert cx[1] == np.float32(np.float32(np.float32(0.3) * d) + np.float32(-1.7)) and cy[2] == np.float32(np.float32(np.float32(0.9) * d) + np.float32(-1.7))
    assert cx[0] == cy[0] == np.float32(-1.7) and cx[3] == cy[3] == np.float32(2.9) and cx.dtype == np.float64
    # a range of two float32 steps: 0.6 * 2 steps rounds to one step, 0.9 * 2 steps to two
    cx, cy = R.controls(R.ulp32(0.75, 0), R.ulp32(0.75, 2), (0.3, 0.6, 0.2, 0.9))
    assert cy.tolist() == [0.75, float(R.ulp32(0.75, 1)), float(R.ulp32(0.75, 2)), float(R.ulp32(0.75, 2))]


def test_runs_counts_sign_changes_of_nonzero_differences():
    assert R.runs([1.0, 2.0, 3.0])[0] == 1 and R.runs([3.0, 3.0, 3.0])[0] == 1 and R.runs([5.0])[0] == 1
    n, b = R.runs([0.0, 1.0, 1.0, 0.5, 0.5, 0.5, 2.0, 1.0])
    assert n == 4 and b.tolist() == [3, 6, 7]          # the flat stretch belongs to the run it sits in
    n, b = R.runs([2.0, 2.0, 1.0, 1.0, 3.0])
    assert n == 2 and b.tolist() == [4]


def test_bezier_cases_fall_in_their_run_categories():
    """Every case of the shared table, on the restatement: one run, 2 .. 16 (the kernel's merge across runs) or more than 16 (its
    general sort).  The seam cases have a run that starts where the table says, counted in the kernel's 98-sample chunks."""
    for group, name, mn, mx, bez, cat_x, cat_y in R.BEZIER_CASES:
        for P, cat in zip(R.controls(mn, mx, bez), (cat_x, cat_y)):
            n, b = R.runs(R.bezier_kernel_order(P))
            assert R.in_category(n, cat), (group, name, n, cat)
            if group == "three" and cat == "few":
                assert n == 3, (name, n)
            if group == "seam" and cat == "few":
                assert n == 3 and int(name) in (b % R.CHUNK).tolist(), (name, b)
    assert {c[0] for c in R.BEZIER_CASES} == {"ordinary", "three", "seam", "fewulp", "overflow"}


def test_in_range_draws_give_one_run():
    """Why the kernel tests need hand-made records: with draws in [0, 1), as the sampler and the reference's random.random() give them,
    the cubic is monotone, so the sorter only ever sees a table that is sorted already (or reversed)."""
    rng = np.random.RandomState(11)
    for bez in rng.random_sample((1000, 4)):
        for P in R.controls(np.float32(-1.7), np.float32(2.9), bez):
            assert R.runs(R.bezier_kernel_order(P))[0] == 1, bez


def test_record_layout_is_112_bytes():
    assert G.REC_DTYPE.itemsize == 112
    assert G.REC_DTYPE.fields["bez"][1] == 80 and G.REC_DTYPE.fields["block_off"][1] == 64


def test_step_lr_closed_form():
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], 1e-2, momentum=0.9)
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=int(50 * 0.8), gamma=0.5)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for epoch in (0, 1, 39, 40, 79, 80, 120, 255):
            sch.step(epoch)
            assert opt.param_groups[0]["lr"] == pytest.approx(G.step_lr(epoch), rel=1e-12), epoch
    assert G.step_lr(0) == 1e-2 and G.step_lr(40) == 5e-3 and G.step_lr(200) == 1e-2 * 0.5 ** 5


def test_config_defaults_and_refusals():
    c = G.GenesisConfig()
    assert (c.batch_size, c.nb_epoch, c.patience, c.optimizer) == (64, 256, 50, "sgd")
    assert c.inpaint_rate == pytest.approx(0.2) and c.exp_name == "Model Genesis-genesis_chest_ct"
    assert G.GenesisConfig(model="MAE").exp_name == "MAE-genesis_chest_ct"
    with pytest.raises(ValueError):
        G.GenesisConfig(model="SimCLR")
    with pytest.raises(ValueError):
        G.GenesisConfig(optimizer="adam")
    assert G.GenesisConfig(flip_rate=0.25, exp_name="x").flip_rate == 0.25
    with pytest.raises(TypeError, match=r"^GenesisConfig: unknown setting 'flip_prob'$"):
        G.GenesisConfig(flip_prob=0.25)


def _unet_shapes():
    """Parameter names / shapes of UNet(out_classes=1) at base 8, depth 3, in model.parameters() order (CPU module, no kernels)."""
    from cmunet_amd.model import UNet
    m = UNet(out_classes=1, base_ch=8, depth=3)
    return m, [(n, p.shape) for n, p in m.named_parameters()]


def test_genesis_checkpoint_loads_as_genesis_layout(tmp_path):
    from cmunet_amd import train
    m, _ = _unet_shapes()
    sd = m.state_dict()
    opt_sd = {"state": {}, "param_groups": [{"lr": 1e-2, "momentum": 0.9, "params": list(range(len(list(m.parameters()))))}]}
    path = train.export_checkpoint(sd, str(tmp_path / "Model Genesis-genesis_chest_ct.pt"), "genesis", epoch=3, optimizer_state=opt_sd)
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer_state_dict"} and ck["epoch"] == 3
    assert all(k.startswith("module.") for k in ck["state_dict"])
    got, label = train.remap_checkpoint(ck, path)
    assert label == "genesis" and "conv_last.weight" not in got
    assert all(torch.equal(got[k], sd[k]) for k in got)


def test_sgd_state_dict_loads_into_torch_sgd():
    """FusedSGD.state_dict's layout (built here from host tensors the way the method lays it out) is torch.optim.SGD's: a torch SGD
    over tensors of the model's parameter shapes, in order, accepts it and steps with those momentum buffers."""
    m, shapes = _unet_shapes()
    bufs = [torch.randn(s, generator=torch.Generator().manual_seed(i)) for i, (_, s) in enumerate(shapes)]
    state = {i: {"momentum_buffer": b.clone()} for i, b in enumerate(bufs)}
    group = {"lr": 1e-2, "momentum": 0.9, "dampening": 0.0, "weight_decay": 0.0, "nesterov": False, "maximize": False,
             "foreach": None, "differentiable": False, "fused": None, "params": list(range(len(shapes)))}
    params = [torch.zeros(s, requires_grad=True) for _, s in shapes]
    opt = torch.optim.SGD(params, 1e-2, momentum=0.9, weight_decay=0.0, nesterov=False)
    opt.load_state_dict({"state": state, "param_groups": [group]})
    for p in params:
        p.grad = torch.zeros_like(p)
    opt.step()
    for p, b in zip(params, bufs):                     # grad 0: buf <- 0.9 buf, p <- -lr * buf
        assert torch.allclose(p.detach(), -1e-2 * 0.9 * b, rtol=1e-6, atol=1e-9)


def test_losses_pickle_keys(tmp_path):
    """The reference's pickle: {'train_losses': {'fold_<epoch>': [...]}, 'valid_losses': {...}} (Genesis_Chest_CT.py:178-181)."""
    d = {"train_losses": {"fold_0": [0.5, 0.25]}, "valid_losses": {"fold_0": [0.3]}}
    p = tmp_path / "x.pkl"
    p.write_bytes(pickle.dumps(d))
    assert set(pickle.loads(p.read_bytes())) == {"train_losses", "valid_losses"}
