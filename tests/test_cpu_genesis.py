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
