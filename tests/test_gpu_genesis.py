"""GPU checks of the Models Genesis / MAE baseline (csrc/genesis.hip, cmunet_amd/genesis.py): the kernels fed with the host replay
reproduce the reference's recorded batches; the device sampler's records follow the reference's laws; device batches equal the numpy
restatement of their own records; determinism in (seed, offset); no host synchronisation; the MSE loss, the K = 1 UNet, SGD steps and a
short pretrain_genesis run against fp64 restatements."""
import math
import os
import random

import numpy as np
import pytest
import torch

import gen_genesis_pairs as GEN
import genesis_restate as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def fix(golden_dir):
    return GEN.load(os.path.join(golden_dir, "genesis_pairs.npz"))[0]


def _cfg(model="Model Genesis", rates=None):
    from cmunet_amd import genesis as G
    c = G.GenesisConfig(model=model)
    for k, v in (rates or {}).items():
        setattr(c, k, v)
    return c


def ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("name", ["flip", "local", "nonlinear", "inpaint", "outpaint", "genesis64", "genesis128", "genesis256", "mae256"])
def test_replayed_records_reproduce_reference(fix, name):
    from cmunet_amd import genesis as G
    case = fix[name]
    src = GEN.inputs(case["H"], case["N"], case["seed"])
    gen = G.GenesisPairGenerator(src, case["B"], _cfg(case["model"], case["rates"]), device=DEV,
                                 reference_stream=(random.Random(case["seed"]), np.random.RandomState(case["seed"])))
    x, y = next(gen)
    x, y = x.cpu().numpy(), y.cpu().numpy()
    ref = case["x"]
    recs = gen.records()["recs"]
    for b in range(case["B"]):
        img = src[int(recs["src"][b])]
        assert (y[b] == R.flip(img, int(case["flips"][b]))).all(), (name, b)
        if int(recs["flags"][b]) & G.GF_NONLIN:
            u = ulps(x[b], ref[b])
            assert u.max() <= 2, f"{name}[{b}]: {int((u > 2).sum())} pixels beyond 2 ulp (max {int(u.max())})"
        else:
            assert (x[b].view(np.int32) == ref[b].view(np.int32)).all(), f"{name}[{b}]: {int((x[b] != ref[b]).sum())} pixels differ"
    assert int(gen.err.item()) == 0


def _sample(B=512, batches=8, H=64, N=4096, seed=5):
    from cmunet_amd import genesis as G
    src = np.random.RandomState(0).standard_normal((N, H, H)).astype(np.float32)
    gen = G.GenesisPairGenerator(src, B, _cfg(), seed=seed, offset=0, device=DEV)
    out = []
    for _ in range(batches):
        next(gen)
        out.append(gen.records())
    return out, H, N


def _within(count, n, p, what):
    sd = math.sqrt(max(p * (1 - p), 1e-12) / n)
    assert abs(count / n - p) <= 4 * sd + 1e-12, f"{what}: {count}/{n} = {count / n:.4f}, expected {p:.4f} (4 sigma {4 * sd:.4f})"


def test_device_sampler_follows_reference_laws():
    from cmunet_amd import genesis as G
    batches, H, N = _sample()
    recs = np.concatenate([b["recs"] for b in batches])
    n = len(recs)
    assert n == 4096
    for b in batches:
        s = b["recs"]["src"]
        assert len(set(s.tolist())) == len(s) and s.min() >= 0 and s.max() < N
    f = recs["flags"].astype(np.int64)
    # flips: k ~ truncated geometric (k < 3: 0.4^k 0.6; k = 3: 0.4^3), each flip on a uniform axis -> parity distribution
    pk = [0.6, 0.4 * 0.6, 0.4 ** 2 * 0.6, 0.4 ** 3]
    par = np.zeros(4)
    for k, p in enumerate(pk):
        for axes in range(2 ** k):
            bits = 0
            for j in range(k):
                bits ^= 2 if (axes >> j) & 1 else 1
            par[bits] += p / 2 ** k
    for bits in range(4):
        _within(int(((f & 3) == bits).sum()), n, par[bits], f"flip parity {bits}")
    _within(int((f & G.GF_LOCAL != 0).sum()), n, 0.5, "local shuffle rate")
    nl = f & G.GF_NONLIN != 0
    _within(int(nl.sum()), n, 0.9, "nonlinear rate")
    _within(int((f[nl] & G.GF_SORTY != 0).sum()), int(nl.sum()), 0.5, "both-sorted branch")
    paint = recs["paint"]
    _within(int((paint != 0).sum()), n, 0.9, "paint rate")
    _within(int((paint == 1).sum()), int((paint != 0).sum()), 0.2, "in-painting share")
    nr_in, nr_out = recs["nrect"][paint == 1], recs["nrect"][paint == 2]
    for m in range(6):
        _within(int((nr_in == m).sum()), len(nr_in), 0.95 ** m * 0.05 if m < 5 else 0.95 ** 5, f"in-painting {m} rectangles")
    for m in range(5):
        _within(int((nr_out == m + 1).sum()), len(nr_out), 0.95 ** m * 0.05 if m < 4 else 0.95 ** 4, f"out-painting {m + 1} windows")
    assert (recs["nrect"][paint == 0] == 0).all()
    for r in recs[paint == 1]:
        for x0, y0, sx, sy in r["rect"][:r["nrect"]]:
            assert H // 6 <= sx <= H // 3 and H // 6 <= sy <= H // 3 and 3 <= x0 <= H - sx - 3 and 3 <= y0 <= H - sy - 3
    for r in recs[paint == 2]:
        for q, (x0, y0, sx, sy) in enumerate(r["rect"][:r["nrect"]]):
            lo = H - 4 * H // 7
            hi = H - 2 * H // 7 if q == 0 else H - 3 * H // 7
            assert lo <= sx <= hi and lo <= sy <= hi and 3 <= x0 <= H - sx - 3 and 3 <= y0 <= H - sy - 3
    bez = recs["bez"][nl]
    assert (bez >= 0).all() and (bez < 1).all() and abs(bez.mean() - 0.5) < 4 * math.sqrt(1 / 12 / bez.size)
    # blocks + permutations of the shuffled images of the first batch
    b0 = batches[0]
    sx_all, perm_first = [], []
    for i, r in enumerate(b0["recs"]):
        if not r["flags"] & G.GF_LOCAL:
            assert r["nblocks"] == 0
            continue
        blk = b0["blocks"][i].astype(np.int64)
        assert ((blk[:, 2] >= 1) & (blk[:, 2] <= H // 25) & (blk[:, 0] >= 0) & (blk[:, 0] <= H - blk[:, 2])).all()
        assert ((blk[:, 3] >= 1) & (blk[:, 3] <= H // 25) & (blk[:, 1] >= 0) & (blk[:, 1] <= H - blk[:, 3])).all()
        sx_all.append(blk[:, 2])
        for k in range(0, 10000, 97):
            nk = int(blk[k, 2] * blk[k, 3])
            p = b0["perms"][i, k, :nk]
            assert sorted(p.tolist()) == list(range(nk))
            if nk == 4:
                perm_first.append(int(p[0]))
    sx_all = np.concatenate(sx_all)
    _within(int((sx_all == 1).sum()), len(sx_all), 0.5, "block height 1 of [1, 2]")
    pf = np.array(perm_first)
    for v in range(4):
        _within(int((pf == v).sum()), len(pf), 0.25, f"first element {v} of a 4-element permutation")


def test_device_batch_equals_restatement_of_its_records():
    from cmunet_amd import genesis as G
    H, N = 64, 32
    src = np.random.RandomState(1).standard_normal((N, H, H)).astype(np.float32)
    gen = G.GenesisPairGenerator(src, 16, _cfg(), seed=9, offset=3, device=DEV)
    x, y = next(gen)
    x, y = x.cpu().numpy(), y.cpu().numpy()
    rec = gen.records()
    rx, ry = R.apply_genesis(src, rec["recs"], rec["blocks"], rec["perms"], None)
    assert (y == ry).all()
    painted = np.isnan(rx)
    assert ((x[painted] >= 0) & (x[painted] <= 1)).all()
    for b in range(16):
        keep = ~painted[b]
        if int(rec["recs"]["flags"][b]) & G.GF_NONLIN:
            assert ulps(x[b][keep], rx[b][keep]).max() <= 2, b
        else:
            assert (x[b][keep].view(np.int32) == rx[b][keep].view(np.int32)).all(), b
    assert int(gen.err.item()) == 0


def test_same_seed_offset_same_bits_other_offset_differs():
    from cmunet_amd import genesis as G
    src = np.random.RandomState(2).standard_normal((20, 64, 64)).astype(np.float32)
    a = next(G.GenesisPairGenerator(src, 8, _cfg(), seed=4, offset=7, device=DEV))
    b = next(G.GenesisPairGenerator(src, 8, _cfg(), seed=4, offset=7, device=DEV))
    c = next(G.GenesisPairGenerator(src, 8, _cfg(), seed=4, offset=8, device=DEV))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0])


def test_mae_batch_is_masked_copy():
    from cmunet_amd import genesis as G
    src = np.random.RandomState(3).standard_normal((10, 256, 256)).astype(np.float32)
    gen = G.GenesisPairGenerator(src, 4, _cfg("MAE"), seed=1, device=DEV)
    x, y = next(gen)
    m = gen.last_mask
    assert int(m.sum()) == 128 * 256
    assert torch.equal(x, y * (1 - m.float())[None])
    idx = gen.records()["recs"]["src"]
    assert torch.equal(y.cpu(), torch.from_numpy(src[idx.astype(np.int64)]))


def _tiny_unet(seed=3, base=16, depth=3, dtype="f32"):
    from cmunet_amd import model as M
    from oracle import unet as OU
    sd = OU.make_state_dict(base_ch=base, depth=depth, out_classes=1, seed=seed)
    net = M.UNet(out_classes=1, base_ch=base, depth=depth, dtype=dtype)
    net.load_state_dict(sd)
    return net.to(DEV), sd


def test_no_host_sync_in_generator_and_step():
    from cmunet_amd import genesis as G
    src = np.random.RandomState(4).standard_normal((12, 64, 64)).astype(np.float32)
    net, _ = _tiny_unet()
    tr = G.GenesisPretrainer(net)
    gen = G.GenesisPairGenerator(src, 4, _cfg(), seed=2, device=DEV)
    x, y = next(gen)
    tr.step(x, y)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, y = next(gen)
        loss = tr.step(x, y)
        tr.evaluate(x, y)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert math.isfinite(float(loss))


def test_mse_fwd_bwd_matches_fp64():
    from cmunet_amd import genesis as G
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(3, 1, 40, 56, generator=g)
    y = torch.randn(3, 40, 56, generator=g)
    loss = torch.zeros(1, device=DEV)
    dl = torch.empty(3, 1, 40, 56, device=DEV)
    G.mse_fwd_bwd(logits.to(DEV), y.to(DEV), loss, dl)
    l64 = logits.double().requires_grad_(True)
    ref = torch.nn.functional.mse_loss(l64.squeeze(1), y.double())
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-6 * float(ref)
    assert torch.allclose(dl.cpu().double(), l64.grad, rtol=1e-5, atol=1e-12)
    loss2 = torch.zeros(1, device=DEV)
    G.mse_fwd_bwd(logits.to(DEV), y.to(DEV), loss2, None)
    assert torch.equal(loss, loss2)


def test_k1_unet_forward_backward_matches_oracle():
    from oracle import unet as OU
    net, sd = _tiny_unet(seed=5)
    x = torch.randn(2, 64, 64, generator=torch.Generator().manual_seed(1))
    out = net(x.to(DEV))
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
    out.backward(g.to(DEV))
    osd = OU.clone_sd({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, requires_grad=True)
    ref = OU.unet_forward(x.double(), osd, training=True)
    assert out.shape == ref.shape == (2, 1, 64, 64)
    ref.backward(g.double())
    err = (out.detach().cpu().double() - ref.detach()).abs().max().item() / ref.abs().max().item()
    assert err <= 2e-4, err
    params = dict(net.named_parameters())
    for k in ("conv_last.weight", "conv_last.bias", "down_conv1.double_conv.double_conv.0.weight"):
        gr, go = params[k].grad.cpu().double(), osd[k].grad
        e = (gr - go).abs().max().item() / max(go.abs().max().item(), 1e-12)
        assert e <= 2e-3, (k, e)


def test_pretrainer_sgd_steps_follow_oracle():
    from cmunet_amd import genesis as G
    from oracle import optim as OO, unet as OU
    net, sd = _tiny_unet(seed=7, base=64, depth=3)
    tr = G.GenesisPretrainer(net)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(2, 64, 64, generator=g) for _ in range(3)]
    ys = [torch.randn(2, 64, 64, generator=g) for _ in range(3)]
    osd = OU.clone_sd({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, requires_grad=True)
    names = [n for n, _ in net.named_parameters()]
    bufs = [torch.zeros_like(osd[n]) for n in names]
    for it in range(3):
        got = float(tr.step(xs[it].to(DEV), ys[it].to(DEV)).item())
        for n in names:
            osd[n].grad = None
        ref = torch.nn.functional.mse_loss(OU.unet_forward(xs[it].double(), osd, training=True).squeeze(1), ys[it].double())
        ref.backward()
        with torch.no_grad():
            OO.sgd_step([osd[n] for n in names], [osd[n].grad for n in names], bufs, 1e-2, momentum=0.9, step=it + 1)
        assert abs(got - float(ref)) <= 1e-4 * max(1.0, float(ref)), (it, got, float(ref))
    w = dict(net.named_parameters())["conv_last.weight"].detach().cpu().double()
    err = (w - osd["conv_last.weight"].detach()).abs().max().item()
    assert err <= 1e-4, err
    # the optimizer half loads into torch.optim.SGD over the same shapes, in order
    sgd_sd = tr.opt.state_dict()
    params = [torch.zeros_like(osd[n]).float().requires_grad_(True) for n in names]
    torch.optim.SGD(params, 1e-2, momentum=0.9).load_state_dict(sgd_sd)
    assert len(sgd_sd["state"]) == len(names)
    i = names.index("conv_last.weight")              # (deep layers' buffers drift further apart with the fp32 / fp64 ReLU gates)
    got_b = sgd_sd["state"][i]["momentum_buffer"].double()
    assert got_b.shape == bufs[i].shape
    assert (got_b - bufs[i]).abs().max().item() <= 2e-3 * bufs[i].abs().max().item()


def test_pretrain_genesis_two_epochs_checkpoint_loads(tmp_path):
    import pickle
    from types import SimpleNamespace
    from cmunet_amd import genesis as G, train
    rng = np.random.RandomState(6)
    imgs = rng.standard_normal((16, 64, 64)).astype(np.float32)
    cfg = G.GenesisConfig(batch_size=4, nb_epoch=2, model_path=str(tmp_path))
    res = G.pretrain_genesis(cfg, imgs[:12], imgs[12:], seed=3, base_ch=16, depth=3, losses_dir=str(tmp_path), log=lambda *a: None)
    assert res["epochs_run"] == 2
    d = pickle.load(open(res["losses_path"], "rb"))
    assert set(d) == {"train_losses", "valid_losses"} and set(d["train_losses"]) == {"fold_0", "fold_1"}
    assert len(d["train_losses"]["fold_0"]) == 3 and len(d["valid_losses"]["fold_1"]) == 1
    assert all(v == round(v, 2) for v in d["train_losses"]["fold_1"])
    ck = torch.load(res["checkpoint"], weights_only=False)
    assert ck["epoch"] in (1, 2)
    model = train.load_model(SimpleNamespace(pretrained=res["checkpoint"], base_ch=16, depth=3))
    assert torch.equal(dict(model.named_parameters())["down_conv1.double_conv.double_conv.0.weight"].detach().cpu(),
                       ck["state_dict"]["module.down_conv1.double_conv.double_conv.0.weight"])
    n = len(list(model.parameters()))
    params = [torch.zeros_like(p).requires_grad_(True) for p in model.parameters()]
    torch.optim.SGD(params, 1e-2, momentum=0.9).load_state_dict(ck["optimizer_state_dict"])
    assert len(ck["optimizer_state_dict"]["state"]) == n
    # resume from the checkpoint: epoch and momentum restored
    cfg2 = G.GenesisConfig(batch_size=4, nb_epoch=ck["epoch"] + 1, model_path=str(tmp_path / "r"), weights=res["checkpoint"])
    res2 = G.pretrain_genesis(cfg2, imgs[:12], imgs[12:], seed=4, base_ch=16, depth=3, losses_dir=str(tmp_path), log=lambda *a: None)
    assert res2["epochs_run"] == 1
