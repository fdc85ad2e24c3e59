"""Host-side runtime behaviour of the HIP path on the GPU: device binding of the C-ABI launches, the shared loss / metric
pass and its cache, the dynamic loss scaler (AmpOptimWrapper of cmunet_config.py:76-78 = torch GradScaler's protocol)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def test_seg_stats_cache_is_keyed_on_tensor_identity(cuda):
    """Two successive no-grad evaluations whose tensors are freed in between: the caching allocator hands the second batch the
    first batch's addresses (version 0 again) -- the loss / Dice / IoU must be those of the second batch."""
    from cmunet_amd import metrics as M
    from oracle import losses as OL
    crit = M.DiceLoss(activation="softmax", threshold=0.5, ignore_channels=[0]) + M.CrossEntropyLoss()
    iou = M.IoU(threshold=0.5, activation="softmax", ignore_channels=[0])
    g = torch.Generator().manual_seed(0)
    seen_ptrs, vals = [], []
    for it in range(6):            # (tensors of 2 / 4 MB: the freed blocks are the only ones of their size in the allocator's pools)
        lo = torch.randn(2, 2, 256, 256, generator=g)
        y1 = (torch.rand(2, 256, 256, generator=g) > 0.7).double()
        y = torch.stack([1 - y1, y1], 1)
        with torch.no_grad():
            p, t = lo.to(cuda), y.to(cuda)
            seen_ptrs.append((p.data_ptr(), t.data_ptr()))
            got = (float(crit(p, t)), float(iou(p, t)))
        del p, t
        ref = (float(OL.dice_ce_loss(lo, y)), float(OL.iou_loss(lo, y)))
        vals.append(got)
        assert abs(got[0] - ref[0]) <= 1e-5 and abs(got[1] - ref[1]) <= 1e-6, (it, got, ref)
    assert len(set(seen_ptrs)) < 6, "the allocator did not reuse the addresses: the scenario was not exercised"
    assert len({v[0] for v in vals}) == 6
    # one pair evaluated by several objects -> one fused pass (same output tensor)
    p, t = torch.randn(1, 2, 16, 16).to(cuda), torch.zeros(1, 2, 16, 16, dtype=torch.float64).to(cuda)
    assert M.seg_stats(p, t) is M.seg_stats(p, t)
    p.add_(1.0)                                                      # in-place change: new pass
    a = M.seg_stats(p, t)
    p.add_(1.0)
    assert M.seg_stats(p, t) is not a


def test_amp_scaler_protocol(cuda):
    """cmu_amp_*: scale on the device; clean steps unscale exactly (power of two) and count towards growth, an inf / nan skips
    the update, halves the scale and resets the tracker; Adam's bias corrections use the number of updates actually taken."""
    from cmunet_amd import ops
    n = 1000
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(5)]
    amp = ops.AmpScaler(cuda, init_scale=1024.0, growth_interval=2)
    p, m, v = p0.clone().to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-2, betas=(0.9, 0.95), weight_decay=0.05)
    sched = [False, True, False, False, False]                       # step 1 carries an inf
    scale, clean = 1024.0, 0
    for it, (gr, bad) in enumerate(zip(grads, sched)):
        gs = (gr * scale).to(cuda)
        if bad:
            gs[17] = float("inf")
        amp.check(gs)
        ops.adam_step(p, gs, m, v, None, 1e-2, 0.9, 0.95, 1e-8, 0.05, True, 10 ** 6, 1.0, amp)    # host step number is ignored
        amp.update()
        if not bad:
            opt.zero_grad()
            ref.grad = gr.clone()
            opt.step()
        assert (p.cpu() - ref.detach()).abs().max().item() <= 2e-6, it
        if bad:
            scale, clean = scale * 0.5, 0
        else:
            clean += 1
            if clean == 2:
                scale, clean = scale * 2.0, 0
    sc, found, tracker, good, skipped = amp.read()
    # clean, skip (x0.5, tracker 0), clean, clean (growth x2, tracker 0), clean
    assert (sc, found, tracker, good, skipped) == (1024.0, 0.0, 1, 4, 1)
    gn = torch.full((n,), float("nan"), device=cuda)
    amp.check(gn)
    assert amp.read()[1] == 1.0


def test_adam_ema_fused_is_bit_identical_to_two_launches(cuda):
    """cmu_adam_ema_step (AdamW + the momentum networks' EMA in one pass over the arena: JointPretrainer's optimiser launch) against
    cmu_adam_step followed by cmu_ema_update per segment: identical bits in parameters, moments and targets, over three steps, with
    a weight-decay mask, under the loss scaler (one step skipped by an inf: the EMA still runs, as MomentumUpdateHook does behind
    a skipped optimiser step), and for elements outside every segment."""
    from cmunet_amd import ops
    n = 4096 + 512
    segs = [(256, 1280), (2048, 4096)]
    g = torch.Generator().manual_seed(3)
    p0, t0 = torch.randn(n, generator=g), [torch.randn(hi - lo, generator=g) for lo, hi in segs]
    wd_mask = (torch.rand(n, generator=g) > 0.3).to(torch.uint8).to(cuda)
    for use_amp in (False, True):
        pa, pb = p0.clone().to(cuda), p0.clone().to(cuda)
        ma, va, mb, vb = (torch.zeros(n, device=cuda) for _ in range(4))
        ta, tb = [t.clone().to(cuda) for t in t0], [t.clone().to(cuda) for t in t0]
        amp_a = ops.AmpScaler(cuda, init_scale=256.0) if use_amp else None
        amp_b = ops.AmpScaler(cuda, init_scale=256.0) if use_amp else None
        for step in range(1, 5):
            gr = (torch.randn(n, generator=g) * (256.0 if use_amp else 1.0)).to(cuda)
            if use_amp and step == 2:
                gr[100] = float("inf")
            for amp in (amp_a, amp_b):
                if amp is not None:
                    amp.check(gr)
            ops.adam_step(pa, gr, ma, va, wd_mask, 1e-2, 0.9, 0.95, 1e-8, 0.05, True, step, 0.5, amp_a)
            for (lo, hi), t in zip(segs, ta):
                ops.ema_update(t, pa[lo:hi], 0.99)
            ops.adam_ema_step(pb, gr, mb, vb, wd_mask, 1e-2, 0.9, 0.95, 1e-8, 0.05, True, step, 0.5, amp_b,
                              [(lo, hi, t) for (lo, hi), t in zip(segs, tb)], 0.99)
            for amp in (amp_a, amp_b):
                if amp is not None:
                    amp.update()
            assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), (use_amp, step)
            for x, y in zip(ta, tb):
                assert torch.equal(x, y), (use_amp, step)
        assert not torch.equal(pa.cpu(), p0) and not torch.equal(ta[0].cpu(), t0[0])
        if use_amp:
            assert amp_b.read()[3:] == (3, 1)                  # three updates taken, one skipped
    from cmunet_amd._lib import CmuError
    with pytest.raises(CmuError):                              # segments must be multiples of four inside the arena
        ops.adam_ema_step(pb, gr, mb, vb, None, 1e-2, 0.9, 0.95, 1e-8, 0.0, True, 1, 1.0, None, [(2, 6, torch.zeros(4, device=cuda))], 0.9)


def test_amp_state_survives_a_checkpoint(cuda):
    """Advisor (round 2): under amp the AdamW kernel takes the bias-correction step from the scaler's ``good_steps``, so the scaler's
    state belongs in the optimiser checkpoint (mmengine's AmpOptimWrapper.state_dict carries ``loss_scaler``).  Train 6 steps, or 3 +
    save + restore into a FRESH trainer + 3: identical parameters.  A checkpoint without the scaler's state (an older build's) seeds
    the counter from the saved step number instead of restarting the bias corrections at 1."""
    from cmunet_amd import model as M, ops
    from cmunet_amd.pretrain import MaskedReconPretrainer, random_patch_mask_device
    from oracle import unet as OU
    sd = OU.make_state_dict(base_ch=16, depth=3, seed=4)
    g = torch.Generator(device=cuda).manual_seed(1)
    batches = [(torch.randn(4, 64, 64, generator=g, device=cuda), random_patch_mask_device(4, 64, 64, 16, 0.5, g, cuda)) for _ in range(6)]

    def trainer(state=None):
        n = M.UNet(base_ch=16, depth=3, dtype="f16")
        n.load_state_dict(sd if state is None else state)
        return n, MaskedReconPretrainer(n.to(cuda).train(), lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, amp=ops.AmpScaler(cuda, growth_interval=2))

    _, full = trainer()
    for x, m in batches:
        full.step(x, m)
    net, first = trainer()
    for x, m in batches[:3]:
        first.step(x, m)
    ck = {"model": {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, "trainer": first.state_dict()}
    assert ck["trainer"]["optimizer"]["loss_scaler"]["good_steps"] == 3 and ck["trainer"]["optimizer"]["loss_scaler"]["scale"] == 2 * 65536.0
    ck = {"model": ck["model"], "trainer": {"optimizer": {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v)
                                                         for k, v in ck["trainer"]["optimizer"].items()}}}
    _, second = trainer(ck["model"])
    second.load_state_dict(ck["trainer"])
    assert second.amp.read() == first.amp.read()
    for x, m in batches[3:]:
        second.step(x, m)
    assert torch.equal(second.flat.arena, full.flat.arena), float((second.flat.arena - full.flat.arena).abs().max())
    assert second.amp.read() == full.amp.read()
    # an older checkpoint: no scaler state -> the step counter comes from the saved step, not from 0
    old = {"optimizer": {k: v for k, v in ck["trainer"]["optimizer"].items() if k != "loss_scaler"}}
    _, third = trainer(ck["model"])
    third.load_state_dict(old)
    assert third.amp.read()[3] == 3
    for x, m in batches[3:]:
        third.step(x, m)
    assert (third.flat.arena - full.flat.arena).abs().max().item() <= 1e-3     # (only the scale history differs: 65536 against 131072)


def test_masked_recon_trainer_f16_amp_tracks_f32(cuda):
    """The bench's default arithmetic on a small model: f16 storage + dynamic loss scale follows the f32 trainer (loss within
    2 %), never skips a step from an overflow at the initial scale, and without the scale the f16 gradients of a large batch of
    pixels underflow (which is why the reference's AMP wrapper scales)."""
    from cmunet_amd import model as M
    from cmunet_amd.pretrain import MaskedReconPretrainer, random_patch_mask_device
    from oracle import unet as OU
    sd = OU.make_state_dict(base_ch=16, depth=3, seed=9)
    nets = {}
    for key, dt, amp in (("f32", "f32", False), ("f16amp", "f16", True)):
        n = M.UNet(base_ch=16, depth=3, dtype=dt)
        n.load_state_dict(sd)
        nets[key] = MaskedReconPretrainer(n.to(cuda).train(), lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, amp=amp)
    g = torch.Generator(device=cuda).manual_seed(0)
    for it in range(4):
        x = torch.randn(4, 64, 64, generator=g, device=cuda)
        mask = random_patch_mask_device(4, 64, 64, 16, 0.5, g, cuda)
        la, lb = float(nets["f32"].step(x, mask)), float(nets["f16amp"].step(x, mask))
        assert math.isfinite(lb) and abs(la - lb) <= 2e-2 * max(1.0, abs(la)), (it, la, lb)
    sc, _, tracker, good, skipped = nets["f16amp"].amp.read()
    assert (good, skipped, tracker) == (4, 0, 4) and sc == 65536.0
    a, b = nets["f32"].flat.arena, nets["f16amp"].flat.arena
    # 4 Adam steps of 1e-3: an element whose tiny gradient changes sign between the two arithmetics moves 2e-3 apart per step
    assert (a - b).abs().max().item() <= 8.1e-3 and (a - b).abs().mean().item() <= 8e-4, ((a - b).abs().max().item(), (a - b).abs().mean().item())


def test_launches_follow_the_tensors_device(cuda):
    """every C-ABI launch is bound to the device that owns its tensors (the reference's driver uses cuda:1,
    Finetuning/train.py:246,451).  With two GPUs: a model on cuda:1 runs there while the current device stays 0."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (tests/test_cpu_abi.py covers the mixed-device check without a GPU)")
    from cmunet_amd import model as M
    from oracle import unet as OU
    sd = OU.make_state_dict(base_ch=16, depth=3, seed=1)
    x = torch.randn(2, 32, 32, generator=torch.Generator().manual_seed(0))
    outs = []
    for d in (0, 1):
        net = M.UNet(base_ch=16, depth=3, dtype="f32")
        net.load_state_dict(sd)
        net = net.to(f"cuda:{d}").eval()
        torch.cuda.set_device(0)
        with torch.no_grad():
            outs.append(net(x.to(f"cuda:{d}")).cpu())
        assert torch.cuda.current_device() == 0
    assert torch.equal(outs[0], outs[1])
    ref = OU.unet_forward(x, sd, training=False)
    assert (outs[1] - ref).abs().max().item() <= 1e-3


def test_mfma_sustained_rate_probe(cuda):
    """bench.py's measured ceiling (cmu_mfma_sustained_rate): the pure MFMA loop reports a plausible rate and clock, and
    all-zero operands run at least as fast as dense random ones (the data-dependent power limit)."""
    from cmunet_amd import ops
    for fed in (False, True):
        dense, clk_d = ops.mfma_sustained_rate("f16", 0, lds_fed=fed, iters=20000, device=cuda)
        zero, clk_z = ops.mfma_sustained_rate("f16", 2, lds_fed=fed, iters=20000, device=cuda)
        print(f"sustained f16 MFMA ({'LDS-fed' if fed else 'registers'}): dense operands {dense:.0f} TFLOP/s @ {clk_d:.0f} MHz, "
              f"zero operands {zero:.0f} TFLOP/s @ {clk_z:.0f} MHz")
        assert 500.0 < dense < 2600.0 and 500.0 < zero < 2600.0
        assert 800.0 < clk_d < 2600.0 and 800.0 < clk_z < 2600.0
        assert zero > 0.97 * dense
    with pytest.raises(Exception, match="dt must be f16 or bf16"):
        ops.mfma_sustained_rate("f32", 0, iters=10, device=cuda)


def test_bench_dump_outputs_and_full(cuda, tmp_path):
    """bench.py at a small size, a plain run and a --full run side by side, both with --dump-outputs: the plain line holds the
    headline only, the --full line adds the roofline, the kernel tables and the CPU baseline; both dump the same arrays (seeded inputs,
    and the --full run's profiled pass comes after the dump), the loss being the one the line reports."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--size", "128"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CMU_DP_REHEARSE")}
    runs = {"plain": [], "full": ["--full"]}
    procs, lines = {}, {}
    try:
        for name, extra in runs.items():
            procs[name] = subprocess.Popen(argv + extra + ["--dump-outputs", str(tmp_path / name)], env=env,
                                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for name, pr in procs.items():
            so, se = pr.communicate(timeout=420)
            assert pr.returncode == 0, se[-2000:]
            lines[name] = json.loads([ln for ln in so.splitlines() if ln.startswith("{")][-1])
    finally:
        for pr in procs.values():
            if pr.poll() is None:
                pr.kill()
            pr.wait()
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        assert line["steps"] == 3 and line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "f16"
        assert line["ms_per_step"] > 0 and abs(line["value"] - 4 * 1000.0 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert not any(k in plain for k in ("roofline", "kernel_ms_per_step", "step_roofline", "cpu_baseline"))
    assert full["roofline"]["launches_per_step"] > 0 and full["kernel_ms_per_step"] and full["cpu_baseline"]["value"] > 0
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "loss.npy" in names and len(names) > 50
    assert sum(os.path.getsize(tmp_path / "plain" / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and np.isfinite(a).all(), n
        assert np.abs(a.astype(np.float64) - b).max(initial=0.0) <= 1e-6 * max(1.0, np.abs(b).max(initial=0.0)), n
    loss = np.load(tmp_path / "plain" / "loss.npy")
    assert loss.dtype == np.float64 and abs(loss[0] - plain["config"]["loss"]) <= 1e-5 * max(1.0, abs(loss[0]))
