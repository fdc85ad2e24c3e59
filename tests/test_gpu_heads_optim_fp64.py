"""The loss, optimiser and loss-scaler kernels (heads.hip, optim.hip, the SparK loss of sparse.hip, soft-clDice) op by op against
float64 references computed on the CPU from the same fp32 inputs.

Element-wise outputs are held to PER-ELEMENT bounds: a few fp32 unit roundoffs (U = 2^-24) of the magnitudes that enter that element,
so a wrong element of small magnitude cannot hide behind a large one elsewhere (a max-error / max-|ref| check would pass an Adam
update that is wrong where v is tiny).  Reductions keep a relative form; what it covers is stated next to each.  Optimiser steps
are compared one step at a time on the kernel's own state of the previous step, so errors do not compound.  Hyperparameters enter
the references as the fp32 values the kernels receive.  Sizes past each kernel's grid cap run the grid-stride passes.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # fp32 unit roundoff
INF, NAN = float("inf"), float("nan")
DEV = "cuda"
CAP_ADAM = 8192 * 256               # adam_kernel / sgd_kernel: elements per grid pass
CAP_ADAM_EMA = 16384 * 256 * 4      # adam_ema_kernel
CAP_EMA = 4096 * 256 * 4            # ema_kernel
CAP_CHECK = 8192 * 256 * 4          # amp_check_kernel
CAP_SCALE = 2048 * 256              # scale_by_device_scalar_kernel
CAP_CE_PIX = 1024 * 256             # ce_dice_kernel


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    return o


def f32(x):
    """A Python float as the kernels receive it (a C float), back in float64."""
    return float(np.float32(x))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def within(got, ref, bound, what):
    """|got - ref| <= bound element by element (NaN where the reference is NaN, equal infinities)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), f"{what}: infinities differ"
    err = (got - ref).abs().masked_fill(nan | inf, 0.0)
    bad = err > bound
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements outside the bound; first at flat index {i}: got "
                             f"{got.flatten()[i].item():.9g}, ref {ref.flatten()[i].item():.9g}, bound {bound.flatten()[i].item():.3g} "
                             f"(worst err / bound {ratio:.3g})")


# ------------------------------------------------------------------------------------------------
# dynamic loss scaler: torch's own CPU ops are the reference
# ------------------------------------------------------------------------------------------------
def torch_scaler_step(scale, tracker, g_cpu, growth, backoff, interval):
    """One GradScaler round on CPU tensors: the non-finite check (unscale by 1) and _amp_update_scale_; -> found_inf."""
    found = torch.zeros(1)
    torch._amp_foreach_non_finite_check_and_unscale_([g_cpu.clone()], found, torch.ones(1))
    torch._amp_update_scale_(scale, tracker, found, growth, backoff, interval)
    return float(found)


@pytest.mark.parametrize("interval", [1, 2, 7])
@pytest.mark.parametrize("init_scale", [1.0, 2.0 ** 16, 2.0 ** 126, 2.0 ** 127])
def test_amp_scaler_schedule_matches_torch(ops, interval, init_scale):
    """200 seeded steps with inf / -inf / NaN injected at random places (the float4 body, the n % 4 tail, the first and last
    element): found_inf after the check, then scale, growth tracker and the step counters after the update, every step.  A growth
    past the fp32 range keeps the old scale, as torch does (the scale must never become inf)."""
    n = 1003
    g = gen(1000 + interval + int(math.log2(init_scale)))
    amp = ops.AmpScaler(DEV, init_scale=init_scale, growth_factor=2.0, backoff_factor=0.5, growth_interval=interval)
    scale, tracker = torch.tensor([init_scale], dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    grads = torch.empty(n, device=DEV)
    good = skipped = 0
    for step in range(200):
        gc = torch.randn(n, generator=g) * 100.0
        kind = int(torch.randint(0, 6, (1,), generator=g))
        if kind >= 3:
            pos = [int(torch.randint(0, n, (1,), generator=g)), 0, n - 1, n - 2, 1000][int(torch.randint(0, 5, (1,), generator=g))]
            gc[pos] = (INF, -INF, NAN)[kind - 3]
        grads.copy_(gc)
        amp.check(grads)
        got = amp.read()
        found = torch_scaler_step(scale, tracker, gc, 2.0, 0.5, interval)
        assert got[1] == found, (step, got, found)
        amp.update()
        good, skipped = good + (found == 0.0), skipped + (found != 0.0)
        got = amp.read()
        assert got[0] == float(scale) and math.isfinite(got[0]), (step, got, float(scale))     # fp32 on both sides: exact
        assert got[1] == 0.0 and got[2] == int(tracker) and got[3] == good and got[4] == skipped, (step, got, int(tracker), good, skipped)


@pytest.mark.parametrize("n,pos", [(1, 0), (2, 1), (3, 2), (5, 4), (1001, 1000), (1002, 1001), (1003, 1002), (1004, 1003),
                                   (CAP_CHECK + 13, CAP_CHECK + 12), (CAP_CHECK + 16, CAP_CHECK + 15), (CAP_CHECK + 16, CAP_CHECK + 4)])
@pytest.mark.parametrize("bad", [INF, -INF, NAN])
def test_amp_check_finite_edges(ops, n, pos, bad):
    """A single non-finite value at the last element (n % 4 = 1, 2, 3, 0; n < 4) and past the first grid-stride pass: found;
    the same array with that element finite (values up to the fp32 maximum): not found.  Agrees with torch's check."""
    g = gen(n % 97)
    x = torch.randn(n, generator=g) * 1e30
    x[0] = 3.4028234663852886e38
    x[-1] = -3.4028234663852886e38 if n > 1 else x[-1]
    d = x.to(DEV)
    amp = ops.AmpScaler(DEV, init_scale=1.0)
    amp.check(d)
    found = torch.zeros(1)
    torch._amp_foreach_non_finite_check_and_unscale_([x.clone()], found, torch.ones(1))
    assert amp.read()[1] == float(found) == 0.0
    d[pos] = bad
    x[pos] = bad
    amp.check(d)
    torch._amp_foreach_non_finite_check_and_unscale_([x.clone()], found, torch.ones(1))
    assert amp.read()[1] == float(found) == 1.0


def test_amp_scale_never_grows_to_inf(ops):
    """The case the reference's GradScaler pins: scale 2^127, growth 2, interval 1 -> the scale stays 2^127 (torch 2.x
    _amp_update_scale_), the tracker restarts, and a later overflow still backs off to 2^126."""
    amp = ops.AmpScaler(DEV, init_scale=2.0 ** 127, growth_interval=1)
    g = torch.ones(8, device=DEV)
    for _ in range(3):
        amp.check(g)
        amp.update()
        scale, found, tracker, good, skipped = amp.read()
        assert scale == 2.0 ** 127 and tracker == 0, (scale, tracker)
    g[3] = INF
    amp.check(g)
    amp.update()
    assert amp.read()[0] == 2.0 ** 126


# ------------------------------------------------------------------------------------------------
# Adam / AdamW, fused AdamW + EMA, EMA
# ------------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, wdm, lr, b1, b2, eps, wd, decoupled, t, gscale):
    """torch.optim.Adam (L2) / AdamW (decoupled) for one step, in float64 from the fp32 state; -> new p, m, v and per-element
    bounds.  m: 4 U of the magnitudes entering b1*m + (1-b1)*g' (g' = g*s + wd*p may cancel); v: 6 U of b2*v + (1-b2)*g'^2 at those
    magnitudes; p: 8 U of |p| + the step + the step at m's magnitude (m's absolute error reaches the update through 1/denom)."""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    p, g, m, v = (x.double() for x in (p, g, m, v))
    w = wd * (wdm.double() if wdm is not None else torch.ones_like(p))
    gs = g * gscale
    if decoupled:
        p1, gg, mag_g = p * (1 - lr * w), gs, gs.abs()
    else:
        p1, gg, mag_g = p, gs + w * p, gs.abs() + (w * p).abs()
    m1 = b1 * m + (1 - b1) * gg
    v1 = b2 * v + (1 - b2) * gg * gg
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    step = (lr / bc1) * m1 / denom
    mag_m = b1 * m.abs() + (1 - b1) * mag_g
    bounds = (8 * U * (p.abs() + step.abs() + (lr / bc1) * mag_m / denom), 4 * U * mag_m, 6 * U * (b2 * v + (1 - b2) * mag_g ** 2))
    return (p1 - step, m1, v1), bounds


def adam_inputs(n, seed):
    """Parameters, gradients spread over 10^-4 .. 10 (v spans ten decades: elements with tiny v), some exact zero gradients, and a
    random weight-decay mask."""
    g = gen(seed)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 5 - 4) for _ in range(4)]
    for gr in grads:
        gr[torch.rand(n, generator=g) < 0.02] = 0.0
    mask = (torch.rand(n, generator=g) < 0.7).to(torch.uint8)
    return p, grads, mask


ADAM_CASES = [
    # decoupled, weight decay, wd mask, grad_scale, n
    (0, 0.0, False, 1.0, 1003),
    (0, 1e-2, True, 0.25, 1003),
    (1, 0.05, False, 1.0 / 3.0, 1003),
    (1, 0.05, True, 1.0, CAP_ADAM + 1003),
    (0, 1e-2, False, 0.5, CAP_ADAM + 5),
]


@pytest.mark.parametrize("use_amp", [False, True])
@pytest.mark.parametrize("case", ADAM_CASES)
def test_adam_step(ops, case, use_amp):
    """Three steps of cmu_adam_step; under amp the second one overflows (p, m, v bit-identical afterwards), the gradients are
    unscaled by the scaler's scale and the bias corrections count only the updates taken."""
    decoupled, wd, masked, gscale, n = case
    p0, grads, mask = adam_inputs(n, 7 + n % 11 + 3 * decoupled)
    lr, b1, b2, eps = 1e-3, 0.9, 0.95, 1e-8
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    wdm = mask.to(DEV) if masked else None
    amp = ops.AmpScaler(DEV, init_scale=2.0 ** 10, growth_interval=1000) if use_amp else None
    taken = 0
    for step in range(1, 4):
        gd = grads[step].to(DEV)
        skip = use_amp and step == 2
        if skip:
            gd[n - 1] = INF
        before = [t.cpu() for t in (p, m, v)]
        if amp is not None:
            scale = amp.read()[0]
            amp.check(gd)
        ops.adam_step(p, gd, m, v, wdm, lr, b1, b2, eps, wd, decoupled, step, gscale, amp)
        if amp is not None:
            amp.update()
        if skip:
            for a, b in zip(before, (p, m, v)):
                assert torch.equal(a, b.cpu()), "a skipped step changed the state"
            continue
        taken += 1
        refs, bounds = adam_ref(before[0], grads[step], before[1], before[2], mask if masked else None, lr, b1, b2, eps, wd, decoupled,
                                taken if amp is not None else step, f32(gscale) / (scale if amp is not None else 1.0))
        for got, ref, bd, name in zip((p, m, v), refs, bounds, "pmv"):
            within(got, ref, bd, f"adam step {step} {name}")


def ema_ref(t, o, mom):
    """t*m + o*(1-m) in float64; bound 3 U of the two terms (the product, the fused add, and 1-m rounded to fp32)."""
    m = f32(mom)
    t, o = t.double(), o.double()
    return t * m + o * (1 - m), 3 * U * (t.abs() * m + o.abs() * (1 - m))


@pytest.mark.parametrize("n", [1, 2, 3, 1003, CAP_EMA + 7, CAP_EMA + 8])
@pytest.mark.parametrize("mom", [0.996, 0.1])
def test_ema_update(ops, n, mom):
    """The n % 4 tail (block 0) and the float4 body past the first grid-stride pass."""
    g = gen(n % 1000)
    t, o = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    td = t.to(DEV)
    ops.ema_update(td, o.to(DEV), mom)
    ref, bd = ema_ref(t, o, mom)
    within(td, ref, bd, f"ema n={n}")


ADAM_EMA_CASES = [
    # n, segments [lo, hi), decoupled, amp
    (1004, [(0, 500), (500, 1004)], 1, False),                     # touching each other and both ends of the arena
    (1004, [(4, 400), (800, 1004)], 0, True),                      # a gap, the second touching the end
    (1004, [(0, 1004)], 1, True),
    (CAP_ADAM_EMA + 12, [(0, 8), (8, CAP_ADAM_EMA + 12)], 1, False),   # past the grid cap; the second segment spans it
]


@pytest.mark.parametrize("case", ADAM_EMA_CASES)
def test_adam_ema_step(ops, case):
    """cmu_adam_ema_step: the AdamW update (as test_adam_step) and target = target*m + p_new*(1-m) on the segments, the targets
    elsewhere untouched; a skipped step (amp) still runs the EMA with the unchanged parameters.  The first step is also checked
    bit-identical against cmu_adam_step followed by cmu_ema_update per segment (the header's promise)."""
    n, segs, decoupled, use_amp = case
    p0, grads, mask = adam_inputs(n, 31 + len(segs))
    lr, b1, b2, eps, wd, mom = 2e-3, 0.9, 0.999, 1e-8, 0.05, 0.99
    p, m, v, wdm = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), mask.to(DEV)
    tg = gen(5)
    targets = [torch.randn(hi - lo, generator=tg).to(DEV) for lo, hi in segs]
    amp = ops.AmpScaler(DEV, init_scale=2.0 ** 4, growth_interval=1000) if use_amp else None
    taken = 0
    for step in range(1, 4):
        gd = grads[step].to(DEV)
        skip = use_amp and step == 2
        if skip:
            gd[0] = NAN
        before = [t.cpu() for t in (p, m, v)]
        tbefore = [t.cpu() for t in targets]
        scale = 1.0
        if amp is not None:
            scale = amp.read()[0]
            amp.check(gd)
        if step == 1:
            twin = [t.clone() for t in (p, m, v)]
            ttwin = [t.clone() for t in targets]
            ops.adam_step(*twin[:1], gd, *twin[1:], wdm, lr, b1, b2, eps, wd, decoupled, step, 1.0, amp)
            for (lo, hi), t in zip(segs, ttwin):
                ops.ema_update(t, twin[0][lo:hi], mom)
        ops.adam_ema_step(p, gd, m, v, wdm, lr, b1, b2, eps, wd, decoupled, step, 1.0, amp,
                          [(lo, hi, t) for (lo, hi), t in zip(segs, targets)], mom)
        if step == 1:
            for a, b in zip(twin + ttwin, [p, m, v] + targets):
                assert torch.equal(a, b), "fused step differs from adam_step + ema_update"
        if amp is not None:
            amp.update()
        if skip:
            for a, b in zip(before, (p, m, v)):
                assert torch.equal(a, b.cpu()), "a skipped step changed the optimiser state"
        else:
            taken += 1
            refs, bounds = adam_ref(before[0], grads[step], before[1], before[2], mask, lr, b1, b2, eps, wd, decoupled,
                                    taken if amp is not None else step, 1.0 / scale)
            for got, ref, bd, name in zip((p, m, v), refs, bounds, "pmv"):
                within(got, ref, bd, f"adam_ema step {step} {name}")
        pn = p.cpu()
        for (lo, hi), t0, t in zip(segs, tbefore, targets):
            ref, bd = ema_ref(t0, pn[lo:hi], mom)             # on the kernel's own new parameters
            within(t, ref, bd, f"adam_ema step {step} target [{lo}, {hi})")


# ------------------------------------------------------------------------------------------------
# SGD: torch.optim.SGD itself, in float64, on the kernel's state
# ------------------------------------------------------------------------------------------------
def sgd_ref(p, g, buf, mask, lr, mom, damp, wd, nesterov, first, gscale):
    """One torch.optim.SGD step in float64 on the fp32 state (the wd mask as two parameter groups; ``first``: no momentum buffer
    yet) -> new p, buf and bounds: 4 U of the magnitudes entering the buffer (mom*|buf| + (1-damp)*(|g s| + wd|p|)) and the
    parameter (|p| + lr * that of the direction)."""
    lr, mom, damp, wd = (f32(x) for x in (lr, mom, damp, wd))
    P, G, B = p.double(), g.double() * gscale, buf.double()
    sel = mask.bool() if mask is not None else torch.ones(p.numel(), dtype=torch.bool)
    groups, idx = [], []
    for on in (True, False):
        ii = sel if on else ~sel
        if bool(ii.any()):
            t = torch.nn.Parameter(P[ii].clone())
            t.grad = G[ii].clone()
            groups.append({"params": [t], "weight_decay": wd if on else 0.0})
            idx.append(ii)
    opt = torch.optim.SGD(groups, lr=lr, momentum=mom, dampening=damp, nesterov=nesterov, foreach=False)
    if mom != 0 and not first:
        for grp, ii in zip(groups, idx):
            opt.state[grp["params"][0]]["momentum_buffer"] = B[ii].clone()
    opt.step()
    Pn, Bn = P.clone(), B.clone()
    for grp, ii in zip(groups, idx):
        Pn[ii] = grp["params"][0].detach()
        if mom != 0:
            Bn[ii] = opt.state[grp["params"][0]]["momentum_buffer"]
    mag_g = G.abs() + wd * sel.double() * P.abs()
    mag_b = mag_g if first else mom * B.abs() + (1 - damp) * mag_g
    mag_d = (mag_g + mom * mag_b if nesterov else mag_b) if mom != 0 else mag_g
    return (Pn, Bn), (4 * U * (P.abs() + lr * mag_d), 4 * U * mag_b)


SGD_CASES = [
    # momentum, dampening, weight decay, nesterov, wd mask, grad_scale, n
    (0.9, 0.0, 1e-4, False, False, 1.0, 1003),
    (0.9, 0.1, 1e-2, False, True, 0.5, 1003),
    (0.9, 0.0, 1e-2, True, True, 1.0 / 3.0, CAP_ADAM + 1003),
    (0.0, 0.0, 1e-2, False, False, 1.0, 1003),
    (0.5, 0.3, 0.0, False, False, 0.25, CAP_ADAM + 5),
]


@pytest.mark.parametrize("case", SGD_CASES)
def test_sgd_step(ops, case):
    mom, damp, wd, nesterov, masked, gscale, n = case
    p0, grads, mask = adam_inputs(n, 50 + n % 7)
    p, buf = p0.to(DEV), torch.zeros(n, device=DEV)
    wdm = mask.to(DEV) if masked else None
    for step in range(1, 4):
        before = [t.cpu() for t in (p, buf)]
        ops.sgd_step(p, grads[step].to(DEV), buf, wdm, 0.03, mom, damp, wd, nesterov, step, gscale)
        (pr, br), (bp, bb) = sgd_ref(before[0], grads[step], before[1], mask if masked else None, 0.03, mom, damp, wd, nesterov,
                                     step == 1, f32(gscale))
        within(p, pr, bp, f"sgd step {step} p")
        if mom != 0:
            within(buf, br, bb, f"sgd step {step} buf")


@pytest.mark.parametrize("damp,nesterov", [(0.0, False), (0.1, False), (0.0, True)])
def test_sgd_step_amp_skipped_first_step(ops, damp, nesterov):
    """Under the loss scaler the first update is the first one the scaler lets through: after an overflowing step 1, step 2 sets
    buf = g' as torch.optim.SGD does (it never ran step 1).  With dampening 0 the old host-step rule happened to agree; with
    dampening != 0 it took buf = (1 - dampening) g'.  Step 4 overflows again in the middle of the run."""
    n = 1003
    p0, grads, mask = adam_inputs(n, 77)
    grads = grads + [torch.randn(n, generator=gen(78)) for _ in range(2)]
    p, buf, wdm = p0.to(DEV), torch.zeros(n, device=DEV), mask.to(DEV)
    amp = ops.AmpScaler(DEV, init_scale=2.0 ** 8, growth_interval=2)
    taken = 0
    for step in range(1, 6):
        gd = grads[step].to(DEV)
        skip = step in (1, 4)
        if skip:
            gd[n // 2] = -INF
        before = [t.cpu() for t in (p, buf)]
        scale = amp.read()[0]
        amp.check(gd)
        ops.sgd_step_amp(p, gd, buf, wdm, 0.03, 0.9, damp, 1e-3, nesterov, step, 1.0, amp)
        amp.update()
        if skip:
            assert torch.equal(before[0], p.cpu()) and torch.equal(before[1], buf.cpu())
            continue
        (pr, br), (bp, bb) = sgd_ref(before[0], grads[step], before[1], mask, 0.03, 0.9, damp, 1e-3, nesterov, taken == 0, 1.0 / scale)
        taken += 1
        within(buf, br, bb, f"sgd amp step {step} buf")
        within(p, pr, bp, f"sgd amp step {step} p")


def _sgd_holder(shapes, seed):
    g = gen(seed)

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes])

    return Holder()


def test_fused_sgd_state_after_a_skipped_first_step(ops):
    """FusedSGD under the scaler against torch.optim.SGD behind a GradScaler-style skip: no momentum state after the skipped first
    step (torch has none), the buffers of the first update taken after it, and a resume (load_state_dict under a fresh scaler)
    that keeps using the loaded buffers."""
    from cmunet_amd.optim import FlatParams, FusedSGD
    shapes = [(5, 7), (13,), (2, 3, 3)]
    flat = FlatParams(_sgd_holder(shapes, 3).to(DEV))
    ref_params = [torch.nn.Parameter(flat.views[nm].detach().cpu().double().clone()) for nm in flat.names]
    opt = FusedSGD(flat, lr=0.05, momentum=0.9, dampening=0.2)
    ref = torch.optim.SGD(ref_params, lr=f32(0.05), momentum=f32(0.9), dampening=f32(0.2))
    amp = ops.AmpScaler(DEV, init_scale=4.0)
    g = gen(4)
    for step in range(1, 4):
        grads = [torch.randn(*s, generator=g) for s in shapes]
        for nm, gr in zip(flat.names, grads):
            flat.grad_views[nm].copy_(gr * amp.read()[0])
        if step == 1:
            flat.grad_views[flat.names[1]][3] = NAN
        amp.check(flat.grad)
        opt.step(amp=amp)
        amp.update()
        if step == 1:
            assert opt.state_dict()["state"] == {} and ref.state_dict()["state"] == {}
            continue
        for prm, gr in zip(ref_params, grads):
            prm.grad = gr.double()
        ref.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == sorted(ref.state_dict()["state"]) == [0, 1, 2]
    for i, prm in enumerate(ref_params):
        bref = ref.state[prm]["momentum_buffer"]
        within(sd["state"][i]["momentum_buffer"], bref, 16 * U * (bref.abs() + 1.0), f"momentum buffer {i}")
        within(flat.views[flat.names[i]], prm.detach(), 16 * U * (prm.detach().abs() + 1.0), f"parameter {i}")
    # resume under a fresh scaler: the loaded buffers are used, not replaced by the next gradient
    flat2 = FlatParams(_sgd_holder(shapes, 3).to(DEV))
    for nm in flat.names:
        flat2.views[nm].data.copy_(flat.views[nm].detach())
    opt2, amp2 = FusedSGD(flat2, lr=0.05, momentum=0.9, dampening=0.2), ops.AmpScaler(DEV, init_scale=4.0)
    opt2.load_state_dict(sd, amp=amp2)
    grads = [torch.randn(*s, generator=g) for s in shapes]
    for nm, gr in zip(flat2.names, grads):
        flat2.grad_views[nm].copy_(gr * 4.0)
    amp2.check(flat2.grad)
    opt2.step(amp=amp2)
    amp2.update()
    for prm, gr in zip(ref_params, grads):
        prm.grad = gr.double()
    ref.step()
    for i, prm in enumerate(ref_params):
        within(flat2.views[flat2.names[i]], prm.detach(), 16 * U * (prm.detach().abs() + 1.0), f"resumed parameter {i}")


# ------------------------------------------------------------------------------------------------
# LAMB against oracle/optim.py
# ------------------------------------------------------------------------------------------------
EPS_RED = 1e-5      # relative error allowed to LAMB's reductions: the global gradient norm (clip factor) and the per-tensor trust
                    # ratio, each a fixed-order sum of fp32 per-block partials (<= 4096 terms per block: ~ 24 U worst case)


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("variant", ["plain", "clip_adapt", "no_bias_corr"])
def test_lamb_step(ops, side, variant):
    """Tensors of exactly LAMB_BLK elements, of more than 64 blocks (the ratio kernel's lane stride), a zero tensor (weight norm 0:
    trust ratio 1), a zero-gradient tensor outside the decay group; the global gradient norm 2 % below / above max_grad_norm on
    step 1.  Per element: 8 U of the magnitudes of |p| and the update, plus EPS_RED of the step for the two reductions."""
    from cmunet_amd import _lib
    from cmunet_amd.optim import FlatParams, FusedLAMB
    from oracle import optim as OO
    blk = _lib.lib().cmu_lamb_block_elems()
    assert blk == 4096
    shapes = [(blk,), (65 * blk + 17,), (300,), (8191,), (37,)]
    wds = [0.02, 0.02, 0.02, 0.0, 0.0]
    flat = FlatParams(_sgd_holder(shapes, 9).to(DEV))
    flat.views[flat.names[2]].data.zero_()
    kw = dict(trust_clip=variant == "clip_adapt", always_adapt=variant == "clip_adapt")
    bias_correction = grad_averaging = variant != "no_bias_corr"
    lr, b1, b2, eps, max_norm, gscale = 0.02, 0.9, 0.98, 1e-6, 2.0, 0.5
    opt = FusedLAMB(flat, lr=lr, betas=(b1, b2), eps=eps, weight_decay=0.02, max_grad_norm=max_norm,
                    decay_filter=lambda name, prm: wds[int(name.split(".")[-1])] != 0.0, bias_correction=bias_correction,
                    grad_averaging=grad_averaging, **kw)
    g = gen(10)
    offs = [flat.offsets[nm] for nm in flat.names]
    for step in range(1, 4):
        grads = [torch.randn(*s, generator=g) * (0.01 if i == 1 else 1.0) for i, s in enumerate(shapes)]
        grads[4].zero_()
        if step == 1:
            norm = math.sqrt(sum(float((gr.double() * gscale).pow(2).sum()) for gr in grads))
            target = max_norm * (0.98 if side == "below" else 1.02)
            grads = [gr * (target / norm) for gr in grads]
        for nm, gr in zip(flat.names, grads):
            flat.grad_views[nm].copy_(gr)
        before = [t.cpu() for t in (flat.arena, opt.m, opt.v)]
        ops.lamb_step(flat.arena, flat.grad, opt.m, opt.v, opt.u, opt.tables, lr, b1, b2, eps, bias_correction, grad_averaging,
                      max_norm, kw["trust_clip"], kw["always_adapt"], step, gscale, opt.ws)
        P = [before[0][o:o + c].double().clone() for o, c in offs]
        M = [before[1][o:o + c].double().clone() for o, c in offs]
        V = [before[2][o:o + c].double().clone() for o, c in offs]
        G = [gr.flatten().float().double() * gscale for gr in grads]
        gn = OO.lamb_step(P, G, M, V, f32(lr), [f32(w) for w in wds], betas=(f32(b1), f32(b2)), eps=f32(eps),
                          bias_correction=bias_correction, grad_averaging=grad_averaging, max_grad_norm=max_norm,
                          trust_clip=kw["trust_clip"], always_adapt=kw["always_adapt"], step=step)
        assert abs(opt.global_grad_norm - gn) <= EPS_RED * gn, (opt.global_grad_norm, gn)
        clip = 1.0 / (gn / max_norm) if gn > max_norm else 1.0
        b3 = 1 - f32(b1) if grad_averaging else 1.0
        bc1 = 1 - f32(b1) ** step if bias_correction else 1.0
        bc2 = 1 - f32(b2) ** step if bias_correction else 1.0
        pa, ma, va = flat.arena.cpu(), opt.m.cpu(), opt.v.cpu()
        for t, (o, c) in enumerate(offs):
            p0, m0, v0 = (x[o:o + c].double() for x in before)
            gg = G[t] * clip
            mag_m = f32(b1) * m0.abs() + b3 * gg.abs()
            denom = V[t].sqrt() / math.sqrt(bc2) + f32(eps)
            upd = (M[t] / bc1) / denom + f32(wds[t]) * p0
            un = float(upd.norm())
            r = float((P[t] - p0).norm()) / (f32(lr) * un) if un > 0 else 1.0
            mag_u = (mag_m / bc1) / denom + f32(wds[t]) * p0.abs()
            within(ma[o:o + c], M[t], 4 * U * mag_m + EPS_RED * b3 * gg.abs(), f"lamb step {step} tensor {t} m")
            within(va[o:o + c], V[t], 6 * U * (f32(b2) * v0 + (1 - f32(b2)) * gg ** 2) + 2 * EPS_RED * (1 - f32(b2)) * gg ** 2,
                   f"lamb step {step} tensor {t} v")
            within(pa[o:o + c], P[t], 8 * U * (p0.abs() + f32(lr) * r * mag_u) + EPS_RED * (P[t] - p0).abs(),
                   f"lamb step {step} tensor {t} p")


# ------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------
MMSE_CASES = [
    # B, K, channel, H, W, storage offset (elements), loss_scale, amp scale
    (3, 2, 1, 20, 64, 0, 1.0, None),        # wave rows + float4 gradient
    (2, 2, 1, 3, 1024, 0, 3.0, 2.0 ** 12),  # the widest wave-rows shape
    (2, 3, 2, 5, 1028, 0, 1.0, 2.0 ** 3),   # W > 1024: block rows + float4 gradient
    (3, 2, 0, 7, 33, 0, 0.5, None),         # W % 4 != 0: block rows + scalar gradient
    (2, 3, 1, 6, 64, 1, 2.0, 2.0 ** 5),     # W % 4 == 0 on misaligned views: block rows + scalar gradient
]


@pytest.mark.parametrize("case", MMSE_CASES)
def test_masked_mse_forms(ops, case):
    """All four kernel forms of cmu_masked_mse_fwd_bwd against oracle.cmunet.masked_mse with float64 autograd, times loss_scale and
    the scaler's scale.  dlogits per element: 4 U of k*(|x| + |t|) plus EPS_ROW of k*(|t| + mean|img| * rstd) for the row's fp32
    mean / variance sums (EPS_ROW = 2 (W/64 + 16) U: the longest chain of adds in a row sum); the other channels exactly 0.  The
    loss is a reduction over every masked pixel: 1e-5 relative (the row statistics and the fp32 row sums; the final sum is fp64)."""
    from cmunet_amd import _lib
    from oracle import cmunet as OC
    B, K, ch, H, W, off, ls, amp_scale = case
    g = gen(200 + W)
    logits = torch.randn(B, K, H, W, generator=g)
    img = torch.randn(B, H, W, generator=g) * 2 + 1
    mask = (torch.rand(B, H, W, generator=g) > 0.4).to(torch.uint8)

    def place(t, dtype):
        buf = torch.zeros(t.numel() + off, dtype=dtype, device=DEV)
        buf[off:].copy_(t.flatten())
        return buf[off:].view(t.shape)

    ld, imd, md = place(logits, torch.float32), place(img, torch.float32), place(mask, torch.uint8)
    if off:
        assert ld.data_ptr() % 16 and imd.data_ptr() % 16 and md.data_ptr() % 4
    dl = place(torch.full(logits.shape, 7.0), torch.float32)
    loss = torch.empty(1, device=DEV)
    ws = torch.empty(_lib.lib().cmu_masked_mse_ws_bytes(B, H), dtype=torch.uint8, device=DEV)
    amp = ops.AmpScaler(DEV, init_scale=amp_scale) if amp_scale else None
    ops.masked_mse_fwd_bwd(ld, ch, imd, md, loss, dl, ls, ws, amp)
    lo = logits.double().requires_grad_(True)
    ref = OC.masked_mse(lo[:, ch], img.double(), mask)
    (ref * ls * (amp_scale or 1.0)).backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    im = img.double()
    mean, std = im.mean(-1, keepdim=True), (im.var(-1, keepdim=True) + 1e-6).sqrt()
    t = (im - mean) / std
    k = 2.0 * ls * (amp_scale or 1.0) / float(mask.sum())
    eps_row = 2 * (W / 64 + 16) * U
    x = logits[:, ch].double()
    bound = torch.zeros(B, K, H, W, dtype=torch.float64)
    bound[:, ch] = k * mask.double() * (4 * U * (x.abs() + t.abs()) + eps_row * (t.abs() + im.abs().mean(-1, keepdim=True) / std))
    within(dl, lo.grad, bound, f"masked mse dlogits {case}")


@pytest.mark.parametrize("case", ["large_onehot", "large_soft", "small_soft"])
def test_softmax_ce_dice(ops, case):
    """More than 262,144 pixels (the grid-stride path of every real finetuning batch), soft targets, exact ties p1 = 0.5 (not
    foreground: 'p > 0.5'), every other pixel at least 1e-3 from a tie.  dlogits per element: (loss_scale/npix) times 8 U of
    p*|y0 + y1| + |y|, plus 2 U of |l - lse| * p*|y0 + y1| (the rounded argument of exp).  Counters tp / sum pr / sum gt and Dice / IoU come from fp64 sums: 2 U of the value.
    CE: mean of per-pixel terms, each within 8 U of y*(|l| + |lse|)."""
    from cmunet_amd import _lib
    from oracle import losses as OL
    B, H, W = {"large_onehot": (5, 256, 256), "large_soft": (3, 240, 384), "small_soft": (2, 12, 20)}[case]
    npix = B * H * W
    if case.startswith("large"):
        assert npix > CAP_CE_PIX
    g = gen(300 + H)
    logits = torch.randn(B, 2, H, W, generator=g) * 2
    d = logits[:, 1] - logits[:, 0]
    near = d.abs() < 1e-3
    logits[:, 1] += torch.where(near, 2e-3 * torch.sign(d + 1e-30), torch.zeros_like(d))
    ties = torch.rand(B, H, W, generator=g) < 0.05
    logits[:, 1] = torch.where(ties, logits[:, 0], logits[:, 1])
    if case == "large_onehot":
        fg = (torch.rand(B, H, W, generator=g) > 0.6).double()
        y1h = torch.stack([1 - fg, fg], 1)
    else:
        y1 = torch.rand(B, H, W, generator=g, dtype=torch.float64)
        y1h = torch.stack([1 - y1, y1], 1)
    ls = 3.0 if case == "large_soft" else 1.0
    out, dl = torch.empty(6, device=DEV), torch.empty(B, 2, H, W, device=DEV)
    ws = torch.empty(_lib.lib().cmu_softmax_ce_dice_ws_bytes(B, H, W), dtype=torch.uint8, device=DEV)
    ops.softmax_ce_dice_fwd_bwd(logits.to(DEV), y1h.to(DEV), out, dl, ls, ws)
    o = out.cpu().double()
    lo = logits.double().requires_grad_(True)
    ce = OL.cross_entropy_prob(lo, y1h)
    (ce * ls).backward()
    L = logits.double()
    lse = torch.logsumexp(L, 1, keepdim=True)
    assert abs(o[0] - ce.item()) <= 8 * U * float((y1h * (L.abs() + lse.abs())).sum() / npix) + U * abs(ce.item())
    pr = (L[:, 1] > L[:, 0]).double()
    assert bool(((torch.softmax(L, 1)[:, 1] > 0.5).double() == pr).all())
    tp, spr, sgt = float((y1h[:, 1] * pr).sum()), float(pr.sum()), float(y1h[:, 1].sum())
    for got, want, name in ((o[3], tp, "tp"), (o[4], spr, "sum pr"), (o[5], sgt, "sum gt"),
                            (o[1], float(OL.dice_loss(L, y1h)), "dice"), (o[2], float(OL.iou_loss(L, y1h)), "iou")):
        assert abs(float(got) - want) <= 2 * U * abs(want) + 1e-12, (name, float(got), want)
    p = torch.softmax(L, 1)
    gs = f32(ls) / npix
    ys = y1h.sum(1, keepdim=True).abs()
    within(dl, lo.grad, gs * U * (8 * (p * ys + y1h.abs()) + 2 * (L - lse).abs() * p * ys), f"ce dlogits {case}")


def _rows_case(B, D, seed):
    """Rows of N(0,1) values plus a zero row and rows with norms 0.5, 0.9, 1.1 and 3 times F.normalize's eps (1e-12) -- none within
    10 % of it, where the backward switches form."""
    g = gen(seed)
    x = torch.randn(B, D, generator=g, dtype=torch.float64)
    x[1] = 0.0
    for r, nrm in zip(range(2, 6), (0.5e-12, 0.9e-12, 1.1e-12, 3e-12)):
        x[r] *= nrm / x[r].norm()
    return x.float()


@pytest.mark.parametrize("D", [1, 63, 300, 4096])
def test_l2_normalize_rows_and_bwd(ops, D):
    """F.normalize(x, dim=1) and its float64 autograd backward.  Forward per element: (D/256 + 16) U of |out| (the row's fp32 sum of
    squares, sqrt, reciprocal, product).  Backward per element: 2 (D/256 + 16) U of |dy|/n + |x| * sum|x*dy| / n^3 (the x.dy sum may
    cancel), with n = max(|x|, eps)."""
    B = 9
    x = _rows_case(B, D, 400 + D)
    dy = torch.randn(B, D, generator=gen(401 + D))
    out, dx = torch.empty(B, D, device=DEV), torch.empty(B, D, device=DEV)
    ops.l2_normalize_rows(x.to(DEV), out)
    ops.l2_normalize_rows_bwd(x.to(DEV), dy.to(DEV), dx)
    xd = x.double().requires_grad_(True)
    ref = F.normalize(xd, dim=1)
    ref.backward(dy.double())
    eps_d = (D / 256 + 16) * U
    within(out, ref.detach(), eps_d * ref.detach().abs(), f"l2 normalize D={D}")
    X, DY = x.double(), dy.double()
    n = X.norm(dim=1, keepdim=True)
    nc = n.clamp_min(1e-12)
    bound = 2 * eps_d * (DY.abs() / nc + (n > 1e-12).double() * X.abs() * (X * DY).abs().sum(1, keepdim=True) / nc ** 3)
    within(dx, xd.grad, bound, f"l2 normalize backward D={D}")


@pytest.mark.parametrize("B,N,D,rank", [(8, 8192, 63, 0), (4, 8192, 4096, 1), (5, 300, 1, 2), (6, 64, 300, 3), (3, 8192, 300, 0)])
def test_infonce_inbatch_limits(ops, B, N, D, rank):
    """cmu_infonce_inbatch_fwd_bwd at its limits (N up to 8192, D up to 4096, dynamic LDS of D + N floats, D not a multiple of 64)
    against oracle.cmunet.infonce_inbatch with float64 autograd.  Both outputs are reductions (over N keys and D features), so the
    bound of an element is relative to the magnitudes that enter it: per row loss 4e-5 of coef/B * (|lse| + 1/T) (the scores are
    fp32 dots amplified by 1/T); dpred 4e-5 of (sum_n |g_n k_nd| + |q_d| sum_d' |q_d'| sum_n |g_n k_nd'|) / |pred| (g = dloss/dscore)."""
    from oracle import cmunet as OC
    T, cw = 0.07, 1.0
    g = gen(500 + N + D)
    pred = torch.randn(B, D, generator=g)
    keys = F.normalize(torch.randn(N, D, generator=g, dtype=torch.float64), dim=1).float()
    loss, dp = torch.empty(1 + B, device=DEV), torch.empty(B, D, device=DEV)
    ops.infonce_inbatch_fwd_bwd(pred.to(DEV), keys.to(DEV), loss, dp, rank, T, cw)
    pd = pred.double().requires_grad_(True)
    K = keys.double()
    ref = OC.infonce_inbatch(pd, K, T, rank, cw)
    ref.backward()
    q = F.normalize(pred.double(), dim=1)
    sc = q @ K.t() / T
    lse = torch.logsumexp(sc, 1)
    coef = cw * 2 * T
    label = torch.arange(B) + B * rank
    rows = coef * (lse - sc[torch.arange(B), label]) / B
    within(loss[1:], rows, 4e-5 * coef / B * (lse.abs() + 1 / T), f"infonce row losses {(B, N, D)}")
    assert abs(loss[0].item() - ref.item()) <= 4e-5 * float((coef / B * (lse.abs() + 1 / T)).sum())
    gsc = coef / B * (torch.softmax(sc, 1) - F.one_hot(label, N).double()) / T
    a = gsc.abs() @ K.abs()                                        # sum_n |g_n k_nd|
    nrm = pred.double().norm(dim=1, keepdim=True)
    mag = (a + q.abs() * (q.abs() * a).sum(1, keepdim=True)) / nrm
    within(dp, pd.grad, 4e-5 * mag, f"infonce dpred {(B, N, D)}")


# ------------------------------------------------------------------------------------------------
# the pieces of the non-fused MoCo API
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 255, 4096])
def test_moco_logits_assemble_split_addpos(ops, K):
    """Rows of K + 1 logits (strides 2, 256, 4097): [q.k | lneg] / T, its backward split and dq += dlogits[:, 0] / T * k.
    Copies and products: U of the value (one rounding); q.k: (D/256 + 16) U of sum|q k| / T (a reduction over D); the fused
    add: 2 U of |c k| + |result|."""
    B, D, T = 5, 300, 0.07
    inv_t = 1.0 / T
    g = gen(600 + K)
    q, k = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    lneg = torch.randn(B, K, generator=g)
    logits = torch.empty(B, K + 1, device=DEV)
    ops.moco_logits_assemble(q.to(DEV), k.to(DEV), lneg.to(DEV), logits, inv_t)
    it = f32(inv_t)
    ref = torch.cat([(q.double() * k.double()).sum(1, keepdim=True), lneg.double()], 1) * it
    bound = torch.cat([(D / 256 + 16) * U * (q.double() * k.double()).abs().sum(1, keepdim=True) * it, U * (lneg.double() * it).abs()], 1)
    within(logits, ref, bound, f"moco logits K={K}")
    dlogits = torch.randn(B, K + 1, generator=g)
    dlneg = torch.empty(B, K, device=DEV)
    ops.moco_logits_split(dlogits.to(DEV), dlneg, inv_t)
    ref = dlogits[:, 1:].double() * it
    within(dlneg, ref, U * ref.abs(), f"moco split K={K}")
    dq0 = torch.randn(B, D, generator=g)
    dq = dq0.to(DEV)
    ops.moco_logits_addpos(dlogits.to(DEV), k.to(DEV), dq, inv_t)
    c = (dlogits[:, :1].double() * it).float().double()          # the kernel's fp32 coefficient
    ref = dq0.double() + c * k.double()
    within(dq, ref, 2 * U * ((c * k.double()).abs() + ref.abs()), f"moco addpos K={K}")


@pytest.mark.parametrize("N", [2, 257, 4097])
def test_row_cross_entropy(ops, N):
    """F.cross_entropy (mean) in float64, its gradient d mean / d logits, and the rank of the target (logits strictly above it), with
    exact ties to the target's logit in every row.  The kernel uses the fast exp / log: per element the bounds allow the exponent's
    scaling (2 U of |x - lse|) and the row's logsumexp (U * (|lse| + 4 |lse - max| + 2 log N + N/256 + 24)) besides 2 U of the
    value."""
    B = 7
    g = gen(700 + N)
    x = torch.randn(B, N, generator=g) * 3
    tgt = torch.randint(0, N, (B,), generator=g)
    for b in range(B):
        nt = min(3, N - 1)
        others = torch.randperm(N, generator=g)[: nt + 1]
        others = others[others != tgt[b]][:nt]
        x[b, others] = float(x[b, tgt[b]])
    loss, dl, rank = ops.row_cross_entropy(x.to(DEV), tgt.to(DEV), want_grad=True, want_rank=True)
    X = x.double().requires_grad_(True)
    ref = F.cross_entropy(X, tgt)
    ref.backward()
    Xd = x.double()
    lse = torch.logsumexp(Xd, 1, keepdim=True)
    mx = Xd.max(1, keepdim=True).values
    e_lse = U * (lse.abs() + 4 * (lse - mx).abs() + 2 * math.log(N) + N / 256 + 24)
    p = torch.softmax(Xd, 1)
    within(dl, X.grad, p / B * (2 * U * (Xd - lse).abs() + e_lse) + 2 * U * X.grad.abs(), f"row ce dlogits N={N}")
    rows = (lse[:, 0] - Xd[torch.arange(B), tgt])
    row_bound = e_lse[:, 0] + 2 * U * rows.abs()
    assert abs(loss.item() - ref.item()) <= float(row_bound.mean()) + (B / 256 + 10) * U * float(rows.abs().mean())
    assert torch.equal(rank.cpu().long(), (Xd > Xd[torch.arange(B), tgt].unsqueeze(1)).sum(1))


def test_row_cross_entropy_target_out_of_range_gives_nan(ops):
    """A target outside [0, N) (F.cross_entropy raises there): that row's loss and the mean are NaN, the other rows exact as usual."""
    from cmunet_amd import _lib
    B, N = 6, 129
    g = gen(710)
    x = torch.randn(B, N, generator=g)
    tgt = torch.randint(0, N, (B,), generator=g)
    tgt[1], tgt[4] = -1, N
    loss, rows = torch.empty(1, device=DEV), torch.empty(B, device=DEV)
    xd, td = x.to(DEV), tgt.to(DEV)
    _lib.call("cmu_row_cross_entropy", ops._p(xd), ops._p(td), ops._p(loss), ops._p(rows), None, None, B, N, ops._stream())
    r = rows.cpu().double()
    assert math.isnan(loss.item()) and math.isnan(r[1]) and math.isnan(r[4])
    ok = torch.tensor([0, 2, 3, 5])
    ref = F.cross_entropy(x.double()[ok], tgt[ok], reduction="none")
    lse = torch.logsumexp(x.double()[ok], 1)
    e_lse = U * (lse.abs() + 4 * (lse - x.double()[ok].max(1).values).abs() + 2 * math.log(N) + N / 256 + 24)
    within(r[ok], ref, e_lse + 2 * U * ref.abs(), "row losses")
    loss2, _, _ = ops.row_cross_entropy(xd, td, want_grad=False)
    assert math.isnan(loss2.item())


@pytest.mark.parametrize("n", [1, 1003, CAP_SCALE + 77])
def test_scale_by_device_scalar(ops, n):
    """v *= s[0] with s on the device, past the 2048-block grid cap: one rounding, U of the value."""
    g = gen(800 + n % 100)
    v = torch.randn(n, generator=g) * 1e3
    s = torch.tensor([0.37])
    vd = v.to(DEV)
    ops.scale_by_device_scalar(vd, s.to(DEV))
    ref = v.double() * float(s)
    within(vd, ref, U * ref.abs(), f"scale by device scalar n={n}")


# ------------------------------------------------------------------------------------------------
# SparK loss
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.0, 0.75, 1.0])
@pytest.mark.parametrize("p,f", [(16, 4), (32, 3)])
def test_spark_loss(ops, ratio, p, f):
    """oracle.spark.recon_loss with float64 autograd (times loss_scale): the masked patches' per-patch normalised L2.  Mask ratio 0
    (every patch kept: loss 0, no gradient), 0.75 and 1 (every patch masked).  drec per element: 4 U of k*(|rec| + |t|) plus
    EPS_PATCH of k*(|t| + mean|img| * rstd) for the patch's fp32 mean / variance sums (EPS_PATCH = 2 (p*p/256 + 16) U).  The loss: a
    reduction, 1e-5 relative."""
    from cmunet_amd import _lib
    from oracle import spark as OS
    B, H = 2, f * p
    g = gen(900 + p + int(ratio * 4))
    img = torch.randn(B, H, H, generator=g) * 1.5 + 0.3
    rec = torch.randn(B, H, H, generator=g)
    active = OS.make_active(B, f, ratio, generator=g)
    if ratio == 0.0:
        assert bool(active.all())
    if ratio == 1.0:
        assert not bool(active.any())
    ls = 2.0
    loss, drec = torch.empty(1, device=DEV), torch.full((B, H, H), 7.0, device=DEV)
    ws = torch.empty(_lib.lib().cmu_spark_loss_ws_bytes(B, f), dtype=torch.uint8, device=DEV)
    ops.spark_loss_fwd_bwd(rec.to(DEV), img.to(DEV), active.to(torch.uint8).to(DEV), loss, drec, ls, p, ws)
    rd = rec.double().view(B, 1, H, H).requires_grad_(True)
    ref = OS.recon_loss(img.double().view(B, 1, H, H), rd, active)
    (ref * ls).backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    # per-pixel target and patch statistics, laid out like the image
    ip = img.double().view(B, f, p, f, p)
    mean = ip.mean((2, 4), keepdim=True)
    std = (ip.var((2, 4), keepdim=True) + 1e-6).sqrt()
    amean = ip.abs().mean((2, 4), keepdim=True)
    t = ((ip - mean) / std).view(B, H, H)
    masked = (~active.view(B, f, 1, f, 1)).expand(B, f, p, f, p).reshape(B, H, H).double()
    k = 2.0 * ls / ((float((~active).sum()) + 1e-8) * p * p)
    eps_p = 2 * (p * p / 256 + 16) * U
    bound = k * masked * (4 * U * (rec.double().abs() + t.abs()) + eps_p * (t.abs() + (amean / std).expand(B, f, p, f, p).reshape(B, H, H)))
    within(drec, rd.grad.view(B, H, H), bound, f"spark drec p={p} ratio={ratio}")


# ------------------------------------------------------------------------------------------------
# soft-clDice
# ------------------------------------------------------------------------------------------------
CLD_SHAPES = [(2, 1, 7), (3, 2, 5), (2, 3, 3), (1, 17, 1), (2, 31, 45), (1, 64, 33)]


def _two_class_logits(B, H, W, g):
    """Logits with exact ties (p1 = 0.5: not foreground) and every other pixel at least 1e-3 from one."""
    lg = torch.randn(B, 2, H, W, generator=g)
    d = lg[:, 1] - lg[:, 0]
    lg[:, 1] += torch.where(d.abs() < 1e-3, 2e-3 * torch.sign(d + 1e-30), torch.zeros_like(d))
    ties = torch.rand(B, H, W, generator=g) < 0.1
    lg[:, 1] = torch.where(ties, lg[:, 0], lg[:, 1])
    return lg


@pytest.mark.parametrize("num_iter", [1, 3, 10])
@pytest.mark.parametrize("shape", CLD_SHAPES)
def test_soft_cldice_pieces(ops, shape, num_iter):
    """softmax2_threshold, soft_skeleton and cldice_sums called as metrics.soft_cldice calls them, against oracle.losses:
    binarised foreground exact; skeletons of 0/1 images exact (min / max / relu of 0 and 1); skeletons of [0, 1]-valued images within
    4 (num_iter + 1) U (three roundings per level, values <= 1); the four sums (non-negative terms) within (n/131072 + 16) U of
    the value; and the clDice loss of metrics.soft_cldice at this num_iter."""
    from cmunet_amd import metrics
    from oracle import losses as OL
    B, H, W = shape
    g = gen(1000 + H * 64 + W + num_iter)
    logits = _two_class_logits(B, H, W, g)
    fg = (torch.rand(B, H, W, generator=g) > 0.5).double()
    y1h = torch.stack([1 - fg, fg], 1)
    yp = torch.empty(B, H, W, device=DEV)
    ops.softmax2_threshold(logits.to(DEV), 0.5, yp)
    ref_yp = (torch.softmax(logits.double(), 1)[:, 1] > 0.5).double()
    assert torch.equal(yp.cpu().double(), ref_yp)
    yt = fg.float().to(DEV)
    sp, st = torch.empty_like(yp), torch.empty_like(yp)
    ops.soft_skeleton(yp, sp, num_iter)
    ops.soft_skeleton(yt, st, num_iter)
    ref_sp = OL.soft_skel(ref_yp.unsqueeze(1), num_iter)[:, 0]
    ref_st = OL.soft_skel(fg.unsqueeze(1), num_iter)[:, 0]
    assert torch.equal(sp.cpu().double(), ref_sp) and torch.equal(st.cpu().double(), ref_st)
    soft = torch.rand(B, H, W, generator=g)
    ss = torch.empty_like(yp)
    ops.soft_skeleton(soft.to(DEV), ss, num_iter)
    within(ss, OL.soft_skel(soft.double().unsqueeze(1), num_iter)[:, 0], 4 * (num_iter + 1) * U, f"soft skeleton of [0,1] {shape}")
    out4 = torch.empty(4, device=DEV)
    ops.cldice_sums(sp, yt, st, yp, out4)
    want = torch.stack([(ref_sp * fg).sum(), ref_sp.sum(), (ref_st * ref_yp).sum(), ref_st.sum()])
    within(out4, want, (B * H * W / 131072 + 16) * U * want, f"cldice sums {shape}")
    m = metrics.soft_cldice(activation="softmax", ignore_channels=[0])
    m.num_iter = num_iter
    got = float(m(logits.to(DEV), y1h.to(DEV)))
    ref = float(OL.soft_cldice(logits.double(), y1h, num_iter=num_iter))
    assert abs(got - ref) <= 1e-9 * max(1.0, abs(ref)), (got, ref)
