"""The kernels that run between the convolutions -- csrc/elementwise.hip (BatchNorm finalisation, BN+ReLU+max-pool, 1x1 head
forward, first-layer conv, layout converters), csrc/backward_elem.hip (BatchNorm+ReLU backward reduce / finalise / apply, max-pool
backward in its three modes, head backward and its fused BatchNorm apply, first-layer weight gradient) and the global-average-pool
pair of csrc/heads.hip -- entry point by entry point against the float64 references of tests/elem_fp64_ref.py (themselves proved
against torch's float64 autograd in tests/test_cpu_elem_ref.py), at f32, f16 and bf16.

Bounds (the convention of test_gpu_heads_optim_fp64.py; U = 2^-24):
  * pure moves (layout converters, zero fill at masked positions, bytes outside a channel slice, gap_bwd across the pixels of
    one channel): bit-exact;
  * element-wise outputs, per element: |got - ref| <= u_dt |ref| + k U m + tiny_dt, m = the sum of the magnitudes of the terms
    that enter the element, k = the number of fp32 roundings on the longest path of the kernel's expression -- counted, and written
    next to each check (``k=``);
  * sums, per output: |got - ref| <= k U sum |terms| with k from the kernel's fp32 chain: terms per thread (``chain``), then the
    fold of the workgroup (``fold_k``), then the cast of the float64 final pass (the helpers below restate the launchers' geometry);
  * the ReLU gate and the pool's arg-max are decided in float64 from the same fp32 vectors, without a tolerance band
    (``gate_is_safe`` is asserted on every input); a pool window whose arg-max the fp32 rounding may decide differently
    (``pool_ambiguous``) is compared by the sum of its four gradients, and such windows may be at most 1e-4 of a test's windows.
Stored intermediate gradients (the pool's dA, the head's dX) enter the references of the fused BatchNorm sums and of the
"never-stored" apply forms as the bits the stored form wrote, after those were checked against float64 themselves.

Not covered (they need tens of GB): the 2^20-workgroup cap of bn_bwd_apply / conv1x1_head_bn_apply / the uncapped max-pool apply,
and every ``> 2^31`` index branch (cmu_pixel_coords' 64-bit divisions, the head kernels' 64-bit (image, pixel) split).  The
cells forms and the conv kernels' fused BatchNorm epilogues stay with their own tests.  The first layer over its tile list
(cmu_conv3x3_c1_fwd_tiles, cmu_conv3x3_c1_wgrad_bn_tiles) is held to the same references restricted to the listed tiles.  NaN / inf inputs are out of scope: the
kernels' fmaxf squashes a NaN activation to 0 where ATen propagates it.

Every comparison records its worst err / bound in ``PARITY`` (group, dtype); profiles/elem_fp64_parity.txt is that table.
"""
import math

import numpy as np
import pytest
import torch

import elem_fp64_ref as R
from elem_fp64_ref import U, D, elem_bound, quant

pytestmark = pytest.mark.gpu

DTS = ["f32", "f16", "bf16"]
EPC = {"f32": 4, "f16": 8, "bf16": 8}             # elements per 16-byte chunk
DEV = "cuda"
EPS = 1e-5
RED_MAX_BLOCKS, POOLB_BLOCKS, HEADB_BLOCKS, HEADF_CAP, HEADA_CAP, POOLF_CAP = 2048, 2048, 768, 8192, 2048, 65536
C1W_BLOCKS, C1F_CAP, LAYOUT_CAP, GAPB_CAP, BN_MAX_SPLITS = 512, 2048, 8192, 4096, 256
PARITY = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    return o


def gen(seed):
    return torch.Generator().manual_seed(seed)


def within(got, ref, bound, what, dt="f32"):
    """|got - ref| <= bound element by element; records the worst err / bound under (what, dt)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()), f"{what}: non-finite values"
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    ratio = 0.0 if float(err.max() if err.numel() else 0.0) == 0.0 else ratio
    key = (what.split(":")[0], dt)
    PARITY[key] = max(PARITY.get(key, 0.0), ratio)
    print(f"[parity] {what} {dt}: worst err / bound {ratio:.3g} over {ref.numel()}")
    bad = err > bound
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what} ({dt}): {int(bad.sum())} of {ref.numel()} outside the bound; first at flat index {i}: got "
                             f"{got.flatten()[i].item():.9g}, ref {ref.flatten()[i].item():.9g}, bound {bound.flatten()[i].item():.3g} "
                             f"(worst err / bound {ratio:.3g})")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def ws_bytes(n):
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=DEV)


def lib():
    from cmunet_amd import _lib
    return _lib.lib()


SENT = 7.0


def to_act(ops, x, dt, pad=0, fill=SENT):
    """NHWC fp32 CPU tensor (already quantised) -> Act on the GPU; ``pad`` > 0: a channel slice [pad, pad + C) of a buffer 2 pad wider
    (pad a multiple of the 16-byte chunk), the rest filled with a sentinel."""
    B, H, W, C = x.shape
    buf = torch.full((B, H, W, C + 2 * pad), fill, dtype=R.TORCH_DT[dt])
    buf[..., pad:pad + C] = x.to(buf.dtype)
    return ops.Act(buf.to(DEV), pad, C)


def empty_act(ops, B, H, W, C, dt, pad=0, fill=SENT):
    return ops.Act(torch.full((B, H, W, C + 2 * pad), fill, dtype=R.TORCH_DT[dt], device=DEV), pad, C)


def read(a):
    return a.buf[..., a.coff:a.coff + a.C].float().cpu()


def slice_untouched(a, fill=SENT):
    return bool((a.buf[..., :a.coff] == fill).all()) and bool((a.buf[..., a.coff + a.C:] == fill).all())


def data(shape, dt, g, mul=1.5, add=0.3):
    return quant(torch.randn(*shape, generator=g) * mul + add, dt)


def cuda(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


# ---- the launchers' geometry, restated (backward_elem.hip: chunk_geometry, fold_rows / sum_over_rows) -----------------------------
def chunk_geometry(nchunk):
    cpb = min(nchunk, 256)
    return cpb, 256 // cpb, -(-nchunk // cpb)


def fold_k(cpb, ppb):
    """fp32 additions of the workgroup fold: a power-of-two chunk count <= 64 folds inside the wave (log2(64 / cpb) shuffle adds)
    and then the four waves (3 adds); otherwise the ppb rows meet in LDS (ppb - 1 adds)."""
    if cpb <= 64 and cpb & (cpb - 1) == 0:
        return int(math.log2(64 // cpb)) + 3
    return max(ppb - 1, 0)


def reduce_chain(n_items, C, dt, per_block, cap):
    """Terms one thread adds in a grid-stride reduction over ``n_items`` (pixels or pooled pixels): the grid is
    min(ceil(n / (ppb * per_block)), cap) workgroups of ppb items per pass; -> (trips per thread, fold additions)."""
    cpb, ppb, _ = chunk_geometry(C // EPC[dt])
    gx = max(1, min(-(-n_items // (ppb * per_block)), cap))
    return -(-n_items // (gx * ppb)), fold_k(cpb, ppb)


def bn_vectors(y, g, gate_off=True):
    """Realistic per-channel vectors from the data, as the fp32 values the kernels receive: mean / invstd of y, scale = gamma invstd with
    negative and (channel 0) zero gamma, and one channel (1) whose every activation is gated off."""
    C = y.shape[-1]
    yd = y.double().reshape(-1, C)
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    gamma = torch.randn(C, generator=g).double()
    gamma[0] = 0.0
    beta = torch.randn(C, generator=g).double() * 0.2
    if gate_off and C > 1:
        gamma[1], beta[1] = 0.5, -100.0
    sc, sh = gamma * invstd, beta - mean * gamma * invstd
    return sc.float(), sh.float(), mean.float(), invstd.float()


def check_sums(got_dgamma, got_dbeta, got_coef, ref, chain, fold, dt, what):
    """dbeta / coef[0]: chain - 1 additions + fold + the final cast -> k = chain + fold; dgamma / coef[1]: + 2 roundings of xhat =
    (v - mean) invstd and the product's -> k = chain + fold + 3.  coef = sums / count: the same chain at 1 / count."""
    k1, k2 = chain + fold, chain + fold + 3
    within(got_dbeta, ref["dbeta"], k1 * U * ref["mag1"], f"{what}: dbeta", dt)
    within(got_dgamma, ref["dgamma"], k2 * U * ref["mag2"], f"{what}: dgamma", dt)
    within(got_coef[0], ref["coef"][0], k1 * U * ref["mag1"] / ref["count"], f"{what}: coef c1", dt)
    within(got_coef[1], ref["coef"][1], k2 * U * ref["mag2"] / ref["count"], f"{what}: coef c2", dt)


K_APPLY = 5     # dY = sc * (dz - c1 - xh * c2), xh = (v - mu) * is: v - mu, * is, * c2, the subtraction, * sc


# ------------------------------------------------------------------------------------------------
# BatchNorm + ReLU backward: reduce, finalise, apply
# ------------------------------------------------------------------------------------------------
# (chunks per pixel, B, H, W, pad): chunk counts 1, 2, 8, 64 (wave fold), 128 / 256 (LDS fold, ppb 2 / 1), 9 / 18 / 136
# (sum_over_rows), 272 (two channel blocks, the second ragged); pixel counts below one trip, and ending mid-trip of the reduce's
# four-pixel passes: npix % (4 ppb) in {1, ppb, 4 ppb - 1}; 2 x 2 and 2 x W images; RED_MAX_BLOCKS: npix > 2048 * 4 * ppb.
BN_CASES = [(1, 1, 2, 2, 0), (1, 3, 2, 171, 1), (2, 1, 1, 513, 0), (8, 1, 3, 43, 0), (8, 2, 8, 10, 2), (8, 1, 15, 17, 0),
            (64, 1, 1, 17, 0), (64, 1, 4, 5, 1), (64, 1, 1, 31, 0), (128, 2, 3, 5, 0), (256, 2, 3, 5, 1), (9, 2, 6, 7, 0),
            (18, 2, 6, 7, 1), (136, 1, 6, 7, 0), (272, 2, 4, 4, 0), (64, 2, 130, 130, 0), (256, 1, 92, 92, 1)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", BN_CASES)
def test_bn_bwd_reduce_and_apply(ops, dt, case):
    nchunk, B, H, W, padc = case
    C, pad, npix = nchunk * EPC[dt], padc * EPC[dt], B * H * W
    g = gen(100 + nchunk + npix)
    y, dA = data((B, H, W, C), dt, g), data((B, H, W, C), dt, g, 1.0, 0.0)
    if C > 2:
        y[..., 2] = 0.625                                   # a constant channel: variance 0, invstd = 1 / sqrt(eps)
    sc, sh, mean, invstd = bn_vectors(y, g)
    assert R.gate_is_safe(y, sc, sh)
    ya = to_act(ops, y, dt, pad).with_transform(*cuda(sc, sh), 0)
    da = to_act(ops, dA, dt, pad)
    dgamma, dbeta, coef = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV)
    ops.bn_bwd_reduce(da, ya, *cuda(mean, invstd), dgamma, dbeta, coef, ws_bytes(lib().cmu_bn_bwd_ws_bytes(C)))
    dy = empty_act(ops, B, H, W, C, dt, pad)
    ops.bn_bwd_apply(da, ya, *cuda(mean, invstd), coef, dy)
    torch.cuda.synchronize()
    chain, fold = reduce_chain(npix, C, dt, 4, RED_MAX_BLOCKS)
    if case == (64, 2, 130, 130, 0):
        assert chain > 4, "this case is meant to run the grid-stride passes past RED_MAX_BLOCKS"
    check_sums(dgamma, dbeta, coef, R.bn_bwd_sums_ref(dA, y, sc, sh, mean, invstd), chain, fold, dt, "bn_bwd_reduce")
    ref, m = R.bn_bwd_apply_ref(dA, y, sc, sh, mean, invstd, coef.cpu())           # the fp32 coef the kernel received
    within(read(dy), ref, elem_bound(ref, m, K_APPLY, dt), "bn_bwd_apply: dY", dt)  # k=5
    assert slice_untouched(dy) and slice_untouched(da) and slice_untouched(ya)


def impulse_positions(npix, ppb, U_=4):
    """First pixel, last pixel, and each position of the last (partial) trip of a U-pixel unrolled loop."""
    trip = ppb * U_
    last0 = (npix - 1) // trip * trip
    return sorted({0, npix - 1} | {p for p in (last0 + u * ppb for u in range(U_)) if p < npix} | {max(last0 - 1, 0)})


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", [(8, 3, 5, 11), (64, 2, 3, 7), (9, 1, 6, 7), (128, 1, 3, 5), (16, 2, 258, 256)])
def test_bn_bwd_reduce_impulses(ops, dt, case):
    """A gradient of one 1.0 (all channels of one pixel, gate open there): dbeta = 1 exactly (adding zeros is exact: k=0, the cast is
    exact too), dgamma = xhat of that pixel within k=3 (v - mean, * invstd, the product).  A rounding bound over all pixels cannot
    see one dropped pixel; this can."""
    nchunk, B, H, W = case
    C, npix = nchunk * EPC[dt], B * H * W
    g = gen(200 + nchunk)
    y = data((B, H, W, C), dt, g)
    sc, sh, mean, invstd = bn_vectors(y, g, gate_off=False)
    sc[0] = 0.25
    ya = to_act(ops, y, dt)
    dgamma, dbeta, coef = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV)
    ws = ws_bytes(lib().cmu_bn_bwd_ws_bytes(C))
    _, ppb, _ = chunk_geometry(nchunk)
    pos = impulse_positions(npix, ppb)
    pos = pos if npix < 10000 else [0, npix - 1]
    for p in pos:
        dA = torch.zeros(B, H, W, C)
        dA.view(-1, C)[p] = 1.0
        yp = y.view(-1, C)[p].double()
        shp = torch.where(sc.double() * yp + sh.double() > 0, sh.double(), (1.0 - sc.double() * yp)).float()   # gate open at p
        assert R.gate_is_safe(y, sc, shp) and bool(R.gate_ref(y, sc, shp).view(-1, C)[p].all())
        ops.bn_bwd_reduce(to_act(ops, dA, dt), ya.with_transform(*cuda(sc, shp), 0), *cuda(mean, invstd), dgamma, dbeta, coef, ws)
        torch.cuda.synchronize()
        xh = (yp - mean.double()) * invstd.double()
        assert bool((dbeta.cpu() == 1.0).all()), (p, dbeta)
        within(dgamma, xh, 3 * U * xh.abs(), "bn_bwd_reduce impulse: dgamma", dt)                # k=3
        within(coef[1], xh / npix, 4 * U * xh.abs() / npix, "bn_bwd_reduce impulse: coef c2", dt)  # k=3 + the division's cast


@pytest.mark.parametrize("dt", DTS)
def test_all_zero_gradient(ops, dt):
    """dA = 0: every sum is exactly 0 and, with the zero coef that follows, dY = sc * (0 - 0 - xhat * 0) is exactly 0 -- in the
    plain, the pooled (two zero skips) and the head form."""
    nchunk, B, H, W, K = 8, 2, 6, 10, 2
    C, npix = nchunk * EPC[dt], B * H * W
    g = gen(250)
    y = data((B, H, W, C), dt, g)
    sc, sh, mean, invstd = bn_vectors(y, g)
    ya = to_act(ops, y, dt).with_transform(*cuda(sc, sh), 0)
    zero = lambda *s: to_act(ops, torch.zeros(*s), dt)
    new = lambda: (torch.full((C,), SENT, device=DEV), torch.full((C,), SENT, device=DEV), torch.full((2, C), SENT, device=DEV))
    outs = []
    dg, db, coef = new()
    ops.bn_bwd_reduce(zero(B, H, W, C), ya, *cuda(mean, invstd), dg, db, coef, ws_bytes(lib().cmu_bn_bwd_ws_bytes(C)))
    dy = empty_act(ops, B, H, W, C, dt)
    ops.bn_bwd_apply(zero(B, H, W, C), ya, *cuda(mean, invstd), coef, dy)
    outs.append((dg, db, coef, dy))
    dg, db, coef = new()
    ws = ws_bytes(lib().cmu_bn_bwd_ws_bytes(C))
    ops.maxpool_bwd(zero(B, H // 2, W // 2, C), zero(B, H, W, C), ya, None, *cuda(mean, invstd), ws, dSkip2=zero(B, H, W, C))
    ops.bn_bwd_finalize(ws, npix, dg, db, coef)
    dy = empty_act(ops, B, H, W, C, dt)
    ops.maxpool_bwd_apply(zero(B, H // 2, W // 2, C), zero(B, H, W, C), ya, *cuda(mean, invstd), coef, dy, dSkip2=zero(B, H, W, C))
    outs.append((dg, db, coef, dy))
    dg, db, coef = new()
    w, dl = torch.randn(K, C, generator=g).to(DEV), torch.zeros(B, K, H, W, device=DEV)
    dW, dbias, ws = torch.full((K, C), SENT, device=DEV), torch.full((K,), SENT, device=DEV), ws_bytes(lib().cmu_bn_bwd_ws_bytes(C))
    ops.conv1x1_head_bwd(dl, ya, w, None, dW, dbias, ws_bytes(lib().cmu_conv1x1_head_bwd_ws_bytes(B, H, W, C, K)), *cuda(mean, invstd), ws)
    ops.bn_bwd_finalize(ws, npix, dg, db, coef)
    dy = empty_act(ops, B, H, W, C, dt)
    ops.conv1x1_head_bn_apply(dl, ya, w, *cuda(mean, invstd), coef, dy)
    outs.append((dg, db, coef, dy))
    torch.cuda.synchronize()
    assert bool((dW == 0).all()) and bool((dbias == 0).all())
    for dg, db, coef, dy in outs:
        assert bool((dg == 0).all()) and bool((db == 0).all()) and bool((coef == 0).all()) and bool((read(dy) == 0).all())


MASKS = ["all", "none", "one", "random"]


def patch_mask(kind, B, f, g):
    if kind == "all":
        return torch.ones(B, f, f, dtype=torch.uint8)
    if kind == "none":
        return torch.zeros(B, f, f, dtype=torch.uint8)
    if kind == "one":
        m = torch.zeros(B, f, f, dtype=torch.uint8)
        m[B - 1, f - 1, 1] = 1
        return m
    return (torch.rand(B, f, f, generator=g) > 0.5).to(torch.uint8)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,shape", [(k, (2, 16, 16, 8, 4)) for k in MASKS] + [("random", (1, 256, 256, 64, 8)), ("random", (3, 8, 8, 9, 8))])
def test_bn_bwd_masked_and_rows(ops, dt, kind, shape):
    """Sparse BatchNorm backward: the patch-mask forms (pixel (y, x) looks up active[b, y >> s, x >> s]) and the pixel-list form
    see only the selected pixels; the apply writes exact zeros elsewhere.  1 x 256 x 256: past RED_MAX_BLOCKS."""
    B, H, W, nchunk, f = shape
    C, npix = nchunk * EPC[dt], B * H * W
    g = gen(300 + nchunk + len(kind))
    y, dA = data((B, H, W, C), dt, g), data((B, H, W, C), dt, g, 1.0, 0.0)
    sc, sh, mean, invstd = bn_vectors(y, g)
    assert R.gate_is_safe(y, sc, sh)
    active = patch_mask(kind, B, f, g)
    sel = R.expand_active(active, H, W)
    count = max(int(sel.sum()), 1)
    ya, da = to_act(ops, y, dt).with_transform(*cuda(sc, sh), 0), to_act(ops, dA, dt, EPC[dt])
    act_d = active.to(DEV)
    ref = R.bn_bwd_sums_ref(dA, y, sc, sh, mean, invstd, count=count, sel=sel)
    chain, fold = reduce_chain(npix, C, dt, 4, RED_MAX_BLOCKS)
    ws = ws_bytes(lib().cmu_bn_bwd_ws_bytes(C))
    dgamma, dbeta, coef = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV)
    ops.bn_bwd_reduce_masked(da, ya, *cuda(mean, invstd), dgamma, dbeta, coef, act_d, count, ws)
    torch.cuda.synchronize()
    check_sums(dgamma, dbeta, coef, ref, chain, fold, dt, "bn_bwd_reduce_masked")
    px = ops.PixelList(act_d, H, W)
    torch.cuda.synchronize()
    n_rows = int(px.count.cpu())
    assert n_rows == int(sel.sum()) and torch.equal(R.rows_to_sel(px.rows.cpu()[:n_rows], B, H, W), sel)
    dgamma2, dbeta2, coef2 = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV)
    ops.bn_bwd_reduce_rows(da, ya, *cuda(mean, invstd), dgamma2, dbeta2, coef2, px, count, ws)
    torch.cuda.synchronize()
    chain_r, fold_r = reduce_chain(px.capacity, C, dt, 4, RED_MAX_BLOCKS)
    check_sums(dgamma2, dbeta2, coef2, ref, chain_r, fold_r, dt, "bn_bwd_reduce_rows")
    dy = empty_act(ops, B, H, W, C, dt, EPC[dt])
    ops.bn_bwd_apply_masked(da, ya, *cuda(mean, invstd), coef, dy, act_d, cells=False)
    torch.cuda.synchronize()
    r, m = R.bn_bwd_apply_ref(dA, y, sc, sh, mean, invstd, coef.cpu(), sel=sel)
    got = read(dy)
    within(got, r, elem_bound(r, m, K_APPLY, dt) * sel.unsqueeze(-1), "bn_bwd_apply_masked: dY", dt)   # k=5; bound 0 (exact zeros) outside
    assert slice_untouched(dy)
    if kind == "none":
        assert bool((got == 0).all()) and bool((dbeta.cpu() == 0).all()) and bool((dgamma.cpu() == 0).all())


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 4096, 4097, 10000])
@pytest.mark.parametrize("C", [1, 17, 64, 65])
def test_bn_bwd_finalize_tiles(ops, rows, C):
    """Slab [rows][2][C] -> dbeta, dgamma, coef: float64 sums (their error enters at D = 2^-53 per row), one cast -> k=1 at |sum|
    plus rows D sum |terms|."""
    g = gen(rows + C)
    slab = torch.randn(rows, 2, C, generator=g) * (torch.rand(rows, 1, 1, generator=g) * 4)
    count = 3 * rows
    dgamma, dbeta, coef = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV)
    ops.bn_bwd_finalize_tiles(slab.to(DEV), count, dgamma, dbeta, coef, ws_bytes(lib().cmu_bn_finalize_ws_bytes(C)))
    torch.cuda.synchronize()
    ref = R.bn_bwd_finalize_tiles_ref(slab, count)
    for got, key, mag in ((dbeta, "dbeta", "mag1"), (dgamma, "dgamma", "mag2")):
        within(got, ref[key], U * ref[key].abs() + rows * D * ref[mag], f"bn_bwd_finalize_tiles: {key}")
    for i, mag in ((0, "mag1"), (1, "mag2")):
        within(coef[i], ref["coef"][i], U * ref["coef"][i].abs() + (rows + 1) * D * ref[mag] / count, f"bn_bwd_finalize_tiles: coef {i}")


# ------------------------------------------------------------------------------------------------
# BatchNorm statistics finalisation
# ------------------------------------------------------------------------------------------------
def finalize_bounds(fin, rows, count, g, b, cb, rm, rv, mom, training):
    """Per-output bounds of cmu_bn_finalize.  Training: the kernel works in float64 (a chain of at most ``rows`` + 40 additions:
    e64 = (rows + 40) D at the magnitudes S1, S2 of the slab) and casts each output once (1 U); running statistics are updated in fp32:
    (1 - mom), * running, the cast of the new value, * mom, the addition -> k=3 on the longest path.  Eval: fp32 throughout --
    invstd = 1 / sqrtf(rv + eps): k=3; scale = g invstd: k=4; shift = b + (cb - rm) scale: k=6; save_mean = rm - cb: k=1."""
    out = {}
    if training:
        S1, S2 = fin["mags"]
        n64 = (rows + 40) * D
        mean, invstd = fin["save_mean"], fin["save_invstd"]
        e_mean = n64 * S1
        e_var = n64 * (S2 + 2 * np.abs(mean) * S1 + mean * mean)
        e_inv = 0.5 * invstd ** 3 * e_var + 4 * D * invstd
        out["save_mean"] = U * np.abs(mean) + e_mean
        out["save_invstd"] = U * invstd + e_inv
        out["scale"] = U * np.abs(fin["scale"]) + np.abs(g) * e_inv
        out["shift"] = U * np.abs(fin["shift"]) + np.abs(g) * (e_mean * invstd + np.abs(mean) * e_inv) + 4 * D * (np.abs(b) + np.abs(mean * g * invstd))
        if rm is not None:
            out["running_mean"] = 3 * U * (np.abs((1 - mom) * rm) + np.abs(mom * (mean + cb))) + mom * e_mean
        if rv is not None:
            unb = fin["var"] * (count / (count - 1.0) if count > 1 else 1.0)
            out["running_var"] = 3 * U * (np.abs((1 - mom) * rv) + np.abs(mom * unb)) + 2 * mom * e_var
    else:
        invstd = fin["save_invstd"]
        out["save_invstd"] = 3 * U * invstd
        out["scale"] = 4 * U * np.abs(fin["scale"])
        out["shift"] = 6 * U * (np.abs(b) + np.abs((cb - rm) * fin["scale"]))
        out["save_mean"] = U * (np.abs(rm) + np.abs(cb))
    return out


def run_bn_finalize(ops, slab, count, C, bias, gamma, beta, rm, rv, mom, training, save=True, what="bn_finalize"):
    d = lambda t: None if t is None else t.clone().to(DEV)
    rm_d, rv_d = d(rm), d(rv)
    scale, shift = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    smean, sinv = (torch.empty(C, device=DEV), torch.empty(C, device=DEV)) if save else (None, None)
    ops.bn_finalize(d(slab), count, d(bias), d(gamma), d(beta), rm_d, rv_d, mom, EPS, training, scale, shift, smean, sinv,
                    ws_bytes(lib().cmu_bn_finalize_ws_bytes(C)))
    torch.cuda.synchronize()
    fin = R.bn_finalize_ref(slab, count, bias, gamma, beta, rm, rv, mom, EPS, training)
    n = lambda t, dflt: np.full(C, dflt) if t is None else t.double().numpy()
    mom32 = float(np.float32(mom))
    bounds = finalize_bounds(fin, 0 if slab is None else slab.shape[0], count, n(gamma, 1.0), n(beta, 0.0), n(bias, 0.0),
                             None if rm is None else rm.double().numpy(), None if rv is None else rv.double().numpy(), mom32, training)
    outs = {"scale": scale, "shift": shift, "save_mean": smean, "save_invstd": sinv}
    if training:
        outs.update(running_mean=rm_d, running_var=rv_d)
    else:
        assert torch.equal(rm_d.cpu(), rm) and torch.equal(rv_d.cpu(), rv), "eval must not touch the running statistics"
    for key, got in outs.items():
        if got is not None:
            within(got, torch.from_numpy(fin[key]), torch.from_numpy(bounds[key]), f"{what}: {key}")
    return fin


def make_slab(rows, C, g, ratio=3.0, count_per_row=3):
    """Rows of (sum, sum of squares) of ``count_per_row`` values ~ N(ratio std, std) per channel (channel-dependent std), as fp32;
    channel 0 (C > 2: channel 2) constant: its variance cancels to ~0 and may come out negative -> clamp."""
    std = (torch.rand(C, generator=g) + 0.5).double()
    v = torch.randn(rows, count_per_row, C, generator=g).double() * std + ratio * std
    if C > 2:
        v[..., 2] = 0.7
    return torch.stack([v.sum(1), (v * v).sum(1)], dim=1).float(), rows * count_per_row


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 4096, 4097, 10000])
@pytest.mark.parametrize("C", [1, 15, 16, 17, 48, 64, 65, 1024])
def test_bn_finalize_train(ops, rows, C):
    """Slab rows 1 .. 10,000 (nsplit 1 -> 256 = BN_MAX_SPLITS, per > 16), C around the 16- and 64-channel block edges; momentum
    0.1; the constant channel clamps a negative variance (invstd = 1 / sqrt(eps) within the float64 noise of the slab)."""
    g = gen(rows * 3 + C)
    slab, count = make_slab(rows, C, g)
    p = lambda s: torch.randn(C, generator=g) * s
    run_bn_finalize(ops, slab, count, C, p(1.0), torch.rand(C, generator=g) + 0.5, p(1.0), p(0.1), torch.rand(C, generator=g) + 0.5, 0.1, True)


@pytest.mark.parametrize("variant", ["count1", "count2", "mom0", "mom1", "ratio1e3", "no_gamma", "no_beta", "no_bias", "no_rm", "no_rv",
                                     "no_save", "eval", "eval_no_bias", "eval_no_affine"])
def test_bn_finalize_variants(ops, variant):
    C, g = 48, gen(len(variant))
    p = lambda s: torch.randn(C, generator=g) * s
    bias, gamma, beta, rm, rv = p(1.0), torch.rand(C, generator=g) + 0.5, p(1.0), p(0.1), torch.rand(C, generator=g) + 0.5
    slab, count = make_slab(40, C, g, ratio=1e3 if variant == "ratio1e3" else 3.0)     # |mean| / std = 1e3: the slab cancels
    mom, training, save = 0.1, not variant.startswith("eval"), variant != "no_save"
    if variant in ("count1", "count2"):
        n = int(variant[-1])
        v = torch.randn(n, C, generator=g)
        slab, count = torch.stack([v.sum(0), (v * v).sum(0)]).unsqueeze(0).contiguous(), n
    mom = {"mom0": 0.0, "mom1": 1.0}.get(variant, mom)
    gamma = None if variant in ("no_gamma", "eval_no_affine") else gamma
    beta = None if variant in ("no_beta", "eval_no_affine") else beta
    bias = None if variant in ("no_bias", "eval_no_bias") else bias
    rm = None if variant == "no_rm" else rm
    rv = None if variant == "no_rv" else rv
    fin = run_bn_finalize(ops, slab if training else None, count, C, bias, gamma, beta, rm, rv, mom, training, save, "bn_finalize variants")
    if variant == "count1":
        assert bool((fin["var"] <= 1e-5).all())


# ------------------------------------------------------------------------------------------------
# BN + ReLU + MaxPool2d(2): forward and the three backward modes
# ------------------------------------------------------------------------------------------------
def dyadic(shape, g, lo=-8, hi=9, step=16.0):
    return torch.randint(lo, hi, shape, generator=g).float() / step


def pool_inputs(case, dt, g):
    """-> y, sc, sh.  "ties": values, scale and shift small multiples of 2^-4 / 2^-2 (exact products): all-equal positive windows,
    all-negative windows, exact zeros under a non-zero gradient."""
    kind, nchunk, B, H, W = case
    C = nchunk * EPC[dt]
    if kind == "ties":
        y = dyadic((B, H, W, C), g, -3, 4, 4.0)
        y[0, 0:2, 0:2], y[0, 0:2, 2:4], y[B - 1, H - 2:, W - 2:] = 0.25, -0.5, 0.0
        sc, sh = dyadic((C,), g, -4, 5, 4.0), dyadic((C,), g, -2, 3, 8.0)
        return y, sc, sh
    y = data((B, H, W, C), dt, g)
    return y, torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.2


# (kind, chunks, B, H, W): 2 x 2 and 2 x W images, chunk counts across the folds, ties; 1 x 260 x 256 x 64 chunks: 16,640 pooled
# pixels > POOLB_BLOCKS * ppb * 2 = 16,384 (the grid-stride pass of the backward)
POOL_CASES = [("rand", 1, 1, 2, 2), ("rand", 8, 2, 2, 22), ("rand", 64, 1, 6, 10), ("rand", 9, 2, 4, 6), ("rand", 128, 1, 4, 6),
              ("rand", 272, 1, 2, 4), ("ties", 8, 2, 8, 12), ("ties", 2, 3, 6, 6), ("rand", 64, 1, 260, 256)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", POOL_CASES)
def test_bnrelu_maxpool_fwd(ops, dt, case):
    """max(0, fma(v, sc, sh)) over the window, rounded to the storage type: k=1 at the window's largest |v sc| + |sh|."""
    _, nchunk, B, H, W = case
    C, pad = nchunk * EPC[dt], EPC[dt]
    g = gen(400 + nchunk + H)
    y, sc, sh = pool_inputs(case, dt, g)
    ya = to_act(ops, y, dt, pad).with_transform(*cuda(sc, sh), 0)
    out = empty_act(ops, B, H // 2, W // 2, C, dt, pad)
    ops.bnrelu_maxpool_fwd(ya, out)
    torch.cuda.synchronize()
    ref, mag = R.pool_fwd_ref(y, sc, sh)
    within(read(out), ref, elem_bound(ref, mag, 1, dt), "bnrelu_maxpool_fwd: out", dt)     # k=1
    assert slice_untouched(out)


@pytest.mark.parametrize("dt", DTS)
def test_bnrelu_maxpool_fwd_past_the_grid_cap(ops, dt):
    """2 x 364 x 364 x 256 chunks: 16.96 M chunk items > POOLF_CAP * 256 = 16.78 M (the grid-stride pass).  Too large to reference in
    float64 as a whole: each image alone (below the cap) must give the batch's bits, and the first and last rows of each image
    are held to float64."""
    nchunk, B, H, W = 256, 2, 364, 364
    C = nchunk * EPC[dt]
    assert B * (H // 2) * (W // 2) * nchunk > POOLF_CAP * 256 > (H // 2) * (W // 2) * nchunk
    g = gen(77)
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.2
    y = torch.empty(B, H, W, C, dtype=R.TORCH_DT[dt])
    for b in range(B):
        for r in range(0, H, 52):
            y[b, r:r + 52] = (torch.randn(52, W, C, generator=g) * 1.5 + 0.3).to(y.dtype)
    ya = ops.Act(y.to(DEV), 0, C).with_transform(*cuda(sc, sh), 0)
    out = ops.new_act(B, H // 2, W // 2, C, dt, DEV)
    ops.bnrelu_maxpool_fwd(ya, out)
    for b in range(B):
        one = ops.new_act(1, H // 2, W // 2, C, dt, DEV)
        ops.bnrelu_maxpool_fwd(ops.Act(ya.buf[b:b + 1].contiguous(), 0, C, ya.scale, ya.shift, 0), one)
        torch.cuda.synchronize()
        assert bits_equal(one.buf[0], out.buf[b]), f"image {b}: batched and single-image outputs differ"
        for r0 in (0, H - 8):
            ref, mag = R.pool_fwd_ref(y[b:b + 1, r0:r0 + 8].float(), sc, sh)
            within(out.buf[b:b + 1, r0 // 2:r0 // 2 + 4].float().cpu(), ref, elem_bound(ref, mag, 1, dt), "bnrelu_maxpool_fwd past cap: out", dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", MASKS)
def test_bnrelu_maxpool_fwd_masked(ops, dt, kind):
    B, H, W, nchunk, f = 2, 16, 16, 8, 4
    C = nchunk * EPC[dt]
    g = gen(450 + len(kind))
    y, sc, sh = pool_inputs(("rand", nchunk, B, H, W), dt, g)
    active = patch_mask(kind, B, f, g)
    out = empty_act(ops, B, H // 2, W // 2, C, dt, EPC[dt])
    ops.bnrelu_maxpool_fwd_masked(to_act(ops, y, dt).with_transform(*cuda(sc, sh), 0), active.to(DEV), out)
    torch.cuda.synchronize()
    ref, mag = R.pool_fwd_ref(y, sc, sh, active)
    within(read(out), ref, elem_bound(ref, mag, 1, dt) * (mag > 0), "bnrelu_maxpool_fwd_masked: out", dt)   # k=1; exact zeros at masked windows
    assert slice_untouched(out)


def check_pool_grad(got, pb, dt, what):
    """dA per element (k = the number of skip gradients: one fp32 addition each; 0 skips: a move), ungated; windows with an
    ambiguous arg-max by the sum of their four gradients."""
    ref = pb["dA"]
    bound = elem_bound(ref, pb["mag"], pb["k"], dt)
    amb = pb["amb"]
    assert int(amb.sum()) <= 1e-4 * amb.numel(), f"{int(amb.sum())} ambiguous windows of {amb.numel()}"
    ambpix = R.unwindows(amb.unsqueeze(3).expand(-1, -1, -1, 4, -1))
    within(torch.where(ambpix, ref, got.double()), ref, bound, f"{what}: dA", dt)
    if bool(amb.any()):
        within(R.windows(got.double()).sum(3)[amb], R.windows(ref).sum(3)[amb], R.windows(bound).sum(3)[amb], f"{what}: dA (ambiguous windows)", dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("skips,case", [(s, c) for c in POOL_CASES for s in (0, 1, 2) if not (c[3] > 100 and s == 1)])   # (past the cap: 0 and 2 skips)
def test_maxpool_bwd_three_modes(ops, dt, skips, case):
    """Stored form (dA + fused BatchNorm sums), sums-only form, and maxpool_bwd_apply (dY straight from the pooled and skip gradients)."""
    kind, nchunk, B, H, W = case
    C, pad, npix = nchunk * EPC[dt], EPC[dt], B * H * W
    g = gen(500 + nchunk + H + skips)
    y, sc, sh = pool_inputs(case, dt, g)
    assert R.gate_is_safe(y, sc, sh)
    mk = (lambda s: quant(dyadic(s, g, -8, 9, 8.0), dt)) if kind == "ties" else (lambda s: data(s, dt, g, 1.0, 0.0))
    dP, dS = mk((B, H // 2, W // 2, C)), [mk((B, H, W, C)) for _ in range(skips)]
    _, _, mean, invstd = bn_vectors(y, g)
    ya = to_act(ops, y, dt, pad).with_transform(*cuda(sc, sh), 0)
    dpa, dsa = to_act(ops, dP, dt, pad), [to_act(ops, s, dt, pad * (i + 1)) for i, s in enumerate(dS)]
    s1, s2 = (dsa + [None, None])[:2]
    nws = lib().cmu_bn_bwd_ws_bytes(C)
    new = lambda: (torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV))
    # stored form
    dA = empty_act(ops, B, H, W, C, dt, pad)
    ws = ws_bytes(nws)
    ops.maxpool_bwd(dpa, s1, ya, dA, *cuda(mean, invstd), ws, dSkip2=s2)
    dg0, db0, coef0 = new()
    ops.bn_bwd_finalize(ws, npix, dg0, db0, coef0)
    # sums only
    ws1 = ws_bytes(nws)
    ops.maxpool_bwd(dpa, s1, ya, None, *cuda(mean, invstd), ws1, dSkip2=s2)
    dg1, db1, coef1 = new()
    ops.bn_bwd_finalize(ws1, npix, dg1, db1, coef1)
    # never-stored apply
    dY = empty_act(ops, B, H, W, C, dt, pad)
    ops.maxpool_bwd_apply(dpa, s1, ya, *cuda(mean, invstd), coef1, dY, dSkip2=s2)
    # without the fused sums
    dA2 = empty_act(ops, B, H, W, C, dt, 0)
    ops.maxpool_bwd(dpa, s1, ya, dA2, dSkip2=s2)
    torch.cuda.synchronize()
    pb = R.pool_bwd_ref(dP, dS, y, sc, sh)
    stored = read(dA)
    check_pool_grad(stored, pb, dt, "maxpool_bwd")
    assert slice_untouched(dA) and slice_untouched(dY) and bits_equal(read(dA2), stored)
    # the sums are taken on the gradient as stored: 4 terms per pooled pixel and thread
    trips, fold = reduce_chain(B * (H // 2) * (W // 2), C, dt, 2, POOLB_BLOCKS)
    if npix > 50000:
        assert trips > 2
    stored = R.as_stored(stored, pb["dA"])
    ref = R.bn_bwd_sums_ref(stored, y, sc, sh, mean, invstd)
    check_sums(dg0, db0, coef0, ref, 4 * trips, fold, dt, "maxpool_bwd fused sums")
    check_sums(dg1, db1, coef1, ref, 4 * trips, fold, dt, "maxpool_bwd sums only")
    r, m = R.bn_bwd_apply_ref(stored, y, sc, sh, mean, invstd, coef1.cpu())
    within(read(dY), r, elem_bound(r, m, K_APPLY, dt), "maxpool_bwd_apply: dY", dt)    # k=5


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("where", ["first", "last"])
def test_maxpool_bwd_impulses(ops, dt, where):
    """One 1.0 in the pooled gradient (first / last pooled pixel of the batch, 2 x 6 x 10: the last one sits in a partial trip):
    the fused sums are the one term of the window's arg-max position when its gate is open, exact zeros otherwise."""
    nchunk, B, H, W = 8, 2, 6, 10
    C = nchunk * EPC[dt]
    g = gen(600)
    y, sc, sh = pool_inputs(("rand", nchunk, B, H, W), dt, g)
    _, _, mean, invstd = bn_vectors(y, g)
    dP = torch.zeros(B, H // 2, W // 2, C)
    dP.view(-1, C)[0 if where == "first" else -1] = 1.0
    ws = ws_bytes(lib().cmu_bn_bwd_ws_bytes(C))
    ops.maxpool_bwd(to_act(ops, dP, dt), None, to_act(ops, y, dt).with_transform(*cuda(sc, sh), 0), None, *cuda(mean, invstd), ws)
    dg, db, coef = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV)
    ops.bn_bwd_finalize(ws, B * H * W, dg, db, coef)
    torch.cuda.synchronize()
    pb = R.pool_bwd_ref(dP, [], y, sc, sh)
    ref = R.bn_bwd_sums_ref(pb["dA"], y, sc, sh, mean, invstd)
    assert int(pb["amb"].sum()) == 0 and bool((ref["mag1"] <= 1).all()) and float(ref["mag1"].sum()) > 0
    assert torch.equal(db.cpu().double(), ref["dbeta"])                                          # k=0: 1.0 or 0.0
    within(dg, ref["dgamma"], 3 * U * ref["mag2"], "maxpool_bwd impulse: dgamma", dt)          # k=3


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("skip", [False, True])
def test_maxpool_bwd_masked(ops, dt, kind, skip):
    """Active windows as the dense form; the pixels of masked windows are left as they were."""
    B, H, W, nchunk, f = 2, 16, 16, 8, 4
    C = nchunk * EPC[dt]
    g = gen(650 + len(kind))
    y, sc, sh = pool_inputs(("rand", nchunk, B, H, W), dt, g)
    dP, dS = data((B, H // 2, W // 2, C), dt, g, 1.0, 0.0), [data((B, H, W, C), dt, g, 1.0, 0.0)] if skip else []
    active = patch_mask(kind, B, f, g)
    dA = empty_act(ops, B, H, W, C, dt, EPC[dt])
    ops.maxpool_bwd_masked(to_act(ops, dP, dt), to_act(ops, dS[0], dt) if skip else None,
                           to_act(ops, y, dt).with_transform(*cuda(sc, sh), 0), dA, active.to(DEV), cells=False)
    torch.cuda.synchronize()
    pb = R.pool_bwd_ref(dP, dS, y, sc, sh, active)
    wr = pb["written"].unsqueeze(-1)
    got = read(dA)
    assert bool((got[~pb["written"]] == SENT).all()) and slice_untouched(dA)
    pb["dA"], pb["mag"] = torch.where(wr, pb["dA"], torch.full((), SENT, dtype=torch.float64)), pb["mag"] * wr
    pb["amb"] = pb["amb"] & R.windows(wr.expand(-1, -1, -1, C))[..., 0, :]
    check_pool_grad(got, pb, dt, "maxpool_bwd_masked")


# ------------------------------------------------------------------------------------------------
# 1x1 head: forward, backward, fused BatchNorm apply
# ------------------------------------------------------------------------------------------------
def k_head_fwd(nchunk, dt):
    """act (1) + EPC fmas in the thread + log2(nchunk) shuffle additions + the bias (1)."""
    return 1 + EPC[dt] + int(math.log2(nchunk)) + 1


HEAD_SHAPES = [(37, 3, 3), (2, 10, 13), (1, 1, 1)]       # images smaller than one grid stride: the carried (image, pixel) counters cross images


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nchunk", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_conv1x1_head_fwd(ops, dt, nchunk, K):
    C = nchunk * EPC[dt]
    for i, (B, H, W) in enumerate(HEAD_SHAPES):
        g = gen(700 + nchunk + K + i)
        x = data((B, H, W, C), dt, g)
        w, b = torch.randn(K, C, generator=g) / C ** 0.5, torch.randn(K, generator=g)
        for tf in (True, False):
            sc, sh = (torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.3) if tf else (None, None)
            xa = to_act(ops, x, dt, EPC[dt] * i)
            logits = torch.full((B, K, H, W), SENT, device=DEV)
            ops.conv1x1_head_fwd(xa.with_transform(*cuda(sc, sh), 0) if tf else xa, *cuda(w, b), logits)
            torch.cuda.synchronize()
            ref, mag = R.head_fwd_ref(x, sc, sh, w, b)
            within(logits, ref, k_head_fwd(nchunk, dt) * U * mag, "conv1x1_head_fwd: logits", dt)


def head_bwd_case(ops, dt, nchunk, K, B, H, W, seed, pad=0, what="conv1x1_head_bwd", impulse=None):
    C, npix = nchunk * EPC[dt], B * H * W
    g = gen(seed)
    x = data((B, H, W, C), dt, g)
    w = torch.randn(K, C, generator=g) / C ** 0.5
    dl = torch.randn(B, K, H, W, generator=g)
    if impulse is not None:
        flat = torch.zeros(npix, K)
        flat[impulse] = 1.0
        dl = flat.view(B, H, W, K).permute(0, 3, 1, 2).contiguous()
    sc, sh, mean, invstd = bn_vectors(x, g)
    assert R.gate_is_safe(x, sc, sh)
    xa = to_act(ops, x, dt, pad).with_transform(*cuda(sc, sh), 0)
    nws, nbws = lib().cmu_conv1x1_head_bwd_ws_bytes(B, H, W, C, K), lib().cmu_bn_bwd_ws_bytes(C)
    new = lambda: (torch.empty(K, C, device=DEV), torch.empty(K, device=DEV))
    dl_d, w_d = cuda(dl, w)
    # with dX and the fused BatchNorm sums
    dX, (dW, db), bws = empty_act(ops, B, H, W, C, dt, pad), new(), ws_bytes(nbws)
    ops.conv1x1_head_bwd(dl_d, xa, w_d, dX, dW, db, ws_bytes(nws), *cuda(mean, invstd), bws)
    dg, dbt, coef = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV)
    ops.bn_bwd_finalize(bws, npix, dg, dbt, coef)
    # without dX (sums only), and without the sums
    (dW1, db1), bws1 = new(), ws_bytes(nbws)
    ops.conv1x1_head_bwd(dl_d, xa, w_d, None, dW1, db1, ws_bytes(nws), *cuda(mean, invstd), bws1)
    dg1, dbt1, coef1 = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(2, C, device=DEV)
    ops.bn_bwd_finalize(bws1, npix, dg1, dbt1, coef1)
    dX2, (dW2, db2) = empty_act(ops, B, H, W, C, dt, 0), new()
    ops.conv1x1_head_bwd(dl_d, xa, w_d, dX2, dW2, db2, ws_bytes(nws))
    dY = empty_act(ops, B, H, W, C, dt, pad)
    ops.conv1x1_head_bn_apply(dl_d, xa, w_d, *cuda(mean, invstd), coef1, dY)
    torch.cuda.synchronize()
    hb = R.head_bwd_ref(dl, x, sc, sh, w)
    stored = read(dX)
    within(stored, hb["dX"], elem_bound(hb["dX"], hb["magX"], K, dt), f"{what}: dX", dt)          # k=K: one fma per class
    assert bits_equal(read(dX2), stored) and slice_untouched(dX) and slice_untouched(dY)
    ppb = 256 // nchunk
    gx = max(1, min(-(-npix // (ppb * 4)), HEADB_BLOCKS))
    chain, fold = 4 * -(-npix // (gx * ppb * 4)), fold_k(nchunk, ppb)
    for a, b_ in ((dW, db), (dW1, db1), (dW2, db2)):
        within(a, hb["dW"], (chain + fold + 1) * U * hb["magW"], f"{what}: dW", dt)               # + 1: the activation's fma
        within(b_, hb["db"], (chain + fold) * U * hb["magb"], f"{what}: dbias", dt)
    stored = R.as_stored(stored, hb["dX"])                         # dX rounded to the storage type before it enters the sums
    ref = R.bn_bwd_sums_ref(stored, x, sc, sh, mean, invstd)
    check_sums(dg, dbt, coef, ref, chain, fold, dt, f"{what} fused sums")
    check_sums(dg1, dbt1, coef1, ref, chain, fold, dt, f"{what} sums only")
    r, m = R.bn_bwd_apply_ref(stored, x, sc, sh, mean, invstd, coef1.cpu())
    within(read(dY), r, elem_bound(r, m, K_APPLY, dt), f"{what.replace('_bwd', '_bn_apply')}: dY", dt)     # k=5
    return chain, hb, (dW, db, dg, dbt), ref


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nchunk", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_conv1x1_head_bwd_and_bn_apply(ops, dt, nchunk, K):
    """K = 1, 2: conv1x1_head_bn_apply runs bn_bwd_apply's head mode; K = 3, 8: the generic kernel."""
    for i, (B, H, W) in enumerate(HEAD_SHAPES):
        head_bwd_case(ops, dt, nchunk, K, B, H, W, 800 + nchunk + K + i, pad=EPC[dt] * (i % 2))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", [2, 3])
def test_conv1x1_head_past_the_grid_caps(ops, dt, K):
    """64 chunks (ppb = 4), 3 x 110 x 110 = 36,300 pixels: past HEADB_BLOCKS * 16 = 12,288 (backward) and HEADA_CAP * 16 = 32,768
    (the head mode of bn_bwd_apply, K = 2); then 600 images of 7 x 9 pixels: every grid step of the carried (image, pixel) counters
    crosses many images."""
    chain, _, _, _ = head_bwd_case(ops, dt, 64, K, 3, 110, 110, 900 + K, what="conv1x1_head_bwd past cap")
    assert chain > 4 and 3 * 110 * 110 > HEADA_CAP * 16
    head_bwd_case(ops, dt, 64, K, 600, 7, 9, 910 + K, what="conv1x1_head_bwd past cap")


@pytest.mark.parametrize("dt", DTS)
def test_conv1x1_head_fwd_past_the_grid_cap(ops, dt):
    """1 chunk per pixel (ppb = 256): 9 x 970 x 970 = 8.47 M pixels > HEADF_CAP * 1024 = 8.39 M."""
    nchunk, K = 1, 2
    C = nchunk * EPC[dt]
    for B, H, W in ((9, 970, 970),):
        assert B * H * W > HEADF_CAP * 1024
        g = gen(950 + H)
        x = data((B, H, W, C), dt, g)
        w, b = torch.randn(K, C, generator=g) / C ** 0.5, torch.randn(K, generator=g)
        sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.3
        logits = torch.empty(B, K, H, W, device=DEV)
        ops.conv1x1_head_fwd(to_act(ops, x, dt).with_transform(*cuda(sc, sh), 0), *cuda(w, b), logits)
        torch.cuda.synchronize()
        ref, mag = R.head_fwd_ref(x, sc, sh, w, b)
        within(logits, ref, k_head_fwd(nchunk, dt) * U * mag, "conv1x1_head_fwd past cap: logits", dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nchunk,K", [(8, 2), (64, 3)])
def test_conv1x1_head_bwd_impulses(ops, dt, nchunk, K):
    """dlogits = 1 at one pixel (all classes): dbias = 1 exactly, dW[k] = the activation of that pixel (k=1: its fma), the fused sums
    their single term -- first pixel, last pixel of the last image, each tail position of the four-pixel loop."""
    B, H, W = 5, 3, 7
    C, npix = nchunk * EPC[dt], B * H * W
    for p in impulse_positions(npix, 256 // nchunk):
        _, hb, (dW, db, dg, dbt), ref = head_bwd_case(ops, dt, nchunk, K, B, H, W, 990, impulse=p, what="conv1x1_head_bwd impulse")
        assert bool((db.cpu() == 1.0).all())
        within(dW, hb["dW"], 1 * U * hb["magW"], "conv1x1_head_bwd impulse: dW (single term)", dt)           # k=1
        within(dg, ref["dgamma"], 3 * U * ref["mag2"], "conv1x1_head_bwd impulse: dgamma (single term)", dt)   # k=3
        assert torch.equal(dbt.cpu().double(), ref["dbeta"])                                                   # the stored dX where the gate is open


# ------------------------------------------------------------------------------------------------
# first layer: direct conv forward (+ statistics) and weight gradient
# ------------------------------------------------------------------------------------------------
def c1_mask(masked, B, H, W, g):
    if not masked:
        return None
    m = (torch.rand(B, H, W, generator=g) > 0.5).to(torch.uint8)
    return m[:1].contiguous() if masked == 1 else m


def c1_chain(B, H, W, nchunk, cap, cout_fwd=None):
    """Terms per thread: tiles per workgroup x pixels per thread and tile; -> (chain, fold additions).  The forward kernel's
    statistics (``cout_fwd``) fold inside the wave only up to 32 chunks and 64 channels, through LDS (ppi - 1 additions) otherwise."""
    ntile = B * -(-H // 16) * -(-W // 16)
    ppi = 256 // nchunk
    fold = fold_k(nchunk, ppi)
    if cout_fwd is not None and not (nchunk & (nchunk - 1) == 0 and nchunk <= 32 and cout_fwd <= 64):
        fold = ppi - 1
    return -(-ntile // min(ntile, cap)) * -(-256 // ppi), fold


# (B, H, W, chunks): partial tiles, 2 x 2, a non-power-of-two chunk count, several tiles per workgroup past the caps
# (4 x 192 x 192: 576 tiles > C1W_BLOCKS = 512; 9 x 256 x 256: 2,304 tiles > C1F_CAP = 2,048)
C1_CASES = [(2, 20, 24, 4), (1, 2, 2, 1), (2, 5, 37, 6), (1, 16, 16, 16), (4, 192, 192, 2), (9, 256, 256, 2)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("masked", [0, 1, 2])
@pytest.mark.parametrize("case", C1_CASES)
def test_conv3x3_c1_fwd(ops, dt, masked, case):
    """y: a chain of 9 fmas -> k=9, then the storage rounding.  Statistics (of the fp32 value before that rounding), rows summed in
    float64 here: sum: chain + fold + 9 (the term's own error); sum of squares: chain + fold + 19 (the squared term: 2 x 9 + 1)."""
    B, H, W, nchunk = case
    Cout = nchunk * EPC[dt]
    g = gen(1000 + H + masked)
    x, w = torch.randn(B, H, W, generator=g), torch.randn(Cout, 1, 3, 3, generator=g) / 3
    mask = c1_mask(masked, B, H, W, g)
    ya = empty_act(ops, B, H, W, Cout, dt, EPC[dt])
    stats = ops.new_stats(B, H, W, Cout, DEV)
    ops.conv3x3_c1_fwd(*cuda(x, w), ya, stats, None if mask is None else mask.to(DEV), masked == 2)
    torch.cuda.synchronize()
    ref, mag = R.c1_fwd_ref(x, w, mask, masked == 2)
    within(read(ya), ref, elem_bound(ref, mag, 9, dt), "conv3x3_c1_fwd: y", dt)          # k=9
    assert slice_untouched(ya)
    chain, fold = c1_chain(B, H, W, nchunk, C1F_CAP, Cout)
    s = stats.double().sum(0).cpu()
    within(s[0], ref.sum((0, 1, 2)), (chain + fold + 9) * U * mag.sum((0, 1, 2)), "conv3x3_c1_fwd: stats sum", dt)
    within(s[1], (ref * ref).sum((0, 1, 2)), (chain + fold + 19) * U * (mag * mag).sum((0, 1, 2)), "conv3x3_c1_fwd: stats sum of squares", dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("masked", [0, 1, 2])
@pytest.mark.parametrize("case", C1_CASES[:5])
def test_conv3x3_c1_wgrad(ops, dt, masked, case):
    """dW[c][t] = sum_p dY[p][c] xm[p + t]: chain fmas + fold + the cast -> k = chain + fold; the fused BatchNorm form adds the
    5 roundings of the apply expression to every term."""
    B, H, W, nchunk = case
    Cout = nchunk * EPC[dt]
    g = gen(1100 + H + masked)
    x = torch.randn(B, H, W, generator=g)
    dY, yraw = data((B, H, W, Cout), dt, g, 1.0, 0.0), data((B, H, W, Cout), dt, g)
    mask = c1_mask(masked, B, H, W, g)
    mask_d = None if mask is None else mask.to(DEV)
    sc, sh, mean, invstd = bn_vectors(yraw, g)
    assert R.gate_is_safe(yraw, sc, sh)
    coef = torch.randn(2, Cout, generator=g) * 0.1
    ws = ws_bytes(lib().cmu_conv3x3_c1_wgrad_ws_bytes(B, H, W, Cout))
    dW, dWb = torch.empty(Cout, 1, 3, 3, device=DEV), torch.empty(Cout, 1, 3, 3, device=DEV)
    da = to_act(ops, dY, dt, EPC[dt])
    ops.conv3x3_c1_wgrad(x.to(DEV), da, dW, ws, mask_d, masked == 2)
    ops.conv3x3_c1_wgrad_bn(x.to(DEV), da, to_act(ops, yraw, dt, 2 * EPC[dt]), *cuda(sc, sh, mean, invstd, coef), dWb, ws, mask_d, masked == 2)
    torch.cuda.synchronize()
    chain, fold = c1_chain(B, H, W, nchunk, C1W_BLOCKS)
    ref, mag = R.c1_wgrad_ref(x, dY, mask, masked == 2)
    within(dW.view(Cout, 9), ref, (chain + fold) * U * mag, "conv3x3_c1_wgrad: dW", dt)
    r, m = R.bn_bwd_apply_ref(dY, yraw, sc, sh, mean, invstd, coef)
    ref, mag = R.c1_wgrad_ref(x, r, mask, masked == 2, mdY=m)
    within(dWb.view(Cout, 9), ref, (chain + fold + K_APPLY) * U * mag, "conv3x3_c1_wgrad_bn: dW", dt)


@pytest.mark.parametrize("dt", DTS)
def test_conv3x3_c1_wgrad_impulses(ops, dt):
    """dY = 1 at one pixel: dW[c][t] is the image's neighbour of that pixel at tap t, exactly (k=0: one exact product, zeros added) --
    first pixel, last pixel of the last image (a partial tile), a pixel in the middle of a later tile of the workgroup."""
    B, H, W, nchunk = 3, 20, 37, 4
    Cout = nchunk * EPC[dt]
    g = gen(1200)
    x = torch.randn(B, H, W, generator=g)
    ws = ws_bytes(lib().cmu_conv3x3_c1_wgrad_ws_bytes(B, H, W, Cout))
    taps = R.c1_taps(x.double()).view(-1, 9)
    for p in (0, B * H * W - 1, H * W + 17 * W + 33):
        dY = torch.zeros(B * H * W, Cout)
        dY[p] = 1.0
        dW = torch.empty(Cout, 1, 3, 3, device=DEV)
        ops.conv3x3_c1_wgrad(x.to(DEV), to_act(ops, dY.view(B, H, W, Cout), dt), dW, ws)
        torch.cuda.synchronize()
        assert torch.equal(dW.view(Cout, 9).cpu().double(), taps[p].expand(Cout, 9)), p


# ---- the first layer over its 16 x 16 tile list (SparK's sparse encoder) ---------------------------------------------------------------
def c1_tile_list(B, H, W, count, g):
    """A hand-built list of ``count`` distinct tiles in a fixed permutation; the entries past the count hold valid, UNLISTED tile ids.
    -> (list int32 (dense tile count,), sel (B, H, W) float64: 1 at the pixels of the listed tiles)."""
    tY, tX = -(-H // 16), -(-W // 16)
    nt = B * tY * tX
    assert 0 < count < nt
    perm = torch.randperm(nt, generator=g)
    tl = torch.cat([perm[:count], perm[count:][torch.arange(nt - count) % (nt - count)]]).to(torch.int32)
    on = torch.zeros(nt, dtype=torch.float64)
    on[perm[:count]] = 1.0
    sel = on.view(B, tY, 1, tX, 1).expand(B, tY, 16, tX, 16).reshape(B, tY * 16, tX * 16)[:, :H, :W].contiguous()
    return tl, sel


def c1_tiles_chain(count, max_tiles, nchunk, cap, cout_fwd=None):
    """The tile walk: min(max_tiles, cap) workgroups, workgroup i takes the list entries i, i + grid, ...: ceil(count / grid) tiles x
    the pixels per thread and tile of the dense kernels; the same folds (``c1_chain``)."""
    grid = min(max(int(max_tiles), 1), cap)
    ppi = 256 // nchunk
    fold = fold_k(nchunk, ppi)
    if cout_fwd is not None and not (nchunk & (nchunk - 1) == 0 and nchunk <= 32 and cout_fwd <= 64):
        fold = ppi - 1
    return -(-count // grid) * -(-256 // ppi), fold


# (B, H, W, chunks, listed tiles, max_tiles): partial tiles in both directions; a count below the host's bound (surplus workgroups write
# zero rows); a non-power-of-two chunk count; more listed tiles than C1W_BLOCKS = 512 workgroups (two tiles for some of them)
C1_TILE_CASES = [(2, 40, 56, 4, 9, 9), (3, 20, 37, 6, 5, 12), (1, 16, 48, 16, 2, 3), (4, 192, 192, 2, 530, 576)]


def namespace_tiles(tl, count):
    import types
    return types.SimpleNamespace(list=tl.to(DEV), count=torch.tensor([count], dtype=torch.int32, device=DEV), tile_h=16, tile_w=16)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("masked", [0, 2])
@pytest.mark.parametrize("case", C1_TILE_CASES)
def test_conv3x3_c1_over_a_tile_list(ops, dt, masked, case):
    """cmu_conv3x3_c1_fwd_tiles and cmu_conv3x3_c1_wgrad_bn_tiles (reading and recomputing form) against the float64 references of the
    dense entries, restricted to the listed tiles.  y: k=9 at the listed pixels, the sentinel elsewhere.  Statistics slab (rows summed in
    float64 here): k = chain + fold + 9 / + 19 as in test_conv3x3_c1_fwd, with the chain of the tile walk.  dW: k = chain + fold +
    K_APPLY as in test_conv3x3_c1_wgrad, both forms against the reference on the BITS the forward stored (the recomputing form must
    reproduce them).  dA is non-zero in the unlisted tiles, which must not count."""
    B, H, W, nchunk, count, max_tiles = case
    Cout = nchunk * EPC[dt]
    g = gen(1300 + H + masked)
    x, w = torch.randn(B, H, W, generator=g), torch.randn(Cout, 1, 3, 3, generator=g) / 3
    mask = c1_mask(masked, B, H, W, g)
    mask_d = None if mask is None else mask.to(DEV)
    tl, sel = c1_tile_list(B, H, W, count, g)
    tiles = namespace_tiles(tl, count)
    ya = empty_act(ops, B, H, W, Cout, dt, EPC[dt])
    slab = ops.conv3x3_c1_fwd_tiles(*cuda(x, w), ya, tiles, max_tiles, mask_d, masked == 2)
    torch.cuda.synchronize()
    assert slab.shape == (min(max_tiles, C1F_CAP), 2, Cout)
    ref, mag = R.c1_fwd_ref(x, w, mask, masked == 2)
    on = sel.bool()
    got = read(ya)
    within(got[on], ref[on], elem_bound(ref[on], mag[on], 9, dt), "conv3x3_c1_fwd_tiles: y", dt)          # k=9
    assert bool((got[~on] == SENT).all()) and slice_untouched(ya), "a pixel outside the listed tiles was written"
    chain, fold = c1_tiles_chain(count, max_tiles, nchunk, C1F_CAP, Cout)
    s = slab.double().sum(0).cpu()
    rs, ms = ref * sel.unsqueeze(-1), mag * sel.unsqueeze(-1)
    within(s[0], rs.sum((0, 1, 2)), (chain + fold + 9) * U * ms.sum((0, 1, 2)), "conv3x3_c1_fwd_tiles: stats sum", dt)
    within(s[1], (rs * rs).sum((0, 1, 2)), (chain + fold + 19) * U * (ms * ms).sum((0, 1, 2)), "conv3x3_c1_fwd_tiles: stats sum of squares", dt)
    # the weight gradient, on the raw output as stored (unlisted pixels: the reference there is masked out by ``sel``)
    yraw = torch.where(on.unsqueeze(-1), got, quant(ref.float(), dt))
    dA = data((B, H, W, Cout), dt, g, 1.0, 0.0)
    sc, sh, mean, invstd = bn_vectors(yraw, g)
    assert R.gate_is_safe(yraw, sc, sh)
    coef = torch.randn(2, Cout, generator=g) * 0.1
    ws = ws_bytes(lib().cmu_conv3x3_c1_wgrad_ws_bytes(B, H, W, Cout))
    da = to_act(ops, dA, dt, EPC[dt])
    r, m = R.bn_bwd_apply_ref(dA, yraw, sc, sh, mean, invstd, coef, sel=sel)
    dref, dmag = R.c1_wgrad_ref(x, r, mask, masked == 2, mdY=m)
    chain, fold = c1_tiles_chain(count, max_tiles, nchunk, C1W_BLOCKS)
    for form, wf in (("read", None), ("recomputed", w.to(DEV))):
        dW = torch.full((Cout, 1, 3, 3), SENT, device=DEV)
        ops.conv3x3_c1_wgrad_bn_tiles(x.to(DEV), da, ya, *cuda(sc, sh, mean, invstd, coef), dW, ws, tiles, max_tiles, mask_d, masked == 2, w=wf)
        torch.cuda.synchronize()
        within(dW.view(Cout, 9), dref, (chain + fold + K_APPLY) * U * dmag, f"conv3x3_c1_wgrad_bn_tiles ({form}): dW", dt)


@pytest.mark.parametrize("dt", DTS)
def test_conv3x3_c1_wgrad_bn_tiles_impulses(ops, dt):
    """dA = 1 at the last pixel of the last listed tile (a partial tile at the image's corner) and 2 in an unlisted tile, coef = 0, scale
    1 with an open gate: dW[c][t] is the image's neighbour of that pixel at tap t (k = K_APPLY: the apply expression on one term, zeros
    added), and the 2.0 does not count."""
    B, H, W, nchunk = 2, 20, 37, 4
    Cout = nchunk * EPC[dt]
    g = gen(1400)
    x, w = torch.randn(B, H, W, generator=g), torch.randn(Cout, 1, 3, 3, generator=g) / 3
    tY, tX = 2, 3
    last, other = B * tY * tX - 1, 1
    tl = torch.tensor([0, 4, last] + [other] * (B * tY * tX - 3), dtype=torch.int32)
    tiles = namespace_tiles(tl, 3)
    ya = empty_act(ops, B, H, W, Cout, dt)
    ops.conv3x3_c1_fwd_tiles(*cuda(x, w), ya, tiles, 3, want_stats=False)
    dA = torch.zeros(B, H, W, Cout)
    dA[B - 1, H - 1, W - 1] = 1.0
    dA[0, 3, 16 + 5] = 2.0                                   # tile 1 of image 0: named by the entries past the count only
    one, zero, big = torch.ones(Cout), torch.zeros(Cout), torch.full((Cout,), 100.0)
    coef = torch.zeros(2, Cout)
    ws = ws_bytes(lib().cmu_conv3x3_c1_wgrad_ws_bytes(B, H, W, Cout))
    taps = R.c1_taps(x.double())[B - 1, H - 1, W - 1]
    for form, wf in (("read", None), ("recomputed", w.to(DEV))):
        dW = torch.full((Cout, 1, 3, 3), SENT, device=DEV)
        ops.conv3x3_c1_wgrad_bn_tiles(x.to(DEV), to_act(ops, dA, dt), ya, *cuda(one, big, zero, one, coef), dW, ws, tiles, 3, w=wf)
        torch.cuda.synchronize()
        ref = taps.expand(Cout, 9)
        within(dW.view(Cout, 9), ref, K_APPLY * U * ref.abs(), f"conv3x3_c1_wgrad_bn_tiles ({form}): impulse", dt)


# ------------------------------------------------------------------------------------------------
# layout converters, global average pool
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(2, 24, 6, 10), (1, 1, 1, 1), (3, 5, 2, 2), (2, 40, 170, 160)])     # 2.18 M elements > LAYOUT_CAP * 256
def test_layout_converters(ops, dt, shape):
    """nchw_to_nhwc and apply_to_nchw without a transform (cmu_nhwc_to_nchw) are moves: bit-exact.  With a transform: one fma, k=1;
    positive and negative relu_from."""
    B, C, H, W = shape
    g = gen(1300 + C)
    x = data((B, C, H, W), dt, g)
    a = empty_act(ops, B, H, W, C, dt, 3)                     # (the converters take any channel offset)
    ops.nchw_to_nhwc(x.to(DEV), a)
    torch.cuda.synchronize()
    xn = R.nchw_to_nhwc_ref(x)
    assert torch.equal(read(a), xn) and slice_untouched(a)
    assert torch.equal(ops.apply_to_nchw(a).cpu(), x)
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    for rf in (0, C // 3, -(C // 3), C, -C):
        out = ops.apply_to_nchw(a.with_transform(*cuda(sc, sh), rf))
        torch.cuda.synchronize()
        ref, mag = R.act_ref(xn, sc, sh, rf)
        within(out, R.nhwc_to_nchw_ref(ref), U * R.nhwc_to_nchw_ref(mag), "apply_to_nchw: out", dt)     # k=1


def k_gap(HW, C, dt):
    """16-byte kernel (C a multiple of the chunk): ceil(HW / 16) terms per thread, each one fma (1), 15 additions of the 16 parts,
    the division; element kernel: ceil(HW / 4) terms, 3 additions."""
    if C % EPC[dt] == 0:
        return -(-HW // 16) + 1 + 15 + 1
    return -(-HW // 4) + 1 + 3 + 1


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", [(2, 5, 7, 40), (3, 16, 16, 128), (2, 9, 4, 64), (3, 4, 4, 20), (1, 70, 3, 8), (1, 1, 1, 8), (2, 1, 65, 136),
                                  (5, 2, 2, 3), (5, 128, 128, 128)])   # the last: 81,920 pixels x 16 / 32 chunks > GAPB_CAP * 256 = 1.05 M chunk items
def test_gap_fwd_bwd(ops, dt, case):
    """gap_fwd with and without a transform; gap_bwd: dout / HW rounded once (k=1) and to the storage type, the same bits at every
    pixel of a channel, the bytes outside the slice untouched."""
    B, H, W, C = case
    g = gen(1400 + C + H)
    y = data((B, H, W, C), dt, g)
    pad = EPC[dt] if C % EPC[dt] == 0 else 0
    for tf in (True, False):
        sc, sh = (torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.3) if tf else (None, None)
        ya = to_act(ops, y, dt, pad)
        out = torch.full((B, C), SENT, device=DEV)
        ops.gap_fwd(ya.with_transform(*cuda(sc, sh), 0) if tf else ya, out)
        torch.cuda.synchronize()
        ref, mag = R.gap_fwd_ref(y, sc, sh)
        within(out, ref, k_gap(H * W, C, dt) * U * mag, "gap_fwd: out", dt)
    dout = torch.randn(B, C, generator=g)
    dA = empty_act(ops, B, H, W, C, dt, pad)
    ops.gap_bwd(dout.to(DEV), dA)
    torch.cuda.synchronize()
    ref, mag = R.gap_bwd_ref(dout, H, W)
    got = read(dA)
    within(got, ref, elem_bound(ref, mag, 1, dt), "gap_bwd: dA", dt)      # k=1
    assert torch.equal(got, got[:, :1, :1].expand_as(got)) and slice_untouched(dA)


@pytest.mark.parametrize("dt", DTS)
def test_gap_fwd_impulse(ops, dt):
    """One non-zero pixel (the last one; the first one): the mean is that value / HW within the division's rounding (k=1)."""
    B, H, W, C = 2, 9, 15, 4 * EPC[dt]
    for p in (0, H * W - 1, H * W - 17):
        y = torch.zeros(B, H * W, C)
        y[B - 1, p] = torch.arange(1, C + 1).float() / 8
        out = torch.empty(B, C, device=DEV)
        ops.gap_fwd(to_act(ops, y.view(B, H, W, C), dt), out)
        torch.cuda.synchronize()
        ref, mag = R.gap_fwd_ref(y.view(B, H, W, C), None, None)
        within(out, ref, U * mag, "gap_fwd impulse: out", dt)


# ------------------------------------------------------------------------------------------------
# argument checks: CmuError, nothing launched
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_bad_arguments_raise_and_launch_nothing(ops, dt):
    from cmunet_amd._lib import CmuError
    e = EPC[dt]
    C = 4 * e
    z = lambda *s: torch.zeros(*s, device=DEV)
    act = lambda B, H, W, C_, pad=0: empty_act(ops, B, H, W, C_, dt, pad)
    sc, sh, mean, invstd, coef = z(C) + 1, z(C), z(C), z(C) + 1, z(2, C)
    y = act(1, 4, 4, C).with_transform(sc, sh, 0)
    out = act(1, 2, 2, C)
    ws = ws_bytes(lib().cmu_bn_bwd_ws_bytes(3 * C))
    cases = {
        "odd H": lambda: ops.bnrelu_maxpool_fwd(act(1, 3, 4, C).with_transform(sc, sh, 0), out),
        "odd W": lambda: ops.maxpool_bwd(out, None, act(1, 4, 3, C).with_transform(sc, sh, 0), act(1, 4, 3, C)),
        "C not a multiple of the chunk": lambda: ops.bn_bwd_apply(ops.Act(act(1, 4, 4, C).buf, 0, C - 1), ops.Act(y.buf, 0, C - 1, sc, sh, 0),
                                                                  mean, invstd, coef, ops.Act(act(1, 4, 4, C).buf, 0, C - 1)),
        "C not a multiple of the chunk (reduce)": lambda: ops.bn_bwd_reduce(ops.Act(act(1, 4, 4, C).buf, 0, C - 1), ops.Act(y.buf, 0, C - 1, sc, sh, 0),
                                                                            mean, invstd, z(C), z(C), coef, ws),
        "head: chunk count not a power of two": lambda: ops.conv1x1_head_fwd(act(1, 4, 4, 3 * e), z(2, 3 * e), z(2), z(1, 2, 4, 4)),
        "head backward: chunk count not a power of two": lambda: ops.conv1x1_head_bwd(z(1, 2, 4, 4), act(1, 4, 4, 3 * e), z(2, 3 * e), None, z(2, 3 * e), z(2),
                                                                                      ws_bytes(1 << 22)),
        "head: K = 9": lambda: ops.conv1x1_head_fwd(act(1, 4, 4, C), z(9, C), z(9), z(1, 9, 4, 4)),
        "dSkip2 without dSkip": lambda: ops.maxpool_bwd(out, None, y, act(1, 4, 4, C), dSkip2=act(1, 4, 4, C)),
        "dSkip2 without dSkip (apply)": lambda: ops.maxpool_bwd_apply(out, None, y, mean, invstd, coef, act(1, 4, 4, C), dSkip2=act(1, 4, 4, C)),
        "dA = NULL without bn_ws": lambda: ops.maxpool_bwd(out, None, y, None),
        "fused sums without save_mean": lambda: ops.maxpool_bwd(out, None, y, act(1, 4, 4, C), None, None, ws),
        "masked pool: H not f times a power of two": lambda: ops.bnrelu_maxpool_fwd_masked(act(1, 6, 6, C).with_transform(sc, sh, 0), torch.ones(1, 4, 4, dtype=torch.uint8, device=DEV),
                                                                                           act(1, 3, 3, C)),
    }
    sentinels = [out, y]
    before = [a.buf.clone() for a in sentinels]
    for name, fn in cases.items():
        with pytest.raises(CmuError):
            fn()
        torch.cuda.synchronize()
    assert all(bits_equal(a.buf, b) for a, b in zip(sentinels, before))
