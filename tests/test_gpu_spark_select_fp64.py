"""The selection / statistics kernels of the SparK path op by op against the float64 references of
tests/necks_fp64_ref.py: ``cmu_mask_select`` (pixel form), ``cmu_mask_select_cells`` (full and ring form), and the masked sums
``cmu_masked_channel_stats``, ``cmu_rows_channel_stats``, ``cmu_cells_channel_stats``, ``cmu_cells_channel_sum``,
``cmu_bn_bwd_reduce_cells``.  Conventions of test_gpu_elem_fp64.py (U = 2^-24, ``k=`` next to each counted bound, ``PARITY``).

  * select: active positions per element against float64 -- k=1 for the fma, then the storage rounding; a pure move (no transform,
    no ReLU) is bit-exact; masked positions are exactly round_dt(fill[c]) or zero; the ring interior and the bytes outside an output
    channel slice keep their sentinel.  The pixel form is also run past its 2,048-workgroup cap at both ends of ``sp_geometry``.
  * sums: integer data (|v| <= 8, at most 2^18 selected pixels: every fp32 partial sum is an exact integer below 2^24) must give the
    exact sums bit for bit, with the slab rows past the work exactly zero; float data per output within k U sum |terms|, k the
    restated upper bound of one thread's chain plus the workgroup fold; one 1.0 at the last active pixel must count and one 2.0 in a
    masked patch must not.
The launchers' geometry (``sp_geometry``, ``cells_geometry``) is restated here, not imported, and each test asserts the branch its
shape is meant to hit.
"""
import numpy as np
import pytest
import torch

import elem_fp64_ref as E
import necks_fp64_ref as R
from elem_fp64_ref import U, D, TORCH_DT, elem_bound, quant  # noqa: F401
from test_gpu_elem_fp64 import PARITY, bits_equal, within  # noqa: F401
from test_gpu_necks_fp64 import exact

pytestmark = pytest.mark.gpu

DTS = ["f32", "f16", "bf16"]
EPC = {"f32": 4, "f16": 8, "bf16": 8}
DEV = "cuda"
SENT = 7.0
SP_ROWS, CSUM_ROWS, SELECT_CAP = 1024, 1024, 2048
# (B, f, H, C): the _CELL_CASES of test_gpu_sparse_tiles.py up to 64 x 64 -- patches of 4, 2, 4, 16, 8, 2, 1, 32, 4, 2, 1, 1 pixels,
# patch maps whose side is no power of two, several small patches side by side per work item
CASES = [(2, 4, 16, 32), (3, 8, 16, 64), (1, 8, 32, 16), (2, 4, 64, 64), (2, 8, 64, 128), (1, 16, 32, 1024), (2, 4, 4, 256), (3, 2, 64, 8),
         (2, 6, 24, 64), (1, 14, 28, 128), (2, 32, 32, 1024), (3, 12, 12, 512)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    return o


def lib():
    from cmunet_amd import _lib
    return _lib.lib()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the launchers' geometry, restated (sparse.hip: sp_geometry, mask_select_t; sparse_elem.hip: cells_geometry, cells_sums_launch) ----
def sp_geometry(nchunk):
    cpb = min(nchunk, 256)
    return cpb, 256 // cpb, -(-nchunk // cpb)


def select_grid(npix, nchunk):
    cpb, ppb, gy = sp_geometry(nchunk)
    return max(1, min(-(-npix // (ppb * 4)), SELECT_CAP)), gy, ppb


def cells_geometry(B, H, C, epc, f, maxlog=10, xlog=10):
    """-> dict(nchunk, nitems, total chunks per work item) of the patch-organised walk; None where the cells form does not apply."""
    nchunk = C // epc
    if H % f or (H // f) & (H // f - 1) or nchunk > 256 or nchunk & (nchunk - 1):
        return None
    sb, cb = (H // f).bit_length() - 1, nchunk.bit_length() - 1
    rb = min(max(maxlog - sb - cb, 0), sb)
    xb = max(xlog - sb - cb - rb, 0)
    while xb > 0 and f & ((1 << xb) - 1):
        xb -= 1
    return {"nchunk": nchunk, "nitems": (B * f * (f >> xb)) << (sb - rb), "total": (1 << rb) << (sb + xb + cb), "xbits": xb}


def masked_k(n, nchunk):
    """Pixel / rows form: a thread adds at most ceil(n / (SP_ROWS ppb)) terms, then ppb partial sums meet in LDS -> (k, ppb)."""
    _, ppb, _ = sp_geometry(nchunk)
    return -(-n // (SP_ROWS * ppb)) + ppb, ppb


def cells_k(geo, rows):
    """Cells form: ``per`` work items per workgroup, ceil(total / 256) chunks of each per thread, then 256 / nchunk partial sums meet
    in LDS -> (k, per)."""
    per = -(-geo["nitems"] // rows)
    return per * -(-geo["total"] // 256) + 256 // geo["nchunk"], per


# ---- data ----------------------------------------------------------------------------------------------------------------------------
def patch_map(B, f, kind, seed):
    """quarter: a random quarter of each image's patches; all; one: a single patch of the last image; none."""
    a = torch.zeros(B, f * f, dtype=torch.uint8)
    g = gen(seed)
    if kind == "quarter":
        for b in range(B):
            a[b, torch.randperm(f * f, generator=g)[:max(1, f * f // 4)]] = 1
    elif kind == "all":
        a[:] = 1
    elif kind == "one":
        a[B - 1, int(torch.randint(0, f * f, (1,), generator=g))] = 1
    return a.view(B, f, f)


def to_act(ops, x, dt, pad=0):
    B, H, W, C = x.shape
    buf = torch.full((B, H, W, C + 2 * pad), SENT, dtype=TORCH_DT[dt])
    buf[..., pad:pad + C] = x.to(buf.dtype)
    return ops.Act(buf.to(DEV), pad, C)


def empty_act(ops, B, H, W, C, dt, pad=0):
    return ops.Act(torch.full((B, H, W, C + 2 * pad), SENT, dtype=TORCH_DT[dt], device=DEV), pad, C)


def read(a):
    return a.buf[..., a.coff:a.coff + a.C].float().cpu()


def slice_untouched(a):
    return bool((a.buf[..., :a.coff] == SENT).all()) and bool((a.buf[..., a.coff + a.C:] == SENT).all())


def cuda(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def ints(shape, g, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------
# mask-select
# ------------------------------------------------------------------------------------------------
def check_select(ops, x, xa, dt, active, sc, sh, relu, fill, invert, form, what):
    """One call of ops.mask_select in ``form`` (pixel / cells / ring) into a channel slice of a sentinel-filled buffer."""
    B, H, W, C = x.shape
    pad = EPC[dt]
    out = empty_act(ops, B, H, W, C, dt, pad)
    xin = xa.with_transform(*cuda(sc, sh), 0) if sc is not None else xa
    ops.mask_select(xin, active.to(DEV), out, relu=relu, invert=invert, fill=None if fill is None else fill.to(DEV),
                    use_transform=sc is not None, ring=form == "ring", cells=form != "pixel")
    sel = R.selection(active, H, W, invert)
    ref, m, moved = R.mask_select_ref(x, sc, sh, relu, sel, fill, dt)
    got = read(out)
    s = sel.unsqueeze(-1).expand_as(ref)
    # k=1: the fma (then the storage rounding); a pure move and every masked position: bound 0
    bound = torch.where(s, elem_bound(ref, m, 0 if moved else 1, dt), torch.zeros((), dtype=torch.float64))
    if moved:
        bound = torch.zeros_like(bound)
    if form == "ring":
        frame = R.ring_frame(active, H)
        inner = ~sel & ~frame
        assert bool((got[inner] == SENT).all()), f"{what}: the interior of a masked patch was written"
        assert bool((got[frame] == 0).all()), f"{what}: the border frame of a masked patch is not zero"
        keep = sel.unsqueeze(-1).expand_as(ref)
        within(got[keep], ref[keep], bound[keep], what, dt)
    else:
        within(got, ref, bound, what, dt)
    assert slice_untouched(out) and slice_untouched(xa), f"{what}: bytes outside the channel slice changed"


VARIANTS = [(True, True, False), (False, True, False), (False, False, False), (True, True, True), (False, False, True)]   # relu, transform, fill


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", CASES)
def test_mask_select_three_forms(ops, dt, case):
    B, f, H, C = case
    g = gen(sum(case))
    active = patch_map(B, f, "quarter", sum(case))
    x = quant(torch.randn(B, H, H, C, generator=g) * 1.5 + 0.3, dt)
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    sc[0] = -sc[0]
    tok = torch.randn(C, generator=g)
    xa = to_act(ops, x, dt, EPC[dt])
    geo = cells_geometry(B, H, C, EPC[dt], f)
    assert geo is not None and ops.cells_supported(xa, active.to(DEV))
    for relu, tr, fl in VARIANTS:
        a = (sc, sh) if tr else (None, None)
        for form in ("pixel", "cells") + (() if fl else ("ring",)):
            check_select(ops, x, xa, dt, active, *a, relu, tok if fl else None, False, form, f"mask_select {form}: out")
        check_select(ops, x, xa, dt, active, *a, relu, tok if fl else None, True, "pixel", "mask_select pixel: out (invert)")
    for kind in ("all", "one", "none"):
        act2 = patch_map(B, f, kind, 3)
        for form in ("pixel", "cells", "ring"):
            check_select(ops, x, xa, dt, act2, sc, sh, True, None, False, form, f"mask_select {form}: out")


# (C in chunks, B, f, H): one chunk per pixel and more than 2,048 * 256 * 4 pixels; 256 chunks per pixel and more than 2,048 * 4
# pixels; 272 chunks: a ragged second channel block
PAST_CAP = [(1, 9, 4, 512), (256, 9, 4, 32), (272, 1, 2, 8)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", PAST_CAP)
def test_mask_select_pixel_form_past_the_workgroup_cap(ops, dt, case):
    nchunk, B, f, H = case
    C, npix = nchunk * EPC[dt], B * H * H
    gx, gy, ppb = select_grid(npix, nchunk)
    if nchunk == 272:
        assert gy == 2 and nchunk - 256 < 256
    else:
        assert gx == SELECT_CAP and npix > SELECT_CAP * ppb * 4 and ppb == (256 if nchunk == 1 else 1), (gx, ppb)
    g = gen(nchunk)
    active = patch_map(B, f, "quarter", nchunk)
    active[B - 1, f - 1, f - 1] = 1                            # the last pixel of the last image is selected
    x = quant(torch.randn(B, H, H, C, generator=g), dt)
    sc, sh, tok = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g)
    xa = to_act(ops, x, dt, EPC[dt])
    check_select(ops, x, xa, dt, active, sc, sh, True, tok, False, "pixel", "mask_select pixel past cap: out")
    check_select(ops, x, xa, dt, active, None, None, False, None, True, "pixel", "mask_select pixel past cap: out (move, invert)")


# ------------------------------------------------------------------------------------------------
# masked / rows / cells statistics, cells_channel_sum, bn_bwd_reduce_cells
# ------------------------------------------------------------------------------------------------
def slab_sums(slab, used_rows, what):
    """The slab rows added in float64 (exact for fp32 rows); rows past the work must be exactly zero."""
    assert used_rows >= slab.shape[0] or bool((slab[used_rows:] == 0).all()), f"{what}: slab rows past the work are not zero"
    return slab.double().sum(0).cpu()


def bn_ws(C):
    return torch.empty(max(int(lib().cmu_bn_bwd_ws_bytes(C)), 16), dtype=torch.uint8, device=DEV)


def run_sums(ops, xa, active, invert, H, C, dt):
    """Every entry that sums x over a selection -> {name: (s1, s2 or None)}; the cells statistics have no inverted form."""
    B, f = active.shape[0], active.shape[-1]
    ad = active.to(DEV)
    nchunk = C // EPC[dt]
    _, ppb, _ = sp_geometry(nchunk)
    npix = B * H * H
    out = {}
    s = slab_sums(ops.masked_channel_stats(xa, ad, invert=invert), -(-npix // ppb), "masked_channel_stats")
    out["masked_channel_stats"] = (s[0], s[1])
    geo = cells_geometry(B, H, C, EPC[dt], f)
    if not invert:
        pl = ops.PixelList(ad, H, H)
        n = int(pl.count.item())
        assert n == int(active.sum()) * (H // f) ** 2
        s = slab_sums(ops.rows_channel_stats(xa, pl), -(-n // ppb), "rows_channel_stats")
        out["rows_channel_stats"] = (s[0], s[1])
        if geo is not None:
            per = -(-geo["nitems"] // CSUM_ROWS)
            s = slab_sums(ops.cells_channel_stats(xa, ad), -(-geo["nitems"] // per), "cells_channel_stats")
            out["cells_channel_stats"] = (s[0], s[1])
    if geo is not None:
        o = torch.full((C,), SENT, device=DEV)
        ops.cells_channel_sum(xa, ad, o, invert=invert)
        out["cells_channel_sum"] = (o.double().cpu(), None)
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["quarter", "all", "one", "none"])
@pytest.mark.parametrize("case", CASES + [(1, 2, 8, 272 * 8), (2, 4, 16, 272 * 8)])
def test_masked_sums_exact_integers(ops, dt, case, kind):
    """Integer data: the exact sums, bit for bit, in every form, inverted too; an empty selection gives exactly 0.  The last two
    cases have more than 256 chunks per pixel (a second channel block; the pixel and rows forms only)."""
    B, f, H, C = case
    if C == 272 * 8:
        C = 272 * EPC[dt]
        assert sp_geometry(C // EPC[dt])[2] == 2 and cells_geometry(B, H, C, EPC[dt], f) is None
    g = gen(sum(case))
    active = patch_map(B, f, kind, sum(case))
    x = ints((B, H, H, C), g)
    assert B * H * H <= 2 ** 18 and float(x.abs().max()) <= 8
    xa = to_act(ops, x, dt, EPC[dt])
    for invert in (False, True):
        sel = R.selection(active, H, H, invert)
        s1, s2, _, _ = R.masked_sums_ref(x, sel)
        if kind == ("all" if invert else "none"):
            assert float(s1.abs().max()) == 0 and float(s2.max()) == 0
        for name, (g1, g2) in run_sums(ops, xa, active, invert, H, C, dt).items():
            exact(g1, s1, f"{name} exact: sum" + (" (invert)" if invert else ""), dt)
            if g2 is not None:
                exact(g2, s2, f"{name} exact: sum of squares" + (" (invert)" if invert else ""), dt)
    if cells_geometry(B, H, C, EPC[dt], f) is None:
        return
    # BatchNorm backward sums over the active patches: integer dA and y, integer scale / shift / mean, invstd = 1 / 2
    dA, y = ints((B, H, H, C), g), ints((B, H, H, C), g)
    sc = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (C,), generator=g)]
    sh, mean, invstd = ints((C,), g, 3), ints((C,), g, 3), torch.full((C,), 0.5)
    sel = R.selection(active, H, H)
    count = max(int(sel.sum()), 1)
    ref = E.bn_bwd_sums_ref(dA, y, sc, sh, mean, invstd, count, sel)
    ya = to_act(ops, y, dt, EPC[dt]).with_transform(*cuda(sc, sh), 0)
    dg, db, coef = (torch.full(s, SENT, device=DEV) for s in ((C,), (C,), (2, C)))
    ops.bn_bwd_reduce_cells(to_act(ops, dA, dt), ya, *cuda(mean, invstd), dg, db, coef, active.to(DEV), count, bn_ws(C))
    exact(db, ref["dbeta"], "bn_bwd_reduce_cells exact: dbeta", dt)
    exact(dg, ref["dgamma"], "bn_bwd_reduce_cells exact: dgamma", dt)
    exact(coef, torch.from_numpy(np.float32(ref["coef"].numpy())).double(), "bn_bwd_reduce_cells exact: coef", dt)     # one rounding of S / count


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", CASES + [(1, 2, 8, 272 * 8)])
def test_masked_sums_float_data(ops, dt, case):
    B, f, H, C = case
    if C == 272 * 8:
        C = 272 * EPC[dt]
    nchunk = C // EPC[dt]
    g = gen(7 + sum(case))
    active = patch_map(B, f, "quarter", sum(case))
    x = quant(torch.randn(B, H, H, C, generator=g) * 1.5 + 0.3, dt)
    xa = to_act(ops, x, dt, EPC[dt])
    geo = cells_geometry(B, H, C, EPC[dt], f)
    npix = B * H * H
    for invert in (False, True):
        sel = R.selection(active, H, H, invert)
        s1, s2, m1, m2 = R.masked_sums_ref(x, sel)
        ks = {"masked_channel_stats": masked_k(npix, nchunk)[0], "rows_channel_stats": masked_k(int(sel.sum()), nchunk)[0]}
        if geo is not None:
            ks["cells_channel_stats"] = cells_k(geo, CSUM_ROWS)[0]
            ks["cells_channel_sum"] = cells_k(geo, min(geo["nitems"], CSUM_ROWS))[0] + 1       # + the cast of the float64 final pass
        for name, (g1, g2) in run_sums(ops, xa, active, invert, H, C, dt).items():
            k = ks[name]                                                                    # k = chain + fold (restated above)
            within(g1, s1, k * U * m1, f"{name}: sum", dt)
            if g2 is not None:
                within(g2, s2, k * U * m2, f"{name}: sum of squares", dt)                   # one fma per term: the same k
    if geo is None:
        return
    dA = quant(torch.randn(B, H, H, C, generator=g), dt)
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    sc[0] = -sc[0]
    yd = x.double().reshape(-1, C)
    mean, invstd = yd.mean(0).float(), (1.0 / torch.sqrt(yd.var(0, unbiased=False) + 1e-5)).float()
    assert E.gate_is_safe(x, sc, sh)
    sel = R.selection(active, H, H)
    count = int(sel.sum())
    ref = E.bn_bwd_sums_ref(dA, x, sc, sh, mean, invstd, count, sel)
    dg, db, coef = (torch.full(s, SENT, device=DEV) for s in ((C,), (C,), (2, C)))
    ops.bn_bwd_reduce_cells(to_act(ops, dA, dt), xa.with_transform(*cuda(sc, sh), 0), *cuda(mean, invstd), dg, db, coef, active.to(DEV), count, bn_ws(C))
    k = cells_k(geo, min(geo["nitems"], CSUM_ROWS))[0] + 1      # chain + fold, the cast of the float64 final pass
    within(db, ref["dbeta"], k * U * ref["mag1"], "bn_bwd_reduce_cells: dbeta", dt)                        # k
    within(dg, ref["dgamma"], (k + 2) * U * ref["mag2"], "bn_bwd_reduce_cells: dgamma", dt)                # k+2: xhat = (y - mean) invstd
    within(coef[0], ref["coef"][0], k * U * ref["mag1"] / count, "bn_bwd_reduce_cells: coef c1", dt)
    within(coef[1], ref["coef"][1], (k + 2) * U * ref["mag2"] / count, "bn_bwd_reduce_cells: coef c2", dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", CASES + [(1, 2, 8, 272 * 8)])
def test_masked_sums_impulses(ops, dt, case):
    """All zeros but a 1.0 (every channel) at the last pixel of the last active patch of the last image, and a 2.0 at the last pixel of
    the last masked patch: the sums are exactly (1, 1), inverted (2, 4).  The BatchNorm sums: dbeta = 1, dgamma = xhat there."""
    B, f, H, C = case
    if C == 272 * 8:
        C = 272 * EPC[dt]
    active = patch_map(B, f, "quarter", 5 + sum(case))
    sel = R.selection(active, H, H)
    flat = sel.reshape(-1)
    p_on, p_off = int(flat.nonzero()[-1]), int((~flat).nonzero()[-1])
    assert p_on // (H * H) == B - 1
    x = torch.zeros(B * H * H, C)
    x[p_on], x[p_off] = 1.0, 2.0
    x = x.view(B, H, H, C)
    xa = to_act(ops, x, dt, EPC[dt])
    for invert, (e1, e2) in ((False, (1.0, 1.0)), (True, (2.0, 4.0))):
        for name, (g1, g2) in run_sums(ops, xa, active, invert, H, C, dt).items():
            exact(g1, torch.full((C,), e1, dtype=torch.float64), f"{name} impulse: sum", dt)
            if g2 is not None:
                exact(g2, torch.full((C,), e2, dtype=torch.float64), f"{name} impulse: sum of squares", dt)
    if cells_geometry(B, H, C, EPC[dt], f) is None:
        return
    g = gen(9)
    y = ints((B, H, H, C), g)
    sc, sh, mean, invstd = torch.ones(C), torch.full((C,), 100.0), ints((C,), g, 3), torch.full((C,), 0.25)
    count = int(sel.sum())
    ref = E.bn_bwd_sums_ref(x, y, sc, sh, mean, invstd, count, sel)
    assert float(ref["dbeta"].min()) == float(ref["dbeta"].max()) == 1.0
    dg, db, coef = (torch.full(s, SENT, device=DEV) for s in ((C,), (C,), (2, C)))
    ops.bn_bwd_reduce_cells(xa, to_act(ops, y, dt).with_transform(*cuda(sc, sh), 0), *cuda(mean, invstd), dg, db, coef, active.to(DEV), count, bn_ws(C))
    exact(db, ref["dbeta"], "bn_bwd_reduce_cells impulse: dbeta", dt)
    exact(dg, ref["dgamma"], "bn_bwd_reduce_cells impulse: dgamma", dt)
