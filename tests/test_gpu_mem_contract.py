"""Every library function that takes a byte workspace, held to its memory contract (tests/mem_contract.py; the harness is proved on
the CPU in tests/test_cpu_mem_contract.py): the workspace is exactly ``cmu_*_ws_bytes`` bytes between two 4 KiB guards and starts
all zero, all 0xFF, and holding the bytes an earlier call left -- the same entry at its largest shape here, and for the buffers the
engine shares between entry points (``_Scratch`` keys "wg", "bnbwd", "bnfin") the bytes another entry point of the key left.  Every
output lies between guards too and starts as NaN (float) or as a value the op cannot produce (integers); every input is compared byte
for byte afterwards; the outputs must have the same bits in every state, and pass the check the entry has in its own test file --
same reference module, same bound; no tolerance is introduced here.

``COVERED`` maps each ``*_ws_bytes`` function to the tests below that use it and to pairs of (small, large) argument tuples for
tests/test_cpu_mem_contract.py; ``ELSEWHERE`` names the tests that already hold the remaining three to this contract.

Shapes are read off the launchers: one workgroup; several with a partly filled last one; and the launcher's cap where that is cheap.
Caps that are NOT reached here (the shape would be far larger than what the contract needs):
  * POOLB_BLOCKS 2048 of the max-pool backward's fused sums (16,900 pixels x 1,024 channels);
  * the 4,096-workgroup caps of soft_skeleton / soft_skeleton_save / soft_skeleton_bwd and the 16,384-workgroup caps of the resizes
    (their workspaces are per element, not per workgroup: the cap does not enter the size).
RED_MAX_BLOCKS 2048 is reached at 1 x 91 x 91 pixels of 1,024 fp32 channels (8.5 M elements: one pixel per pass needs 256 chunks per
pixel); the other caps at far smaller shapes (each test's docstring names its own).

Where the entries differ from the wrappers' names: cmu_skinny_gemm_wgrad and the 16-bit input / weight gradients take no workspace
(cmu_skinny_gemm_bwd_ws_bytes sizes the fp32 input gradient's only); cmu_sparse_pixel_list_ws_bytes sizes the patch list of
cmu_sparse_pixel_list (ops.PixelList), not ops.build_lists, which takes none; ops.PixelList, the resizes, the skinny GEMMs, the geometry
kernels, label_components and the augmentation's resize allocate their workspaces themselves and are called through ``_lib.call``.

Every entry prints one ``[memcontract]`` line: entry, case, dtype, ws_bytes, workgroups of the first pass (0 where the launcher's grid
is not restated here) and whether its cap was hit, the states run, the worst err / bound of the reference check.
"""
import math
import time
import types

import numpy as np
import pytest
import torch

import elem_fp64_ref as R
import mem_contract as MC
import test_gpu_elem_fp64 as E
from elem_fp64_ref import U, D, TORCH_DT
from mem_contract import Case, Out, check_call
from test_gpu_elem_fp64 import EPC, chunk_geometry, fold_k, reduce_chain, within

pytestmark = pytest.mark.gpu

DEV = "cuda"
I32, U8, F64 = torch.int32, torch.uint8, torch.float64

ELSEWHERE = {
    "cmu_moco_ws_bytes": ["test_gpu_moco_fused_fp64.py"],
    "cmu_conv3x3_wgrad_ws_bytes": ["test_gpu_wgrad_exact.py", "test_gpu_wgrad_tiles_exact.py"],
    "cmu_convT2x2_wgrad_ws_bytes": ["test_gpu_wgrad_exact.py"],
}

# name -> entries: the tests below (test_<entry>); sizes: (small, large) argument tuples of the size function at the table's shapes;
# not_sizes: positions of arguments that are no sizes (a dtype code, an iteration count)
COVERED = {
    "cmu_bn_finalize_ws_bytes": {"entries": ["bn_finalize", "bn_bwd_finalize_tiles"], "sizes": [((16,), (256,)), ((1,), (1024,))]},
    "cmu_bn_bwd_ws_bytes": {"entries": ["bn_bwd_reduce", "bn_bwd_reduce_masked_rows_cells", "maxpool_bwd_bn_ws", "conv1x1_head_bwd"],
                            "sizes": [((16,), (256,)), ((4,), (1024,))]},
    "cmu_conv3x3_c1_wgrad_ws_bytes": {"entries": ["conv3x3_c1_wgrad", "conv3x3_c1_wgrad_bn_tiles"], "sizes": [((1, 2, 2, 4), (4, 192, 192, 64))]},
    "cmu_conv1x1_head_bwd_ws_bytes": {"entries": ["conv1x1_head_bwd"], "sizes": [((1, 1, 1, 4, 1), (1, 111, 111, 256, 3))]},
    "cmu_masked_mse_ws_bytes": {"entries": ["masked_mse_fwd_bwd"], "sizes": [((1, 1), (3, 20))]},
    "cmu_mse_ws_bytes": {"entries": ["mse_fwd_bwd"], "sizes": [((), ())]},
    "cmu_softmax_ce_dice_ws_bytes": {"entries": ["softmax_ce_dice_fwd_bwd"], "sizes": [((1, 3, 5), (5, 230, 230))]},
    "cmu_seg_stats_ws_bytes": {"entries": ["seg_stats_fwd"], "sizes": [((2,), (8,))]},
    "cmu_pointwise_loss_ws_bytes": {"entries": ["pointwise_loss_fwd"], "sizes": [((), ())]},
    "cmu_index_ce_ws_bytes": {"entries": ["index_ce_fwd"], "sizes": [((), ())]},
    "cmu_spark_loss_ws_bytes": {"entries": ["spark_loss_fwd_bwd"], "sizes": [((1, 1), (3, 5))]},
    "cmu_cells_channel_sum_ws_bytes": {"entries": ["cells_channel_sum"], "sizes": [((32,), (1024,))]},
    "cmu_sparse_pixel_list_ws_bytes": {"entries": ["sparse_pixel_list"], "sizes": [((1, 1), (3, 8))]},
    "cmu_soft_skeleton_ws_bytes": {"entries": ["soft_skeleton_and_cldice_sums"], "sizes": [((1,), (2 * 64 * 65,))]},
    "cmu_soft_skeleton_save_ws_bytes": {"entries": ["soft_skeleton_save_and_bwd"], "sizes": [((1, 1), (2 * 64 * 65, 10))]},
    "cmu_soft_skeleton_bwd_ws_bytes": {"entries": ["soft_skeleton_save_and_bwd"], "sizes": [((1,), (2 * 64 * 65,))]},
    "cmu_cldice_sums_ws_bytes": {"entries": ["soft_skeleton_and_cldice_sums"], "sizes": [((), ())]},
    "cmu_skinny_gemm_ws_bytes": {"entries": ["skinny_gemms"], "sizes": [((1, 1, 16), (65, 130, 4096))]},
    "cmu_skinny16_gemm_ws_bytes": {"entries": ["skinny_gemms"], "sizes": [((1, 1, 16), (65, 130, 4096))]},
    "cmu_skinny_gemm_bwd_ws_bytes": {"entries": ["skinny_gemms"], "sizes": [((1, 1), (65, 130))]},
    "cmu_lamb_ws_bytes": {"entries": ["lamb_step"], "sizes": [((1, 1), (71, 5))]},
    "cmu_resize_bicubic_ws_bytes": {"entries": ["resizes"], "sizes": [((1, 1, 1, 1, 1), (3, 100, 77, 96, 80))]},
    "cmu_resize_bicubic_u8_ws_bytes": {"entries": ["resizes"], "sizes": [((1, 1, 1, 1, 1), (3, 100, 77, 96, 80))]},
    "cmu_resize_nearest_u8_ws_bytes": {"entries": ["resizes"], "sizes": [((1, 1), (96, 80))]},
    "cmu_ftaug_resize_ws_bytes": {"entries": ["ftaug_resize_onehot"], "sizes": [((1, 475, 64), (3, 475, 128))]},
    "cmu_genesis_bezier_ws_bytes": {"entries": ["genesis_bezier"], "sizes": [((1,), (16,))]},
    "cmu_contour_points_ws_bytes": {"entries": ["contour_points"], "sizes": [((1, 1, 2), (3, 64, 64))]},
    "cmu_lattice_nearest_ws_bytes": {"entries": ["lattice_nearest"], "sizes": [((1, 1, 1), (3, 64, 64))]},
    "cmu_label_components_ws_bytes": {"entries": ["label_components"], "sizes": [((1, 1, 1), (3, 64, 64))]},
}

LEFT = {}          # entry -> the workspace bytes its largest case left


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def record_table():
    """The wall time of the file behind the entries' ``[memcontract]`` lines (profiles/mem_contract.txt holds those lines of one run)."""
    t0, n0 = time.time(), len(MC.RECORDS)
    yield
    print(f"\n[memcontract] {len(MC.RECORDS) - n0} calls held to the contract; wall time of tests/test_gpu_mem_contract.py: {time.time() - t0:.1f} s")


def lib():
    from cmunet_amd import _lib
    return _lib.lib()


def call(*a):
    from cmunet_amd import _lib
    return _lib.call(*a)


def gen(seed):
    return torch.Generator().manual_seed(seed)


class worst_of:
    """The worst err / bound that the ``within`` / ``exact`` helpers of the entries' own test files record inside the block."""

    def __enter__(self):
        self.saved = dict(E.PARITY)
        E.PARITY.clear()
        return self

    def __exit__(self, *exc):
        self.worst = max(E.PARITY.values(), default=0.0)
        for k, v in self.saved.items():
            E.PARITY[k] = max(E.PARITY.get(k, 0.0), v)
        return False


def hold(entry, cases):
    """``cases``: (Case, run, check) with the LARGEST shape first: its bytes are the "leftover" state of the others.  ``check(outs)``
    asserts with the entry's own helpers; the worst ratio they record goes into the entry's line."""
    for case, run, check in cases:
        if entry in LEFT:
            case.leftovers["largest case"] = LEFT[entry]

        def ref_check(outs, check=check):
            with worst_of() as w:
                check(outs)
            return w.worst
        try:
            rec = check_call(entry, case, run, ref_check)
        except RuntimeError as e:       # a GPU fault under a poisoned workspace is a finding about a kernel that trusts stale memory as an index
            if "HIP error" in str(e) or "illegal memory access" in str(e):     # or a count: nothing more is started on the device in this session
                pytest.exit(f"{entry} [{case.name}]: GPU fault, the run stops here: {e}", returncode=3)
            raise
        LEFT.setdefault(entry, rec["ws_after"])


def dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def act_in(ops, x, dt):
    return ops.Act(x.to(TORCH_DT[dt]).to(DEV).contiguous(), 0, x.shape[-1])


def left_by(fn, nbytes):
    """The bytes a call leaves in a zeroed plain workspace of ``nbytes`` (a leftover source from another entry point)."""
    ws = torch.zeros(int(nbytes), dtype=U8, device=DEV)
    fn(ws)
    torch.cuda.synchronize()
    return ws


# ------------------------------------------------------------------------------------------------------------------------------------
# "bnfin": cmu_bn_finalize, cmu_bn_bwd_finalize_tiles
# ------------------------------------------------------------------------------------------------------------------------------------
def bn_finalize_case(ops, rows, C, leftovers=None):
    g = gen(rows * 3 + C)
    slab, count = E.make_slab(rows, C, g)
    p = lambda s: torch.randn(C, generator=g) * s
    bias, gamma, beta, rm, rv = p(1.0), torch.rand(C, generator=g) + 0.5, p(1.0), p(0.1), torch.rand(C, generator=g) + 0.5
    ins = dict(zip(("slab", "bias", "gamma", "beta", "rm", "rv"), dev(slab, bias, gamma, beta, rm, rv)))
    upd = "updated in place: (1 - momentum) old + momentum new; run() loads the old value into the guarded buffer first"
    outs = {k: Out((C,)) for k in ("scale", "shift", "save_mean", "save_invstd")}
    outs.update(running_mean=Out((C,), prefill=0.0, accumulates=True, why=upd), running_var=Out((C,), prefill=0.0, accumulates=True, why=upd))
    nsplit = max(1, min(rows // 16, E.BN_MAX_SPLITS))

    def run(ws, o):
        o["running_mean"].copy_(ins["rm"])
        o["running_var"].copy_(ins["rv"])
        ops.bn_finalize(ins["slab"], count, ins["bias"], ins["gamma"], ins["beta"], o["running_mean"], o["running_var"], 0.1, E.EPS, True,
                        o["scale"], o["shift"], o["save_mean"], o["save_invstd"], ws)

    fin = R.bn_finalize_ref(slab, count, bias, gamma, beta, rm, rv, 0.1, E.EPS, True)
    n = lambda t: t.double().numpy()
    bounds = E.finalize_bounds(fin, rows, count, n(gamma), n(beta), n(bias), n(rm), n(rv), float(np.float32(0.1)), True)

    def check(o):
        for k, got in o.items():
            within(got, torch.from_numpy(fin[k]), torch.from_numpy(bounds[k]), f"bn_finalize: {k}")
    case = Case(f"rows {rows} C {C}", lib().cmu_bn_finalize_ws_bytes(C), outs, ins, DEV, "f32", -(-C // 64) * nsplit, rows // 16 > E.BN_MAX_SPLITS, leftovers)
    return case, run, check


def test_bn_finalize(ops):
    """rows 10,000: nsplit = BN_MAX_SPLITS = 256 (the cap; all of the workspace is written); rows 17 / 1: one split of 256 sized.
    "bnfin" serves every layer width: C = 16 after C = 256, and bn_finalize after bn_bwd_finalize_tiles."""
    tiles = left_by(lambda ws: ops.bn_bwd_finalize_tiles(torch.randn(4097, 2, 256, device=DEV), 9, *(torch.empty(s, device=DEV) for s in (256, 256, (2, 256))), ws),
                    lib().cmu_bn_finalize_ws_bytes(256))
    hold("bn_finalize", [bn_finalize_case(ops, 10000, 256), bn_finalize_case(ops, 17, 48), bn_finalize_case(ops, 1, 1),
                         bn_finalize_case(ops, 40, 16, {"bn_bwd_finalize_tiles C=256": tiles})])


def test_bn_bwd_finalize_tiles(ops):
    def one(rows, C, leftovers=None):
        g = gen(rows + C)
        slab = torch.randn(rows, 2, C, generator=g) * (torch.rand(rows, 1, 1, generator=g) * 4)
        count = 3 * rows
        ins = {"slab": slab.to(DEV)}
        ref = R.bn_bwd_finalize_tiles_ref(slab, count)

        def run(ws, o):
            ops.bn_bwd_finalize_tiles(ins["slab"], count, o["dgamma"], o["dbeta"], o["coef"], ws)

        def check(o):
            for key, mag in (("dbeta", "mag1"), ("dgamma", "mag2")):
                within(o[key], ref[key], U * ref[key].abs() + rows * D * ref[mag], f"bn_bwd_finalize_tiles: {key}")
            for i, mag in ((0, "mag1"), (1, "mag2")):
                within(o["coef"][i], ref["coef"][i], U * ref["coef"][i].abs() + (rows + 1) * D * ref[mag] / count, f"bn_bwd_finalize_tiles: coef {i}")
        nsplit = max(1, min(rows // 16, E.BN_MAX_SPLITS))
        return (Case(f"rows {rows} C {C}", lib().cmu_bn_finalize_ws_bytes(C), {"dgamma": Out((C,)), "dbeta": Out((C,)), "coef": Out((2, C))}, ins, DEV, "f32",
                     -(-C // 64) * nsplit, rows // 16 > E.BN_MAX_SPLITS, leftovers), run, check)
    fin = bn_finalize_case(ops, 10000, 256)
    left = left_by(lambda ws: fin[1](ws, {k: torch.zeros(256, device=DEV) for k in fin[0].outs}), fin[0].ws_bytes)
    hold("bn_bwd_finalize_tiles", [one(4097, 256), one(17, 65), one(1, 1), one(100, 16, {"bn_finalize C=256": left})])


# ------------------------------------------------------------------------------------------------------------------------------------
# "bnbwd": cmu_bn_bwd_reduce (+ _masked, _rows, _cells), the fused sums of cmu_maxpool_bwd and cmu_conv1x1_head_bwd + cmu_bn_bwd_finalize
# ------------------------------------------------------------------------------------------------------------------------------------
def bn_inputs(case, dt, seed):
    nchunk, B, H, W = case
    C = nchunk * EPC[dt]
    g = gen(seed)
    y, dA = E.data((B, H, W, C), dt, g), E.data((B, H, W, C), dt, g, 1.0, 0.0)
    sc, sh, mean, invstd = E.bn_vectors(y, g)
    assert R.gate_is_safe(y, sc, sh)
    return C, g, y, dA, sc, sh, mean, invstd


SUMS = lambda C: {"dgamma": Out((C,)), "dbeta": Out((C,)), "coef": Out((2, C))}


def bn_reduce_case(ops, case, dt, leftovers=None):
    nchunk, B, H, W = case
    C, g, y, dA, sc, sh, mean, invstd = bn_inputs(case, dt, 100 + nchunk + B * H * W)
    npix = B * H * W
    ins = dict(zip(("dA", "y", "sc", "sh", "mean", "invstd"), (act_in(ops, dA, dt).buf, act_in(ops, y, dt).buf) + dev(sc, sh, mean, invstd)))

    def run(ws, o):
        ops.bn_bwd_reduce(ops.Act(ins["dA"]), ops.Act(ins["y"], 0, C, ins["sc"], ins["sh"], 0), ins["mean"], ins["invstd"], o["dgamma"], o["dbeta"], o["coef"], ws)
    chain, fold = reduce_chain(npix, C, dt, 4, E.RED_MAX_BLOCKS)
    ref = R.bn_bwd_sums_ref(dA, y, sc, sh, mean, invstd)
    _, ppb, gy = chunk_geometry(nchunk)
    gx = -(-npix // (4 * ppb))
    check = lambda o: E.check_sums(o["dgamma"], o["dbeta"], o["coef"], ref, chain, fold, dt, "bn_bwd_reduce")
    return Case(f"{B}x{H}x{W} C {C}", lib().cmu_bn_bwd_ws_bytes(C), SUMS(C), ins, DEV, dt, min(gx, 2048) * gy, gx > 2048, leftovers), run, check


def test_bn_bwd_reduce(ops):
    """1 x 91 x 91 pixels of 256 chunks (one pixel per pass): 8,281 pixels > RED_MAX_BLOCKS * 4 -- the cap branch, 8.5 M elements, the smallest shape
    that reaches it (the rows of the slab are per workgroup: 2,048 of them are sized, written and read).  3 x 33 x 40 of 12 chunks (C = 48 / 96: a
    multiple of the chunk, not of 64): 48 workgroups, the last one partly filled.  "bnbwd" serves every layer width: C = 16 after C = 256."""
    big = bn_reduce_case(ops, (64, 1, 30, 30), "f32")
    left256 = left_by(lambda ws: big[1](ws, {k: torch.zeros(o.shape, device=DEV) for k, o in big[0].outs.items()}), big[0].ws_bytes)
    hold("bn_bwd_reduce", [bn_reduce_case(ops, (256, 1, 91, 91), "f32"), bn_reduce_case(ops, (12, 3, 33, 40), "f32"), bn_reduce_case(ops, (12, 3, 33, 40), "bf16"),
                           bn_reduce_case(ops, (1, 1, 2, 2), "f16"), bn_reduce_case(ops, (4, 2, 5, 7), "f32", {"bn_bwd_reduce C=256": left256})])


def test_bn_bwd_reduce_masked_rows_cells(ops):
    """The three sparse forms on one patch map each: a random map, an EMPTY one (no pixel selected, an empty list: every workgroup's slab row
    must still be written), and one active patch.  Integer data (the exact sums, bit for bit: test_gpu_spark_select_fp64.py) for the
    cells form; float data against the counted bound for the masked and rows forms (test_gpu_elem_fp64.py).  The pixel list's capacity
    is its host bound rounded to 256: the list is shorter than it in every case here but the full one (512 of 512)."""
    import necks_fp64_ref as NR
    from test_gpu_necks_fp64 import exact
    from test_gpu_spark_select_fp64 import ints, patch_map
    for dt, (B, f, H, nchunk), kind in (("f32", (2, 8, 64, 16), "quarter"), ("f32", (2, 4, 16, 8), "none"), ("bf16", (3, 4, 16, 8), "one"),
                                        ("f16", (2, 4, 16, 8), "all")):
        C, npix = nchunk * EPC[dt], B * H * H
        g = gen(300 + nchunk + len(kind))
        active = patch_map(B, f, kind, 11 + B)
        sel = R.expand_active(active, H, H)
        count = max(int(sel.sum()), 1)
        y, dA = E.data((B, H, H, C), dt, g), E.data((B, H, H, C), dt, g, 1.0, 0.0)
        sc, sh, mean, invstd = E.bn_vectors(y, g)
        assert R.gate_is_safe(y, sc, sh)
        ref = R.bn_bwd_sums_ref(dA, y, sc, sh, mean, invstd, count=count, sel=sel)
        act_d = active.to(DEV)
        px = ops.PixelList(act_d, H, H, max_rows=max(int(sel.sum()), 1) + 1)
        torch.cuda.synchronize()
        assert int(px.count.cpu()) == int(sel.sum()) <= px.capacity
        ins = dict(zip(("dA", "y", "sc", "sh", "mean", "invstd", "active", "rows", "n_rows"),
                       (act_in(ops, dA, dt).buf, act_in(ops, y, dt).buf) + dev(sc, sh, mean, invstd) + (act_d, px.rows, px.count)))
        ya = lambda: ops.Act(ins["y"], 0, C, ins["sc"], ins["sh"], 0)
        args = lambda o: (ops.Act(ins["dA"]), ya(), ins["mean"], ins["invstd"], o["dgamma"], o["dbeta"], o["coef"])
        nws = lib().cmu_bn_bwd_ws_bytes(C)
        _, ppb, gy = chunk_geometry(nchunk)
        # masked
        chain, fold = reduce_chain(npix, C, dt, 4, E.RED_MAX_BLOCKS)
        hold("bn_bwd_reduce_masked", [(Case(f"{B}x{H}x{H} C {C} f {f} {kind}", nws, SUMS(C), ins, DEV, dt, min(-(-npix // (4 * ppb)), 2048) * gy, False),
                                       lambda ws, o: ops.bn_bwd_reduce_masked(*args(o), ins["active"], count, ws),
                                       lambda o, chain=chain, fold=fold: E.check_sums(o["dgamma"], o["dbeta"], o["coef"], ref, chain, fold, dt, "bn_bwd_reduce_masked"))])
        # rows
        chain, fold = reduce_chain(px.capacity, C, dt, 4, E.RED_MAX_BLOCKS)
        hold("bn_bwd_reduce_rows", [(Case(f"{B}x{H}x{H} C {C} list {int(sel.sum())} of {px.capacity} ({kind})", nws, SUMS(C), ins, DEV, dt,
                                          min(-(-px.capacity // (4 * ppb)), 2048) * gy, False),
                                     lambda ws, o: ops.bn_bwd_reduce_rows(*args(o), px, count, ws),
                                     lambda o, chain=chain, fold=fold: E.check_sums(o["dgamma"], o["dbeta"], o["coef"], ref, chain, fold, dt, "bn_bwd_reduce_rows"))])
        # cells: integer data, exact
        dAi, yi = ints((B, H, H, C), g), ints((B, H, H, C), g)
        sci = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (C,), generator=g)]
        shi, meani, invi = ints((C,), g, 3), ints((C,), g, 3), torch.full((C,), 0.5)
        refi = R.bn_bwd_sums_ref(dAi, yi, sci, shi, meani, invi, count, NR.selection(active, H, H))
        ini = dict(zip(("dA", "y", "sc", "sh", "mean", "invstd", "active"), (act_in(ops, dAi, dt).buf, act_in(ops, yi, dt).buf) + dev(sci, shi, meani, invi) + (act_d,)))
        assert ops.cells_supported(ops.Act(ini["y"]), act_d)

        def check_cells(o, refi=refi, dt=dt):
            exact(o["dbeta"], refi["dbeta"], "bn_bwd_reduce_cells exact: dbeta", dt)
            exact(o["dgamma"], refi["dgamma"], "bn_bwd_reduce_cells exact: dgamma", dt)
            exact(o["coef"], torch.from_numpy(np.float32(refi["coef"].numpy())).double(), "bn_bwd_reduce_cells exact: coef", dt)
        hold("bn_bwd_reduce_cells", [(Case(f"{B}x{H}x{H} C {C} f {f} {kind}", nws, SUMS(C), ini, DEV, dt, 0, False),
                                      lambda ws, o, ini=ini: ops.bn_bwd_reduce_cells(ops.Act(ini["dA"]), ops.Act(ini["y"], 0, C, ini["sc"], ini["sh"], 0), ini["mean"],
                                                                                     ini["invstd"], o["dgamma"], o["dbeta"], o["coef"], ini["active"], count, ws), check_cells)])


def test_maxpool_bwd_bn_ws(ops):
    """maxpool_bwd(..., bn_ws=) writes the slab, bn_bwd_finalize reads it: stored form (dA is an output) and sums-only form (dA = None), one
    skip gradient.  6 x 10 of 8 chunks: one workgroup; 2 x 34 x 38 of 12 chunks: several, the last one partly filled."""
    for dt, (nchunk, B, H, W) in (("f32", (12, 2, 34, 38)), ("bf16", (12, 2, 34, 38)), ("f32", (8, 1, 6, 10))):
        C, npix = nchunk * EPC[dt], B * H * W
        g = gen(500 + nchunk + H)
        y, sc, sh = E.pool_inputs(("rand", nchunk, B, H, W), dt, g)
        assert R.gate_is_safe(y, sc, sh)
        dP, dS = E.data((B, H // 2, W // 2, C), dt, g, 1.0, 0.0), E.data((B, H, W, C), dt, g, 1.0, 0.0)
        _, _, mean, invstd = E.bn_vectors(y, g)
        ins = dict(zip(("dP", "dS", "y", "sc", "sh", "mean", "invstd"), tuple(act_in(ops, t, dt).buf for t in (dP, dS, y)) + dev(sc, sh, mean, invstd)))
        pb = R.pool_bwd_ref(dP, [dS], y, sc, sh)
        trips, fold = reduce_chain(B * (H // 2) * (W // 2), C, dt, 2, E.POOLB_BLOCKS)
        _, ppb, gy = chunk_geometry(nchunk)
        blocks = min(-(-(npix // 4) // (2 * ppb)), E.POOLB_BLOCKS) * gy
        kept = {}                         # the gradient as the stored form wrote it: the sums of both forms are taken on those bits
        for stored in (True, False):
            outs = SUMS(C)
            if stored:
                outs["dA"] = Out((B, H, W, C), TORCH_DT[dt])

            def run(ws, o, stored=stored):
                ops.maxpool_bwd(ops.Act(ins["dP"]), ops.Act(ins["dS"]), ops.Act(ins["y"], 0, C, ins["sc"], ins["sh"], 0), ops.Act(o["dA"]) if stored else None,
                                ins["mean"], ins["invstd"], ws)
                ops.bn_bwd_finalize(ws, npix, o["dgamma"], o["dbeta"], o["coef"])

            def check(o, stored=stored):
                if stored:
                    got = o["dA"].float().cpu()
                    E.check_pool_grad(got, pb, dt, "maxpool_bwd")
                    kept["dA"] = R.as_stored(got, pb["dA"])
                ref = R.bn_bwd_sums_ref(kept["dA"], y, sc, sh, mean, invstd)
                E.check_sums(o["dgamma"], o["dbeta"], o["coef"], ref, 4 * trips, fold, dt, "maxpool_bwd fused sums" if stored else "maxpool_bwd sums only")
            hold("maxpool_bwd(bn_ws=) " + ("stored" if stored else "sums only"),
                 [(Case(f"{B}x{H}x{W} C {C}", lib().cmu_bn_bwd_ws_bytes(C), outs, ins, DEV, dt, blocks, False), run, check)])


def test_conv1x1_head_bwd(ops):
    """Two workspaces: the head's own slab (``ws``: the one under the three states) and, with ``bn_ws``, the BatchNorm slab that
    bn_bwd_finalize reads (a second guarded buffer in the same state).  1 x 111 x 111 of 64 chunks: 12,321 pixels > HEADB_BLOCKS * 16 = 12,288 (the
    cap).  3 x 7 x 9 of 4 chunks: 189 pixels in workgroups of 256: one partly filled workgroup; 37 x 3 x 3 of 16 chunks: several."""
    def one(dt, nchunk, K, B, H, W, bn):
        C, npix = nchunk * EPC[dt], B * H * W
        g = gen(800 + nchunk + K + B)
        x = E.data((B, H, W, C), dt, g)
        w, dl = torch.randn(K, C, generator=g) / C ** 0.5, torch.randn(B, K, H, W, generator=g)
        sc, sh, mean, invstd = E.bn_vectors(x, g)
        assert R.gate_is_safe(x, sc, sh)
        ins = dict(zip(("dl", "x", "w", "sc", "sh", "mean", "invstd"), (dl.to(DEV), act_in(ops, x, dt).buf) + dev(w, sc, sh, mean, invstd)))
        outs = {"dX": Out((B, H, W, C), TORCH_DT[dt]), "dW": Out((K, C)), "dbias": Out((K,))}
        aux = {}
        if bn:
            outs.update(SUMS(C))
            aux = {"bn_ws": lib().cmu_bn_bwd_ws_bytes(C)}

        def run(ws, o):
            xa = ops.Act(ins["x"], 0, C, ins["sc"], ins["sh"], 0)
            if bn:
                ops.conv1x1_head_bwd(ins["dl"], xa, ins["w"], ops.Act(o["dX"]), o["dW"], o["dbias"], ws, ins["mean"], ins["invstd"], o["ws:bn_ws"])
                ops.bn_bwd_finalize(o["ws:bn_ws"], npix, o["dgamma"], o["dbeta"], o["coef"])
            else:
                ops.conv1x1_head_bwd(ins["dl"], xa, ins["w"], ops.Act(o["dX"]), o["dW"], o["dbias"], ws)
        hb = R.head_bwd_ref(dl, x, sc, sh, w)
        ppb = 256 // nchunk
        gx = max(1, min(-(-npix // (ppb * 4)), E.HEADB_BLOCKS))
        chain, fold = 4 * -(-npix // (gx * ppb * 4)), fold_k(nchunk, ppb)

        def check(o):
            stored = o["dX"].float().cpu()
            within(stored, hb["dX"], R.elem_bound(hb["dX"], hb["magX"], K, dt), "conv1x1_head_bwd: dX", dt)
            within(o["dW"], hb["dW"], (chain + fold + 1) * U * hb["magW"], "conv1x1_head_bwd: dW", dt)
            within(o["dbias"], hb["db"], (chain + fold) * U * hb["magb"], "conv1x1_head_bwd: dbias", dt)
            if bn:
                ref = R.bn_bwd_sums_ref(R.as_stored(stored, hb["dX"]), x, sc, sh, mean, invstd)
                E.check_sums(o["dgamma"], o["dbeta"], o["coef"], ref, chain, fold, dt, "conv1x1_head_bwd fused sums")
        case = Case(f"{B}x{H}x{W} C {C} K {K}" + (" +bn_ws" if bn else ""), lib().cmu_conv1x1_head_bwd_ws_bytes(B, H, W, C, K), outs, ins, DEV, dt, gx,
                    -(-npix // (ppb * 4)) > E.HEADB_BLOCKS, aux_ws=aux)
        return case, run, check
    hold("conv1x1_head_bwd", [one("f32", 64, 3, 1, 111, 111, True), one("bf16", 16, 2, 37, 3, 3, True), one("f32", 4, 3, 3, 7, 9, False),
                              one("f16", 1, 1, 1, 1, 1, True)])


# ------------------------------------------------------------------------------------------------------------------------------------
# "wg": cmu_conv3x3_c1_wgrad, cmu_conv3x3_c1_wgrad_bn (reading and recomputing), cmu_conv3x3_c1_wgrad_bn_tiles
# ------------------------------------------------------------------------------------------------------------------------------------
def wg_leftovers(ops):
    """The bytes conv3x3_wgrad at 64 -> 64 channels and convT2x2_wgrad leave in "wg" (the engine hands the same buffer to the first layer next)."""
    if "wg" not in LEFT:
        B, H, W, dt = 2, 32, 32, "bf16"
        g = gen(5)
        x, dY = act_in(ops, torch.randn(B, H, W, 64, generator=g), dt), act_in(ops, torch.randn(B, H, W, 64, generator=g), dt)
        a = left_by(lambda ws: ops.conv3x3_wgrad(x, dY, torch.empty(64, 64, 3, 3, device=DEV), ws), lib().cmu_conv3x3_wgrad_ws_bytes(B, H, W, 64, 64, ops.dt_code(dt)))
        dO = act_in(ops, torch.randn(B, 2 * H, 2 * W, 32, generator=g), dt)
        b = left_by(lambda ws: ops.convT2x2_wgrad(x, dO, torch.empty(64, 32, 2, 2, device=DEV), torch.empty(32, device=DEV), ws),
                    lib().cmu_convT2x2_wgrad_ws_bytes(B, H, W, 64, 32, ops.dt_code(dt)))
        LEFT["wg"] = {"conv3x3_wgrad 64->64": a, "convT2x2_wgrad 64->32": b}
    return LEFT["wg"]


def test_conv3x3_c1_wgrad(ops):
    """4 x 192 x 192: 576 tiles > C1W_BLOCKS = 512 (the cap: two tiles for some workgroups); 2 x 5 x 37 of 6 chunks: 6 partial tiles; 1 x 2 x 2: one
    workgroup.  The three dense forms share the geometry: plain, fused BatchNorm reading yraw, fused BatchNorm recomputing it from ``w``."""
    wg = wg_leftovers(ops)

    def one(dt, case, masked, form, leftovers=None):
        B, H, W, nchunk = case
        Cout = nchunk * EPC[dt]
        g = gen(1100 + H + masked)
        x, w = torch.randn(B, H, W, generator=g), torch.randn(Cout, 1, 3, 3, generator=g) / 3
        mask = E.c1_mask(masked, B, H, W, g)
        dY = E.data((B, H, W, Cout), dt, g, 1.0, 0.0)
        yref, _ = R.c1_fwd_ref(x, w, mask, masked == 2)
        yraw = R.quant(yref.float(), dt)
        if form == "bn_w":          # the recomputing form must reproduce the bits the forward stored: take them from the forward kernel
            ya = ops.new_act(B, H, W, Cout, dt, DEV)
            ops.conv3x3_c1_fwd(*dev(x, w), ya, None, None if mask is None else mask.to(DEV), masked == 2)
            yraw = ya.buf.float().cpu()
        sc, sh, mean, invstd = E.bn_vectors(yraw, g)
        assert R.gate_is_safe(yraw, sc, sh)
        coef = torch.randn(2, Cout, generator=g) * 0.1
        ins = dict(zip(("x", "w", "dY", "yraw", "sc", "sh", "mean", "invstd", "coef"),
                       dev(x, w) + (act_in(ops, dY, dt).buf, act_in(ops, yraw, dt).buf) + dev(sc, sh, mean, invstd, coef)))
        if mask is not None:
            ins["mask"] = mask.to(DEV)

        def run(ws, o):
            m = ins.get("mask")
            if form == "plain":
                ops.conv3x3_c1_wgrad(ins["x"], ops.Act(ins["dY"]), o["dW"], ws, m, masked == 2)
            else:
                ops.conv3x3_c1_wgrad_bn(ins["x"], ops.Act(ins["dY"]), ops.Act(ins["yraw"]), ins["sc"], ins["sh"], ins["mean"], ins["invstd"], ins["coef"], o["dW"], ws,
                                        m, masked == 2, w=ins["w"] if form == "bn_w" else None)
        chain, fold = E.c1_chain(B, H, W, nchunk, E.C1W_BLOCKS)
        if form == "plain":
            ref, mag = R.c1_wgrad_ref(x, dY, mask, masked == 2)
            k = chain + fold
        else:
            r, m_ = R.bn_bwd_apply_ref(dY, yraw, sc, sh, mean, invstd, coef)
            ref, mag = R.c1_wgrad_ref(x, r, mask, masked == 2, mdY=m_)
            k = chain + fold + E.K_APPLY
        ntile = B * -(-H // 16) * -(-W // 16)
        check = lambda o: within(o["dW"].view(Cout, 9), ref, k * U * mag, f"conv3x3_c1_wgrad ({form}): dW", dt)
        return (Case(f"{B}x{H}x{W} Cout {Cout} mask {masked}", lib().cmu_conv3x3_c1_wgrad_ws_bytes(B, H, W, Cout), {"dW": Out((Cout, 1, 3, 3))}, ins, DEV, dt,
                     min(ntile, E.C1W_BLOCKS), ntile > E.C1W_BLOCKS, leftovers), run, check)
    hold("conv3x3_c1_wgrad", [one("f32", (4, 192, 192, 2), 0, "plain"), one("bf16", (2, 5, 37, 6), 2, "plain"), one("f16", (1, 2, 2, 1), 1, "plain"),
                              one("f32", (2, 20, 24, 4), 0, "plain", {"convT2x2_wgrad 64->32": wg["convT2x2_wgrad 64->32"]})])
    hold("conv3x3_c1_wgrad_bn", [one("bf16", (4, 192, 192, 2), 2, "bn"), one("f32", (2, 5, 37, 6), 1, "bn"), one("f32", (1, 2, 2, 1), 0, "bn"),
                                 one("bf16", (2, 20, 24, 4), 0, "bn", {"conv3x3_wgrad 64->64": wg["conv3x3_wgrad 64->64"]})])
    hold("conv3x3_c1_wgrad_bn(w=)", [one("f32", (4, 192, 192, 2), 0, "bn_w"), one("bf16", (2, 5, 37, 6), 2, "bn_w"),
                                     one("f16", (2, 20, 24, 4), 0, "bn_w", {"conv3x3_wgrad 64->64": wg["conv3x3_wgrad 64->64"]})])


def test_conv3x3_c1_wgrad_bn_tiles(ops):
    """The tile-list form: 530 listed tiles of 576 (max_tiles 576 > C1W_BLOCKS: the cap); a list ONE SHORTER than max_tiles (11 of 12: the surplus
    workgroup writes a zero row); an EMPTY list (count 0 of max_tiles 3: every workgroup's row must still be written, dW is exactly 0)."""
    def one(dt, case, masked, recompute):
        B, H, W, nchunk, count, max_tiles = case
        Cout = nchunk * EPC[dt]
        g = gen(1300 + H + masked)
        x, w = torch.randn(B, H, W, generator=g), torch.randn(Cout, 1, 3, 3, generator=g) / 3
        mask = E.c1_mask(masked, B, H, W, g)
        mask_d = None if mask is None else mask.to(DEV)
        tY, tX = -(-H // 16), -(-W // 16)
        if count > 0:
            tl, sel = E.c1_tile_list(B, H, W, count, g)
        else:
            tl, sel = torch.randperm(B * tY * tX, generator=g).to(I32), torch.zeros(B, H, W, dtype=F64)
        tiles = types.SimpleNamespace(list=tl.to(DEV), count=torch.tensor([count], dtype=I32, device=DEV), tile_h=16, tile_w=16)
        ya = ops.Act(torch.zeros(B, H, W, Cout, dtype=TORCH_DT[dt], device=DEV))
        ops.conv3x3_c1_fwd_tiles(*dev(x, w), ya, tiles, max(max_tiles, 1), mask_d, masked == 2, want_stats=False)
        ref, _ = R.c1_fwd_ref(x, w, mask, masked == 2)
        yraw = torch.where(sel.bool().unsqueeze(-1), ya.buf.float().cpu(), R.quant(ref.float(), dt))
        dA = E.data((B, H, W, Cout), dt, g, 1.0, 0.0)
        sc, sh, mean, invstd = E.bn_vectors(yraw, g)
        assert R.gate_is_safe(yraw, sc, sh)
        coef = torch.randn(2, Cout, generator=g) * 0.1
        ins = dict(zip(("x", "w", "dA", "yraw", "sc", "sh", "mean", "invstd", "coef", "list", "count"),
                       dev(x, w) + (act_in(ops, dA, dt).buf, ya.buf) + dev(sc, sh, mean, invstd, coef) + (tiles.list, tiles.count)))
        if mask_d is not None:
            ins["mask"] = mask_d
        r, m = R.bn_bwd_apply_ref(dA, yraw, sc, sh, mean, invstd, coef, sel=sel)
        dref, dmag = R.c1_wgrad_ref(x, r, mask, masked == 2, mdY=m)
        chain, fold = E.c1_tiles_chain(count, max_tiles, nchunk, E.C1W_BLOCKS)

        def run(ws, o):
            ops.conv3x3_c1_wgrad_bn_tiles(ins["x"], ops.Act(ins["dA"]), ops.Act(ins["yraw"]), ins["sc"], ins["sh"], ins["mean"], ins["invstd"], ins["coef"], o["dW"], ws,
                                          tiles, max_tiles, mask_d, masked == 2, w=ins["w"] if recompute else None)

        def check(o):
            within(o["dW"].view(Cout, 9), dref, (chain + fold + E.K_APPLY) * U * dmag, f"conv3x3_c1_wgrad_bn_tiles ({'recomputed' if recompute else 'read'}): dW", dt)
            if count == 0:
                assert bool((o["dW"] == 0).all())
        return (Case(f"{B}x{H}x{W} Cout {Cout} list {count} of {max_tiles}" + (" w=" if recompute else ""), lib().cmu_conv3x3_c1_wgrad_ws_bytes(B, H, W, Cout),
                     {"dW": Out((Cout, 1, 3, 3))}, ins, DEV, dt, min(max_tiles, E.C1W_BLOCKS), max_tiles > E.C1W_BLOCKS), run, check)
    hold("conv3x3_c1_wgrad_bn_tiles", [one("f32", (4, 192, 192, 2, 530, 576), 0, False), one("bf16", (4, 192, 192, 2, 530, 576), 2, True),
                                       one("f32", (3, 20, 37, 6, 11, 12), 2, False), one("bf16", (3, 20, 37, 6, 11, 12), 0, True),
                                       one("f32", (1, 16, 48, 4, 0, 3), 0, False), one("f16", (1, 16, 48, 4, 0, 3), 0, True)])


# ------------------------------------------------------------------------------------------------------------------------------------
# losses: every one a two-pass reduction (per-workgroup or per-row partials, one final workgroup)
# ------------------------------------------------------------------------------------------------------------------------------------
def ratio_note(what, ratio):
    """A check that is a plain assertion in its own test file: its err / bound goes into the entry's line the same way."""
    E.PARITY[(what, "f32")] = max(E.PARITY.get((what, "f32"), 0.0), float(ratio))


def test_masked_mse_fwd_bwd(ops):
    """One slot group per image row (no cap: (4 B H + 4) floats).  The four kernel forms of test_gpu_heads_optim_fp64.py's MMSE_CASES at
    small shapes: wave rows (W % 4 == 0, W <= 1024), block rows + float4 gradient (W > 1024), block rows + scalar gradient (W % 4 != 0)."""
    from oracle import cmunet as OC

    def one(B, K, ch, H, W, ls):
        g = gen(200 + W)
        logits, img = torch.randn(B, K, H, W, generator=g), torch.randn(B, H, W, generator=g) * 2 + 1
        mask = (torch.rand(B, H, W, generator=g) > 0.4).to(U8)
        ins = dict(zip(("logits", "img", "mask"), dev(logits, img, mask)))
        lo = logits.double().requires_grad_(True)
        ref = OC.masked_mse(lo[:, ch], img.double(), mask)
        (ref * ls).backward()
        im = img.double()
        mean, std = im.mean(-1, keepdim=True), (im.var(-1, keepdim=True) + 1e-6).sqrt()
        t = (im - mean) / std
        k = 2.0 * ls / float(mask.sum())
        eps_row = 2 * (W / 64 + 16) * U
        bound = torch.zeros(B, K, H, W, dtype=F64)
        bound[:, ch] = k * mask.double() * (4 * U * (logits[:, ch].double().abs() + t.abs()) + eps_row * (t.abs() + im.abs().mean(-1, keepdim=True) / std))

        def check(o):
            assert abs(o["loss"].item() - ref.item()) <= 1e-5 * abs(ref.item())
            ratio_note("masked_mse loss", abs(o["loss"].item() - ref.item()) / (1e-5 * abs(ref.item())))
            within(o["dlogits"], lo.grad, bound, "masked mse dlogits")
        return (Case(f"{B}x{K}x{H}x{W} ch {ch}", lib().cmu_masked_mse_ws_bytes(B, H), {"loss": Out((1,)), "dlogits": Out((B, K, H, W))}, ins, DEV, "f32", B * H, False),
                lambda ws, o: ops.masked_mse_fwd_bwd(ins["logits"], ch, ins["img"], ins["mask"], o["loss"], o["dlogits"], ls, ws, None), check)
    hold("masked_mse_fwd_bwd", [one(3, 2, 1, 20, 64, 1.0), one(2, 3, 2, 5, 1028, 1.0), one(3, 2, 0, 7, 33, 0.5), one(1, 2, 1, 1, 4, 3.0)])


def test_mse_fwd_bwd(ops):
    """genesis.mse_fwd_bwd: MSE_MAX_BLOCKS = 1024 workgroups of 4,096 pixels -- the cap needs 4.2 M pixels and one more: 5 x 916 x 916
    (4,195,280 pixels, K = 1: as many logits); 3 x 40 x 56 = 6,720 pixels: two workgroups, the second partly filled; 1 x 3 x 5: one."""
    from cmunet_amd import genesis as G

    def one(B, H, W):
        g = gen(B + H)
        logits, y = torch.randn(B, 1, H, W, generator=g), torch.randn(B, H, W, generator=g)
        ins = dict(zip(("logits", "y"), dev(logits, y)))
        ref = torch.nn.functional.mse_loss(logits.double().squeeze(1), y.double())
        gref = 2.0 * (logits.double() - y.double().unsqueeze(1)) / (B * H * W)

        def check(o):
            assert abs(float(o["loss"]) - float(ref)) <= 1e-6 * float(ref)
            ratio_note("mse loss", abs(float(o["loss"]) - float(ref)) / (1e-6 * float(ref)))
            assert torch.allclose(o["dlogits"].cpu().double(), gref, rtol=1e-5, atol=1e-12)
        n = B * H * W
        return (Case(f"{B}x{H}x{W}", lib().cmu_mse_ws_bytes(), {"loss": Out((1,)), "dlogits": Out((B, 1, H, W))}, ins, DEV, "f32", min(-(-n // 4096), 1024), n > 4096 * 1024),
                lambda ws, o: G.mse_fwd_bwd(ins["logits"], ins["y"], o["loss"], o["dlogits"], 1.0, None, ws), check)
    hold("mse_fwd_bwd", [one(5, 916, 916), one(3, 40, 56), one(1, 3, 5)])


def test_softmax_ce_dice_fwd_bwd(ops):
    """CE_MAX_BLOCKS = 1024 workgroups of 256 pixels: 5 x 230 x 230 = 264,500 pixels is past it; 2 x 12 x 20 = 480: two workgroups, the second
    partly filled; 1 x 3 x 5: one.  The checks of test_gpu_heads_optim_fp64.py::test_softmax_ce_dice."""
    from oracle import losses as OL
    from test_gpu_heads_optim_fp64 import f32

    def one(B, H, W, ls):
        npix = B * H * W
        g = gen(300 + H)
        logits = torch.randn(B, 2, H, W, generator=g) * 2
        d = logits[:, 1] - logits[:, 0]
        logits[:, 1] += torch.where(d.abs() < 1e-3, 2e-3 * torch.sign(d + 1e-30), torch.zeros_like(d))
        ties = torch.rand(B, H, W, generator=g) < 0.05
        logits[:, 1] = torch.where(ties, logits[:, 0], logits[:, 1])
        y1 = torch.rand(B, H, W, generator=g, dtype=F64)
        y1h = torch.stack([1 - y1, y1], 1).contiguous()
        ins = dict(zip(("logits", "y1h"), dev(logits, y1h)))
        lo = logits.double().requires_grad_(True)
        ce = OL.cross_entropy_prob(lo, y1h)
        (ce * ls).backward()
        L = logits.double()
        lse = torch.logsumexp(L, 1, keepdim=True)
        pr = (L[:, 1] > L[:, 0]).double()
        tp, spr, sgt = float((y1h[:, 1] * pr).sum()), float(pr.sum()), float(y1h[:, 1].sum())
        p = torch.softmax(L, 1)
        gs = f32(ls) / npix
        ys = y1h.sum(1, keepdim=True).abs()

        def check(o_):
            o = o_["out"].cpu().double()
            bce = 8 * U * float((y1h * (L.abs() + lse.abs())).sum() / npix) + U * abs(ce.item())
            assert abs(o[0] - ce.item()) <= bce
            ratio_note("ce_dice ce", abs(float(o[0]) - ce.item()) / bce)
            for got, want, name in ((o[3], tp, "tp"), (o[4], spr, "sum pr"), (o[5], sgt, "sum gt"),
                                    (o[1], float(OL.dice_loss(L, y1h)), "dice"), (o[2], float(OL.iou_loss(L, y1h)), "iou")):
                assert abs(float(got) - want) <= 2 * U * abs(want) + 1e-12, (name, float(got), want)
            within(o_["dlogits"], lo.grad, gs * U * (8 * (p * ys + y1h.abs()) + 2 * (L - lse).abs() * p * ys), "ce dlogits")
        return (Case(f"{B}x{H}x{W}", lib().cmu_softmax_ce_dice_ws_bytes(B, H, W), {"out": Out((6,)), "dlogits": Out((B, 2, H, W))}, ins, DEV, "f32",
                     min(-(-npix // 256), 1024), npix > 256 * 1024),
                lambda ws, o: ops.softmax_ce_dice_fwd_bwd(ins["logits"], ins["y1h"], o["out"], o["dlogits"], ls, ws), check)
    hold("softmax_ce_dice_fwd_bwd", [one(5, 230, 230, 3.0), one(2, 12, 20, 1.0), one(1, 3, 5, 1.0)])


def test_seg_stats_fwd(ops):
    """The cases of test_gpu_seg_criterion_fp64.py: "odd" (2 x 9 x 13: one workgroup, scalar path), "vec" (3 x 64 x 64: several), and
    "scalar_stride" (5 x 257 x 257 = 330,245 pixels on the one-pixel-per-lane path: 1,291 workgroups' worth, past the 1,024 cap); K = 2, 3, 8:
    the slot width 1 + 5 K of the workspace."""
    import test_gpu_seg_criterion_fp64 as S
    cases = []
    for K, shape, target in ((3, "scalar_stride", "soft64"), (8, "vec", "onehot32"), (2, "vec", "soft64"), (3, "odd", "onehot64")):
        c = S.make_case(K, shape, target)
        ins = dict(zip(("logits", "y", "w"), dev(c.logits, c.y_dev, c.w)))

        def check(o, c=c, K=K):
            t = o["table"].cpu()
            ce = float(S.ce_weighted(c.L, c.y, c.w.double()))
            ce_bound = 8 * U * float((c.w.double().view(1, K, 1, 1) * c.y * (c.L.abs() + c.lse.abs())).sum() / c.npix)
            assert abs(float(t[0]) - ce) <= ce_bound
            ratio_note("seg_stats ce", abs(float(t[0]) - ce) / ce_bound)
            for name, got, want, k in (("tp_soft", t[1:1 + K], c.tp_soft, 16), ("spr_soft", t[1 + K:1 + 2 * K], c.spr_soft, 16),
                                       ("tp_hard", t[1 + 2 * K:1 + 3 * K], c.tp_hard, 2), ("spr_hard", t[1 + 3 * K:1 + 4 * K], c.spr_hard, 2),
                                       ("sgt", t[1 + 4 * K:], c.sgt, 2)):
                err = (got - want).abs()
                assert bool((err <= k * U * want.abs()).all()), (name, got.tolist(), want.tolist())
                ratio_note("seg_stats " + name, float((err / (k * U * want.abs()).clamp_min(1e-300)).max()))
        V = 1 if (c.H * c.W) % (2 if K > 4 else 4) else (2 if K > 4 else 4)
        nb = -(-(c.npix // V) // 256)
        cases.append((Case(f"K {K} {shape} {target}", lib().cmu_seg_stats_ws_bytes(K), {"table": Out((1 + 5 * K,), F64)}, ins, DEV, "f32", min(nb, 1024), nb > 1024),
                      lambda ws, o, ins=ins, c=c: ops.seg_stats_fwd(ins["logits"], ins["y"], ins["w"], c.thr, o["table"], ws), check))
    hold("seg_stats_fwd", cases)


def test_pointwise_loss_fwd(ops):
    """The cases of test_gpu_pointwise_losses_fp64.py: "scalar_stride" (330,245 elements, one per lane: past the 1,024-workgroup cap), "vec"
    (3 x C x 64 x 64), "odd" (2 x C x 9 x 13: inner = 117, the scalar path), one kind each and all four kinds on "odd"."""
    import pointwise_loss_ref as PR
    import test_gpu_pointwise_losses_fp64 as P
    cases = []
    for kind, shape, C, ydt in [("bce_with_logits", "scalar_stride", 1, "f64"), ("mse", "vec", 3, "f32"), ("l1", "vec", 8, "f64")] + [(k, "odd", 2, "f64") for k in PR.KINDS]:
        x, y, w, pw = P.pw_case(kind, shape, C, ydt)
        r = PR.pointwise_ref(kind, x, y, w, pw, 0.37 / x.numel())
        ins = {k: v.to(DEV) for k, v in (("x", x), ("y", y), ("w", w), ("pw", pw)) if v is not None}

        def check(o, r=r):
            s_ratio = abs(float(o["out"][0]) - float(r["S"])) / (P.C_GRAD * U * float(r["S_mag"]))
            assert math.isfinite(float(o["out"][0])) and s_ratio <= 1.0
            ratio_note("pointwise_loss S", s_ratio)
        V = 4 if x[0, 0].numel() % 4 == 0 else 1
        nb = -(-(x.numel() // V) // 256)
        cases.append((Case(f"{kind} {shape} C {C} {ydt}", lib().cmu_pointwise_loss_ws_bytes(), {"out": Out((1,), F64)}, ins, DEV, "f32", min(nb, 1024), nb > 1024),
                      lambda ws, o, ins=ins, kind=kind: ops.pointwise_loss_fwd(kind, ins["x"], ins["y"], ins.get("w"), ins.get("pw"), o["out"], ws), check))
    hold("pointwise_loss_fwd", cases)


def test_index_ce_fwd(ops):
    """The cases of test_gpu_pointwise_losses_fp64.py: "scalar_stride" (5 x 257 x 257, one pixel per lane: past the 1,024-workgroup cap), "vec"
    and "odd"; label planes and one-hot planes, log-probability input, ignored pixels."""
    import pointwise_loss_ref as PR
    import test_gpu_pointwise_losses_fp64 as P
    cases = []
    for K, shape, target, log_input, keep in ((3, "scalar_stride", "oh32", False, (0, 2)), (8, "vec", "oh64", False, (1, 2, 3, 4, 5, 6, 7)), (3, "vec", "u8", True, None),
                                              (5, "odd", "i64", True, None), (2, "odd", "f32", False, None)):
        x, tgt, labels, ign = P.ice_case(K, shape, target, log_input, keep)
        onehot, keep_l = target.startswith("oh"), None if keep is None else list(keep)
        w = torch.tensor(P.WEIGHTS[:K])
        r = PR.index_ce_ref(x, labels, w, ign, log_input, keep_l, 0.37 / labels.numel(), 0.011 / labels.numel())
        ins = dict(zip(("x", "target", "w"), dev(x, tgt, w)))

        def check(o, r=r):
            T = o["table"].cpu()
            for i, k in ((0, P.C_GRAD), (1, 2), (2, P.C_GRAD)):
                ratio = abs(float(T[i]) - float(r["T"][i])) / max(k * U * float(r["T_mag"][i]), 1e-300)
                assert math.isfinite(float(T[i])) and ratio <= 1.0, i
                ratio_note(f"index_ce T{i}", ratio)
        B, H, W = P.ICE_SHAPES[shape]
        V = 1 if (H * W) % (2 if K > 4 else 4) else (2 if K > 4 else 4)
        nb = -(-(B * H * W // V) // 256)
        cases.append((Case(f"K {K} {shape} {target} log_input {log_input}", lib().cmu_index_ce_ws_bytes(), {"table": Out((3,), F64)}, ins, DEV, "f32", min(nb, 1024), nb > 1024),
                      lambda ws, o, ins=ins, a=(onehot, log_input, keep_l, ign): ops.index_ce_fwd(ins["x"], ins["target"], a[0], a[1], a[2], ins["w"], a[3], o["table"], ws),
                      check))
    hold("index_ce_fwd", cases)


def test_spark_loss_fwd_bwd(ops):
    """One workgroup per patch, three slots each, one final workgroup (no cap).  Mask ratio 0.75; 1 (every patch masked); 0 (every patch
    kept: loss 0 and, as the kernel documents, NO gradient -- drec is exactly 0 everywhere, so it is still written)."""
    from oracle import spark as OS

    def one(B, p, f, ratio):
        H = f * p
        g = gen(900 + p + int(ratio * 4))
        img, rec = torch.randn(B, H, H, generator=g) * 1.5 + 0.3, torch.randn(B, H, H, generator=g)
        active = OS.make_active(B, f, ratio, generator=g)
        ls = 2.0
        ins = dict(zip(("rec", "img", "active"), dev(rec, img, active.to(U8))))
        rd = rec.double().view(B, 1, H, H).requires_grad_(True)
        ref = OS.recon_loss(img.double().view(B, 1, H, H), rd, active)
        (ref * ls).backward()
        ip = img.double().view(B, f, p, f, p)
        mean, std = ip.mean((2, 4), keepdim=True), (ip.var((2, 4), keepdim=True) + 1e-6).sqrt()
        amean = ip.abs().mean((2, 4), keepdim=True)
        t = ((ip - mean) / std).view(B, H, H)
        masked = (~active.view(B, f, 1, f, 1)).expand(B, f, p, f, p).reshape(B, H, H).double()
        k = 2.0 * ls / ((float((~active).sum()) + 1e-8) * p * p)
        eps_p = 2 * (p * p / 256 + 16) * U
        bound = k * masked * (4 * U * (rec.double().abs() + t.abs()) + eps_p * (t.abs() + (amean / std).expand(B, f, p, f, p).reshape(B, H, H)))

        def check(o):
            assert abs(o["loss"].item() - ref.item()) <= 1e-5 * abs(ref.item())
            within(o["drec"], rd.grad.view(B, H, H), bound, f"spark drec p={p} ratio={ratio}")
        return (Case(f"{B}x{H}x{H} p {p} f {f} ratio {ratio}", lib().cmu_spark_loss_ws_bytes(B, f), {"loss": Out((1,)), "drec": Out((B, H, H))}, ins, DEV, "f32", B * f * f, False),
                lambda ws, o: ops.spark_loss_fwd_bwd(ins["rec"], ins["img"], ins["active"], o["loss"], o["drec"], ls, p, ws), check)
    hold("spark_loss_fwd_bwd", [one(3, 16, 5, 0.75), one(2, 32, 3, 1.0), one(2, 16, 4, 0.0), one(1, 2, 1, 1.0)])


def test_soft_skeleton_and_cldice_sums(ops):
    """soft_skeleton(ws=): two ping-pong planes of the image's size; binary images give the exact skeleton of oracle.losses.soft_skel, [0, 1]
    images within 4 (num_iter + 1) U (test_gpu_heads_optim_fp64.py::test_soft_cldice_pieces).  cldice_sums(ws=): CLD_BLOCKS = 512 workgroups of
    1,024 elements: 2 x 513 x 513 = 526,338 elements is past the cap; 2 x 31 x 45 = 2,790: three workgroups, the last partly filled."""
    from oracle import losses as OL
    sk_cases, sum_cases = [], []
    for (B, H, W), num_iter in (((2, 64, 65), 10), ((2, 31, 45), 3), ((1, 17, 1), 1), ((1, 1, 1), 3)):
        g = gen(1000 + H * 64 + W + num_iter)
        fg = (torch.rand(B, H, W, generator=g) > 0.5).float()
        soft = torch.rand(B, H, W, generator=g)
        for name, img in (("binary", fg), ("soft", soft)):
            ref = OL.soft_skel(img.double().unsqueeze(1), num_iter)[:, 0]
            ins = {"img": img.to(DEV)}

            def check(o, ref=ref, name=name, num_iter=num_iter):
                if name == "binary":
                    assert torch.equal(o["skel"].cpu().double(), ref)
                else:
                    within(o["skel"], ref, 4 * (num_iter + 1) * U, "soft skeleton of [0,1]")
            n = B * H * W
            sk_cases.append((Case(f"{B}x{H}x{W} {name} num_iter {num_iter}", lib().cmu_soft_skeleton_ws_bytes(n), {"skel": Out((B, H, W))}, ins, DEV, "f32", -(-n // 256), False),
                             lambda ws, o, ins=ins, num_iter=num_iter: ops.soft_skeleton(ins["img"], o["skel"], num_iter, ws), check))
    hold("soft_skeleton", sk_cases)
    for B, H, W in ((2, 513, 513), (2, 31, 45), (1, 3, 5)):
        g = gen(B * H + W)
        t = [torch.rand(B, H, W, generator=g) for _ in range(4)]
        t[1], t[3] = (t[1] > 0.5).float(), (t[3] > 0.5).float()
        ins = dict(zip(("sp", "yt", "st", "yp"), dev(*t)))
        d = [x.double() for x in t]
        want = torch.stack([(d[0] * d[1]).sum(), d[0].sum(), (d[2] * d[3]).sum(), d[2].sum()])
        n = B * H * W
        sum_cases.append((Case(f"{B}x{H}x{W}", lib().cmu_cldice_sums_ws_bytes(), {"out4": Out((4,))}, ins, DEV, "f32", min(-(-n // 1024), 512), n > 512 * 1024),
                          lambda ws, o, ins=ins: ops.cldice_sums(ins["sp"], ins["yt"], ins["st"], ins["yp"], o["out4"], ws),
                          lambda o, want=want, n=n: within(o["out4"], want, (n / 131072 + 16) * U * want, "cldice sums")))
    hold("cldice_sums", sum_cases)


def test_soft_skeleton_save_and_bwd(ops):
    """soft_skeleton_save: the kept buffer (cmu_soft_skeleton_save_ws_bytes) is the workspace under the three states -- and an OUTPUT of the
    call, read by soft_skeleton_bwd next: the pair is held together (save into the guarded buffer, then the reverse sweep with its own
    guarded workspace in the same state).  References and bars of test_gpu_cldice_grad_fp64.py: the saving forward has the bits of
    cmu_soft_skeleton; the gradient per element within max(4 e32, 8 u max|g64|)."""
    import cldice_grad_restate as CR
    from test_gpu_cldice_grad_fp64 import grad_bar, worst_ratio
    cases = []
    for kind, shape, N, sign in (("vessels", (2, 64, 65), 10, 0), ("saturated", (3, 5, 7), 3, 1), ("smooth", (2, 17, 33), 1, 0), ("vessels", (1, 1, 1), 3, 0),
                                 ("saturated", (2, 2, 2), 0, 1)):
        img = CR.tie_planes(kind, shape, seed=2)
        gup = CR.upstream(shape, N, sign)
        want64, _ = CR.skel_grad_autograd(img, gup, N, torch.float64)
        want32, _ = CR.skel_grad_autograd(img, gup, N, torch.float32)
        ins = {"img": torch.from_numpy(img).to(DEV), "g": torch.from_numpy(gup).to(DEV)}
        plain = torch.empty_like(ins["img"])
        ops.soft_skeleton(ins["img"], plain, N)
        n = int(np.prod(shape))

        def run(ws, o, ins=ins, N=N):
            ops.soft_skeleton_save(ins["img"], o["skel"], N, kept=ws)
            ops.soft_skeleton_bwd(ins["img"], ws, N, o["dimg"], g_skel=ins["g"], ws=o["ws:bwd"])

        def check(o, plain=plain, want64=want64, want32=want32):
            assert torch.equal(o["skel"], plain), "the saving forward differs from cmu_soft_skeleton"
            ratio_note("skel_bwd", worst_ratio(o["dimg"], want64, grad_bar(want64, want32), "skel_bwd"))
        cases.append((Case(f"{kind} {'x'.join(map(str, shape))} N {N}", lib().cmu_soft_skeleton_save_ws_bytes(n, N), {"skel": Out(shape), "dimg": Out(shape)}, ins, DEV,
                           "f32", -(-n // 256), False, aux_ws={"bwd": lib().cmu_soft_skeleton_bwd_ws_bytes(n)}), run, check))
    hold("soft_skeleton_save + soft_skeleton_bwd", cases)


# ------------------------------------------------------------------------------------------------------------------------------------
# SparK: the mask-token sum and the pixel list
# ------------------------------------------------------------------------------------------------------------------------------------
def test_cells_channel_sum(ops):
    """Integer data: the exact sums bit for bit (test_gpu_spark_select_fp64.py), active and inverted.  5 x 32 x 32 patches of one pixel at 256
    chunks: 1,280 work items > CSUM_ROWS = 1024 (the cap: two items for some workgroups); 3 x 8 x 8 patches of 2 x 2: 16 chunks; an empty
    and a full selection (the other form's sum is then exactly 0 and every slab row must still be written)."""
    import necks_fp64_ref as NR
    from test_gpu_necks_fp64 import exact
    from test_gpu_spark_select_fp64 import cells_geometry, ints, patch_map
    cases = []
    for dt, (B, f, H, C), kind, invert in (("f32", (5, 32, 32, 1024), "quarter", True), ("bf16", (3, 8, 16, 128), "quarter", False), ("f32", (2, 4, 16, 32), "none", False),
                                           ("f16", (2, 4, 16, 64), "all", True), ("f32", (2, 4, 4, 256), "one", True)):
        g = gen(sum((B, f, H, C)))
        active = patch_map(B, f, kind, B + f)
        x = ints((B, H, H, C), g)
        geo = cells_geometry(B, H, C, EPC[dt], f)
        assert geo is not None
        s1, _, _, _ = NR.masked_sums_ref(x, NR.selection(active, H, H, invert))
        ins = {"x": act_in(ops, x, dt).buf, "active": active.to(DEV)}
        cases.append((Case(f"{B}x{H}x{H} C {C} f {f} {kind}{' inverted' if invert else ''}", lib().cmu_cells_channel_sum_ws_bytes(C), {"out": Out((C,))}, ins, DEV, dt,
                           min(geo["nitems"], 1024), geo["nitems"] > 1024),
                      lambda ws, o, ins=ins, invert=invert: ops.cells_channel_sum(ops.Act(ins["x"]), ins["active"], o["out"], invert=invert, ws=ws),
                      lambda o, s1=s1, dt=dt: exact(o["out"], s1, "cells_channel_sum exact: sum", dt)))
    hold("cells_channel_sum", cases)


def test_sparse_pixel_list(ops):
    """cmu_sparse_pixel_list (ops.PixelList allocates its workspace itself: called through the C ABI here): the listed pixels are exactly the
    active patches' pixels, patch-major, the rest of the capacity is -1 and the count is the number of rows written.  An EMPTY patch map, a
    full one (the list fills its capacity exactly), a capacity ONE SHORTER than the list (the first rows are kept), one active patch."""
    from test_gpu_spark_select_fp64 import patch_map
    cases = []
    for (B, f, H), kind, short in (((3, 8, 64), "quarter", 0), ((2, 4, 16), "none", 0), ((2, 4, 16), "all", 0), ((2, 4, 16), "quarter", 1), ((1, 1, 1), "all", 0),
                                   ((3, 4, 8), "one", 0)):
        active = patch_map(B, f, kind, 3 + B)
        sel = R.expand_active(active, H, H)
        n = int(sel.sum())
        cap = max(256, -(-n // 256) * 256) if not short else n - 1
        ins = {"active": active.to(DEV)}

        def check(o, sel=sel, n=n, cap=cap, B=B, H=H):
            rows, cnt = o["rows"].cpu(), int(o["count"].cpu())
            assert cnt == min(n, cap), (cnt, n, cap)
            assert bool((rows[cnt:] == -1).all()), "rows past the count are not -1"
            got = R.rows_to_sel(rows[:cnt], B, H, H)
            assert len(set(rows[:cnt].tolist())) == cnt and bool((got & ~sel).sum() == 0) and (cnt < n or torch.equal(got, sel))
        cases.append((Case(f"{B}x{H}x{H} f {f} {kind}: {n} pixels, capacity {cap}", lib().cmu_sparse_pixel_list_ws_bytes(B, f),
                           {"rows": Out((cap,), I32, prefill=-2), "count": Out((1,), I32, prefill=-1)}, ins, DEV, "i32", min(-(-cap // 256), 4096), False),
                      lambda ws, o, ins=ins, a=(f, B, H, cap): call("cmu_sparse_pixel_list", ops._p(ins["active"]), a[0], a[1], a[2], a[2], ops._p(o["rows"]), a[3],
                                                                     ops._p(o["count"]), ops._p(ws), ops._stream()), check))
    hold("sparse_pixel_list", cases)


# ------------------------------------------------------------------------------------------------------------------------------------
# necks: skinny GEMMs (split-K slabs) and LAMB
# ------------------------------------------------------------------------------------------------------------------------------------
def test_skinny_gemms(ops):
    """Integer operands: the exact product, whatever the split (test_gpu_necks_fp64.py).  The forward's slab is one split-K slab of min(M, 32)
    rows reused by every 32-row group; the input gradient's workspace holds the transposed dy of one group.  (cmu_skinny_gemm_wgrad and the
    16-bit input / weight gradients take no workspace.)  M = 33 / 65: a ragged last group AFTER a full one -- the group that reuses the slab;
    K = 80: several splits with a short last one; K = 8: one split."""
    import necks_fp64_ref as NR
    from test_gpu_necks_fp64 import exact, fwd_kind, ints
    for form in ("f32", "f16", "bf16"):
        cases = []
        for M, K, N in ((65, 80, 70), (33, 4096, 130), (7, 80, 3), (1, 16, 1)):
            g = gen(M * 131 + K * 7 + N)
            x, w, b = ints((M, K), g), ints((N, K), g), ints((N,), g)
            ins = dict(zip(("x", "w", "b"), dev(x, w, b)))
            size = lib().cmu_skinny_gemm_ws_bytes if form == "f32" else lib().cmu_skinny16_gemm_ws_bytes

            def run(ws, o, ins=ins, a=(M, N, K)):
                if form == "f32":
                    call("cmu_skinny_gemm_fwd", ops._p(ins["x"]), ops._p(ins["w"]), ops._p(ins["b"]), ops._p(o["y"]), *a, ops._p(ws), ops._stream())
                else:
                    call("cmu_skinny16_gemm_fwd", ops._p(ins["x"]), ops._p(ins["w"]), ops._p(ins["b"]), ops._p(o["y"]), *a, ops.dt_code(form), ops._p(ws), ops._stream())
            cases.append((Case(f"M {M} K {K} N {N} ({fwd_kind(form, N, K)} split)", size(M, N, K), {"y": Out((M, N))}, ins, DEV, form, 0, False), run,
                          lambda o, r=NR.gemm_fwd_ref(x, w, b): exact(o["y"], r, "skinny_fwd exact: y", form)))
        hold(f"skinny_gemm_fwd {form}", cases)
    cases = []
    for M, K, N in ((65, 80, 70), (33, 64, 130), (7, 80, 3), (1, 4, 1)):
        g = gen(M * 131 + K * 7 + N + 1)
        dy, w = ints((M, N), g), ints((N, K), g)
        ins = dict(zip(("dy", "w"), dev(dy, w)))
        cases.append((Case(f"M {M} K {K} N {N}", lib().cmu_skinny_gemm_bwd_ws_bytes(M, N), {"dx": Out((M, K))}, ins, DEV, "f32", 0, False),
                      lambda ws, o, ins=ins, a=(M, N, K): call("cmu_skinny_gemm_dgrad", ops._p(ins["dy"]), ops._p(ins["w"]), ops._p(o["dx"]), *a, ops._p(ws), ops._stream()),
                      lambda o, r=NR.gemm_dgrad_ref(dy, w): exact(o["dx"], r, "skinny_dgrad exact: dx", "f32")))
    hold("skinny_gemm_dgrad", cases)


def test_lamb_step(ops):
    """One LAMB step on the tensors of test_gpu_heads_optim_fp64.py::test_lamb_step (exactly one block, 66 blocks with a ragged last one, a
    zero tensor, a zero-gradient tensor) against oracle/optim.py with that test's bounds.  p, m and v are updated in place (a finite
    prefill: run() loads the state before the step); u is scratch the step writes completely."""
    import test_gpu_heads_optim_fp64 as H
    from cmunet_amd.optim import FlatParams, FusedLAMB
    from oracle import optim as OO
    blk = lib().cmu_lamb_block_elems()
    shapes, wds = [(blk,), (65 * blk + 17,), (300,), (8191,), (37,)], [0.02, 0.02, 0.02, 0.0, 0.0]
    flat = FlatParams(H._sgd_holder(shapes, 9).to(DEV))
    flat.views[flat.names[2]].data.zero_()
    lr, b1, b2, eps, max_norm, gscale, f32 = 0.02, 0.9, 0.98, 1e-6, 2.0, 0.5, H.f32
    opt = FusedLAMB(flat, lr=lr, betas=(b1, b2), eps=eps, weight_decay=0.02, max_grad_norm=max_norm,
                    decay_filter=lambda name, prm: wds[int(name.split(".")[-1])] != 0.0)
    g = gen(10)
    grads = [torch.randn(*s, generator=g) * (0.01 if i == 1 else 1.0) for i, s in enumerate(shapes)]
    grads[4].zero_()
    norm = math.sqrt(sum(float((gr.double() * gscale).pow(2).sum()) for gr in grads))
    grads = [gr * (max_norm * 1.02 / norm) for gr in grads]
    for nm, gr in zip(flat.names, grads):
        flat.grad_views[nm].copy_(gr)
    n = flat.arena.numel()
    p0, m0, v0 = flat.arena.detach().clone(), torch.randn(n, generator=g).to(DEV) * 0.1, torch.rand(n, generator=g).to(DEV) * 0.1
    ins = {"p0": p0, "m0": m0, "v0": v0, "g": flat.grad, **{f"table{i}": t for i, t in enumerate(opt.tables)}}
    why = "optimiser state, updated in place; run() loads the state before the step"
    outs = {"p": Out((n,), prefill=0.0, accumulates=True, why=why), "m": Out((n,), prefill=0.0, accumulates=True, why=why),
            "v": Out((n,), prefill=0.0, accumulates=True, why=why),
            "u": Out((n,), marks_unwritten=False, why="scratch of the arena's size: the alignment padding between two tensors is never written")}
    step = 2

    def run(ws, o):
        o["p"].copy_(p0); o["m"].copy_(m0); o["v"].copy_(v0)
        ops.lamb_step(o["p"], ins["g"], o["m"], o["v"], o["u"], opt.tables, lr, b1, b2, eps, True, True, max_norm, False, False, step, gscale, ws)
    offs = [flat.offsets[nm] for nm in flat.names]
    before = [t.cpu() for t in (p0, m0, v0)]
    P, M, V = ([before[i][o:o + c].double().clone() for o, c in offs] for i in range(3))
    G = [gr.flatten().float().double() * gscale for gr in grads]
    gn = OO.lamb_step(P, G, M, V, f32(lr), [f32(w) for w in wds], betas=(f32(b1), f32(b2)), eps=f32(eps), bias_correction=True, grad_averaging=True,
                      max_grad_norm=max_norm, trust_clip=False, always_adapt=False, step=step)
    clip = 1.0 / (gn / max_norm) if gn > max_norm else 1.0
    b3, bc1, bc2 = 1 - f32(b1), 1 - f32(b1) ** step, 1 - f32(b2) ** step

    def check(o):
        pa, ma, va = o["p"].cpu(), o["m"].cpu(), o["v"].cpu()
        for t, (of, c) in enumerate(offs):
            p_, m_, v_ = (x[of:of + c].double() for x in before)
            gg = G[t] * clip
            mag_m = f32(b1) * m_.abs() + b3 * gg.abs()
            denom = V[t].sqrt() / math.sqrt(bc2) + f32(eps)
            upd = (M[t] / bc1) / denom + f32(wds[t]) * p_
            un = float(upd.norm())
            r = float((P[t] - p_).norm()) / (f32(lr) * un) if un > 0 else 1.0
            mag_u = (mag_m / bc1) / denom + f32(wds[t]) * p_.abs()
            within(ma[of:of + c], M[t], 4 * U * mag_m + H.EPS_RED * b3 * gg.abs(), f"lamb tensor {t} m")
            within(va[of:of + c], V[t], 6 * U * (f32(b2) * v_ + (1 - f32(b2)) * gg ** 2) + 2 * H.EPS_RED * (1 - f32(b2)) * gg ** 2, f"lamb tensor {t} v")
            within(pa[of:of + c], P[t], 8 * U * (p_.abs() + f32(lr) * r * mag_u) + H.EPS_RED * (P[t] - p_).abs(), f"lamb tensor {t} p")
    nblk = opt.tables[0].numel()
    hold("lamb_step", [(Case(f"{len(shapes)} tensors, {nblk} blocks", lib().cmu_lamb_ws_bytes(nblk, len(shapes)), outs, ins, DEV, "f32", nblk, False), run, check)])


# ------------------------------------------------------------------------------------------------------------------------------------
# input pipeline: resizes (row tables / the horizontally resized intermediate), the finetuning augmentation's resize, Genesis' Bezier tables
# ------------------------------------------------------------------------------------------------------------------------------------
def test_resizes(ops):
    """Bit-exact against oracle/augment.py (test_gpu_augment.py).  The workspaces are per element (B x Hs x Wo intermediate; Ho + Wo table
    entries): the grid caps do not enter the sizes.  Float and 8-bit, whole images and crop windows + flip, up- and down-sampling, one-pixel
    sources and outputs."""
    from oracle import augment as OA
    rng = np.random.RandomState(1)
    f_cases, u_cases, n_cases = [], [], []
    for shape, out, boxed in (((3, 100, 77), (64, 48), True), ((2, 51, 77), (96, 80), False), ((2, 1, 1), (8, 8), False), ((1, 37, 29), (1, 1), False)):
        B, Hs, Ws = shape
        a = (rng.standard_normal(shape) * 3 + 0.5).astype(np.float32)
        a8 = rng.randint(0, 256, shape).astype(np.uint8)
        a8[0] = np.where(rng.rand(*shape[1:]) < 0.5, 0, 255)
        m = rng.randint(0, 3, shape).astype(np.uint8)
        boxes = flips = None
        if boxed:
            boxes = np.array([[0, 0, Ws, Hs], [10, 20, 40, 57], [Ws - 1, Hs - 1, 1, 1]], np.int32)
            flips = np.array([0, 1, 1], np.uint8)
        for src, name, fn, cases, size in ((a, "cmu_resize_bicubic", OA.resize_bicubic, f_cases, lib().cmu_resize_bicubic_ws_bytes),
                                           (a8, "cmu_resize_bicubic_u8", OA.resize_bicubic_u8, u_cases, lib().cmu_resize_bicubic_u8_ws_bytes)):
            if boxed and src.dtype == np.float32:
                ref = OA.resize_bicubic_crop(src, boxes, flips, *out)
            elif boxed:
                ref = np.stack([(lambda r, fl: r[:, ::-1] if fl else r)(fn(src[b, y0:y0 + h, x0:x0 + w], *out), flips[b]) for b, (x0, y0, w, h) in enumerate(boxes)])
            else:
                ref = np.stack([fn(x, *out) for x in src])
            ins = {"src": torch.from_numpy(src).to(DEV)}
            if boxed:
                ins.update(boxes=torch.from_numpy(boxes).to(DEV), flip=torch.from_numpy(flips).to(DEV))
            tdt = torch.float32 if src.dtype == np.float32 else U8
            cases.append((Case(f"{shape} -> {out}{' boxes + flip' if boxed else ''}", size(B, Hs, Ws, *out), {"out": Out((B,) + out, tdt) if tdt == torch.float32 else
                                Out((B,) + out, tdt, 0xA7, marks_unwritten=False, why="every byte value is a legitimate pixel: the bit-exact reference carries completeness")},
                               ins, DEV, "f32" if tdt == torch.float32 else "u8", -(-B * Hs * out[1] // 256), False),
                          lambda ws, o, ins=ins, name=name, a_=(B, Hs, Ws), out=out: call(name, ops._p(ins["src"]), *a_, ops._p(ins.get("boxes")), ops._p(ins.get("flip")),
                                                                                         ops._p(o["out"]), *out, ops._p(ws), ops._stream()),
                          lambda o, ref=np.ascontiguousarray(ref): _same_bytes(o["out"], ref)))
        ins = {"src": torch.from_numpy(m).to(DEV)}
        n_cases.append((Case(f"{shape} -> {out}", lib().cmu_resize_nearest_u8_ws_bytes(*out), {"out": Out((B,) + out, U8, 0xFF)}, ins, DEV, "u8", -(-B * out[0] * out[1] // 256), False),
                        lambda ws, o, ins=ins, a_=(B, Hs, Ws), out=out: call("cmu_resize_nearest_u8", ops._p(ins["src"]), *a_, ops._p(o["out"]), *out, ops._p(ws), ops._stream()),
                        lambda o, ref=np.stack([OA.resize_nearest(x, *out) for x in m]): _same_bytes(o["out"], ref)))
    hold("resize_bicubic", f_cases)
    hold("resize_bicubic_u8", u_cases)
    hold("resize_nearest_u8", n_cases)


def _same_bytes(got, ref):
    got, ref = got.cpu().numpy(), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), f"{int((got != ref).sum())} elements differ"


def test_ftaug_resize_onehot(ops):
    """The finetuning augmentation's fused resize + one-hot (its tables and the horizontally resized intermediate live in the workspace):
    bit for bit the restatement's crop (tests/ft_augment_restate.py, exact transforms only: crop + flips / rot90) followed by the oracle's
    bicubic / NEAREST resize and one-hot, as test_gpu_ft_augment.py::test_full_chain_matches_restatement_then_segmentation_batch has it."""
    import ft_augment_restate as FR
    from cmunet_amd import ft_augment as FA
    from oracle import augment as OA
    from test_gpu_ft_augment import _data, _recs
    cases = []
    for B, size, oneof in ((3, 128, 2), (2, 97, 0), (1, 64, 1)):          # (the kernel takes at most 32 taps: 475 -> 62 or more)
        aug = FA.DeviceTrainingAugmentation(FA.FinetuneAugmentConfig(clip_float=False), size=size, seed=5)
        S = int(aug.config.crop)
        img, mask = _data(B, seed=oneof)
        recs = _recs(B, FR.OP_ONEOF, seed=oneof + 2, oneof=oneof, rot_k=[1, 2, 3][:B])
        noise = np.random.RandomState(4).standard_normal((2, B, S, S))
        imd, mkd = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
        nd = torch.from_numpy(noise).to(DEV)
        rd = aug._records(recs, B, img.shape[1], img.shape[2], S, imd.device)
        Pd = aug._photometric(imd, rd, nd, B, img.shape[1], img.shape[2], S)
        ra, rm = FR.augment_batch(img, mask, recs, noise, S, False)
        ri = np.stack([OA.resize_bicubic(x, size, size) for x in ra])
        lab = np.stack([OA.resize_nearest(x, size, size) for x in rm])
        ro = np.stack([(lab == v) for v in (0, 1)], 1).astype(np.float64)
        ins = {"P": Pd, "masks": mkd, "recs": rd, "noise": nd}

        def run(ws, o, ins=ins, aug=aug, a=(B, img.shape[1], img.shape[2]), S=S, size=size):
            call("cmu_ftaug_resize_onehot", ops._p(ins["P"]), ops._p(ins["masks"]), *a, ops._p(ins["recs"]), ops._p(ins["noise"]), aug.seed, aug.last_offset, 0,
                 aug._cls, 2, ops._p(o["img"]), ops._p(o["onehot"]), S, size, ops._p(ws), ops._stream())

        def check(o, ri=ri, ro=ro):
            _same_bytes(o["img"], ri)
            _same_bytes(o["onehot"], ro)
        cases.append((Case(f"{B} crops of {S} -> {size}", lib().cmu_ftaug_resize_ws_bytes(B, S, size), {"img": Out((B, size, size)), "onehot": Out((B, 2, size, size), F64)},
                           ins, DEV, "f32", 0, False), run, check))
    hold("ftaug_resize_onehot", cases)


def test_genesis_bezier(ops):
    """cmu_genesis_bezier fills the workspace with the batch's Bezier tables and cmu_genesis_intensity_paint reads them: the pair is held
    together, against the restatement of the batch's own records (test_gpu_genesis.py::test_device_batch_equals_restatement_of_its_records:
    bit for bit without the nonlinear transform, 2 ulp with it, painted pixels in [0, 1]).  x is transformed in place (run() loads the
    gather / shuffle output first); the error word is OR-ed into.  The last case is a batch of a constant 0.75 image and an image of two
    neighbouring float32 values with nonlinear_rate = 1: their sampled cubics are rounding noise with far more than 16 monotone runs, so
    the tables go through the kernel's general sort, which works in place in the workspace."""
    import genesis_restate as GR
    from cmunet_amd import genesis as G
    from test_gpu_genesis import _cfg, ulps
    cases = []
    for B, H, N, seed, flat in ((16, 64, 32, 9, False), (3, 48, 5, 2, False), (1, 42, 1, 4, False), (2, 42, 2, 6, True)):
        src = np.random.RandomState(1).standard_normal((N, H, H)).astype(np.float32)
        if flat:
            src[0] = 0.75
            src[1] = np.where(src[1] > 0, np.nextafter(np.float32(1), np.float32(2)), np.float32(1))
        gen_ = G.GenesisPairGenerator(src, B, _cfg(rates={"nonlinear_rate": 1.0} if flat else None), seed=seed, offset=3, device=DEV)
        p = ops._p
        call("cmu_genesis_sample", p(gen_.recs), p(gen_.blocks), p(gen_.perms), gen_.N, B, H, H, 0, *(float(v) for v in (gen_.config.flip_rate, gen_.config.local_rate,
             gen_.config.nonlinear_rate, gen_.config.paint_rate, gen_.config.inpaint_rate)), gen_.seed, gen_.offset, ops._stream())
        x0, y0 = torch.empty(B, H, H, device=DEV), torch.empty(B, H, H, device=DEV)
        call("cmu_genesis_gather_shuffle", p(gen_.src), p(gen_.recs), p(gen_.blocks), p(gen_.perms), p(x0), p(y0), p(gen_.minmax), B, H, H, ops._stream())
        torch.cuda.synchronize()
        rec = gen_.records()
        rx, _ = GR.apply_genesis(src, rec["recs"], rec["blocks"], rec["perms"], None)
        ins = {"recs": gen_.recs, "minmax": gen_.minmax, "x0": x0}

        def run(ws, o, ins=ins, a=(B, H, H), gen_=gen_):
            o["x"].copy_(ins["x0"])
            call("cmu_genesis_bezier", p(ins["recs"]), p(ins["minmax"]), *a, p(ws), p(o["err"]), ops._stream())
            call("cmu_genesis_intensity_paint", p(ins["recs"]), p(ws), None, gen_.seed, gen_.offset, p(o["x"]), *a, ops._stream())

        def check(o, rx=rx, rec=rec, B=B, flat=flat):
            assert not flat or all(int(f) & G.GF_NONLIN for f in rec["recs"]["flags"])
            x = o["x"].cpu().numpy()
            painted = np.isnan(rx)
            assert int(o["err"].item()) == 0 and ((x[painted] >= 0) & (x[painted] <= 1)).all()
            for b in range(B):
                keep = ~painted[b]
                if int(rec["recs"]["flags"][b]) & G.GF_NONLIN:
                    assert ulps(x[b][keep], rx[b][keep]).max() <= 2, b
                else:
                    assert (x[b][keep].view(np.int32) == rx[b][keep].view(np.int32)).all(), b
        cases.append((Case(f"{B}x{H}x{H}" + (" near-constant" if flat else ""), lib().cmu_genesis_bezier_ws_bytes(B),
                           {"x": Out((B, H, H), prefill=0.0, accumulates=True, why="transformed in place; run() loads the gather / shuffle output first"),
                            "err": Out((1,), I32, prefill=0, accumulates=True, why="the error word is OR-ed into")}, ins, DEV, "f32", 2 * B, False), run, check))
    hold("genesis_bezier + intensity_paint", cases)


# ------------------------------------------------------------------------------------------------------------------------------------
# geometry metrics and connected components
# ------------------------------------------------------------------------------------------------------------------------------------
def geometry_masks(H, W, seed):
    """B = 3 masks: an empty image, a full one and random blobs."""
    rng = np.random.RandomState(seed)
    blobs = rng.rand(H, W) < 0.45
    return np.stack([np.zeros((H, W), bool), np.ones((H, W), bool), blobs]).astype(np.uint8)


def test_contour_points(ops):
    """Weight maps and counts exact against tests/geometry_lattice.py.  Three images per call (empty, full, random) at 5 x 7, 33 x 40 and 64 x 64,
    and the 1 x 1 mask, whose workspace size is 0: the call gets a 1-byte payload, as metrics._contour_points passes."""
    import geometry_lattice as L
    cases = []
    for H, W in ((64, 64), (33, 40), (5, 7), (1, 1)):
        m = geometry_masks(H, W, H + W)
        B = m.shape[0]
        wref = np.stack([L.lattice_weights(x) for x in m])
        cref = np.array([L.counts(x) for x in m], np.int32)
        ins = {"mask": torch.from_numpy(m).to(DEV)}

        def check(o, wref=wref, cref=cref):
            assert np.array_equal(o["wmap"].cpu().numpy(), wref) and np.array_equal(o["counts"].cpu().numpy(), cref)
        NS = ((2 * H - 1) * (2 * W - 1) - 1) // 2
        cases.append((Case(f"{B}x{H}x{W}", lib().cmu_contour_points_ws_bytes(B, H, W), {"wmap": Out((B, 2 * H - 1, 2 * W - 1), U8, 0xFF), "counts": Out((B, 2), I32, -1)},
                           ins, DEV, "u8", min(-(-NS // 256), 1024) * B, False, min_ws=1),
                      lambda ws, o, ins=ins, a=(B, H, W): call("cmu_contour_points", ops._p(ins["mask"]), ops._p(o["wmap"]), ops._p(o["counts"]), *a, ops._p(ws), ops._stream()),
                      check))
    hold("contour_points", cases)


def test_lattice_nearest(ops):
    """Both query modes: lattice queries with weights (the Hausdorff distance: every contour point of b to the contour of a) and pixel queries
    (the artery radius: skeleton pixels to the contour).  sum w and the counts exact, distances to 1e-9 relative as ``_close`` of
    test_gpu_geometry_metrics.py has it; an image without seeds or without queries gives four zeros."""
    import geometry_lattice as L
    from test_gpu_geometry_metrics import _close
    cases = []
    for H, W in ((64, 64), (33, 40), (5, 7), (1, 1)):
        a, b = geometry_masks(H, W, H + W), geometry_masks(H, W, H * W + 1)[[2, 1, 0]]          # pairs: empty / random, shifted random / random, random / empty
        b[1] = a[2] if H > 1 else b[1]
        a[1] = np.roll(a[2], 2, 1) if H > 1 else a[1]
        B = a.shape[0]
        wa, wb = np.stack([L.lattice_weights(x) for x in a]), np.stack([L.lattice_weights(x) for x in b])
        for qmode, seeds, queries in ((0, wa, wb), (1, wa, b)):
            ref = np.zeros((B, 4))
            for i in range(B):
                if qmode == 0:
                    qi, qj = np.nonzero(queries[i])
                    wq = queries[i][qi, qj].astype(np.float64)
                else:
                    qi, qj = np.nonzero(queries[i])
                    wq, qi, qj = np.ones(len(qi)), 2 * qi, 2 * qj
                if len(qi) and seeds[i].any():
                    d = np.sqrt(L.sq_dist_at(seeds[i] > 0, qi, qj).astype(np.float64)) / 2
                    ref[i] = ((d * wq).sum(), wq.sum(), d.max(), d.min())
            ins = {"seeds": torch.from_numpy(seeds).to(DEV), "queries": torch.from_numpy(np.ascontiguousarray(queries)).to(DEV)}

            def check(o, ref=ref, B=B):
                got = o["out"].cpu().numpy()
                for i in range(B):
                    assert got[i, 1] == ref[i, 1] and all(_close(g, r) for g, r in zip(got[i], ref[i])), (i, got[i], ref[i])
            cases.append((Case(f"{B}x{H}x{W} {'pixel' if qmode else 'lattice'} queries", lib().cmu_lattice_nearest_ws_bytes(B, H, W), {"out": Out((B, 4), F64)}, ins, DEV, "f64",
                               -(-B * (2 * H - 1) // 64), False),
                          lambda ws, o, ins=ins, qmode=qmode, a_=(B, H, W): call("cmu_lattice_nearest", ops._p(ins["seeds"]), ops._p(ins["queries"]), qmode, ops._p(o["out"]), *a_,
                                                                                 ops._p(ws), ops._stream()), check))
    hold("lattice_nearest", cases)


def test_label_components(ops):
    """Labels and counts exact against tests/components_ref.py (a flood fill), 4- and 8-connectivity; three images per call (empty, full, random)
    at 64 x 64, 33 x 40, 5 x 7 and 1 x 1.  The kernel's union-find lives in the workspace."""
    import components_ref as CR
    cases = []
    for H, W in ((64, 64), (33, 40), (5, 7), (1, 1)):
        m = geometry_masks(H, W, 7 * H + W)
        B = m.shape[0]
        for conn in (4, 8):
            lab, cnt = CR.label_batch(m, conn)
            ins = {"src": torch.from_numpy(m).to(DEV)}

            def check(o, lab=lab, cnt=cnt):
                assert np.array_equal(o["counts"].cpu().numpy(), cnt), (o["counts"].tolist(), cnt.tolist())
                assert np.array_equal(o["labels"].cpu().numpy(), lab)
            cases.append((Case(f"{B}x{H}x{W} connectivity {conn}", lib().cmu_label_components_ws_bytes(B, H, W), {"labels": Out((B, H, W), I32, -1), "counts": Out((B,), I32, -1)},
                               ins, DEV, "i32", 0, False),
                          lambda ws, o, ins=ins, conn=conn, a=(B, H, W): call("cmu_label_components", ops._p(ins["src"]), -1, conn, ops._p(o["labels"]), ops._p(o["counts"]), *a,
                                                                             ops._p(ws), ops._stream()), check))
    hold("label_components", cases)


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end: the engine's grow-only scratch buffers, as production has them
# ------------------------------------------------------------------------------------------------------------------------------------
def seeded_step_is_bit_equal(make_model, step, what):
    """``step(model) -> (loss, {name: grad})``.  Two fresh models from the same state give the same bits (the step is reproducible); a third
    whose engine starts with every scratch buffer the fresh run ended with -- twice the size, every byte 0xFF -- gives them again.  The
    only test here that compares the code with itself: it is the production condition, the entries above carry the references."""
    runs = []
    for seeded in (False, False, True):
        model = make_model()
        eng = model._engine(torch.device("cuda", torch.cuda.current_device()))
        if seeded:
            assert runs[0][2], f"{what}: the fresh run used no scratch buffer"
            for k, nbytes in runs[0][2].items():
                eng.scratch.bufs[k] = torch.full((2 * nbytes,), 0xFF, dtype=U8, device=eng.device)
        loss, grads = step(model)
        torch.cuda.synchronize()
        assert model._engine(eng.device) is eng, f"{what}: the step ran on another engine than the seeded one"
        runs.append((MC.bits(loss), {k: MC.bits(g) for k, g in grads.items()}, {k: b.numel() for k, b in eng.scratch.bufs.items()}))
        assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(g).all()) for g in grads.values()), f"{what}: non-finite loss / gradient"
    for i, name in ((1, "a second fresh run"), (2, "0xFF-seeded scratch buffers of twice the size")):
        assert MC.same_bits(runs[i][0], runs[0][0]), f"{what}: the loss differs under {name}"
        for k in runs[0][1]:
            assert MC.same_bits(runs[i][1][k], runs[0][1][k]), f"{what}: the gradient of {k} differs under {name}"
    print(f"[memcontract] {what}: loss and {len(runs[0][1])} gradients bit-equal; scratch keys {sorted(runs[0][2])}")
    return runs[0][2]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_unet_step_on_seeded_scratch(ops, golden_dir, dt):
    import torch.nn.functional as F
    from cmunet_amd import model as M
    from test_gpu_model import load_fx, load_sd
    fx = load_fx(golden_dir, "unet_small")

    def make():
        m = M.UNet(base_ch=16, depth=3, dtype=dt).cuda().train()
        load_sd(m, fx)
        return m

    def step(m):
        loss = F.cross_entropy(m(fx["x"].cuda()), fx["y1h"].cuda())
        loss.backward()
        return loss.detach(), {k: p.grad for k, p in m.named_parameters()}
    keys = seeded_step_is_bit_equal(make, step, f"UNet training step {dt}")
    assert {"bnfin", "wg"} <= set(keys), keys


def test_spark_step_on_seeded_scratch(ops, golden_dir):
    from test_gpu_pretrain import _spark_from_fixture
    d = np.load(f"{golden_dir}/spark_unet.npz")
    x, active = torch.from_numpy(d["x"]).cuda(), torch.from_numpy(d["active"]).bool().cuda()

    def step(m):
        loss = m(x, active_b1ff=active)
        loss.backward()
        return loss.detach(), {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    keys = seeded_step_is_bit_equal(lambda: _spark_from_fixture(d, "bf16", "cuda"), step, "SparK step bf16")
    assert {"bnfin", "wg", "sploss"} <= set(keys), keys
