"""The 3x3 implicit-GEMM kernels (conv_igemm_kernel, conv_igemm3_kernel, conv_igemm3p_kernel,
conv_igemm5_kernel) pinned bit for bit: ``cmu_conv3x3_fwd`` and ``cmu_conv3x3_dgrad_bn`` (the flipped pack) against the exact float64
references of conv_exact_ref.py.  Three kinds of data per case of ``CASES``:

  * integer operands: every fp32 sum is an integer below 2**24 (asserted from the reference alone in test_cpu_conv_exact_ref.py), so
    the output as stored, the statistics slab of the fp32 accumulators and the BatchNorm-backward sums on dX as stored are exact;
  * a one-hot weight against random float activations: the output channel is the shifted input channel, every other channel 0;
  * impulses at the first pixel, the last pixel and both sides of every tile seam, against integer weights.

Every case forces its dispatch, asserts the kernel tag of the launch and the template form the restated launcher rule gives for the
device's CU count.  ``torch.equal`` on the bits is the only comparison."""
import pytest
import torch

import conv_exact_gpu as G
import conv_exact_ref as R

pytestmark = pytest.mark.gpu

FWD = [(c, dt) for c in R.CASES if c["fam"] == "c3f" for dt in c["dts"]]
DG = [(c, dt) for c in R.CASES if c["fam"] == "c3dg" for dt in c["dts"]]


def ident(v):
    return f"{v['id']}" if isinstance(v, dict) else str(v)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as O
    return O


def launch_fwd(ops, case, dt, x, w, tf, want_stats):
    B, H, W, K, N = case["shape"]
    xa = G.in_act(ops, x, dt, case["xs"], tf)
    ya = G.out_act(ops, B, H, W, N, dt, case["ys"])
    st = G.nan_stats(ops, B, H, W, N) if want_stats else None
    with G.knobs(ops, case):
        ops.conv3x3_fwd(xa, ops.pack_conv3x3(w.cuda().contiguous(), dt), ya, st)
        torch.cuda.synchronize()
        kernel = G.last_kernel()
    rule, form = G.conv3_rule(case, dt, G.cu_count(), tf is not None, False, G.library_knobs())
    G.assert_form(case, dt, rule, form)
    assert kernel == case["kernel"], f"{kernel} ran"
    return ya, st


def launch_dgrad(ops, case, dt, dy, w_layer, yraw, bn):
    B, H, W, K, N = case["shape"]
    da = G.in_act(ops, dy, dt, case["xs"])
    xa = G.out_act(ops, B, H, W, N, dt, case["ys"])
    ya = G.in_act(ops, yraw, dt, 8, (bn[0], bn[1], 0))
    slab = G.nan_stats(ops, B, H, W, N)
    with G.knobs(ops, case):
        ops.conv3x3_dgrad_bn(da, ops.pack_conv3x3(w_layer.cuda().contiguous(), dt, transpose_flip=True), xa, ya, bn[2].cuda(), bn[3].cuda(), slab)
        torch.cuda.synchronize()
        kernel = G.last_kernel()
    rule, form = G.conv3_rule(case, dt, G.cu_count(), False, True, G.library_knobs())
    G.assert_form(case, dt, rule, form)
    assert kernel == case["kernel"], f"{kernel} ran"
    return xa, slab


@pytest.mark.parametrize("case,dt", FWD, ids=ident)
def test_forward_integer_operands(ops, case, dt):
    o, ref = R.reference_of(case, dt, "cuda")
    ya, st = launch_fwd(ops, case, dt, o["x"], o["w"], o["tf"], case["stats"])
    G.check_out(ya, ref["stored"])
    if case["stats"]:
        G.check_slab(st, ref["stats"], "statistics of the fp32 accumulators")


@pytest.mark.parametrize("case,dt", FWD, ids=ident)
def test_forward_one_hot_weight_moves_float_activations(ops, case, dt):
    """Tap by tap: four one-hot columns per launch (the corner channels of the first and last N block), each fed by a corner channel of the
    first and last K slice.  An identity transform (scale 1, shift 0, no channel activated) keeps the case's template form."""
    B, H, W, K, N = case["shape"]
    x = R.stored(R.float_operands((B, H, W, K), R.case_seed(case)).double(), dt).cuda()
    tf = None if case["tf"] is None else (torch.ones(K), torch.zeros(K), K)
    cis, cos = G.corner_channels(K, 64 // G.ES[dt]), G.corner_channels(N, 64)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        w = torch.zeros(N, K, 3, 3)
        want = torch.zeros(B, H, W, N, dtype=x.dtype, device="cuda")
        for j, co in enumerate(cos):
            ci = cis[(tap + j) % len(cis)]
            w[co, ci, ky, kx] = 1.0
            want[..., co] = R.shift2d(x[..., ci:ci + 1], ky - 1, kx - 1)[..., 0]
        ya, _ = launch_fwd(ops, case, dt, x, w, tf, False)
        G.check_out(ya, want)


@pytest.mark.parametrize("case,dt", FWD, ids=ident)
def test_forward_impulses_at_the_tile_seams(ops, case, dt):
    B, H, W, K, N = case["shape"]
    o, _ = R.reference_of(case, dt, "cuda")
    x = torch.zeros(B, H, W, K, device="cuda")
    cis = G.corner_channels(K, 64 // G.ES[dt])
    for i, (b, h, w_) in enumerate(G.seam_pixels(B, H, W)):
        x[b, h, w_, cis[i % len(cis)]] = 1.0
    ref = R.conv3x3_exact(x, o["w"], o["tf"], dt)
    R.assert_exact_caps(ref, dt, case["stats"])
    ya, st = launch_fwd(ops, case, dt, x, o["w"], o["tf"], case["stats"])
    G.check_out(ya, ref["stored"])
    if case["stats"]:
        G.check_slab(st, ref["stats"], "statistics of the fp32 accumulators")


@pytest.mark.parametrize("case,dt", DG, ids=ident)
def test_data_gradient_integer_operands_and_bn_backward_sums(ops, case, dt):
    o, ref = R.reference_of(case, dt, "cuda")
    xa, slab = launch_dgrad(ops, case, dt, o["dy"], o["w"], o["yraw"], o["bn"])
    G.check_out(xa, ref["stored"])
    G.check_slab(slab, ref["bstats"], "BatchNorm-backward sums on dX as stored")


@pytest.mark.parametrize("case,dt", DG, ids=ident)
def test_data_gradient_one_hot_weight_and_impulses(ops, case, dt):
    """The flipped pack: a one-hot LAYER weight (k, n, ky, kx) moves dY's channel k to dX's channel n shifted the OTHER way; then impulses in
    dY against the integer weight, with the sums."""
    B, H, W, K, N = case["shape"]
    o, _ = R.reference_of(case, dt, "cuda")
    dy = R.stored(R.float_operands((B, H, W, K), R.case_seed(case)).double(), dt).cuda()
    cks, cns = G.corner_channels(K, 64 // G.ES[dt]), G.corner_channels(N, 64)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        w = torch.zeros(K, N, 3, 3)
        want = torch.zeros(B, H, W, N, dtype=dy.dtype, device="cuda")
        for j, n in enumerate(cns):
            k = cks[(tap + j) % len(cks)]
            w[k, n, ky, kx] = 1.0
            want[..., n] = R.shift2d(dy[..., k:k + 1], 1 - ky, 1 - kx)[..., 0]
        xa, _ = launch_dgrad(ops, case, dt, dy, w, o["yraw"], o["bn"])
        G.check_out(xa, want)
    imp = torch.zeros(B, H, W, K, device="cuda")
    for i, (b, h, w_) in enumerate(G.seam_pixels(B, H, W)):
        imp[b, h, w_, cks[i % len(cks)]] = 1.0
    ref = R.conv3x3_dgrad_bn_exact(imp, o["w"], o["yraw"], *o["bn"], dt=dt)
    R.assert_exact_caps(ref, dt)
    xa, slab = launch_dgrad(ops, case, dt, imp, o["w"], o["yraw"], o["bn"])
    G.check_out(xa, ref["stored"])
    G.check_slab(slab, ref["bstats"], "BatchNorm-backward sums on dX as stored")


def test_the_cases_cover_every_form_of_the_3x3_kernels():
    """Built from CASES: the kernels and the template forms this file pins (NB 64 / 128, 16- / 32-pixel tiles, PART, WRES, TF, BST)."""
    seen = set()
    for c in R.CASES:
        if c["fam"] in ("c3f", "c3dg"):
            f = c["form"]
            seen.add((c["kernel"], f.get("NB"), f.get("TW"), f.get("PART"), f.get("WRES"), c["tf"] is not None, c["fam"] == "c3dg"))
    kernels = {s[0] for s in seen}
    assert kernels == {"conv_igemm_kernel", "conv_igemm3_kernel", "conv_igemm3p_kernel", "conv_igemm5_kernel"}
    for k, nbs, tws in (("conv_igemm3_kernel", {64, 128}, {16, 32}), ("conv_igemm3p_kernel", {64, 128}, {None})):
        assert {s[1] for s in seen if s[0] == k} == nbs and {s[2] for s in seen if s[0] == k} == tws
    p3 = [s for s in seen if s[0] == "conv_igemm3p_kernel"]
    assert {s[3] for s in p3} == {True, False} and {s[4] for s in p3} == {True, False}
    for k in kernels:
        assert {s[5] for s in seen if s[0] == k} == {True, False}, f"{k}: with and without a transform"
        assert {s[6] for s in seen if s[0] == k} == {True, False}, f"{k}: forward and data gradient"
