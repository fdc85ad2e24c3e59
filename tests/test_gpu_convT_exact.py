"""The ConvTranspose 2x2 / stride 2 GEMMs (conv_gemm_s_kernel, conv_gemm_kernel and the MODE_CONVT_* forms of
conv_igemm_kernel) pinned bit for bit: ``cmu_convT2x2_fwd`` with an integer bias, ``cmu_convT2x2_dgrad`` and ``cmu_convT2x2_dgrad_bn``
against the exact float64 references of conv_exact_ref.py, on integer operands, on one-hot weights against float activations (the four
sub-pixel positions) and on impulses.  Every case asserts the kernel tag and, through its ``form``, the number of 128-byte K steps the restated
rule of conv_gemm.inc gives (the shallow form takes at most four; the data gradient's steps must stay inside one sub-pixel position:
``(K / 4) % KSC == 0``).  ``torch.equal`` on the bits is the only comparison."""
import pytest
import torch

import conv_exact_gpu as G
import conv_exact_ref as R

pytestmark = pytest.mark.gpu

FWD = [(c, dt) for c in R.CASES if c["fam"] == "ctf" for dt in c["dts"]]
DG = [(c, dt) for c in R.CASES if c["fam"] in ("ctdg", "ctdgbn") for dt in c["dts"]]


def ident(v):
    return f"{v['id']}" if isinstance(v, dict) else str(v)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as O
    return O


def launch_fwd(ops, case, dt, x, w, bias, tf):
    B, H, W, K, N = case["shape"]
    xa = G.in_act(ops, x, dt, case["xs"], tf)
    oa = G.out_act(ops, B, 2 * H, 2 * W, N, dt, case["ys"])
    with G.knobs(ops, case):
        ops.convT2x2_fwd(xa, ops.pack_convT2x2(w.cuda().contiguous(), dt, 0), bias.float().cuda(), oa)
        torch.cuda.synchronize()
        kernel = G.last_kernel()
    rule, form = G.convT_rule(case, dt, False, tf is not None, G.library_knobs())
    G.assert_form(case, dt, rule, form)
    assert kernel == case["kernel"], f"{kernel} ran"
    return oa


def launch_dgrad(ops, case, dt, dout, w_layer, yraw=None, bn=None):
    B, H, W, K, N = case["shape"]
    da = G.in_act(ops, dout, dt, case["xs"])
    xa = G.out_act(ops, B, H, W, N, dt, case["ys"])
    slab = None
    with G.knobs(ops, case):
        wp = ops.pack_convT2x2(w_layer.cuda().contiguous(), dt, 1)
        if case["fam"] == "ctdg":
            ops.convT2x2_dgrad(da, wp, xa)
        else:
            slab = G.nan_stats(ops, B, H, W, N)
            ya = G.in_act(ops, yraw, dt, 8, (bn[0], bn[1], 0))
            ops.convT2x2_dgrad_bn(da, wp, xa, ya, bn[2].cuda(), bn[3].cuda(), slab)
        torch.cuda.synchronize()
        kernel = G.last_kernel()
    rule, form = G.convT_rule(case, dt, True, False, G.library_knobs())
    G.assert_form(case, dt, rule, form)
    assert kernel == case["kernel"], f"{kernel} ran"
    return xa, slab


@pytest.mark.parametrize("case,dt", FWD, ids=ident)
def test_forward_integer_operands_and_bias(ops, case, dt):
    o, ref = R.reference_of(case, dt, "cuda")
    oa = launch_fwd(ops, case, dt, o["x"], o["w"], o["bias"], o["tf"])
    G.check_out(oa, ref["stored"])


@pytest.mark.parametrize("case,dt", FWD, ids=ident)
def test_forward_one_hot_weight_and_impulses(ops, case, dt):
    B, H, W, K, N = case["shape"]
    o, _ = R.reference_of(case, dt, "cuda")
    x = R.stored(R.float_operands((B, H, W, K), R.case_seed(case)).double(), dt).cuda()
    tf = None if case["tf"] is None else (torch.ones(K), torch.zeros(K), K)
    cis, cos = G.corner_channels(K, 128 // G.ES[dt]), G.corner_channels(N, 64)
    for ij in range(4):
        i, j = divmod(ij, 2)
        w = torch.zeros(K, N, 2, 2)
        want = torch.zeros(B, 2 * H, 2 * W, N, dtype=x.dtype, device="cuda")
        for q, co in enumerate(cos):
            ci = cis[(ij + q) % len(cis)]
            w[ci, co, i, j] = 1.0
            want[:, i::2, j::2, co] = x[..., ci]
        oa = launch_fwd(ops, case, dt, x, w, torch.zeros(N), tf)
        G.check_out(oa, want)
    imp = torch.zeros(B, H, W, K, device="cuda")
    for q, (b, h, w_) in enumerate(G.seam_pixels(B, H, W)):
        imp[b, h, w_, cis[q % len(cis)]] = 1.0
    ref = R.convT2x2_exact(imp, o["w"], o["bias"], o["tf"], dt)
    R.assert_exact_caps(ref, dt)
    G.check_out(launch_fwd(ops, case, dt, imp, o["w"], o["bias"], o["tf"]), ref["stored"])


@pytest.mark.parametrize("case,dt", DG, ids=ident)
def test_data_gradient_integer_operands(ops, case, dt):
    o, ref = R.reference_of(case, dt, "cuda")
    xa, slab = launch_dgrad(ops, case, dt, o["dout"], o["w"], o.get("yraw"), o.get("bn"))
    G.check_out(xa, ref["stored"])
    if case["fam"] == "ctdgbn":
        G.check_slab(slab, ref["bstats"], "BatchNorm-backward sums on dX as stored")


@pytest.mark.parametrize("case,dt", DG, ids=ident)
def test_data_gradient_one_hot_weight_and_impulses(ops, case, dt):
    B, H, W, K, N = case["shape"]
    o, _ = R.reference_of(case, dt, "cuda")
    dout = R.stored(R.float_operands((B, 2 * H, 2 * W, K), R.case_seed(case)).double(), dt).cuda()
    cks, cns = G.corner_channels(K, 128 // G.ES[dt]), G.corner_channels(N, 64)
    for ij in range(4):
        i, j = divmod(ij, 2)
        w = torch.zeros(N, K, 2, 2)
        want = torch.zeros(B, H, W, N, dtype=dout.dtype, device="cuda")
        for q, n in enumerate(cns):
            k = cks[(ij + q) % len(cks)]
            w[n, k, i, j] = 1.0
            want[..., n] = dout[:, i::2, j::2, k]
        xa, _ = launch_dgrad(ops, case, dt, dout, w, o.get("yraw"), o.get("bn"))
        G.check_out(xa, want)
    imp = torch.zeros(B, 2 * H, 2 * W, K, device="cuda")
    for q, (b, h, w_) in enumerate(G.seam_pixels(B, 2 * H, 2 * W)):
        imp[b, h, w_, cks[q % len(cks)]] = 1.0
    if case["fam"] == "ctdg":
        ref = R.convT2x2_dgrad_exact(imp, o["w"], dt)
    else:
        ref = R.convT2x2_dgrad_bn_exact(imp, o["w"], o["yraw"], *o["bn"], dt=dt)
    R.assert_exact_caps(ref, dt)
    xa, slab = launch_dgrad(ops, case, dt, imp, o["w"], o.get("yraw"), o.get("bn"))
    G.check_out(xa, ref["stored"])
    if case["fam"] == "ctdgbn":
        G.check_slab(slab, ref["bstats"], "BatchNorm-backward sums on dX as stored")


def test_the_cases_cover_the_three_convT_kernels_and_the_step_rules():
    """Built from CASES: each kernel in the forward and in the data gradient; the shallow form at one and at four K steps and NOT at
    five; a data gradient whose 128-byte step would straddle two sub-pixel positions stays on the first kernel."""
    seen = {(c["kernel"], c["fam"] != "ctf") for c in R.CASES if c["fam"] in ("ctf", "ctdg", "ctdgbn")}
    assert seen == {(k, g) for k in ("conv_gemm_s_kernel", "conv_gemm_kernel", "conv_igemm_kernel") for g in (False, True)}
    steps = {}
    for c in R.CASES:
        if c["fam"] == "ctf" and "f16" in c["dts"]:
            kernel, form = G.convT_rule(c, "f16", False, c["tf"] is not None)
            steps.setdefault(kernel, set()).add(form["steps"])
    assert {1, 4} <= steps["conv_gemm_s_kernel"] and 5 in steps["conv_gemm_kernel"]
    straddle = [c for c in R.CASES if c["fam"] == "ctdg" and c["form"].get("inside") is False and c["shape"][4] % 256 == 0]
    assert straddle and all(c["kernel"] == "conv_igemm_kernel" and c["form"]["steps"] <= 4 for c in straddle)
