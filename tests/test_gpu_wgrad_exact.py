"""The weight-gradient kernels (conv_wgrad_kernel, conv_wgrad2_kernel plain and swapped, conv_wgrad2s_kernel,
conv_wgrad2f_kernel, conv_wgradT2_kernel with 128 and 256 X channels per workgroup, conv_wgradT2f_kernel) and their split-K reductions
pinned bit for bit: ``cmu_conv3x3_wgrad`` and ``cmu_convT2x2_wgrad`` (with ``dbias``) against the exact float64 references of
conv_exact_ref.py, on integer operands and on impulses in dY (dW is then the window of x around each pixel: one dropped pixel cannot hide).
The split-K geometry of every form (the rows of WG_FORMS, through wg_plan and wg_geometry) is restated in conv_exact_gpu.py and tied to the library
through the workspace size it reports (cmu_*_wgrad_ws_bytes is a function of the same split counts); CMU_WGRAD_BLOCKS / CMU_WGRAD_BLOCKS1
steer it to one split, equal splits, a short last split and more splits than tiles, and every case asserts the one it is named after.
``torch.equal`` on the bits is the only comparison."""
import pytest
import torch

import conv_exact_gpu as G
import conv_exact_ref as R

pytestmark = pytest.mark.gpu

W3 = [(c, dt) for c in R.CASES if c["fam"] == "wg3" for dt in c["dts"]]
WT = [(c, dt) for c in R.CASES if c["fam"] == "wgt" for dt in c["dts"]]


def ident(v):
    return f"{v['id']}" if isinstance(v, dict) else str(v)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as O
    return O


def workspace(nbytes):
    """The split-K slab, NaN-filled, with a NaN guard of 4 KiB behind it that must survive the launch."""
    assert nbytes > 0
    n = (int(nbytes) + 3) // 4
    ws = torch.full((n + 1024,), float("nan"), dtype=torch.float32, device="cuda")
    return ws


def launch_w3(ops, case, dt, x, dy, tf):
    from cmunet_amd import _lib
    B, H, W, Cin, Cout = case["shape"]
    xa = G.in_act(ops, x, dt, case["xs"], tf)
    da = G.in_act(ops, dy, dt, case["ys"])
    dW = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
    with G.knobs(ops, case):
        need = _lib.lib().cmu_conv3x3_wgrad_ws_bytes(B, H, W, Cin, Cout, ops.dt_code(dt))      # (the split count follows the knobs)
        ws = workspace(need)
        ops.conv3x3_wgrad(xa, da, dW, ws)
        torch.cuda.synchronize()
        kernel = G.last_kernel()
    rule, form, splits, ntiles = G.wgrad3_rule(case, dt, G.library_knobs())
    G.assert_form(case, dt, rule, form)
    assert kernel == case["kernel"], f"{kernel} ran"
    # the restated split count against the library's own geometry: its workspace size is the largest slab of the candidate kernels
    assert need == G.wgrad3_ws_bytes(case, dt, G.library_knobs()) and need >= G.slab_bytes(case, dt, kernel, splits)
    if kernel == "conv_wgrad_kernel":
        assert need == G.slab_bytes(case, dt, kernel, splits), "the first kernel is the only candidate: its slabs are the workspace"
    assert bool(torch.isnan(ws[(need + 3) // 4:]).all()), "a slab store landed behind the workspace"
    return dW


def launch_wt(ops, case, dt, x, dout, tf):
    from cmunet_amd import _lib
    B, H, W, Cin, Cout = case["shape"]
    xa = G.in_act(ops, x, dt, case["xs"], tf)
    da = G.in_act(ops, dout, dt, case["ys"])
    dW = torch.full((Cin, Cout, 2, 2), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    with G.knobs(ops, case):
        need = _lib.lib().cmu_convT2x2_wgrad_ws_bytes(B, H, W, Cin, Cout, ops.dt_code(dt))
        ws = workspace(need)
        ops.convT2x2_wgrad(xa, da, dW, db, ws)
        torch.cuda.synchronize()
        kernel = G.last_kernel()
    rule, form, splits, ntiles = G.wgradT_rule(case, dt, G.library_knobs())
    G.assert_form(case, dt, rule, form)
    assert kernel == case["kernel"], f"{kernel} ran"
    assert need == G.wgradT_ws_bytes(case, dt, G.library_knobs()) and need >= G.slab_bytes(case, dt, kernel, splits)
    assert bool(torch.isnan(ws[(need + 3) // 4:]).all()), "a slab store landed behind the workspace"
    return dW, db


def check_grad(got, want, what):
    want = want.to(torch.float32)
    if not G.same_bits(got, want):
        bad = (G.bits(got) != G.bits(want.to(got.device))).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} entries differ; first at {i}: got {float(got[i])}, exact {float(want[i])}")


def impulses(B, H, W, C):
    """One 1.0 per seam pixel, each in a channel of its own (corner channels first)."""
    imp = torch.zeros(B, H, W, C, device="cuda")
    chans = G.corner_channels(C, 64) + [c for c in range(1, C) if c not in G.corner_channels(C, 64)]
    for q, (b, h, w_) in enumerate(G.seam_pixels(B, H, W)):
        imp[b, h, w_, chans[q % len(chans)]] = 1.0
    return imp


@pytest.mark.parametrize("case,dt", W3, ids=ident)
def test_conv3x3_wgrad_integer_operands(ops, case, dt):
    o, ref = R.reference_of(case, dt, "cuda")
    check_grad(launch_w3(ops, case, dt, o["x"], o["dy"], o["tf"]), ref["dW"], "dW")


@pytest.mark.parametrize("case,dt", W3, ids=ident)
def test_conv3x3_wgrad_impulses_in_dY_give_the_windows_of_x(ops, case, dt):
    B, H, W, Cin, Cout = case["shape"]
    o, _ = R.reference_of(case, dt, "cuda")
    imp = impulses(B, H, W, Cout)
    ref = R.conv3x3_wgrad_exact(o["x"], imp, o["tf"])
    R.assert_exact_caps(ref)
    dW = launch_w3(ops, case, dt, o["x"], imp, o["tf"])
    check_grad(dW, ref["dW"], "dW")
    # the first impulse, spelled out: pixel (0, 0, 0), channel 0 of dY -> dW[0, :, ky, kx] = xa[0, ky - 1, kx - 1, :], zero outside
    xa = R.apply_transform(o["x"], o["tf"])
    for ky in range(3):
        for kx in range(3):
            inside = 0 <= ky - 1 < H and 0 <= kx - 1 < W
            want = xa[0, ky - 1, kx - 1].float() if inside else torch.zeros(Cin, device="cuda")
            if len(G.seam_pixels(B, H, W)) <= Cout:            # (channel 0 then carries this impulse alone)
                assert torch.equal(dW[0, :, ky, kx], want)


@pytest.mark.parametrize("case,dt", WT, ids=ident)
def test_convT2x2_wgrad_integer_operands_and_dbias(ops, case, dt):
    o, ref = R.reference_of(case, dt, "cuda")
    dW, db = launch_wt(ops, case, dt, o["x"], o["dout"], o["tf"])
    check_grad(dW, ref["dW"], "dW")
    check_grad(db, ref["dbias"], "dbias")


@pytest.mark.parametrize("case,dt", WT, ids=ident)
def test_convT2x2_wgrad_impulses_in_dOut(ops, case, dt):
    B, H, W, Cin, Cout = case["shape"]
    o, _ = R.reference_of(case, dt, "cuda")
    imp = impulses(B, 2 * H, 2 * W, Cout)
    ref = R.convT2x2_wgrad_exact(o["x"], imp, o["tf"])
    R.assert_exact_caps(ref)
    dW, db = launch_wt(ops, case, dt, o["x"], imp, o["tf"])
    check_grad(dW, ref["dW"], "dW")
    check_grad(db, ref["dbias"], "dbias")


def test_the_cases_cover_every_weight_gradient_kernel_and_split_geometry():
    """Built from CASES with the restated geometry: every kernel form, and per kernel family the split classes it can reach."""
    seen = {}
    for c in R.CASES:
        if c["fam"] in ("wg3", "wgt"):
            for dt in c["dts"]:
                kernel, form, splits, ntiles = (G.wgrad3_rule if c["fam"] == "wg3" else G.wgradT_rule)(c, dt)
                G.assert_form(c, dt, kernel, form)
                key = (c["fam"], kernel, form.get("SWAP"), form.get("NAI"), form.get("NXI"))
                seen.setdefault(key, set()).add(form["splits"])
    assert set(seen) == {("wg3", "conv_wgrad_kernel", None, None, None), ("wg3", "conv_wgrad2_kernel", False, None, None),
                         ("wg3", "conv_wgrad2_kernel", True, None, None), ("wg3", "conv_wgrad2s_kernel", None, None, None),
                         ("wg3", "conv_wgrad2f_kernel", None, 2, None), ("wg3", "conv_wgrad2f_kernel", None, 4, None),
                         ("wgt", "conv_wgrad_kernel", None, None, None), ("wgt", "conv_wgradT2_kernel", None, None, 2),
                         ("wgt", "conv_wgradT2_kernel", None, None, 4), ("wgt", "conv_wgradT2f_kernel", None, None, None)}
    classes = set().union(*seen.values())
    assert classes == {"one", "equal", "short", "clamped"}
    for fam_kernel in (("wg3", "conv_wgrad_kernel"), ("wg3", "conv_wgrad2_kernel"), ("wg3", "conv_wgrad2s_kernel"), ("wgt", "conv_wgradT2_kernel")):
        got = set().union(*(v for k, v in seen.items() if k[:2] == fam_kernel))
        assert len(got) >= 3, f"{fam_kernel}: split classes {got}"


def test_all_three_files_together_name_every_pinned_kernel():
    assert {c["kernel"] for c in R.CASES} == R.PINNED_KERNELS
