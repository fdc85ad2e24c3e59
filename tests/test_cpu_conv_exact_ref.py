"""The exact references of tests/conv_exact_ref.py proved against torch (``F.conv2d``, ``F.conv_transpose2d``,
``torch.nn.grad.conv2d_weight``, float64 autograd for the BatchNorm-backward sums) on integer and on random float data, and the
condition that makes the GPU cases exact -- every fp32 sum below 2**24, from the reference alone -- asserted for every entry of
``CASES``.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_ref as R


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def close(a, b, exact, rel=1e-12):
    """Integer data: equal.  Float data: to float64 rounding (``rel`` 1e-5 where the helper returns an fp32 slab)."""
    if exact:
        return torch.equal(a.double(), b.double())
    return float((a.double() - b.double()).abs().max()) <= rel * max(1.0, float(b.double().abs().max()))


def operands(shape, exact, seed, lo=-3, hi=3):
    if exact:
        return R.int_operands(shape, lo, hi, 0.8, seed)
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def transform(C, exact, seed, relu_from):
    if exact:
        sc = R.int_operands((C,), 1, 2, 1.0, seed) * (R.int_operands((C,), 0, 1, 1.0, seed + 1) * 2 - 1)
        return sc, R.int_operands((C,), -2, 2, 1.0, seed + 2), relu_from
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=g), torch.randn(C, generator=g), relu_from


def torch_transform(x, tf):
    """The pending transform written out channel by channel (a second, slower statement of cmu_relu_on)."""
    if tf is None:
        return x.double()
    sc, sh, rf = tf
    out = x.double().clone()
    for c in range(x.shape[-1]):
        z = x[..., c].double() * float(sc[c]) + float(sh[c])
        on = (c >= rf) if rf >= 0 else (c < -rf)
        out[..., c] = torch.relu(z) if on else z
    return out


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("relu_from", [None, 0, 8, -8, 16])
def test_conv3x3_exact_is_conv2d(exact, relu_from):
    B, H, W, Cin, Cout = 2, 19, 35, 16, 24
    x, w = operands((B, H, W, Cin), exact, 1), operands((Cout, Cin, 3, 3), exact, 2)
    tf = None if relu_from is None else transform(Cin, exact, 3, relu_from)
    r = R.conv3x3_exact(x, w, tf, "bf16")
    ref = nhwc(F.conv2d(nchw(torch_transform(x, tf)), w.double(), padding=1))
    assert close(r["y"], ref, exact)
    assert torch.equal(r["stored"], ref.float().to(torch.bfloat16)) or not exact
    # statistics: per 16 x 16 tile of the unrounded values, tile index (b, ty, tx) row-major
    st = r["stats"].double()
    assert st.shape == (B * 2 * 3, 2, Cout)
    t = (1 * 2 + 1) * 3 + 2                                            # image 1, tile row 1 (3 valid rows), tile column 2 (3 valid columns)
    blk = ref[1, 16:19, 32:35]
    assert close(st[t, 0], blk.sum((0, 1)), exact, 1e-5) and close(st[t, 1], (blk * blk).sum((0, 1)), exact, 1e-5)
    assert close(st[:, 0].sum(0), ref.sum((0, 1, 2)), exact, 1e-5) and close(st[:, 1].sum(0), (ref * ref).sum((0, 1, 2)), exact, 1e-5)
    mag = nhwc(F.conv2d(nchw(torch_transform(x, tf)).abs(), w.double().abs(), padding=1))
    assert close(r["mag"], mag, exact)


@pytest.mark.parametrize("exact", [True, False])
def test_conv3x3_dgrad_is_the_adjoint_and_its_sums_are_autograd_of_batchnorm(exact):
    B, H, W, K, N = 2, 17, 20, 24, 16
    dy, w = operands((B, H, W, K), exact, 4), operands((K, N, 3, 3), exact, 5)
    yraw = operands((B, H, W, N), exact, 6)
    bscale, bshift, mean, invstd = R.bn_consts(N, 7)
    if not exact:
        g = torch.Generator().manual_seed(8)
        bscale, bshift, mean, invstd = (torch.randn(N, generator=g) for _ in range(4))
    r = R.conv3x3_dgrad_bn_exact(dy, w, yraw, bscale, bshift, mean, invstd, "f32")
    xin = torch.zeros(B, N, H, W, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xin, w.double(), padding=1) * nchw(dy.double())).sum().backward()
    assert close(r["y"], nhwc(xin.grad), exact)
    # the sums are the gradients of BatchNorm's beta and gamma: out = relu(xhat * gamma + beta) with gamma = bscale / invstd and
    # beta = bshift + mean * bscale, so that xhat * gamma + beta = yraw * bscale + bshift, the gate's argument
    dx = r["stored"].double()
    xhat = (yraw.double() - mean.double()) * invstd.double()
    gamma = (bscale.double() / invstd.double()).requires_grad_(True)
    beta = (bshift.double() + mean.double() * bscale.double()).requires_grad_(True)
    (torch.relu(xhat * gamma + beta) * dx).sum().backward()
    a, b = beta, gamma
    got = r["bstats"].double().sum(0)
    assert close(got[0], a.grad, exact, 1e-5) and close(got[1], b.grad, exact, 1e-5)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("relu_from", [None, 8, -8])
def test_conv3x3_wgrad_exact_is_conv2d_weight(exact, relu_from):
    B, H, W, Cin, Cout = 2, 9, 21, 16, 8
    x, dy = operands((B, H, W, Cin), exact, 9), operands((B, H, W, Cout), exact, 10)
    tf = None if relu_from is None else transform(Cin, exact, 11, relu_from)
    r = R.conv3x3_wgrad_exact(x, dy, tf)
    ref = torch.nn.grad.conv2d_weight(nchw(torch_transform(x, tf)), (Cout, Cin, 3, 3), nchw(dy.double()), padding=1)
    assert close(r["dW"], ref, exact)
    # an impulse in dY: dW is the 3 x 3 window of x around the pixel (zero outside the image)
    imp = torch.zeros(B, H, W, Cout)
    imp[1, H - 1, 0, 3] = 1.0
    d = R.conv3x3_wgrad_exact(x, imp, None)["dW"]
    assert torch.equal(d[3, :, 0, 1], x[1, H - 2, 0].double()) and torch.equal(d[3, :, 1, 2], x[1, H - 1, 1].double())
    assert float(d[3, :, 2].abs().max()) == 0 and float(d[3, :, :, 0].abs().max()) == 0 and float(d[:3].abs().max()) == 0


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("relu_from", [None, 8])
def test_convT2x2_forms_are_conv_transpose2d_and_its_gradients(exact, relu_from):
    B, H, W, Cin, Cout = 2, 5, 9, 16, 8
    x, w, bias = operands((B, H, W, Cin), exact, 12), operands((Cin, Cout, 2, 2), exact, 13), operands((Cout,), exact, 14, -50, 50)
    dout = operands((B, 2 * H, 2 * W, Cout), exact, 15)
    tf = None if relu_from is None else transform(Cin, exact, 16, relu_from)
    xa = nchw(torch_transform(x, tf)).requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    out = F.conv_transpose2d(xa, wd, bd, stride=2)
    (out * nchw(dout.double())).sum().backward()
    assert close(R.convT2x2_exact(x, w, bias, tf, "f16")["y"], nhwc(out.detach()), exact)
    assert close(R.convT2x2_dgrad_exact(dout, w, "f16")["y"], nhwc(xa.grad), exact)
    g = R.convT2x2_wgrad_exact(x, dout, tf)
    assert close(g["dW"], wd.grad, exact) and close(g["dbias"], bd.grad, exact)
    yraw = operands((B, H, W, Cin), True, 17)
    bn = R.bn_consts(Cin, 18)
    r = R.convT2x2_dgrad_bn_exact(dout, w, yraw, *bn, dt="bf16")
    slab, _ = R.bn_bwd_sums(r["stored"], yraw, *bn)
    assert torch.equal(slab, r["bstats"]) and slab.shape == (B * 1 * 1, 2, Cin)


@pytest.mark.parametrize("exact", [True, False])
def test_rows_reference_is_conv2d_at_the_listed_pixels_and_the_sentinel_elsewhere(exact):
    """fam c3rows: the reference read at the listed pixels equals torch's float64 convolution there -- at every border, corner and image
    seam of a non-square batch, in the list's own order -- and the buffer keeps what it held everywhere else; with the flipped pack the
    packed weight is the flipped transpose of the layer's."""
    case = next(c for c in R.CASES if c["id"] == "rows every pixel of 3 x 5 x 11, flipped pack")
    part = dict(case, rows={"count": 100, "cap": "slack"})
    for c in (case, part):
        B, H, W, K, N = c["shape"]
        x, w = operands((B, H, W, K), exact, 21), operands((N, K, 3, 3), exact, 22)
        rows, count = R.rows_list(c)
        assert rows.dtype == torch.int32 and len(rows) == R.rows_capacity(c, count) and len(rows) % 256 == 0
        assert int(rows.min()) >= 0 and int(rows.max()) < B * H * W and len(set(rows[:count].tolist())) == count
        r = R.conv3x3_exact(x, w, None, "f32")
        before = torch.full((B, H, W, N), -1536.0, dtype=torch.float64)
        got = R.rows_expected(r["y"], rows, count, before)
        ref = nhwc(F.conv2d(nchw(x.double()), w.double(), padding=1))
        listed = torch.zeros(B * H * W, dtype=torch.bool)
        listed[rows[:count].long()] = True
        listed = listed.view(B, H, W)
        assert int(listed.sum()) == count and close(got[listed], ref[listed], exact)
        assert bool((got[~listed] == -1536.0).all())
        if count < B * H * W:                  # the entries past the count name unlisted pixels
            assert not bool(listed.view(-1)[rows[count:].long()].any())
        # the flipped pack: conv with w == the data gradient of the layer whose weight is layer_weight(w, True)
        wl = R.layer_weight(w, True)
        xin = torch.zeros(B, N, H, W, dtype=torch.float64, requires_grad=True)
        (F.conv2d(xin, wl.double(), padding=1) * nchw(x.double())).sum().backward()
        assert close(nhwc(xin.grad), ref, exact) and R.layer_weight(w, False) is w


def test_pixel_list_of_is_the_patch_major_order():
    act = torch.tensor([[[0, 1], [1, 0]]], dtype=torch.uint8)
    assert R.pixel_list_of(act, 4).tolist() == [2, 3, 6, 7, 8, 9, 12, 13]


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("th", [8, 16])
def test_wgrad_tiles_reference_is_conv2d_weight_of_the_masked_gradient(exact, th):
    """fam wg3tiles: dW of dY restricted to the listed tiles, against torch's float64 weight gradient of dY zeroed OUTSIDE them pixel by
    pixel (a loop over tiles: a second statement of the dense tile numbering (b * tilesY + ty) * tilesX + tx, partial tiles included)."""
    case = next(c for c in R.CASES if c["fam"] == "wg3tiles" and c["tiles"]["th"] == th and c["tiles"].get("cls") == "remainder"
                and c["tiles"]["order"] == "perm")
    B, H, W, K, N = case["shape"]
    x, dy = operands((B, H, W, K), exact, 23), operands((B, H, W, N), exact, 24)
    tf = transform(K, exact, 25, 8)
    tl, count = R.tiles_list(case, 4)
    tY, tX = -(-H // th), -(-W // 16)
    assert len(tl) == B * tY * tX and 0 < count < len(tl) and len(set(tl[:count].tolist())) == count
    assert not set(tl[:count].tolist()) & set(tl[count:].tolist())
    d = torch.zeros(B, H, W, N, dtype=torch.float64)
    for t in tl[:count].tolist():
        b, ty, tx = t // (tY * tX), (t // tX) % tY, t % tX
        d[b, ty * th:(ty + 1) * th, tx * 16:(tx + 1) * 16] = dy[b, ty * th:(ty + 1) * th, tx * 16:(tx + 1) * 16].double()
    ref = torch.nn.grad.conv2d_weight(nchw(torch_transform(x, tf)), (N, K, 3, 3), nchw(d), padding=1)
    assert close(R.wgrad_tiles_exact(case, x, dy, tl, count, tf)["dW"], ref, exact)
    assert not close(R.conv3x3_wgrad_exact(x, dy, tf)["dW"], ref, exact)


def test_rounding_report_counts_ties():
    y = torch.tensor([256.0, 257.0, 258.0, 259.0, 513.0, 514.0, 515.0, 2049.0, 2050.0, 4097.0, 4098.0])
    # bf16 keeps 8 bits: step 2 from 256 (257, 259 are ties), 4 from 512 (514 is one; 513, 515 are not), 16 from 2048, 32 from 4096
    assert R.rounding_report(y.double(), "bf16") == (9 / 11, 3)
    # f16 keeps 11 bits: step 2 from 2048 (2049 is a tie), 4 from 4096 (4098 is one; 4097 is not)
    assert R.rounding_report(y.double(), "f16") == (3 / 11, 2)
    assert R.rounding_report(y.double(), "f32") == (0.0, 0)


def test_transform_follows_cmu_relu_on():
    x = R.int_operands((1, 2, 3, 16), -3, 3, 1.0, 0)
    sc, sh = torch.full((16,), -1.0), torch.full((16,), 1.0)
    for rf in (0, 8, 16, -8, -16):
        z = R.apply_transform(x, (sc, sh, rf))
        assert torch.equal(z, torch_transform(x, (sc, sh, rf)))
    assert bool((R.apply_transform(x, (sc, sh, -8))[..., :8] >= 0).all()) and bool((R.apply_transform(x, (sc, sh, -8))[..., 8:] < 0).any())


IDS = [f"{c['fam']}-{c['id']}-{dt}" for c in R.CASES for dt in c["dts"]]
_REPORT = {}


@pytest.mark.parametrize("case,dt", [(c, dt) for c in R.CASES for dt in c["dts"]], ids=IDS)
def test_every_case_keeps_every_fp32_sum_below_2_pow_24(case, dt):
    ops, ref = R.reference_of(case, dt)
    rep = R.assert_exact_caps(ref, dt, case["stats"])
    _REPORT[(case["fam"], case["id"], dt)] = rep
    # (the impulse and one-hot runs of the GPU files use the same weights against at most one 1.0 per window: fewer, smaller terms)


@pytest.mark.parametrize("dt,fams", [("f16", ("c3f",)), ("bf16", ("c3f",)), ("f16", ("ctf",)), ("bf16", ("ctf",)), ("bf16", ("c3dg",)),
                                     ("bf16", ("ctdgbn",)), ("f16", ("c3rows",)), ("bf16", ("c3rows",))])
def test_each_family_has_a_case_with_exact_ties(dt, fams):
    """Round-to-nearest-even is only told from other roundings on exact ties: each 16-bit type has them in a forward case of each
    family (the row-list family c3rows included) (f16 through the power-of-two lift of every eighth input channel).  The data gradients have a bf16 case whose dX is inexact,
    so that sums taken on the unrounded dX differ (in f16 every integer dX of these cases is below 2048 and exact)."""
    ties = 0
    for c in R.CASES:
        if c["fam"] in fams and dt in c["dts"]:
            _, ref = R.reference_of(c, dt)
            rep = R.assert_exact_caps(ref, dt, c["stats"])
            ties += rep["ties"] if fams[0] in ("c3f", "ctf", "c3rows") else int(rep["inexact"] > 0)
    assert ties > 0


def test_cases_name_every_pinned_kernel_and_are_unique():
    assert {c["kernel"] for c in R.CASES} == R.PINNED_KERNELS
    assert len({(c["fam"], c["id"]) for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:
        assert set(c["dts"]) <= {"f32", "f16", "bf16"} and c["fam"] in ("c3f", "c3dg", "ctf", "ctdg", "ctdgbn", "wg3", "wgt", "c3rows", "wg3tiles")
        assert (c["rows"] is not None) == (c["fam"] == "c3rows") and (c["tiles"] is not None) == (c["fam"] == "wg3tiles")
        epc = 4 if "f32" in c["dts"] else 8
        assert all(v % epc == 0 for v in (c["xs"], c["ys"], c["shape"][3], c["shape"][4]))
        assert c["tf"] is None or c["tf"] % epc == 0


@pytest.mark.parametrize("case,dt", [(c, dt) for c in R.CASES for dt in c["dts"]], ids=IDS)
def test_the_restated_launcher_rules_give_each_case_its_kernel_on_256_cus(case, dt):
    """The GPU files assert this with the device's CU count; here with the MI355X's 256, so that a case list that drifts from the
    rules fails without a GPU."""
    import conv_exact_gpu as G
    fam = case["fam"]
    if fam in ("c3f", "c3dg"):
        kernel, form = G.conv3_rule(case, dt, 256, case["tf"] is not None, fam == "c3dg")
    elif fam in ("ctf", "ctdg", "ctdgbn"):
        kernel, form = G.convT_rule(case, dt, fam != "ctf", case["tf"] is not None)
    elif fam == "c3rows":
        kernel, form = G.gather_rule(case, dt, 256, R.rows_capacity(case, R.rows_count(case), 256))
    elif fam == "wg3tiles":
        kernel, form = G.wgrad3_tiles_rule(case, dt)[:2]
    else:
        kernel, form = (G.wgrad3_rule if fam == "wg3" else G.wgradT_rule)(case, dt)[:2]
    G.assert_form(case, dt, kernel, form)


def test_pinned_kernels_are_every_tag_of_the_library_but_one():
    """Every tag ``cmu_set_kernel_tag`` can set (read from the sources), apart from conv_igemm6_kernel, is asserted by a case: a new kernel
    tag, or a case list that loses one, fails here.  Per source file: every C entry of the convolution sources that takes a device-side
    list (a ``tile_list`` / ``rows`` / ``lists`` argument) is named in ``LIST_ENTRIES`` with the test file that holds it to an independent
    reference, that file exists and calls it, and every kernel that reads ``p.tile_list`` belongs to a pinned tag: a new gather or list
    form cannot go untested."""
    import glob
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cmunet_amd", "csrc")
    tags = set()
    for path in glob.glob(os.path.join(csrc, "*")):
        with open(path, errors="replace") as f:
            tags |= set(re.findall(r'cmu_set_kernel_tag\("([a-zA-Z0-9_]+)"\)', f.read()))
    assert tags - {"conv_igemm6_kernel"} == R.PINNED_KERNELS
    assert {c["kernel"] for c in R.CASES} == R.PINNED_KERNELS
    tests = os.path.dirname(os.path.abspath(__file__))
    entries, readers = set(), set()
    for path in glob.glob(os.path.join(csrc, "*")):
        with open(path, errors="replace") as f:
            text = f.read()
        # extern "C" entries of the convolution and list sources with a device-side list among their arguments
        for name, args in re.findall(r'extern "C" int (cmu_(?:conv3x3|sparse)_[a-z0-9_]+)\((.*?)\)\s*\{', text, re.S):
            if re.search(r"\*\s*(const\*\s*)?(tile_list|rows|list|lists)\b", args):
                entries.add(name)
        if "p.tile_list" in text:
            readers.add(os.path.basename(path))
    assert entries == set(R.LIST_ENTRIES), sorted(entries ^ set(R.LIST_ENTRIES))
    for entry, fname in R.LIST_ENTRIES.items():
        with open(os.path.join(tests, fname)) as f:
            text = f.read()
        called = entry[4:] in text or {"cmu_sparse_tile_list": "TileList(", "cmu_sparse_tile_lists": "build_lists(", "cmu_sparse_pixel_list": "PixelList(",
                                       "cmu_sparse_pixel_lists": "build_lists("}.get(entry, entry) in text
        assert called, f"{fname} does not call {entry}"
    # the sources whose kernels walk a list: each has cases of the list families
    assert readers == {"conv_gather.inc", "conv_igemm.hip", "conv_igemm3p.inc", "conv_igemm5.inc", "conv_igemm6.inc", "conv_wgrad.hip",
                       "conv_wgrad2.inc", "conv_wgrad2s.inc"}, f"a new source reads a device-side list: give it exact cases ({sorted(readers)})"
    assert {c["kernel"] for c in R.CASES if c["fam"] == "c3rows"} == {"conv_gather_kernel"}
    assert {c["kernel"] for c in R.CASES if c["fam"] == "wg3tiles"} == {"conv_wgrad_kernel", "conv_wgrad2_kernel", "conv_wgrad2s_kernel"}


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kernel", ["conv_igemm_kernel", "conv_igemm3_kernel", "conv_igemm3p_kernel", "conv_igemm5_kernel"])
def test_each_statistics_kernel_has_a_case_whose_rounded_slab_differs(kernel, dt):
    """Each of the four 3x3 kernels has its own statistics code.  Sums taken from the STORED outputs instead of the fp32 accumulators are
    only told apart where an output is inexact in the storage type: each kernel has such a statistics case in each 16-bit type (K = 1024
    with weights in [-2, 2] for bf16; one output per tile and channel lifted past 2048 for f16 and bf16), one of them through a partial
    tile, and the slab built from the rounded values differs from the reference slab there."""
    differing, partial = 0, 0
    for c in R.CASES:
        if c["fam"] == "c3f" and c["stats"] and c["kernel"] == kernel and dt in c["dts"]:
            _, ref = R.reference_of(c, dt)
            R.assert_exact_caps(ref, dt, True)
            s = ref["stored"].double()
            n = int((R.tile_stats(s, s * s).to(torch.float32) != ref["stats"]).sum())
            differing += n
            partial += n if (c["shape"][1] % 16 or c["shape"][2] % 32) else 0
    assert differing > 0
    assert partial > 0 or kernel == "conv_igemm5_kernel"          # (conv_igemm5 takes whole tiles only)


def test_workspace_restatement_covers_the_slabs_of_the_kernel_that_runs():
    """The restated workspace size is never below the slabs the restated split count needs (the GPU files compare it with the library's)."""
    import conv_exact_gpu as G
    for c in R.CASES:
        if c["fam"] in ("wg3", "wgt"):
            for dt in c["dts"]:
                kernel, form, splits, ntiles = (G.wgrad3_rule if c["fam"] == "wg3" else G.wgradT_rule)(c, dt)
                need = (G.wgrad3_ws_bytes if c["fam"] == "wg3" else G.wgradT_ws_bytes)(c, dt)
                assert need >= G.slab_bytes(c, dt, kernel, splits), (c["id"], dt)
