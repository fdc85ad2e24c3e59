"""The weight gradient over a device-side tile list (``cmu_conv3x3_wgrad_tiles``: the list path of conv_wgrad_kernel with 16 x 16 tiles
and of conv_wgrad2_kernel / conv_wgrad2s_kernel with 8 x 16 tiles) pinned bit for bit against ``conv3x3_wgrad_exact`` of dY restricted to
the listed tiles (conv_exact_ref.wgrad_tiles_exact).

Split s of the launch walks the list entries s, s + splits, ...; the split count is the dense launch's, restated in
conv_exact_gpu.wgrad3_tiles_rule and tied to the library through ``cmu_conv3x3_wgrad_ws_bytes``.  The hand-built lists have counts
relative to it: 0 (dW is exactly zero), fewer entries than splits (empty splits), as many, a multiple, a multiple plus a remainder, every
tile (the dense launch's bits); ascending and permuted; on a 20 x 40 image (partial tiles in both directions).  Guards: the workspace is
NaN before every call (a slab that an empty split leaves unwritten shows), dW is prefilled, the entries past the count hold valid,
unlisted tile ids, dY is non-zero in EVERY tile (the kernel must visit the list only), x is non-zero everywhere (the halo of a listed
tile reads unlisted ones) and carries a pending integer transform.  Builder-made lists (``ops.TileList``) at 32 x 32 and 64 x 64.
``torch.equal`` on the bits is the only comparison."""
import types

import pytest
import torch

import conv_exact_gpu as G
import conv_exact_ref as R

pytestmark = pytest.mark.gpu

TILES = [(c, dt) for c in R.CASES if c["fam"] == "wg3tiles" for dt in c["dts"]]
HAND = [(c, dt) for c, dt in TILES if "builder" not in c["tiles"]]
BUILT = [(c, dt) for c, dt in TILES if "builder" in c["tiles"]]


def ident(v):
    return f"{v['id']}" if isinstance(v, dict) else str(v)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as O
    return O


def rule_of(case, dt):
    kernel, form, splits, ntiles = G.wgrad3_tiles_rule(case, dt, G.library_knobs())
    G.assert_form(case, dt, kernel, form)
    return kernel, splits, ntiles


def namespace(case, tlist, count):
    return types.SimpleNamespace(list=tlist.cuda(), count=torch.tensor([count], dtype=torch.int32, device="cuda"), tile_h=case["tiles"]["th"],
                                 tile_w=16)


def launch(ops, case, dt, x, dy, tf, tiles):
    from cmunet_amd import _lib
    B, H, W, Cin, Cout = case["shape"]
    kernel, splits, ntiles = rule_of(case, dt)
    xa = G.in_act(ops, x, dt, case["xs"], tf)
    da = G.in_act(ops, dy, dt, case["ys"])
    dW = torch.full((Cout, Cin, 3, 3), -1536.0, device="cuda")
    with G.knobs(ops, case):
        need = _lib.lib().cmu_conv3x3_wgrad_ws_bytes(B, H, W, Cin, Cout, ops.dt_code(dt))
        ws = torch.full(((need + 3) // 4 + 1024,), float("nan"), dtype=torch.float32, device="cuda")
        ops.conv3x3_wgrad_tiles(xa, da, dW, ws, tiles)
        torch.cuda.synchronize()
        ran = G.last_kernel()
    assert ran == case["kernel"] == kernel, f"{ran} ran, the rule gives {kernel}"
    assert need == G.wgrad3_ws_bytes(case, dt, G.library_knobs()) and need >= G.slab_bytes(case, dt, kernel, splits)
    if dt != "f32" and (Cout % 64 or Cin % 64):
        assert need == G.slab_bytes(case, dt, kernel, splits), "the first kernel is the only candidate: its slabs are the workspace"
    assert bool(torch.isnan(ws[(need + 3) // 4:]).all()), "a slab store landed behind the workspace"
    return dW


def check_grad(got, want, what):
    want = want.to(torch.float32)
    if not G.same_bits(got, want):
        bad = (G.bits(got) != G.bits(want.to(got.device))).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} entries differ; first at {i}: got {float(got[i])}, exact {float(want[i])}")


@pytest.mark.parametrize("case,dt", HAND, ids=ident)
def test_wgrad_tiles_integer_operands(ops, case, dt):
    kernel, splits, ntiles = rule_of(case, dt)
    o, ref = R.reference_of(case, dt, "cuda", splits=splits)
    tl, count = o["tiles"], o["count"]
    assert len(tl) == ntiles and int(tl.min()) >= 0 and int(tl.max()) < ntiles, "every entry handed to the kernel is a valid tile"
    dW = launch(ops, case, dt, o["x"], o["dy"], o["tf"], namespace(case, tl, count))
    check_grad(dW, ref["dW"], "dW")
    cls = case["tiles"]["cls"]
    if cls == "zero":
        assert count == 0 and G.same_bits(dW, torch.zeros_like(dW)), "an empty list: dW is exactly +0"
    else:
        assert bool((ref["dW"] != 0).any())
    if cls == "all":
        # every tile listed: the bits of the dense launch
        from cmunet_amd import _lib
        B, H, W, Cin, Cout = case["shape"]
        dense = torch.full_like(dW, float("nan"))
        with G.knobs(ops, case):
            ws = torch.full(((_lib.lib().cmu_conv3x3_wgrad_ws_bytes(B, H, W, Cin, Cout, ops.dt_code(dt)) + 3) // 4,), float("nan"), device="cuda")
            ops.conv3x3_wgrad(G.in_act(ops, o["x"], dt, case["xs"], o["tf"]), G.in_act(ops, o["dy"], dt, case["ys"]), dense, ws)
        assert count == ntiles and G.same_bits(dW, dense)
    else:
        # dY is non-zero in the unlisted tiles: the dense sum differs, so a kernel that visited them would show
        assert not torch.equal(R.conv3x3_wgrad_exact(o["x"], o["dy"], o["tf"])["dW"], ref["dW"])


@pytest.mark.parametrize("case,dt", [(c, dt) for c, dt in HAND if c["tiles"]["cls"] in ("below", "remainder")], ids=ident)
def test_wgrad_tiles_impulses_at_the_corners_of_a_listed_tile_next_to_an_unlisted_one(ops, case, dt):
    """dY = one 1.0 at the first and one at the last (valid) pixel of a listed tile that has an unlisted neighbour, and a 2.0 just across
    the border inside that neighbour: dW is the window of x around the two listed pixels -- the halo comes from the unlisted tile -- and
    the 2.0 does not count."""
    B, H, W, Cin, Cout = case["shape"]
    kernel, splits, ntiles = rule_of(case, dt)
    o, _ = R.reference_of(case, dt, "cuda", splits=splits)
    tl, count = o["tiles"], o["count"]
    _, tY, tX, th = R.tiles_geometry(case)
    listed = set(tl[:count].tolist())
    pick = None
    for t in tl[:count].tolist():
        b, ty, tx = t // (tY * tX), (t // tX) % tY, t % tX
        for dy_, dx_ in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            if 0 <= ty + dy_ < tY and 0 <= tx + dx_ < tX and ((b * tY + ty + dy_) * tX + tx + dx_) not in listed:
                pick = (b, ty, tx, dy_, dx_)
                break
        if pick:
            break
    assert pick is not None, "no listed tile with an unlisted neighbour"
    b, ty, tx, dy_, dx_ = pick
    y0, x0, y1, x1 = ty * th, tx * 16, min(H, (ty + 1) * th) - 1, min(W, (tx + 1) * 16) - 1
    imp = torch.zeros(B, H, W, Cout, device="cuda")
    c0, c1 = 0, Cout - 1
    imp[b, y0, x0, c0] = 1.0
    imp[b, y1, x1, c1] = 1.0
    # the pixel just across the border, in the unlisted neighbour
    ny = y1 + 1 if dy_ == 1 else (y0 - 1 if dy_ == -1 else y0)
    nx = x1 + 1 if dx_ == 1 else (x0 - 1 if dx_ == -1 else x0)
    imp[b, ny, nx, c0] = 2.0
    ref = R.wgrad_tiles_exact(case, o["x"], imp, tl, count, o["tf"])
    R.assert_exact_caps(ref)
    dW = launch(ops, case, dt, o["x"], imp, o["tf"], namespace(case, tl, count))
    check_grad(dW, ref["dW"], "dW")
    xa = R.apply_transform(o["x"], o["tf"])
    for (py, px, ch) in ((y0, x0, c0), (y1, x1, c1)):
        for ky in range(3):
            for kx in range(3):
                yy, xx = py + ky - 1, px + kx - 1
                want = xa[b, yy, xx].float() if 0 <= yy < H and 0 <= xx < W else torch.zeros(Cin, device="cuda")
                assert torch.equal(dW[ch, :, ky, kx], want), (py, px, ky, kx)


@pytest.mark.parametrize("case,dt", BUILT, ids=ident)
def test_wgrad_tiles_over_builder_made_lists(ops, case, dt):
    """``ops.TileList`` on a square level: the list is first held to the patch map (a tile is listed iff it holds an active pixel), then
    the kernel to the reference over that list."""
    B, H, W, Cin, Cout = case["shape"]
    f, keep = case["tiles"]["builder"]
    th = case["tiles"]["th"]
    act = R.patch_map(B, f, keep, R.case_seed(case) + 14)
    tl = ops.TileList(act.cuda(), H, W, th, 16)
    up = act.repeat_interleave(H // f, 1).repeat_interleave(W // f, 2)
    want = [(b * (H // th) + ty) * (W // 16) + tx for b in range(B) for ty in range(H // th) for tx in range(W // 16)
            if int(up[b, ty * th:(ty + 1) * th, tx * 16:(tx + 1) * 16].max())]
    count = int(tl.count.item())
    assert 0 < count < tl.n_dense and tl.list[:count].cpu().tolist() == want
    o, full = R.reference_of(case, dt, "cuda")
    ref = R.wgrad_tiles_exact(case, o["x"], o["dy"], tl.list.cpu(), count, o["tf"])
    R.assert_exact_caps(ref)
    dW = launch(ops, case, dt, o["x"], o["dy"], o["tf"], tl)
    check_grad(dW, ref["dW"], "dW")
    assert not torch.equal(full["dW"], ref["dW"])


def test_the_cases_cover_every_list_kernel_and_count_class():
    seen = {}
    for c, dt in HAND:
        kernel, form, splits, ntiles = G.wgrad3_tiles_rule(c, dt)
        G.assert_form(c, dt, kernel, form)
        assert kernel == c["kernel"]
        seen.setdefault((kernel, dt == "f32"), set()).add((c["tiles"]["cls"], c["tiles"]["order"]))
    assert set(seen) == {("conv_wgrad_kernel", False), ("conv_wgrad_kernel", True), ("conv_wgrad2_kernel", False), ("conv_wgrad2s_kernel", False)}
    for k, v in seen.items():
        assert {"zero", "below", "equal", "remainder", "all"} <= {cls for cls, _ in v}, k
        assert {"asc", "perm"} <= {order for _, order in v}, k
    assert all("multiple" in {cls for cls, _ in v} for k, v in seen.items() if not k[1])
    assert {c["kernel"] for c, _ in BUILT} == {"conv_wgrad_kernel", "conv_wgrad2_kernel", "conv_wgrad2s_kernel"}
