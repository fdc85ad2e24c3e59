"""The SparK row-list convolution (conv_gather_kernel of conv_gather.inc, entry ``cmu_conv3x3_fwd_rows``) pinned bit
for bit.  The contract: ``y[rows[m], :]`` is the full 3x3 convolution of the DENSE ``x`` at that pixel, whatever ``x`` holds at its
neighbours, for m < *n_rows; everything else in ``y``'s buffer keeps its previous bits.

The lists are built by hand (conv_exact_ref.rows_list): a fixed random permutation of pixels, every entry past the count a valid,
unlisted pixel whose previous bits must survive (a read past the count shows without an out-of-range access), capacities of the count
rounded up to 256 rows and of three row tiles more (whole workgroups return early), every pixel of a non-square batch of three (every
border, corner and image seam: a wrapped neighbour lands on finite, wrong data), grids the XCD remap splits evenly and unevenly.  Two
cases take their list from ``ops.PixelList``.  ``x`` is a channel slice between guard channels, ``y`` a channel slice of a buffer filled
with a sentinel; both weight packs.  Three kinds of data per case, as in test_gpu_conv3x3_exact.py: integer operands, a one-hot weight
per tap against random floats, impulses.  Every case asserts the kernel tag and the form (NB = 128 | 256, the grid) the restated launcher
rule gives; ``torch.equal`` on the bits is the only comparison."""
import types

import pytest
import torch

import conv_exact_gpu as G
import conv_exact_ref as R

pytestmark = pytest.mark.gpu

ROWS = [(c, dt) for c in R.CASES if c["fam"] == "c3rows" for dt in c["dts"]]
SENTINEL = -1536.0          # exact in every storage type; no reference value of these cases in a guard channel


def ident(v):
    return f"{v['id']}" if isinstance(v, dict) else str(v)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as O
    return O


def the_list(ops, case):
    """-> (namespace with the fields ops.conv3x3_fwd_rows reads, rows on the host, count)."""
    B, H, W = case["shape"][:3]
    if "plist" in case["rows"]:
        f, keep = case["rows"]["plist"]
        act = R.patch_map(B, f, keep, R.case_seed(case) + 13)
        want = R.pixel_list_of(act, H)
        pl = ops.PixelList(act.cuda(), H, W, max_rows=len(want))
        rows = pl.rows.cpu()
        assert int(pl.count.item()) == len(want) and torch.equal(rows[:len(want)], want) and bool((rows[len(want):] == -1).all())
        assert pl.capacity == R.rows_capacity(case, len(want))
        return pl, rows, len(want)
    rows, count = R.rows_list(case, G.cu_count())
    assert int(rows.min()) >= 0 and int(rows.max()) < B * H * W, "every entry handed to the kernel is a valid pixel"
    ns = types.SimpleNamespace(rows=rows.cuda(), count=torch.tensor([count], dtype=torch.int32, device="cuda"), capacity=len(rows),
                               max_rows=max(count, 1))
    return ns, rows, count


def launch(ops, case, dt, x, w, lst):
    """``w`` (N, K, 3, 3) is the weight the kernel multiplies with: packed as it is, or -- flip -- as the flipped pack of the layer weight
    whose data gradient it is.  -> the whole output buffer (guard channels and unlisted pixels included) and what it held before."""
    B, H, W, K, N = case["shape"]
    flip = bool(case["rows"].get("flip"))
    xa = G.in_act(ops, x, dt, case["xs"])
    ld = N if case["ys"] == 0 else case["ys"] + N + 8
    buf = torch.full((B, H, W, ld), SENTINEL, dtype=G.torch_dt(dt), device="cuda")
    before = buf.clone()
    ya = ops.Act(buf, case["ys"], N)
    wp = ops.pack_conv3x3(R.layer_weight(w, flip).cuda().contiguous(), dt, transpose_flip=flip)
    assert ops.conv3x3_rows_supported(B, H, W, K, N, dt)
    with G.knobs(ops, case):
        ops.conv3x3_fwd_rows(xa, wp, ya, lst)
        torch.cuda.synchronize()
        kernel = G.last_kernel()
    rule, form = G.gather_rule(case, dt, G.cu_count(), lst.capacity, G.library_knobs())
    G.assert_form(case, dt, rule, form)
    assert kernel == "conv_gather_kernel", f"{kernel} ran"
    return buf, before


def check(case, buf, before, stored_y, rows, count):
    """The channel slice holds the reference at the listed pixels; every other element of the buffer keeps its bits."""
    N, ys = case["shape"][4], case["ys"]
    want = before.clone()
    want[..., ys:ys + N] = R.rows_expected(stored_y.to(before.device), rows, count, before[..., ys:ys + N])
    if not G.same_bits(buf, want):
        bad = (G.bits(buf) != G.bits(want)).nonzero()
        i = tuple(int(v) for v in bad[0])
        listed = (i[0] * buf.shape[1] + i[1]) * buf.shape[2] + i[2] in set(rows[:count].tolist())
        raise AssertionError(f"{len(bad)} of {buf.numel()} elements differ; first at (b, h, w, c) = {i} ({'a listed' if listed else 'an UNLISTED'} pixel, "
                             f"channel slice [{ys}, {ys + N})): got {float(buf[i])}, want {float(want[i])}")


@pytest.mark.parametrize("case,dt", ROWS, ids=ident)
def test_rows_integer_operands(ops, case, dt):
    o, ref = R.reference_of(case, dt, "cuda")
    lst, rows, count = the_list(ops, case)
    buf, before = launch(ops, case, dt, o["x"], o["w"], lst)
    check(case, buf, before, ref["stored"], rows, count)
    if count == 0:
        assert G.same_bits(buf, before), "an empty list wrote something"


@pytest.mark.parametrize("case,dt", ROWS, ids=ident)
def test_rows_one_hot_weight_moves_float_activations(ops, case, dt):
    """Tap by tap: one-hot columns at the corner channels of the first and last N block (of 128 and of 256 channels), each fed by a corner
    channel of the first and last 128-byte K step: the output channel is the shifted input channel, bit for bit, every other one 0."""
    B, H, W, K, N = case["shape"]
    x = R.stored(R.float_operands((B, H, W, K), R.case_seed(case)).double(), dt).cuda()
    cis = G.corner_channels(K, 128 // G.ES[dt])
    cos = sorted(set(G.corner_channels(N, 128)) | set(G.corner_channels(N, 256)))
    lst, rows, count = the_list(ops, case)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        w = torch.zeros(N, K, 3, 3)
        want = torch.zeros(B, H, W, N, dtype=x.dtype, device="cuda")
        for j, co in enumerate(cos):
            ci = cis[(tap + j) % len(cis)]
            w[co, ci, ky, kx] = 1.0
            want[..., co] = R.shift2d(x[..., ci:ci + 1], ky - 1, kx - 1)[..., 0]
        buf, before = launch(ops, case, dt, x, w, lst)
        check(case, buf, before, want, rows, count)


@pytest.mark.parametrize("case,dt", ROWS, ids=ident)
def test_rows_impulses_at_the_first_and_last_pixel_and_across_the_image_seam(ops, case, dt):
    """One 1.0 at the first pixel, at the last pixel of the last image and on both sides of an image seam: the outputs at the (up to) nine
    neighbours of each are the weights, and a neighbour taken from the next image of the batch shows."""
    B, H, W, K, N = case["shape"]
    o, _ = R.reference_of(case, dt, "cuda")
    cis = G.corner_channels(K, 128 // G.ES[dt])
    px = [(0, 0, 0), (B - 1, H - 1, W - 1)] + ([(0, H - 1, W - 1), (1, 0, 0)] if B > 1 else [])
    x = torch.zeros(B, H, W, K, device="cuda")
    for i, (b, h, w_) in enumerate(sorted(set(px))):
        x[b, h, w_, cis[i % len(cis)]] = 1.0
    ref = R.conv3x3_exact(x, o["w"], None, dt)
    R.assert_exact_caps(ref, dt)
    lst, rows, count = the_list(ops, case)
    buf, before = launch(ops, case, dt, x, o["w"], lst)
    check(case, buf, before, ref["stored"], rows, count)
    if case["rows"].get("count") == "all" and H > 1 and W > 1:
        # spelled out for the impulse at (0, 0, 0), channel cis[0]: y[0, 1, 1] reads it through tap (0, 0), y[0, 0, 0] through the centre
        ys = case["ys"]
        w = o["w"].to(G.torch_dt(dt)).cuda()
        assert torch.equal(buf[0, 1, 1, ys:ys + N], w[:, cis[0], 0, 0]) and torch.equal(buf[0, 0, 0, ys:ys + N], w[:, cis[0], 1, 1])
        # and across the seam: the first pixel of image 1 sees nothing of the impulse at the last pixel of image 0
        i1 = sorted(set(px)).index((1, 0, 0))
        assert torch.equal(buf[1, 0, 0, ys:ys + N], w[:, cis[i1 % len(cis)], 1, 1])


def test_the_cases_cover_the_forms_grids_and_counts_of_the_gather_kernel():
    """Built from CASES with the restated rule (256 CUs): K steps per tap 1, 2, 3; Cout 128, 256, 384; both NB forms, forced and by the
    launcher's own rule; the counts and grid sizes the XCD remap splits evenly (8) and unevenly (1, 3, 9, 17); both packs."""
    steps, couts, forms, grids, counts, packs = set(), set(), set(), set(), set(), set()
    for c in R.CASES:
        if c["fam"] != "c3rows":
            continue
        for dt in c["dts"]:
            _, form = G.gather_rule(c, dt, 256, R.rows_capacity(c, R.rows_count(c)))
            G.assert_form(c, dt, "conv_gather_kernel", form)
            steps.add(form["steps"])
            couts.add(c["shape"][4])
            forms.add((form["NB"], c["knobs"].get("GATHER_NB", 0)))
            grids.add(form["grid"])
            counts.add(c["rows"].get("count"))
            packs.add(bool(c["rows"].get("flip")))
    assert {1, 2, 3} <= steps and couts == {128, 256, 384} and packs == {True, False}
    assert {(128, 128), (256, 256), (128, 0), (256, 0)} <= forms
    assert {1, 3, 8, 9, 17} <= grids and {0, 1, 255, 256, 257, 700, "all"} <= counts
