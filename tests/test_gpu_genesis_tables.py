"""The Models Genesis kernels (csrc/genesis.hip) at their seams, entry by entry, against numpy: the Bezier tables and their sort
(cmu_genesis_bezier), np.interp through them (cmu_genesis_intensity_paint), gather / flip / local shuffle with its owner map and row
segments (cmu_genesis_gather_shuffle) and the MSE loss (cmu_mse_fwd_bwd).  The kernels are driven through ``_lib.call`` with hand-made
records (genesis.REC_DTYPE) and a hand-filled ``minmax`` buffer: records drawn by the sampler (draws in [0, 1)) only ever give a
monotone cubic -- tests/test_cpu_genesis.py::test_in_range_draws_give_one_run -- so the end-to-end tests never reach the sort's
cross-run code, and they look at a handful of the 100,000 table entries.  The case table is genesis_restate.BEZIER_CASES, whose run
categories are proved on the CPU restatement in tests/test_cpu_genesis.py.

Every bound here is derived (the docstrings say how) or is exact equality."""
import numpy as np
import pytest
import torch

import genesis_restate as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NT = R.NT
PREFILL = 0x7FF80000DEADBEEF          # a NaN no arithmetic produces: a table entry that still holds it was never written
GROUPS = ("ordinary", "three", "seam", "fewulp", "overflow")
SEG_H, SEG_W = 96, 352                # 33,792 words: two row segments (93 + 3 rows), so minmax holds two entries per image


def _mods():
    from cmunet_amd import _lib, genesis, ops
    return _lib, genesis, ops


def ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _dev(arr):
    arr = np.ascontiguousarray(arr)
    return torch.from_numpy(arr.view(np.uint8) if arr.dtype.names else arr).reshape(-1).to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------------
# Bezier tables
# ------------------------------------------------------------------------------------------------------------------------------------
class Tables:
    """One launch of cmu_genesis_bezier per group of BEZIER_CASES (several records each; the last group carries one more record
    without GF_NONLIN), into slices of one workspace that starts as PREFILL everywhere; each launch has its own error word.  minmax
    has two segments per image: (mn, mn) and (mx, mx), so the controls come from the minimum / maximum over the segments."""

    def __init__(self, sorty):
        _lib, G, ops = _mods()
        self.sorty = sorty
        self.cases = sorted(R.BEZIER_CASES, key=lambda c: GROUPS.index(c[0]))
        B = len(self.cases) + 1
        self.B, self.idle = B, B - 1
        recs = np.zeros(B, G.REC_DTYPE)
        minmax = np.zeros((B, 2, 2), np.float32)
        for b, (_, _, mn, mx, bez, _, _) in enumerate(self.cases):
            recs[b]["flags"] = G.GF_NONLIN | (G.GF_SORTY if sorty else 0)
            recs[b]["bez"] = bez
            minmax[b] = [[mn, mn], [mx, mx]]
        recs[self.idle]["bez"] = (0.3, 0.6, 0.2, 0.9)       # no GF_NONLIN: its tables are not written
        minmax[self.idle] = [[-1.0, -1.0], [1.0, 1.0]]
        assert _lib.lib().cmu_genesis_segments(SEG_H, SEG_W) == 2
        assert _lib.lib().cmu_genesis_bezier_ws_bytes(B) == B * 4 * NT * 8
        self.recs, self.minmax = _dev(recs), _dev(minmax)
        self.ws = torch.full((B * 4 * NT,), PREFILL, dtype=torch.int64, device=DEV)
        self.err = torch.zeros(len(GROUPS), dtype=torch.int32, device=DEV)
        rb = G.REC_DTYPE.itemsize
        self.group_of = {}
        for g, name in enumerate(GROUPS):
            idx = [b for b in range(B - 1) if self.cases[b][0] == name]
            b0, n = idx[0], len(idx)
            assert idx == list(range(b0, b0 + n)) and n >= 3
            self.group_of.update({b: g for b in idx})
            if g == len(GROUPS) - 1:
                assert b0 + n == self.idle
                n += 1
                self.group_of[self.idle] = g
            _lib.call("cmu_genesis_bezier", ops._p(self.recs[b0 * rb:]), ops._p(self.minmax[b0 * 4:]), n, SEG_H, SEG_W,
                      ops._p(self.ws[b0 * 4 * NT:]), ops._p(self.err[g:]), ops._stream())
        torch.cuda.synchronize()
        self.host = self.ws.cpu().numpy().reshape(B, 4, NT)              # int64 bit patterns
        self.err_host = self.err.cpu().numpy()

    def table(self, b, which):
        """raw x, raw y, sorted x, sorted y (0 .. 3) of image b as fp64."""
        return self.host[b, which].view(np.float64)


@pytest.fixture(scope="module")
def tables():
    """sorty -> Tables, launched once and shared by the tests of this file (80 MB of tables each: released with the module)."""
    cache = {}

    def get(sorty):
        if sorty not in cache:
            cache[sorty] = Tables(sorty)
        return cache[sorty]
    yield get
    cache.clear()


CASE_IDS = [f"{c[0]}:{c[1]}" for c in sorted(R.BEZIER_CASES, key=lambda c: GROUPS.index(c[0]))]


@pytest.mark.parametrize("sorty", [False, True], ids=["sortx", "sortxy"])
@pytest.mark.parametrize("b", range(len(CASE_IDS)), ids=CASE_IDS)
def test_bezier_tables(tables, b, sorty):
    """Raw tables: per element within 16 * 2^-53 * max|P_i| of genesis_restate.bezier_kernel_order -- each Bernstein term carries at
    most 4 roundings (pow included), its product with P_i and the three additions add at most 4 more, against terms that sum to at
    most max|P_i|: 8 u per evaluation, and two evaluations are compared (measured on an MI355X: at most 0.38 of the bound over the
    table, the device's pow and its t = k * (1 / (NT - 1)) included).  Sorted tables: np.sort of the DEVICE's own raw table, bit for
    bit (x always; y with GF_SORTY -- without it the raw y table stays in t order and sorted y is not read).  The error word of the
    case's launch is 0, and the run count of the device's raw table lies in the case's category, which proves the path taken: one run,
    the rank merge across 2 .. 16 runs, or the general sort above 16.  A seam case has a run that starts on the named sample of a
    98-sample thread chunk, on the device's table."""
    T = tables(sorty)
    group, name, mn, mx, bez, cat_x, cat_y = T.cases[b]
    assert int(T.err_host[T.group_of[b]]) == 0, f"error word {int(T.err_host[T.group_of[b]]):#x} in the launch of group '{group}'"
    for which, P, cat in zip((0, 1), R.controls(mn, mx, bez), (cat_x, cat_y)):
        raw = T.table(b, which)
        assert not (T.host[b, which] == PREFILL).any(), "raw table not fully written"
        ref = R.bezier_kernel_order(P)
        bound = 16 * 2.0 ** -53 * np.abs(P).max()
        err = np.abs(raw - ref).max()
        n, bnd = R.runs(raw)
        print(f"[genesis-tables] {group}:{name} {'xy'[which]} sorty {int(sorty)}: runs {n}, raw err / bound {err / bound if bound else 0:.3f}")
        assert err <= bound, f"{'xy'[which]}: {err:.3e} > {bound:.3e}"
        assert R.in_category(n, cat), f"{'xy'[which]}: {n} runs on the device's table, expected '{cat}'"
        if group == "seam" and cat == "few":
            assert int(name) in (bnd % R.CHUNK).tolist(), (name, bnd)
        if which == 0 or sorty:
            got, want = T.host[b, 2 + which], np.sort(raw).view(np.int64)
            diff = np.nonzero(got != want)[0]
            assert diff.size == 0, (f"sorted {'xy'[which]} ({n} runs) differs from np.sort at {diff.size} entries, first {int(diff[0])}"
                                    + (" (never written)" if (got == PREFILL).any() else ""))


@pytest.mark.parametrize("sorty", [False, True], ids=["sortx", "sortxy"])
def test_bezier_leaves_images_without_the_transform_alone(tables, sorty):
    T = tables(sorty)
    assert (T.host[T.idle] == PREFILL).all()


def test_chunk_seam_is_reached_on_the_device(tables):
    """At least one three-run table has a run that starts on the first or the last sample of a thread's chunk (index mod 98 in {0, 97})."""
    T = tables(True)
    hit = set()
    for b, c in enumerate(T.cases):
        if c[0] == "seam":
            n, bnd = R.runs(T.table(b, 0))
            assert n == 3
            hit |= set((bnd % R.CHUNK).tolist())
    assert hit & {0, 97}, hit


# ------------------------------------------------------------------------------------------------------------------------------------
# np.interp
# ------------------------------------------------------------------------------------------------------------------------------------
def _interp_inputs(T, b, n, rng):
    """n float32 pixels chosen against the device's tables of image b: below xs[0] and above xs[-1]; exactly mn and mx; interior nodes
    that are float32 values; every float32 in [mn, mx] where these are few; random values from a range 10 % wider than [mn, mx]."""
    _, _, mn, mx, _, _, _ = T.cases[b]
    xs = T.table(b, 2)
    f = np.float32
    lo, hi = f(xs[0]), f(xs[-1])
    if lo >= xs[0]:
        lo = np.nextafter(lo, f(-np.inf))
    if hi <= xs[-1]:
        hi = np.nextafter(hi, f(np.inf))
    assert lo < xs[0] and hi > xs[-1]
    special = [lo, f(lo - 1), f(-3e38), f(-np.inf), hi, f(hi + 1), f(3e38), f(np.inf), mn, mx, f(xs[0]), f(xs[-1])]
    inner = xs[1:-1]
    nodes = np.unique(inner[inner.astype(f).astype(np.float64) == inner]).astype(f)[:64]
    every = []
    v = f(mn)
    while v <= mx and len(every) <= 8:
        every.append(v)
        v = np.nextafter(v, f(np.inf))
    if len(every) > 8:
        every = []
    d = np.float64(mx) - np.float64(mn)
    rand = (np.float64(mn) - 0.1 * d + rng.random_sample(n) * 1.2 * d).astype(f)
    head = np.concatenate([np.array(special, f), nodes, np.array(every, f)])
    x = np.concatenate([head, rand])[:n]
    assert len(x) == n and n - len(head) >= 4096
    return x, len(nodes), len(every)


@pytest.mark.parametrize("sorty", [False, True], ids=["sortx", "sortxy"])
@pytest.mark.parametrize("H,W", [(320, 320), (67, 71)], ids=["102400px", "4757px"])
def test_interp_matches_numpy_on_the_device_tables(tables, H, W, sorty):
    """cmu_genesis_intensity_paint in paint mode 0 against np.interp(x, xs, ys) on the DEVICE's own tables (ys = sorted y with
    GF_SORTY, else the raw y in t order): 0 ulp, because the kernel restates numpy's arr_interp operation for operation (last index
    with xs[j] <= x; the exact-hit, last-node and below / above branches; slope * (x - xs[j]) + ys[j] with its two NaN fall-backs) under
    -ffp-contract=off.  320 x 320 has more pixels than the table has nodes (numpy then precomputes the slopes), 67 x 71 fewer."""
    _lib, G, ops = _mods()
    T = tables(sorty)
    rng = np.random.RandomState(H + 2 * int(sorty))
    x = np.empty((T.B, H * W), np.float32)
    exact_nodes = few = 0
    for b in range(T.B - 1):
        x[b], nn, ne = _interp_inputs(T, b, H * W, rng)
        exact_nodes += nn
        few += ne > 0
    x[T.idle] = rng.standard_normal(H * W)
    assert exact_nodes > 0 and few >= 7          # the few-step, one-step and constant ranges are walked value by value
    xd = _dev(x)
    _lib.call("cmu_genesis_intensity_paint", ops._p(T.recs), ops._p(T.ws), None, 0, 0, ops._p(xd), T.B, H, W, ops._stream())
    got = xd.cpu().numpy().reshape(T.B, H * W)
    assert (got[T.idle].view(np.int32) == x[T.idle].view(np.int32)).all()
    worst = 0
    for b in range(T.B - 1):
        ys = T.table(b, 3 if sorty else 1)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ref = np.interp(x[b].astype(np.float64), T.table(b, 2), ys).astype(np.float32)
        nan = np.isnan(ref)
        assert (np.isnan(got[b]) == nan).all(), T.cases[b][:2]
        u = ulps(got[b][~nan], ref[~nan])
        worst = max(worst, int(u.max()))
        assert u.max() == 0, f"{T.cases[b][0]}:{T.cases[b][1]}: {int((u > 0).sum())} pixels differ from np.interp, worst {int(u.max())} ulp"
    print(f"[genesis-tables] interp {H}x{W} sorty {int(sorty)}: worst {worst} ulp over {T.B - 1} tables, {exact_nodes} exact interior nodes")


# ------------------------------------------------------------------------------------------------------------------------------------
# gather, flip, local shuffle
# ------------------------------------------------------------------------------------------------------------------------------------
def _hand_blocks(H, W, R_, sx, sy):
    """Twelve hand-made blocks (x0, y0, bx, by) and the block that overlaps number 3.  R_: rows per segment (the seam between the
    first two, if there is a second).  Sizes shrink with the permutation slot sx * sy (42 at 96 x 352, 4 at 64 x 64)."""
    big = sx * sy >= 15
    seam = min(R_, H - 2)
    tall, ov, wide = ((3, 4), (3, 5), (2, 6)) if big else ((2, 2), (2, 2), (1, 4))
    hand = [
        (seam - 1, 5) + tall,                                            # 0 straddles the segment seam (rows seam-1 ..)
        (H - 2, W - 3, 2, 3) if big else (H - 2, W - 2, 2, 2),           # 1 ends on the last row and the last column
        (10, 10) + ov,                                                   # 2 loses to 5 at (11, 11)
        (20, 30) + wide,                                                 # 3 loses to the extra block
        (40, 3, 1, 1),                                                   # 4 a 1 x 1 block
        (11, 11) + ov,                                                   # 5 overlaps 2
        (0, 0, sx, sy),                                                  # 6 a block of slot size, in the first row and column
        (30, 40, 2, 2),                                                  # 7 loses to 8 at (31, 41)
        (31, 41, 2, 2),                                                  # 8 overlaps 7
        (seam - 2, 20, 2, 7) if big else (seam - 2, 20, 2, 2),           # 9 ends on the last row of the first segment
        (min(seam, H - 1), 30, 1, 5) if big else (seam, 30, 1, 4),       # 10 starts on the first row of the second segment
        (50, W - 1, 3, 1),                                               # 11 a column on the last column
    ]
    return hand, (20, 32, 2, 5) if big else (20, 32, 2, 2)


@pytest.mark.parametrize("flips", [(0, 1, 2), (3, 2, 1)], ids=["flips012", "flips321"])
@pytest.mark.parametrize("H,W", [(96, 352), (64, 64)], ids=["96x352", "64x64"])
def test_gather_flip_shuffle_with_hand_made_blocks(H, W, flips):
    """x, y and minmax of cmu_genesis_gather_shuffle against genesis_restate.flip / shuffle and numpy's min / max per band, bit for bit.
    96 x 352 is 33,792 words: two row segments of 93 and 3 rows (non-square, ragged); 64 x 64 is one.  B = 3 images with different
    ``src`` indices and block / permutation offsets; twelve hand-made blocks each (_hand_blocks).  The last image carries 1,027 blocks:
    blocks 12 .. 1025 are 1 x 1 fillers, and block 1026 -- handled by thread 2 -- overlaps block 3 and must win although its thread
    id is the lower one.  All four flip parities over the two parametrisations."""
    _lib, G, ops = _mods()
    rng = np.random.RandomState(H + flips[0])
    N, B = 4, 3
    nseg = _lib.lib().cmu_genesis_segments(H, W)
    R_ = H if H < 32768 // W else 32768 // W
    assert nseg == -(-H // R_) == (2 if H == 96 else 1)
    sx, sy = H // 25, W // 25
    slot = sx * sy
    src = rng.standard_normal((N, H, W)).astype(np.float32)
    hand, extra = _hand_blocks(H, W, R_, sx, sy)
    counts = [12, 9, 1027]
    offs = np.concatenate([[0], np.cumsum(counts)])
    blocks = np.zeros((offs[-1], 4), np.int16)
    perms = np.zeros((offs[-1], slot), np.uint8)
    recs = np.zeros(B, G.REC_DTYPE)
    for b in range(B):
        bl = list(hand[:counts[b]])
        if counts[b] > 12:
            free = np.array([p for p in range(H * W) if p // W not in (10, 11, 20, 21, 30, 31)])       # the pixels the last assertion names
            fill = rng.permutation(free)[:counts[b] - 13]
            bl += [(int(p) // W, int(p) % W, 1, 1) for p in fill] + [extra]
        for k, (x0, y0, bx, by) in enumerate(bl):
            assert 0 <= x0 and x0 + bx <= H and 0 <= y0 and y0 + by <= W and 1 <= bx * by <= slot, (k, x0, y0, bx, by)
            blocks[offs[b] + k] = (x0, y0, bx, by)
            perms[offs[b] + k, :bx * by] = rng.permutation(bx * by)
        recs[b]["src"], recs[b]["flags"] = (2, 0, 3)[b], flips[b] | G.GF_LOCAL
        recs[b]["nblocks"], recs[b]["slot"] = counts[b], slot
        recs[b]["block_off"], recs[b]["perm_off"] = offs[b], offs[b] * slot
    x = torch.full((B, H, W), float("nan"), device=DEV)
    y = torch.full((B, H, W), float("nan"), device=DEV)
    mm = torch.full((B * nseg * 2,), float("nan"), device=DEV)
    assert (recs["src"] < N).all() and (recs["block_off"] + recs["nblocks"] <= len(blocks)).all() and (recs["perm_off"] == recs["block_off"] * slot).all()
    src_d, recs_d, blocks_d, perms_d = _dev(src), _dev(recs), _dev(blocks), _dev(perms)      # (kept alive until the results are read)
    _lib.call("cmu_genesis_gather_shuffle", ops._p(src_d), ops._p(recs_d), ops._p(blocks_d), ops._p(perms_d), ops._p(x), ops._p(y), ops._p(mm),
              B, H, W, ops._stream())
    x, y, mm = x.cpu().numpy(), y.cpu().numpy(), mm.cpu().numpy().reshape(B, nseg, 2)
    for b in range(B):
        want_y = R.flip(src[int(recs[b]["src"])], flips[b])
        bl, pm = blocks[offs[b]:offs[b + 1]], perms[offs[b]:offs[b + 1]]
        want_x = R.shuffle(want_y, bl, pm)
        assert (y[b].view(np.int32) == want_y.view(np.int32)).all(), b
        bad = np.argwhere(x[b].view(np.int32) != want_x.view(np.int32))
        assert bad.size == 0, f"image {b}: {len(bad)} pixels differ, first at {bad[0].tolist()}"
        assert (want_x != want_y).any()                           # the blocks do move pixels
        for s in range(nseg):
            band = want_x[s * R_:min(H, (s + 1) * R_)]
            assert mm[b, s, 0].tobytes() == band.min().tobytes() and mm[b, s, 1].tobytes() == band.max().tobytes(), (b, s)
    # the overlaps decide as stated: the pixel both blocks of a pair cover reads through the higher-numbered one's permutation
    own = np.full((H, W), -1)
    for k, (x0, y0, bx, by) in enumerate(blocks[offs[2]:offs[3]].astype(int)):
        own[x0:x0 + bx, y0:y0 + by] = k
    assert own[11, 11] == 5 and own[10, 10] == 2 and own[31, 41] == 8 and own[30, 40] == 7 and own[20, 32] == 1026 and own[20, 30] == 3


# ------------------------------------------------------------------------------------------------------------------------------------
# MSE
# ------------------------------------------------------------------------------------------------------------------------------------
_MSE_DATA = {}


def _mse_data(B, H, W):
    """Logits (3 channels: the K = 1, 2 tests take the first ones' storage anew), target and the fp64 reference, computed once."""
    if (B, H, W) not in _MSE_DATA:
        g = torch.Generator().manual_seed(B * 7 + H)
        l0, y = torch.randn(B, H, W, generator=g), torch.randn(B, H, W, generator=g)
        d = (l0 - y).numpy()                                           # float32 differences, rounded as the kernel rounds them
        _MSE_DATA[(B, H, W)] = (l0, y, d, float(np.mean(d.astype(np.float64) ** 2)), g)
    return _MSE_DATA[(B, H, W)]


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 40, 56), (17, 512, 512)], ids=["1x1x1", "3x40x56", "17x512x512"])
def test_mse_fwd_bwd_bits(B, H, W, K):
    """cmu_mse_fwd_bwd for K = 1, 2, 3 channels, loss_scale 1 and 1024, with and without an AMP state of scale 2^14, and with
    ``dlogits`` NULL.  17 x 512 x 512 is 4,456,448 elements: more than MSE_MAX_BLOCKS x 4,096, so the grid is capped and workgroups
    take a second trip.  Gradient of channel 0: bit for bit float32(k) * float32(l - y) with k = float32(2 * scale) / float32(n) in
    float32; channels 1 .. K-1: exactly zero.  Loss: within 1 float32 ulp of the fp64 mean of the squared float32 differences (the
    kernel sums the same fp64 squares, in another order: n * 2^-53 relative at worst, far below the rounding to float32)."""
    _lib, G, ops = _mods()
    l0, y, d, ref, g = _mse_data(B, H, W)
    n = B * H * W
    assert (n > 1024 * 4096) == (B == 17)
    logits = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(K))
    logits[:, 0] = l0
    ld, yd = logits.to(DEV), y.to(DEV)
    ref32 = np.float32(ref)
    first = None
    for loss_scale in (1.0, 1024.0):
        for amp_scale in (None, 2.0 ** 14):
            amp = None if amp_scale is None else ops.AmpScaler(DEV, init_scale=amp_scale)
            loss = torch.full((1,), float("nan"), device=DEV)
            dl = torch.full((B, K, H, W), float("nan"), device=DEV)
            G.mse_fwd_bwd(ld, yd, loss, dl, loss_scale, amp)
            k = np.float32(2.0 * loss_scale * (amp_scale or 1.0)) / np.float32(n)
            assert k.dtype == np.float32
            want = k * d
            got = dl.cpu().numpy()
            assert (got[:, 0].view(np.int32) == want.view(np.int32)).all(), (loss_scale, amp_scale)
            assert (got[:, 1:].view(np.int32) == 0).all(), "channels 1 .. K-1 must be +0"
            lv = loss.cpu().numpy()
            assert ulps(lv, np.array([ref32])).max() <= 1, (float(lv[0]), ref)
            first = lv if first is None else first
            assert lv.tobytes() == first.tobytes()                    # the loss does not depend on the scales
    loss2 = torch.full((1,), float("nan"), device=DEV)
    G.mse_fwd_bwd(ld, yd, loss2, None, 1024.0, None)
    assert loss2.cpu().numpy().tobytes() == first.tobytes()
    assert torch.equal(ld.cpu(), logits)                              # the logits are only read
