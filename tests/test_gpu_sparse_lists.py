"""The device-side list builders of the SparK step (``cmu_sparse_tile_list(s)``, ``cmu_sparse_pixel_list(s)``: conv_igemm.hip) against
numpy -- never one builder against the other.  Tile lists: totals around every threshold of the bit-run extraction (one tile per thread
up to 1,024 tiles; 2 ... 64 consecutive tiles per thread, whose run of bits starts anywhere in a 64-bit word and may span two; a second
and a third trip past 65,536 tiles), patch maps that are full, empty, alternating, random and active in the last tile only, tiles that
span several patches, patches that span several tiles, a tile that reaches past the level's edge.  Pixel lists: patches of one pixel,
capacities above, equal to and below the number of active pixels.  Every list is prefilled with a sentinel that the entries past the
count (tile lists) or past the capacity (pixel lists) must keep.  Exact comparisons only."""
import numpy as np
import pytest
import torch

import conv_exact_ref as R

pytestmark = pytest.mark.gpu
SENT = -7


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as O
    return O


def tile_list_ref(act, H, th, tw):
    """Ascending ids (b * tilesY + ty) * tilesX + tx of the tiles that hold a pixel of an active patch (numpy, from the pixel map)."""
    a = act.numpy()
    B, f = a.shape[0], a.shape[-1]
    px = np.repeat(np.repeat(a, H // f, 1), H // f, 2)
    tY, tX = -(-H // th), -(-H // tw)
    pad = np.zeros((B, tY * th, tX * tw), dtype=a.dtype)
    pad[:, :H, :H] = px
    on = pad.reshape(B, tY, th, tX, tw).max(axis=(2, 4)).reshape(-1)
    return np.nonzero(on)[0].astype(np.int32), B * tY * tX


def maps_of(B, f, seed):
    n = B * f * f
    g = torch.Generator().manual_seed(seed)
    full, none = torch.ones(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
    alt = (torch.arange(n) % 2).to(torch.uint8)
    rnd = (torch.rand(n, generator=g) < 0.25).to(torch.uint8)
    last = none.clone()
    last[-1] = 1
    return {k: v.view(B, f, f) for k, v in (("all", full), ("none", none), ("alternating", alt), ("random", rnd), ("last", last))}


def build_tile_list(ops, act, H, th, tw, batched):
    tl = ops.TileList(act, H, H, th, tw, defer=True)
    tl.list.fill_(SENT)
    tl.count.fill_(SENT)
    if batched:
        ops.build_lists(act, [tl])
    else:
        B, f = act.shape[0], act.shape[-1]
        ops.call("cmu_sparse_tile_list", ops._p(act), f, B, H, H, th, tw, ops._p(tl.list), ops._p(tl.count), ops._stream())
    return tl


def check_tile_list(ops, act, H, th, tw, what):
    ref, dense = tile_list_ref(act, H, th, tw)
    for batched in (False, True):
        tl = build_tile_list(ops, act.cuda(), H, th, tw, batched)
        got = tl.list.cpu().numpy()
        n = int(tl.count.item())
        assert tl.n_dense == dense == len(got)
        assert n == len(ref), (what, batched, n, len(ref))
        assert np.array_equal(got[:n], ref), (what, batched, int(np.nonzero(got[:n] != ref)[0][0]))
        assert (got[n:] == SENT).all(), (what, batched, "an entry past the count was written")


@pytest.mark.parametrize("total", [1, 1023, 1024, 1025, 3 * 1024 + 5, 40000, 65536, 65537, 140001])
def test_tile_list_totals_around_the_run_and_trip_thresholds(ops, total):
    """B = total, H = f = 1, 1 x 1 tiles: one tile per image, so the total is free.  1,024 threads take ceil(total / 1024) (at most 64)
    consecutive tiles each: 2, 4, 40 (a run that starts inside a word and spans two), 64, and with 65,537 and 140,001 tiles a second and
    a third trip."""
    for name, act in maps_of(total, 1, total).items():
        check_tile_list(ops, act, 1, 1, 1, name)


@pytest.mark.parametrize("geom", [(3, 8, 16, 4, 8), (3, 8, 16, 16, 16), (2, 2, 32, 8, 16), (5, 2, 64, 16, 32), (3, 6, 24, 16, 32), (2, 6, 24, 8, 16),
                                  (7, 12, 48, 16, 16), (40, 8, 64, 8, 16)])
def test_tile_list_geometries(ops, geom):
    """(B, f, H, th, tw): tiles that span several patches (2-pixel patches under 4 x 8 and 16 x 16 tiles), patches that span several tiles,
    tiles that reach past the edge of a 24-pixel level (16 x 32 and 8 x 16 tiles: the patches a tile overlaps stop at f), a patch map
    whose side is no power of two, and 1,280 tiles (two per thread) of a real geometry."""
    B, f, H, th, tw = geom
    for name, act in maps_of(B, f, sum(geom)).items():
        check_tile_list(ops, act, H, th, tw, name)


def test_build_lists_fills_more_lists_than_one_launch_holds_against_numpy(ops):
    from cmunet_amd import _lib
    mx = _lib.lib().cmu_sparse_tile_lists_max()
    B, f = 3, 8
    act = R.patch_map(B, f, 19, 3)
    specs = [(256, 16, 32), (256, 16, 16), (128, 8, 16), (64, 16, 32), (32, 4, 4), (256, 8, 16), (128, 16, 32), (64, 8, 16), (16, 2, 2), (8, 1, 1),
             (512, 16, 32), (512, 16, 16), (512, 8, 16), (64, 16, 16), (8, 16, 32)]
    assert len(specs) > mx
    tls = [ops.TileList(act.cuda(), H, H, th, tw, defer=True) for H, th, tw in specs]
    for t in tls:
        t.list.fill_(SENT)
    sides = [256, 128, 64, 32, 16, 8, 8, 16, 32, 64, 128, 256, 8, 16]
    assert len(sides) > mx
    pls = [ops.PixelList(act.cuda(), H, H, max_rows=19 * B * (H // f) ** 2 + 100 * (i % 3), defer=True) for i, H in enumerate(sides)]
    for p in pls:
        p.rows.fill_(SENT)
    cells = ops.build_lists(act.cuda(), tls, pls)
    assert int(cells.count.item()) == 19 * B
    for t, (H, th, tw) in zip(tls, specs):
        ref, _ = tile_list_ref(act, H, th, tw)
        n = int(t.count.item())
        got = t.list.cpu().numpy()
        assert n == len(ref) and np.array_equal(got[:n], ref) and (got[n:] == SENT).all(), (H, th, tw)
    for p, H in zip(pls, sides):
        ref = R.pixel_list_of(act, H).numpy()
        got = p.rows.cpu().numpy()
        assert int(p.count.item()) == len(ref) <= p.capacity and np.array_equal(got[:len(ref)], ref) and (got[len(ref):] == -1).all(), H


def pixel_list(ops, act, H, cap, batched):
    """A list of ``cap`` rows inside a buffer with 64 sentinel entries behind it -> (rows with the tail, count)."""
    pl = ops.PixelList(act, H, H, defer=True)
    buf = torch.full((cap + 64,), SENT, dtype=torch.int32, device="cuda")
    pl.rows, pl.capacity = buf[:cap], cap
    pl.count.fill_(SENT)
    if batched:
        ops.build_lists(act, (), [pl])
    else:
        from cmunet_amd import _lib
        B, f = act.shape[0], act.shape[-1]
        ws = torch.empty(_lib.lib().cmu_sparse_pixel_list_ws_bytes(B, f), dtype=torch.uint8, device="cuda")
        ops.call("cmu_sparse_pixel_list", ops._p(act), f, B, H, H, ops._p(pl.rows), cap, ops._p(pl.count), ops._p(ws), ops._stream())
    torch.cuda.synchronize()
    return buf.cpu().numpy(), int(pl.count.item())


@pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
@pytest.mark.parametrize("geom", [(3, 16, 16, 100), (2, 4, 32, 5), (2, 8, 64, 9), (1, 4, 64, 16), (2, 6, 24, 7), (2, 16, 16, 0)])
def test_pixel_list_capacities_above_equal_and_below_the_active_pixels(ops, geom, batched):
    """(B, f, H, active patches per image).  Patch-major order (conv_exact_ref.pixel_list_of: loops).  Capacity above n: padded with -1;
    equal to n; below n: the first ``capacity`` rows and a count of at most the capacity -- cmu_rows_channel_stats and
    cmu_bn_bwd_reduce_rows loop to the count and never see the capacity, so an overstated count would send them past the list.  Only the
    list and the count are read back here; no consumer runs on them.  Nothing behind the capacity is written."""
    B, f, H, keep = geom
    act = R.patch_map(B, f, keep, sum(geom))
    ref = R.pixel_list_of(act, H).numpy()
    n = len(ref)
    caps = sorted({n + 256, n + 1, n, n - 1, n // 2 + 1, 1} - {0, -1}) if n else [1, 256]
    for cap in caps:
        got, count = pixel_list(ops, act.cuda(), H, cap, batched)
        m = min(n, cap)
        assert count == m, f"capacity {cap}, {n} active pixels: the count is {count}"
        assert np.array_equal(got[:m], ref[:m]) and (got[m:cap] == -1).all(), cap
        assert (got[cap:] == SENT).all(), f"capacity {cap}: a row behind the capacity was written"
