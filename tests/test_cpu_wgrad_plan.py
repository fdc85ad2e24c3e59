"""CPU suite: the host side of the convolution library that needs no device.

1. The weight-gradient plan (csrc/conv_wgrad.hip: WG_FORMS, wg_plan, wg_ws_bytes) through its three host-only queries --
   cmu_conv3x3_wgrad_ws_bytes, cmu_convT2x2_wgrad_ws_bytes, cmu_conv3x3_wgrad_tile_h -- against the rule restated in conv_exact_gpu.py
   (wgrad3_ws_bytes, wgradT_ws_bytes, wgrad3_tile_h), over a grid of shapes and dtypes and under the knobs the rule reads.
2. The refusals of the shared activation-view check (csrc/common.h: cmu_check_act) at every entry point that runs it.  Every call is
   refused before anything touches a device: no pointer passed here is valid, and a second view of each entry stays null.
On the library that test_cpu_abi builds.  No GPU call anywhere."""
import os
import re

import pytest

import conv_exact_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": 0, "f16": 1, "bf16": 2}
CMU_ERR_ARG = -1

BATCH = (1, 2, 3)
IMAGE = ((4, 16), (8, 16), (16, 16), (24, 40), (64, 64))
CHANNELS = ((8, 8), (24, 40), (64, 64), (64, 128), (128, 64), (128, 128), (64, 192), (192, 64), (96, 64), (256, 128), (128, 256))
KNOBS = ([{}] + [{k: 0} for k in ("WGRAD_WIDE", "WGRAD_SWAP", "WGRAD_SQUARE", "WGRAD_WIDE_F32", "WGT2_NX256")] +
         [{"WGRAD_BLOCKS": v} for v in (8, 64, 4096)] + [{"WGRAD_BLOCKS1": v} for v in (8, 4096)])
PAST_RANGE = (1, 4096, 4096, 64, 64)     # one f16 image of dY is 2^31 bytes: past a buffer descriptor's range


@pytest.fixture(scope="module")
def l():
    from cmunet_amd import _lib
    _lib.build()
    return _lib.lib()


def plan_rows(l):
    """(knobs, shape, dtype, library's (ws3, wsT, tile_h), restated (ws3, wsT, tile_h)) over the grid; every override is reset."""
    base = G.library_knobs()
    rows = []
    for kn in KNOBS:
        for k, v in kn.items():
            assert l.cmu_set_dispatch_override(("CMU_" + k).encode(), v) == 0
        try:
            shapes = [(B, H, W, Cin, Cout) for B in BATCH for H, W in IMAGE for Cin, Cout in CHANNELS]
            for shape in shapes + ([PAST_RANGE] if not kn else []):
                for dt in (("f16",) if shape == PAST_RANGE else DT):
                    case = {"shape": shape, "knobs": kn}
                    got = (l.cmu_conv3x3_wgrad_ws_bytes(*shape, DT[dt]), l.cmu_convT2x2_wgrad_ws_bytes(*shape, DT[dt]),
                           l.cmu_conv3x3_wgrad_tile_h(*shape, DT[dt]))
                    want = (G.wgrad3_ws_bytes(case, dt, base), G.wgradT_ws_bytes(case, dt, base), G.wgrad3_tile_h(case, dt, base))
                    rows.append((kn, shape, dt, got, want))
        finally:
            for k in kn:
                assert l.cmu_set_dispatch_override(("CMU_" + k).encode(), -1) == 0
    return rows


def test_plan_queries_equal_the_restated_rule(l):
    rows = plan_rows(l)
    assert len(rows) == len(KNOBS) * len(BATCH) * len(IMAGE) * len(CHANNELS) * len(DT) + 1
    bad = [r for r in rows if r[3] != r[4]]
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; first (knobs, shape, dtype, library, restated): {bad[0]}"
    # the grid reaches both answers of the tile-height query, and the shape past the buffer range falls back to 16 x 16 tiles
    assert {r[3][2] for r in rows} == {8, 16}
    assert [r[3][2] for r in rows if r[1] == PAST_RANGE] == [16]
    assert G.wgrad3_tile_h({"shape": (1, 64, 64, 64, 64), "knobs": {}}, "f16", G.library_knobs()) == 8


def test_plan_queries_refuse_bad_arguments(l):
    for q in (l.cmu_conv3x3_wgrad_ws_bytes, l.cmu_convT2x2_wgrad_ws_bytes, l.cmu_conv3x3_wgrad_tile_h):
        assert q(1, 16, 16, 64, 64, 3) == -1 and q(0, 16, 16, 64, 64, 1) == -1 and q(1, 16, 16, 0, 64, 1) == -1


# entry -> (the view under test: tensor, its stride, its channel count; pointers an earlier check of the entry wants non-null).  The view is
# the first one the entry checks; in the weight-gradient, cells and cmu_bn_bwd_* entries that check is the very first statement.
FAKE = 0x1000          # aligned, never dereferenced: every call below is refused
ENTRIES = {
    "cmu_conv3x3_fwd": ("x", "ldx", "Cin", ()), "cmu_convT2x2_fwd": ("x", "ldx", "Cin", ()),
    "cmu_convT2x2_dgrad": ("dOut", "ldd", "Cout", ()), "cmu_conv3x3_fwd_tiles": ("x", "ldx", "Cin", ("tile_list", "tile_count")),
    "cmu_conv3x3_fwd_rows": ("x", "ldx", "Cin", ("rows", "n_rows")), "cmu_conv3x3_dgrad_bn": ("dY", "ldd", "K", ()),
    "cmu_convT2x2_dgrad_bn": ("dOut", "ldd", "Cout", ()),
    "cmu_conv3x3_wgrad": ("x", "ldx", "Cin", ()), "cmu_conv3x3_wgrad_tiles": ("x", "ldx", "Cin", ()), "cmu_convT2x2_wgrad": ("x", "ldx", "Cin", ()),
    "cmu_bn_bwd_apply_cells": ("dA", "ldd", "C", ()), "cmu_mask_select_cells": ("x", "ldx", "C", ()), "cmu_maxpool_bwd_cells": ("dP", "ldp", "C", ()),
    "cmu_cells_channel_sum": ("x", "ldx", "C", ()), "cmu_cells_channel_stats": ("x", "ldx", "C", ()), "cmu_bn_bwd_reduce_cells": ("dA", "ldd", "C", ()),
    "cmu_bn_bwd_reduce": ("dA", "ldd", "C", ()), "cmu_bn_bwd_reduce_masked": ("dA", "ldd", "C", ()), "cmu_bn_bwd_reduce_rows": ("dA", "ldd", "C", ()),
    "cmu_bn_bwd_apply": ("dA", "ldd", "C", ()), "cmu_bn_bwd_apply_masked": ("dA", "ldd", "C", ()),
    "cmu_maxpool_bwd": ("dP", "ldp", "C", ()), "cmu_maxpool_bwd2": ("dP", "ldp", "C", ()),
    "cmu_maxpool_bwd_masked": ("dP", "ldp", "C", ("active", "dA", "scale", "shift")),
    "cmu_maxpool_bwd_apply": ("dP", "ldp", "C", ("scale", "shift", "save_mean", "save_invstd", "coef", "dY")),
}
# f16: chunks of 8 elements.  (tensor, C, ld, dtype) of each refusal
REFUSALS = {"null": (0, 64, 64, 1), "unaligned": (FAKE + 8, 64, 64, 1), "C % chunk": (FAKE, 60, 64, 1), "ld < C": (FAKE, 64, 56, 1),
            "ld % chunk": (FAKE, 64, 68, 1), "dtype": (FAKE, 64, 64, 3)}
INTS = {"B": 1, "H": 16, "W": 16, "f": 1, "tile_h": 16, "max_rows": 1, "count": 1}


def parameters(name):
    """[(is a pointer, name)] of the entry's prototype in the header."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(ROOT, "include", "cmunet_hip.h")).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, src).group(1).split(",")
    return [("*" in p, p.replace("*", " ").split()[-1]) for p in params]


def test_every_entry_of_the_view_check_is_listed():
    src = "".join(open(os.path.join(ROOT, "cmunet_amd", "csrc", f)).read() for f in ("conv_igemm.hip", "conv_wgrad.hip", "sparse_elem.hip",
                                                                                   "backward_elem.hip"))
    named = set(re.findall(r"(?:check_act|wg_check|check_cells_act|check_pair)\(\"(cmu_\w+)", src))
    assert named == set(ENTRIES)


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_view_check_refuses(l, what):
    tensor, C, ld, dt = REFUSALS[what]
    for name, (view, ldname, cname, wanted) in ENTRIES.items():
        args = []
        for pointer, p in parameters(name):
            if pointer:
                args.append(tensor if p == view else FAKE if p in wanted else 0)
            elif p == "dt":
                args.append(dt)
            elif p == ldname:
                args.append(ld)
            elif p == cname:
                args.append(C)
            elif p.startswith("ld") or p in ("C", "Cin", "Cout", "K", "N"):
                args.append(64)
            else:
                args.append(INTS.get(p, 0))
        assert getattr(l, name)(*args) == CMU_ERR_ARG, (name, what)
        entry = "cmu_maxpool_bwd" if name == "cmu_maxpool_bwd2" else name
        assert l.cmu_last_error().decode().startswith(entry), (name, what, l.cmu_last_error())
