"""What the exact GPU files (test_gpu_conv3x3_exact.py, test_gpu_convT_exact.py, test_gpu_wgrad_exact.py, and for the SparK list forms
test_gpu_conv_rows_exact.py, test_gpu_wgrad_tiles_exact.py) share: guard-banded buffers, the kernel tag of the last launch, bit
comparison, and the launchers' dispatch rules RESTATED from the C++ (conv_igemm3.inc, conv_igemm3p.inc, conv_igemm5.inc, conv_gemm.inc,
conv_gather.inc, conv_wgrad.hip) so that every case asserts the kernel and the template form it is named after.  The only comparison is
``torch.equal`` on the bits."""
import contextlib
import ctypes

import torch

import conv_exact_ref as R

IN_GUARD = 1024.0          # exact in every storage type: a read outside the channel slice that reaches a product changes the result


def torch_dt(dt):
    return R.TORCH_DT[dt]


def cu_count():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def last_kernel():
    from cmunet_amd import _lib
    lib = _lib.lib()
    lib.cmu_last_kernel.restype = ctypes.c_char_p
    return lib.cmu_last_kernel().decode()


@contextlib.contextmanager
def knobs(ops, case):
    """The case's dispatch overrides (keys of the CMU_KNOBS table of common.h without the CMU_ prefix)."""
    with contextlib.ExitStack() as st:
        for k, v in case["knobs"].items():
            st.enter_context(ops.dispatch_override("CMU_" + k, v))
        yield


def in_act(ops, x, dt, off, transform=None):
    """Input view: channels [off, off + C) of a buffer whose other channels (``off`` before, 8 behind when sliced) hold IN_GUARD."""
    B, H, W, C = x.shape
    ld = C if off == 0 else off + C + 8
    buf = torch.full((B, H, W, ld), IN_GUARD, dtype=torch_dt(dt), device="cuda")
    buf[..., off:off + C] = x.to(device="cuda", dtype=torch_dt(dt))
    a = ops.Act(buf, off, C)
    if transform is not None:
        sc, sh, rf = transform
        a = a.with_transform(sc.float().cuda().contiguous(), sh.float().cuda().contiguous(), rf)
    return a


def out_act(ops, B, H, W, C, dt, off):
    """Output view between NaN guard bands."""
    ld = C if off == 0 else off + C + 8
    buf = torch.full((B, H, W, ld), float("nan"), dtype=torch_dt(dt), device="cuda")
    return ops.Act(buf, off, C)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want.to(got.device)))


def check_out(act, want):
    """The view holds ``want`` bit for bit and every guard channel is still NaN."""
    o, C = act.coff, act.C
    got = act.buf[..., o:o + C]
    if not same_bits(got, want):
        bad = (bits(got) != bits(want.to(got.device))).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{len(bad)} of {got.numel()} outputs differ; first at (b, h, w, c) = {i}: got {float(got[i])}, exact {float(want[i])}")
    rest = torch.cat([act.buf[..., :o], act.buf[..., o + C:]], -1)
    assert bool(torch.isnan(rest).all()), "a store landed outside the channel slice"


def check_slab(got, want, what):
    assert not bool(torch.isnan(got).any()), f"{what}: a slab row was not written"
    if not torch.equal(got, want.to(got.device)):
        bad = (got != want.to(got.device)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} sums differ; first at {i}: got {float(got[i])}, exact {float(want.to(got.device)[i])}")


def nan_stats(ops, B, H, W, C):
    return torch.full_like(ops.new_stats(B, H, W, C, "cuda"), float("nan"))


def corner_channels(C, block):
    """First and last channel of the first and of the last ``block`` of C channels."""
    b = min(block, C)
    return sorted({0, b - 1, C - b, C - 1})


def seam_pixels(B, H, W):
    """(b, h, w) of the impulses: the first pixel, the last pixel of the last image (the last valid pixel of a partial tile when
    the image has one), and both sides of every 16-row / 16-column / 32-column tile seam the image has."""
    px = [(0, 0, 0), (B - 1, H - 1, W - 1)]
    if H > 16:
        px += [(0, 15, min(3, W - 1)), (B - 1, 16, min(5, W - 1))]
    for c in (16, 32):
        if W > c:
            px += [(B - 1, min(2, H - 1), c - 1), (0, min(7, H - 1), c)]
    if H > 16 and W > 16:
        px += [(0, 15, 15), (B - 1, 16, 16)]
    return sorted(set(px))


# ------------------------------------------------------------------------------------------------
# the launchers' rules, restated
# ------------------------------------------------------------------------------------------------
DEFAULTS = {"CONV_NARROW": 1, "CONV_SLIM": 1, "CONV_PERSIST_PART": 1, "CONV_V5": 1, "CONV_PERSIST": 1, "CONV_WRES": 1, "CONV_WIDE": 1,
            "CONV_V6": 0, "V5_MIN_K": 128, "V5_MIN_K_BST": 256, "CONVT_SMALL": 1, "CONVT_GEMM": 1, "CONVT_SMALL_STEPS": 4,
            "WGRAD_WIDE": 1, "WGRAD_SWAP": 1, "WGRAD_SQUARE": 1, "WGRAD_WIDE_F32": 1, "WGT2_NX256": 1, "WGR_VEC": 1,
            "WGRAD_BLOCKS1": 512, "WGRAD_BLOCKS": 256, "GATHER_NB": 0, "SPARK_GATHER": 1}
ES = {"f32": 4, "f16": 2, "bf16": 2}
_LIBRARY_KNOBS = {}


def library_knobs():
    """The value IN EFFECT of every knob the rules below read, asked of the library (cmu_get_dispatch_knob: the environment's value
    when a CMU_* variable is set on the machine, else the table's default), with no override set.  The table's own defaults must be
    the ones restated in DEFAULTS.  The GPU files pass this to the rules; without a GPU the rules fall back on DEFAULTS."""
    if not _LIBRARY_KNOBS:
        from cmunet_amd import _lib
        lib = _lib.lib()
        for name, dflt in DEFAULTS.items():
            v, d = ctypes.c_int(0), ctypes.c_int(0)
            assert lib.cmu_get_dispatch_knob(("CMU_" + name).encode(), ctypes.byref(v), ctypes.byref(d)) == 0, name
            assert d.value == dflt, f"CMU_{name}: the library's default is {d.value}, restated as {dflt}"
            _LIBRARY_KNOBS[name] = v.value
    return dict(_LIBRARY_KNOBS)


def knob_values(case, base):
    return dict(DEFAULTS if base is None else base, **case["knobs"])


def cdiv(a, b):
    return -(-a // b)


def conv3_rule(case, dt, cus, tf, bst, base=None):
    """conv3x3_fwd_t -> igemm3_eligible -> launch_igemm3_any: (kernel tag, template form) for a (B, H, W, K, N) launch with / without
    a pending transform (``tf``) and the BatchNorm-backward epilogue (``bst``)."""
    B, H, W, K, N = case["shape"]
    kn = knob_values(case, base)
    es = ES[dt]
    kc = 64 // es
    whole = H % 16 == 0 and W % 32 == 0
    persist = bool(kn["CONV_PERSIST"]) and (whole or bool(kn["CONV_PERSIST_PART"]))

    def narrow(tw):
        return bool(kn["CONV_NARROW"]) and N % 128 == 0 and 2 * B * cdiv(W, tw) * cdiv(H, 16) * (N // 128) <= cus

    c16 = cdiv(W, 16)
    slim = bool(kn["CONV_SLIM"]) and c16 % 2 == 1 and (c16 == 1 or (es == 4 and c16 <= 7 and B * cdiv(W, 32) * cdiv(H, 16) * cdiv(N, 128) >= cus))
    eligible = (kn["CONV_WIDE"] != 0 and not (N == 64 and kn["CONV_WIDE"] != 2 and not persist and K < 128) and not (tf and K > 1024)
                and N % 64 == 0 and (N <= 64 or N % 128 == 0) and K % kc == 0 and K >= kc)
    if not eligible:
        return "conv_igemm_kernel", {"TF": tf, "BST": bst}

    def one_tile():
        tw = 16 if slim else 32
        return "conv_igemm3_kernel", {"NB": 128 if N % 128 == 0 and not narrow(tw) else 64, "TW": tw, "TF": tf, "BST": bst}
    if not kn["CONV_PERSIST"]:
        return one_tile()
    assert not kn["CONV_V6"]
    if (es == 2 and kn["CONV_V5"] and not (tf and bst) and N % 128 == 0 and K % 64 == 0 and K >= kn["V5_MIN_K"]
            and not (bst and K < kn["V5_MIN_K_BST"]) and whole and not narrow(32)):
        return "conv_igemm5_kernel", {"TF": tf, "BST": bst}
    if (tf and bst) or K // (32 // es) < 4:
        return one_tile()
    nb = 128 if N % 128 == 0 and not narrow(32) else 64
    if not whole:
        if not kn["CONV_PERSIST_PART"] or slim:
            return one_tile()
        return "conv_igemm3p_kernel", {"NB": nb, "PART": True, "WRES": False, "TF": tf, "BST": bst}
    wres = nb == 64 and es == 2 and bool(kn["CONV_WRES"]) and N == 64 and K == 64
    return "conv_igemm3p_kernel", {"NB": nb, "PART": False, "WRES": wres, "TF": tf, "BST": bst}


def convT_rule(case, dt, dg, tf, base=None):
    """convT_fwd_t / convT_dgrad_t: the GEMM runs over N = 4 Cout columns (forward) or over K = 4 Cout (sub-pixel, channel) terms (data
    gradient); there a 128-byte K step must stay inside one sub-pixel position: (K / 4) % KSC == 0.  -> (kernel tag, form: the K steps -- None when K
    is no whole number of them -- and ``inside``)."""
    B, H, W, K, N = case["shape"]
    kn = knob_values(case, base)
    es = ES[dt]
    ksc = 128 // es
    Kg, Ng = (4 * K, N) if dg else (K, 4 * N)
    inside = (not dg) or (Kg // 4) % ksc == 0
    steps = Kg // ksc if Kg % ksc == 0 else None
    if (kn["CONVT_SMALL"] and es == 2 and Ng % 128 == 0 and steps is not None and steps <= kn["CONVT_SMALL_STEPS"] and inside
            and not (tf and Kg > 1024)):
        return "conv_gemm_s_kernel", {"steps": steps, "inside": inside}
    if kn["CONVT_GEMM"] and Ng % 256 == 0 and steps is not None and inside and not (tf and Kg > 1024):
        return "conv_gemm_kernel", {"steps": steps, "inside": inside}
    return "conv_igemm_kernel", {"steps": steps, "inside": inside}


def split_class(want, ntiles):
    """Split s walks the K tiles s, s + splits, ...: 'one' split; 'clamped' (the aim asked for more splits than there are tiles: one
    tile each); 'equal' (every split the same count); 'short' (the last splits one tile fewer)."""
    splits = max(1, min(want, ntiles))
    if splits == 1:
        return 1, "one"
    if want > ntiles:
        return splits, "clamped"
    return splits, "equal" if ntiles % splits == 0 else "short"


def wgrad3_rule(case, dt, base=None):
    """cmu_conv3x3_wgrad: CA = Cout, CB = Cin -> (kernel tag, form, splits, K tiles)."""
    B, H, W, CB, CA = case["shape"]
    kn = knob_values(case, base)
    es = ES[dt]
    wide = bool(kn["WGRAD_WIDE"])
    if wide and es == 2 and CA % 128 == 0 and CB % 64 == 0:
        kernel, form, th, nbase = "conv_wgrad2_kernel", {"SWAP": False}, 8, (CA // 128) * (CB // 64)
    elif wide and kn["WGRAD_SWAP"] and es == 2 and CA == 64 and CB % 128 == 0:
        kernel, form, th, nbase = "conv_wgrad2_kernel", {"SWAP": True}, 8, (CB // 128) * (CA // 64)
    elif wide and kn["WGRAD_SQUARE"] and es == 2 and CA % 64 == 0 and CB % 64 == 0:
        kernel, form, th, nbase = "conv_wgrad2s_kernel", {}, 8, (CA // 64) * (CB // 64)
    elif wide and kn["WGRAD_WIDE_F32"] and es == 4 and CA % 64 == 0 and CB % 64 == 0:
        nai = 4 if CA % 128 == 0 else 2
        kernel, form, th, nbase = "conv_wgrad2f_kernel", {"NAI": nai}, 4, (CA // (128 if nai == 4 else 64)) * (CB // 64)
    else:
        cw = 128 // es
        kernel, form, th, nbase = "conv_wgrad_kernel", {}, 16, cdiv(CA, cw) * cdiv(CB, cw)
    ntiles = B * cdiv(W, 16) * cdiv(H, th)
    aim = kn["WGRAD_BLOCKS1"] if kernel == "conv_wgrad_kernel" else kn["WGRAD_BLOCKS"]
    splits, cls = split_class(aim // nbase, ntiles)
    return kernel, dict(form, splits=cls), splits, ntiles


def gather_rule(case, dt, cus, capacity, base=None):
    """cmu_conv3x3_rows_supported + launch_conv_gather (conv_gather.inc): -> (kernel tag, form: NB, the channels per workgroup, and the
    grid).  256 channels per workgroup where N allows and the 256-channel grid -- ceil(capacity / 256) row tiles x N / 256 -- fills the
    CUs; CMU_GATHER_NB = 128 | 256 forces a form."""
    B, H, W, K, N = case["shape"]
    kn = knob_values(case, base)
    assert kn["SPARK_GATHER"] and N % 128 == 0 and K % (128 // ES[dt]) == 0, "not a shape of the gather kernel"
    wide = N % 256 == 0
    if wide and kn["GATHER_NB"] == 0:
        wide = cdiv(capacity, 256) * (N // 256) >= cus
    if kn["GATHER_NB"] == 128:
        wide = False
    nb = 256 if wide else 128
    return "conv_gather_kernel", {"NB": nb, "grid": cdiv(capacity, 256) * (N // nb), "steps": K // (128 // ES[dt])}


def wgrad3_tiles_rule(case, dt, base=None):
    """cmu_conv3x3_wgrad_tiles: the list's tile height names the kernel -- 16: the first kernel, any shape; 8: the 64 x 64 form where it
    serves the shape, else the wide kernel (never swapped) -> (kernel tag, form, splits, dense tile count).  The splits are the dense
    launch's (wg_geometry on the form's row of WG_FORMS), whatever the list's count."""
    B, H, W, CB, CA = case["shape"]
    kn = knob_values(case, base)
    assert kn["WGRAD_BLOCKS"] >= 8 and kn["WGRAD_BLOCKS1"] >= 8, "a value below the table's floor (8) falls back to the default"
    es = ES[dt]
    th = case["tiles"]["th"]
    wide = bool(kn["WGRAD_WIDE"]) and es == 2 and CA % 128 == 0 and CB % 64 == 0
    swap = bool(kn["WGRAD_WIDE"]) and bool(kn["WGRAD_SWAP"]) and es == 2 and CA == 64 and CB % 128 == 0
    square = bool(kn["WGRAD_WIDE"]) and bool(kn["WGRAD_SQUARE"]) and es == 2 and CA % 64 == 0 and CB % 64 == 0 and not wide and not swap
    if th == 8 and square:
        kernel, nbase, aim = "conv_wgrad2s_kernel", (CA // 64) * (CB // 64), kn["WGRAD_BLOCKS"]
    elif th == 8:
        assert wide, "an 8 x 16 list needs a shape of the wide kernel"
        kernel, nbase, aim = "conv_wgrad2_kernel", (CA // 128) * (CB // 64), kn["WGRAD_BLOCKS"]
    else:
        cw = 128 // es
        kernel, nbase, aim = "conv_wgrad_kernel", cdiv(CA, cw) * cdiv(CB, cw), kn["WGRAD_BLOCKS1"]
    ntiles = B * cdiv(W, 16) * cdiv(H, th)
    splits = split_class(aim // nbase, ntiles)[0]
    return kernel, {"splits": splits}, splits, ntiles


def wgradT_rule(case, dt, base=None):
    """cmu_convT2x2_wgrad: CA = Cout, CB = Cin -> (kernel tag, form, splits, K tiles)."""
    B, H, W, CB, CA = case["shape"]
    kn = knob_values(case, base)
    es = ES[dt]
    if kn["WGRAD_WIDE"] and es == 2 and CA % 64 == 0 and CB % 128 == 0:
        nxi = 4 if kn["WGT2_NX256"] and CB % 256 == 0 else 2
        kernel, form, th, nbase, aim = "conv_wgradT2_kernel", {"NXI": nxi}, 4, (CA // 64) * (CB // (64 * nxi)), kn["WGRAD_BLOCKS"]
    elif kn["WGRAD_WIDE"] and kn["WGRAD_WIDE_F32"] and es == 4 and CA % 64 == 0 and CB % 128 == 0:
        kernel, form, th, nbase, aim = "conv_wgradT2f_kernel", {}, 2, (CA // 64) * (CB // 128), kn["WGRAD_BLOCKS"]
    else:
        cw = 128 // es
        kernel, form, th, nbase, aim = "conv_wgrad_kernel", {}, 16, cdiv(CA, cw) * cdiv(CB, cw) * 4, 512     # (one workgroup per sub-pixel)
    ntiles = B * cdiv(W, 16) * cdiv(H, th)
    splits, cls = split_class(aim // nbase, ntiles)
    return kernel, dict(form, splits=cls), splits, ntiles


def wgrad3_ws_bytes(case, dt, base=None):
    """cmu_conv3x3_wgrad_ws_bytes restated: the largest split-K slab of the kernels that may serve the shape (splits x taps x CA x CB
    fp32 each; the first kernel pads both channel counts to 128 bytes; the 64 x 64 forms write one slab per wave half)."""
    B, H, W, CB, CA = case["shape"]
    kn = knob_values(case, base)
    es = ES[dt]
    cw = 128 // es
    na, nb = cdiv(CA, cw), cdiv(CB, cw)
    need = split_class(kn["WGRAD_BLOCKS1"] // (na * nb), B * cdiv(W, 16) * cdiv(H, 16))[0] * 9 * na * cw * nb * cw * 4
    wide = bool(kn["WGRAD_WIDE"]) and es == 2 and CA % 128 == 0 and CB % 64 == 0
    swap = bool(kn["WGRAD_WIDE"]) and bool(kn["WGRAD_SWAP"]) and es == 2 and CA == 64 and CB % 128 == 0
    t8, t4 = B * cdiv(W, 16) * cdiv(H, 8), B * cdiv(W, 16) * cdiv(H, 4)
    if wide or swap:
        nbase = (CA // 128) * (CB // 64) if wide else (CB // 128) * (CA // 64)
        need = max(need, split_class(kn["WGRAD_BLOCKS"] // nbase, t8)[0] * 9 * CA * CB * 4)
    if es == 2 and CA % 64 == 0 and CB % 64 == 0:
        need = max(need, split_class(kn["WGRAD_BLOCKS"] // ((CA // 64) * (CB // 64)), t8)[0] * 2 * 9 * CA * CB * 4)
    if es == 4 and CA % 64 == 0 and CB % 64 == 0:
        big = CA % 128 == 0
        need = max(need, split_class(kn["WGRAD_BLOCKS"] // ((CA // (128 if big else 64)) * (CB // 64)), t4)[0] * (1 if big else 2) * 9 * CA * CB * 4)
    return need


def wgradT_ws_bytes(case, dt, base=None):
    """cmu_convT2x2_wgrad_ws_bytes restated (slabs of 4 sub-pixels + the bias gradient's partial sums: 256 rows, or one per split)."""
    B, H, W, CB, CA = case["shape"]
    kn = knob_values(case, base)
    es = ES[dt]
    cw = 128 // es
    na, nb = cdiv(CA, cw), cdiv(CB, cw)
    need = (split_class(512 // (na * nb * 4), B * cdiv(W, 16) * cdiv(H, 16))[0] * 4 * na * cw * nb * cw + 256 * CA) * 4
    if kn["WGRAD_WIDE"] and es == 2 and CA % 64 == 0 and CB % 128 == 0:
        nxi = 4 if kn["WGT2_NX256"] and CB % 256 == 0 else 2
        s = split_class(kn["WGRAD_BLOCKS"] // ((CA // 64) * (CB // (64 * nxi))), B * cdiv(W, 16) * cdiv(H, 4))[0]
        need = max(need, s * (4 * CA * CB + CA) * 4)
    if es == 4 and CA % 64 == 0 and CB % 128 == 0:
        s = split_class(kn["WGRAD_BLOCKS"] // ((CA // 64) * (CB // 128)), B * cdiv(W, 16) * cdiv(H, 2))[0]
        need = max(need, (s * 4 * CA * CB + 256 * CA) * 4)
    return need


def wgrad3_tile_h(case, dt, base=None):
    """cmu_conv3x3_wgrad_tile_h restated: 8 where the dense launch on contiguous tensors runs the wide kernel unswapped or the 64 x 64
    form -- the rule names one of them and an image of dY, and of X with its halo row, lies within a buffer descriptor's range -- else 16."""
    B, H, W, CB, CA = case["shape"]
    kernel, form = wgrad3_rule(case, dt, base)[:2]
    in_range = (H * W * CA + CA) * ES[dt] < 0x7fff0000 and ((H * W + W + 1) * CB + CB) * ES[dt] < 0x7fff0000
    return 8 if in_range and kernel in ("conv_wgrad2_kernel", "conv_wgrad2s_kernel") and not form.get("SWAP") else 16


def slab_bytes(case, dt, kernel, splits):
    """Bytes of split-K slabs the kernel that runs writes: what ties the restated split count to the library's workspace size."""
    B, H, W, CB, CA = case["shape"]
    taps = 9 if case["fam"] in ("wg3", "wg3tiles") else 4
    if kernel == "conv_wgrad_kernel":
        cw = 128 // ES[dt]
        return splits * taps * cdiv(CA, cw) * cw * cdiv(CB, cw) * cw * 4
    parts = 2 if kernel == "conv_wgrad2s_kernel" or (kernel == "conv_wgrad2f_kernel" and CA % 128) else 1
    return splits * parts * taps * CA * CB * 4


def assert_form(case, dt, kernel, form):
    """The restated rule names the kernel the case is for, with the template form the case is for."""
    assert kernel == case["kernel"], f"the launcher's rule gives {kernel} for this case, not {case['kernel']}"
    for k, v in case["form"].items():
        want = v[dt] if isinstance(v, dict) else v
        assert form.get(k) == want, f"form {k}: the rule gives {form.get(k)}, the case is for {want}"
