"""Tensor-level wrappers over the C-ABI (include/cmunet_hip.h).  PyTorch is used only for device
memory and streams; every op below runs a hand-written HIP kernel and raises if the library or a
GPU is missing (no CPU / eager fallback).

``Act`` describes an NHWC activation that may be a channel slice of a wider buffer and may carry a
*pending transform* (a training-mode BatchNorm+ReLU left for the consumer to apply while it stages
its input tile) -- see the header for the convention.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import CONST, F32, F16, BF16, call

TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
DT_OF = {v: k for k, v in TORCH_DT.items()}
DT_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
NAME_DT = {"f32": F32, "fp32": F32, "float32": F32, "f16": F16, "fp16": F16, "float16": F16, "bf16": BF16, "bfloat16": BF16}


def dt_code(dt):
    if isinstance(dt, str):
        return NAME_DT[dt]
    if isinstance(dt, torch.dtype):
        return DT_OF[dt]
    return int(dt)


def _stream():
    """The launch stream: resolved by ``_lib.call`` to the current stream of the device that owns the call's tensors."""
    return _lib.STREAM


def _p(t):
    if t is None:
        return None
    assert t.is_cuda, "HIP path: tensor must live on the GPU"
    return _lib.devptr(t.data_ptr(), t.device.index)


def workspace(size_fn_name, device, *size_args):
    """The uint8 workspace of ``size_fn_name(*size_args)`` bytes on ``device`` (``size_fn_name``: one of the ``cmu_*_ws_bytes`` queries)."""
    if not size_fn_name.endswith("_ws_bytes") or size_fn_name not in _lib._SIGS:
        raise _lib.CmuError(f"{size_fn_name} is not a workspace size query of the library")
    return torch.empty(getattr(_lib.lib(), size_fn_name)(*size_args), dtype=torch.uint8, device=device)


def mfma_sustained_rate(dt="f16", pattern=0, lds_fed=False, iters=60000, device="cuda"):
    """(TFLOP/s, shader clock in MHz) of back-to-back 16-bit MFMAs on every SIMD of the device (cmu_mfma_sustained_rate):
    the rate the chip's power management lets the matrix pipes hold on ``pattern`` 0 = dense ~N(0,1) operands, 1 = ReLU'd
    operands (half zeros), 2 = zeros; ``lds_fed``: operands read from LDS at the persistent conv kernel's fragment ratio instead
    of held in registers.  ~70 ms at the default ``iters``.  Measurement support for bench.py, not on the hot path."""
    scratch = torch.zeros(8, dtype=torch.int64, device=device)
    tf, clk = ctypes.c_double(0.0), ctypes.c_double(0.0)
    call("cmu_mfma_sustained_rate", dt_code(dt), int(pattern), int(bool(lds_fed)), int(iters), _p(scratch), ctypes.byref(tf),
         ctypes.byref(clk), _stream())
    return tf.value, clk.value


class dispatch_override:
    """``with ops.dispatch_override("CMU_CONV_NARROW", 0): ...`` -- force one of the library's dispatch knobs (any row of the table in
    tools/README.md: 0 / 1 for the on / off and opt-in knobs, a number >= 0 for the others) for the launches inside the block
    (cmu_set_dispatch_override; the knobs' environment variables are read once, not per launch).  CMU_CONV_NARROW, CMU_CONV_SLIM,
    CMU_CONV_PERSIST_PART, CMU_WGRAD_SQUARE and CMU_WGRAD_WIDE_F32 give the same bits either way; every other knob is equal to rounding."""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), int(value)

    def __enter__(self):
        call("cmu_set_dispatch_override", self.name, self.value)
        return self

    def __exit__(self, *exc):
        call("cmu_set_dispatch_override", self.name, -1)
        return False


def _f32c(t):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    return t


class Act:
    """NHWC activation view: channels [coff, coff+C) of ``buf`` (B,H,W,ld) + optional pending transform."""

    __slots__ = ("buf", "coff", "C", "scale", "shift", "relu_from")

    def __init__(self, buf, coff=0, C=None, scale=None, shift=None, relu_from=0):
        assert buf.dim() == 4 and buf.is_contiguous() and buf.is_cuda
        self.buf, self.coff = buf, coff
        self.C = buf.shape[3] - coff if C is None else C
        self.scale, self.shift, self.relu_from = scale, shift, relu_from

    @property
    def B(self):
        return self.buf.shape[0]

    @property
    def H(self):
        return self.buf.shape[1]

    @property
    def W(self):
        return self.buf.shape[2]

    @property
    def ld(self):
        return self.buf.shape[3]

    @property
    def dt(self):
        return DT_OF[self.buf.dtype]

    def ptr(self):
        return _lib.devptr(self.buf.data_ptr() + self.coff * self.buf.element_size(), self.buf.device.index)

    def with_transform(self, scale, shift, relu_from=0):
        return Act(self.buf, self.coff, self.C, scale, shift, relu_from)

    def plain(self):
        return Act(self.buf, self.coff, self.C)


def new_act(B, H, W, C, dt, device):
    return Act(torch.empty((B, H, W, C), dtype=TORCH_DT[dt_code(dt)], device=device))


# ------------------------------------------------------------------------------------------------
# packing
# ------------------------------------------------------------------------------------------------
def pack_conv3x3(w, dt, transpose_flip=False):
    dt = dt_code(dt)
    Cout, Cin = w.shape[0], w.shape[1]
    n = _lib.lib().cmu_pack_conv3x3_elems(Cin, Cout, dt, int(transpose_flip))
    out = torch.empty(n, dtype=TORCH_DT[dt], device=w.device)
    call("cmu_pack_conv3x3", _p(_f32c(w)), _p(out), Cin, Cout, dt, int(transpose_flip), _stream())
    return out


def pack_convT2x2(w, dt, mode):
    dt = dt_code(dt)
    Cin, Cout = w.shape[0], w.shape[1]
    n = _lib.lib().cmu_pack_convT2x2_elems(Cin, Cout, dt, mode)
    out = torch.empty(n, dtype=TORCH_DT[dt], device=w.device)
    call("cmu_pack_convT2x2", _p(_f32c(w)), _p(out), Cin, Cout, dt, mode, _stream())
    return out


class PackPlan:
    """Every conv / conv-transpose weight pack of a model as ONE launch (cmu_pack_batch).  ``items``: list of
    (weight fp32 tensor, kind 0 conv3x3 / 1 convT2x2, mode) -- conv3x3 mode = transpose_flip, convT mode 0 fwd / 1 dgrad.
    ``outs[i]`` is the packed tensor of item i (allocated once; the weights must keep their storage, as the flat parameter
    arena guarantees)."""

    def __init__(self, items, dt):
        import struct
        dt = dt_code(dt)
        l = _lib.lib()
        assert l.cmu_pack_desc_bytes() == 48
        self.dt, self.outs, recs, block = dt, [], [], 0
        dev = items[0][0].device
        for w, kind, mode in items:
            assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4
            if kind == 0:
                Cout, Cin = w.shape[0], w.shape[1]
                n = l.cmu_pack_conv3x3_elems(Cin, Cout, dt, int(mode))
            else:
                Cin, Cout = w.shape[0], w.shape[1]
                n = l.cmu_pack_convT2x2_elems(Cin, Cout, dt, int(mode))
            out = torch.empty(n, dtype=TORCH_DT[dt], device=dev)
            self.outs.append(out)
            recs.append(struct.pack("<QQiiiiqq", w.data_ptr(), out.data_ptr(), Cin, Cout, int(mode), kind, n, block))
            block += l.cmu_pack_desc_blocks(kind, Cin, Cout, dt, int(mode))
        self.ptrs = [w.data_ptr() for w, _, _ in items]
        self.items = items
        self.total_blocks = block
        self.descs = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(dev)

    def run(self):
        assert all(w.data_ptr() == q for (w, _, _), q in zip(self.items, self.ptrs)), "a packed weight moved"
        call("cmu_pack_batch", _p(self.descs), len(self.items), self.total_blocks, self.dt, _stream())


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
def ntiles(B, H, W):
    return _lib.lib().cmu_conv_ntiles(B, H, W)


def new_stats(B, H, W, C, device):
    return torch.empty((ntiles(B, H, W), 2, C), dtype=torch.float32, device=device)


def conv3x3_c1_fwd(x_bhw, w, out, stats=None, mask=None, mask_per_sample=False):
    B, H, W = x_bhw.shape
    Cout = w.shape[0]
    assert out.C == Cout and (out.B, out.H, out.W) == (B, H, W)
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_contiguous()
    call("cmu_conv3x3_c1_fwd", _p(_f32c(x_bhw)), _p(mask), int(mask_per_sample), _p(_f32c(w)), out.ptr(), out.ld,
         _p(stats), B, H, W, Cout, out.dt, _stream())


def conv3x3_c1_fwd_tiles(x_bhw, w, out, tiles, max_tiles, mask=None, mask_per_sample=False, want_stats=True):
    """``conv3x3_c1_fwd`` over a TileList of 16 x 16 tiles (``out`` elsewhere untouched) -> slab [rows][2][Cout] of the sums over the
    listed tiles' pixels (None unless ``want_stats``).  ``max_tiles``: host-side upper bound of the list's count."""
    B, H, W = x_bhw.shape
    Cout = w.shape[0]
    assert out.C == Cout and (out.B, out.H, out.W) == (B, H, W) and (tiles.tile_h, tiles.tile_w) == (16, 16)
    stats = None
    if want_stats:
        stats = torch.empty((_lib.lib().cmu_conv3x3_c1_fwd_tiles_rows(int(max_tiles)), 2, Cout), dtype=torch.float32, device=out.buf.device)
    call("cmu_conv3x3_c1_fwd_tiles", _p(_f32c(x_bhw)), _p(mask), int(mask_per_sample), _p(_f32c(w)), out.ptr(), out.ld, _p(stats),
         _p(tiles.list), _p(tiles.count), int(max_tiles), B, H, W, Cout, out.dt, _stream())
    return stats


def conv3x3_c1_wgrad_bn_tiles(x_bhw, dA, yraw, scale, shift, save_mean, save_invstd, coef, dW, ws, tiles, max_tiles, mask=None,
                              mask_per_sample=False, w=None):
    """``conv3x3_c1_wgrad_bn`` with the contraction restricted to a TileList of 16 x 16 tiles (the gradient vanishes elsewhere)."""
    B, H, W = x_bhw.shape
    assert (tiles.tile_h, tiles.tile_w) == (16, 16)
    call("cmu_conv3x3_c1_wgrad_bn_tiles", _p(_f32c(x_bhw)), _p(mask), int(mask_per_sample), dA.ptr(), dA.ld,
         None if w is not None else yraw.ptr(), 0 if w is not None else yraw.ld, None if w is None else _p(_f32c(w)), _p(scale), _p(shift),
         _p(save_mean), _p(save_invstd), _p(coef), _p(tiles.list), _p(tiles.count), int(max_tiles), _p(_f32c(dW)), B, H, W, dW.shape[0], dA.dt,
         _p(ws), _stream())


def conv3x3_fwd(x, wpacked, out, stats=None):
    assert x.dt == out.dt and (x.B, x.H, x.W) == (out.B, out.H, out.W)
    call("cmu_conv3x3_fwd", x.ptr(), x.ld, _p(x.scale), _p(x.shift), x.relu_from, _p(wpacked), out.ptr(), out.ld,
         _p(stats), x.B, x.H, x.W, x.C, out.C, x.dt, _stream(), work=2.0 * 9 * x.C * out.C * x.B * x.H * x.W)


def bn_finalize(stats, count, conv_bias, gamma, beta, running_mean, running_var, momentum, eps, training,
                scale, shift, save_mean, save_invstd, ws):
    C = scale.numel()
    nt = 0 if stats is None else stats.shape[0]
    need = _lib.lib().cmu_bn_finalize_ws_bytes(C)
    assert ws is None or ws.numel() * ws.element_size() >= need
    call("cmu_bn_finalize", _p(stats), nt, int(count), _p(conv_bias), _p(gamma), _p(beta), _p(running_mean),
         _p(running_var), float(momentum), float(eps), int(training), _p(scale), _p(shift), _p(save_mean),
         _p(save_invstd), C, _p(ws), _stream())


def bnrelu_maxpool_fwd(y, out):
    assert y.scale is not None
    call("cmu_bnrelu_maxpool_fwd", y.ptr(), y.ld, _p(y.scale), _p(y.shift), out.ptr(), out.ld, y.B, y.H, y.W, y.C,
         y.dt, _stream())


def convT2x2_fwd(x, wpacked, bias, out):
    Cout = out.C
    assert (out.H, out.W) == (2 * x.H, 2 * x.W)
    call("cmu_convT2x2_fwd", x.ptr(), x.ld, _p(x.scale), _p(x.shift), x.relu_from, _p(wpacked), _p(_f32c(bias)),
         out.ptr(), out.ld, x.B, x.H, x.W, x.C, Cout, x.dt, _stream(), work=2.0 * 4 * x.C * Cout * x.B * x.H * x.W)


def conv1x1_head_fwd(x, w, bias, logits):
    K = w.shape[0]
    call("cmu_conv1x1_head_fwd", x.ptr(), x.ld, _p(x.scale), _p(x.shift), _p(_f32c(w)), _p(_f32c(bias)),
         _p(_f32c(logits)), x.B, x.H, x.W, x.C, K, x.dt, _stream())


def head_predict(x_act, w, bias, labels, prob=None, prob_class=0, logit_threshold=0.0, lut=None):
    """The 1x1 head fused with its argmax (K >= 2) or ``logit > logit_threshold`` (K == 1): ``labels`` (B,H,W) uint8 receives the
    class index (``lut[index]`` with ``lut``: max(K,2) uint8 values on the device), ``prob`` (B,H,W) f32 or None the softmax
    probability of ``prob_class`` (the sigmoid for K == 1).  The logits are the bits ``conv1x1_head_fwd`` writes, never stored."""
    K = w.shape[0]
    assert labels.dtype == torch.uint8 and labels.is_contiguous() and tuple(labels.shape) == (x_act.B, x_act.H, x_act.W)
    assert prob is None or (tuple(prob.shape) == tuple(labels.shape) and _f32c(prob) is prob)
    assert lut is None or (lut.dtype == torch.uint8 and lut.is_contiguous() and lut.numel() == max(K, 2))
    call("cmu_head_predict", x_act.ptr(), x_act.ld, _p(x_act.scale), _p(x_act.shift), _p(_f32c(w)), _p(_f32c(bias)),
         float(logit_threshold), _p(lut), _p(labels), _p(prob), int(prob_class), x_act.B, x_act.H, x_act.W, x_act.C, K, x_act.dt, _stream())
    return labels


class TileGrid:
    """The geometry the three tiled-prediction passes share, checked once on the host and kept on the device: images of size
    (H, W), tiles (TH, TW) at ``ystarts`` x ``xstarts`` on the canvas max(H,TH) x max(W,TW), ``codes`` = the dihedral codes of the
    copies made at every position (bit 0 flips W, bit 1 flips H, bit 2 transposes).  Raises ValueError for a start outside the
    canvas, a pixel no tile covers, an invalid or repeated code, or a transposing code on a non-square tile."""

    def __init__(self, H, W, TH, TW, ystarts, xstarts, codes=(0,), device="cuda"):
        self.H, self.W, self.TH, self.TW = int(H), int(W), int(TH), int(TW)
        self.ystarts, self.xstarts, self.codes = [int(v) for v in ystarts], [int(v) for v in xstarts], [int(c) for c in codes]
        if min(self.H, self.W, self.TH, self.TW) < 1:
            raise ValueError(f"TileGrid: sizes must be positive, got image {H} x {W}, tile {TH} x {TW}")
        for name, starts, L, T in (("ystarts", self.ystarts, self.H, self.TH), ("xstarts", self.xstarts, self.W, self.TW)):
            if not starts or sorted(set(starts)) != starts:
                raise ValueError(f"TileGrid: {name} must be strictly increasing and not empty, got {starts}")
            if starts[0] < 0 or starts[-1] + T > max(L, T):
                raise ValueError(f"TileGrid: {name}={starts} leaves the canvas of {max(L, T)} for tiles of {T}")
            gap = uncovered(starts, T, L)
            if gap is not None:
                raise ValueError(f"TileGrid: no tile covers index {gap} ({name}={starts}, tile {T}, length {L})")
        if not self.codes or len(set(self.codes)) != len(self.codes) or any(not 0 <= c <= 7 for c in self.codes):
            raise ValueError(f"TileGrid: codes must be distinct integers in 0..7, got {self.codes}")
        self.transposes = any(c & 4 for c in self.codes)
        if self.transposes and self.TH != self.TW:
            raise ValueError(f"TileGrid: transposing codes {[c for c in self.codes if c & 4]} need a square tile, got {TH} x {TW}")
        self.ny, self.nx, self.A = len(self.ystarts), len(self.xstarts), len(self.codes)
        self.per_image = self.ny * self.nx * self.A
        self.ys_dev = torch.tensor(self.ystarts, dtype=torch.int32).to(device)
        self.xs_dev = torch.tensor(self.xstarts, dtype=torch.int32).to(device)
        self.codes_dev = torch.tensor(self.codes, dtype=torch.uint8).to(device)
        self._tile_codes = None

    def tile_codes(self, n_images):
        """The code of every tile of ``n_images`` images, in tile order (uint8 on the device; kept for the largest count asked)."""
        n = n_images * self.per_image
        if self._tile_codes is None or self._tile_codes.numel() < n:
            self._tile_codes = self.codes_dev.repeat(n_images * self.ny * self.nx)
        return self._tile_codes[:n]


def uncovered(starts, T, L):
    """The first index in [0, L) that none of the windows [s, s + T) covers, or None."""
    end = 0
    for s in sorted(starts):
        if s > end:
            break
        end = max(end, s + T)
    return None if end >= L else end


PAD_MODES = {"zero": 0, "reflect": 1}


def extract_tiles(src, grid, pad="reflect", out=None):
    """``src`` (N,H,W) float32 / uint8 -> (N * ny * nx * A, TH, TW) float32: every window of ``grid`` in the forward view of each of
    its codes; canvas pixels outside the image are zero (``pad='zero'``) or reflected without repeating the edge (``'reflect'``)."""
    assert src.is_cuda and src.is_contiguous() and src.dim() == 3 and tuple(src.shape[1:]) == (grid.H, grid.W)
    if src.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"extract_tiles: the source must be float32 or uint8, got {src.dtype}")
    if pad not in PAD_MODES:
        raise ValueError(f"extract_tiles: pad must be one of {sorted(PAD_MODES)}, got {pad!r}")
    N = src.shape[0]
    if out is None:
        out = torch.empty((N * grid.per_image, grid.TH, grid.TW), dtype=torch.float32, device=src.device)
    assert tuple(out.shape) == (N * grid.per_image, grid.TH, grid.TW) and _f32c(out) is out
    call("cmu_extract_tiles", _p(src), int(src.dtype == torch.uint8), N, grid.H, grid.W, _p(grid.ys_dev), grid.ny, _p(grid.xs_dev), grid.nx,
         _p(grid.codes_dev), grid.A, grid.TH, grid.TW, PAD_MODES[pad], _p(out), _stream())
    return out


def head_probs(x_act, w, bias, probs, codes=None, transposes=False):
    """The 1x1 head + softmax (K >= 2) / sigmoid (K == 1) storing every class: ``probs`` (n, K', H, W) f32, K' = max(K, 1) planes.
    ``codes``: n uint8 on the device, the dihedral code of the view each image of ``x_act`` is in; its planes are stored in the
    un-augmented frame.  ``transposes``: whether any code transposes (then H == W is required).  The logits are the bits
    ``conv1x1_head_fwd`` writes, never stored."""
    K = w.shape[0]
    assert tuple(probs.shape) == (x_act.B, max(K, 1), x_act.H, x_act.W) and _f32c(probs) is probs
    assert codes is None or (codes.dtype == torch.uint8 and codes.is_contiguous() and codes.numel() == x_act.B)
    if transposes and x_act.H != x_act.W:
        raise ValueError(f"head_probs: transposing codes need a square tile, got {x_act.H} x {x_act.W}")
    call("cmu_head_probs", x_act.ptr(), x_act.ld, _p(x_act.scale), _p(x_act.shift), _p(_f32c(w)), _p(_f32c(bias)), _p(codes),
         int(bool(transposes)), _p(probs), x_act.B, x_act.H, x_act.W, x_act.C, K, x_act.dt, _stream())
    return probs


def blend_tiles(probs, grid, wy, wx, labels, prob=None, prob_class=0, threshold=0.5, lut=None):
    """``probs`` (N * ny * nx * A, K', TH, TW) f32 in the un-augmented frame -> ``labels`` (N,H,W) uint8: per pixel the covering tiles'
    probabilities weighted by ``wy[y - y0] * wx[x - x0]`` and summed in the fixed order iy, ix, a; argmax (ties to the smaller
    index) for K' >= 2, ``num / den > threshold`` for K' == 1; ``prob`` (N,H,W) f32 or None receives ``num[prob_class] / den``.
    ``grid`` has checked that every pixel is covered."""
    N = labels.shape[0]
    KP = probs.shape[1]
    assert labels.dtype == torch.uint8 and labels.is_contiguous() and tuple(labels.shape) == (N, grid.H, grid.W)
    assert tuple(probs.shape) == (N * grid.per_image, KP, grid.TH, grid.TW) and _f32c(probs) is probs
    assert _f32c(wy).numel() == grid.TH and _f32c(wx).numel() == grid.TW
    assert prob is None or (tuple(prob.shape) == tuple(labels.shape) and _f32c(prob) is prob)
    assert lut is None or (lut.dtype == torch.uint8 and lut.is_contiguous() and lut.numel() == max(KP, 2))
    call("cmu_blend_tiles", _p(probs), N, grid.H, grid.W, _p(grid.ys_dev), grid.ny, _p(grid.xs_dev), grid.nx, grid.A, grid.TH, grid.TW, KP,
         _p(wy), _p(wx), float(threshold), _p(lut), _p(labels), _p(prob), int(prob_class), _stream())
    return labels


def apply_to_nchw(y, out=None):
    if out is None:
        out = torch.empty((y.B, y.C, y.H, y.W), dtype=torch.float32, device=y.buf.device)
    call("cmu_apply_to_nchw", y.ptr(), y.ld, _p(y.scale), _p(y.shift), y.relu_from, _p(out), y.B, y.H, y.W, y.C,
         y.dt, _stream())
    return out


def nchw_to_nhwc(x_nchw, out):
    B, C, H, W = x_nchw.shape
    call("cmu_nchw_to_nhwc", _p(_f32c(x_nchw)), out.ptr(), out.ld, B, H, W, C, out.dt, _stream())


# ------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------
def bn_bwd_reduce(dA, y, save_mean, save_invstd, dgamma, dbeta, coef, ws):
    call("cmu_bn_bwd_reduce", dA.ptr(), dA.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(save_mean), _p(save_invstd),
         _p(dgamma), _p(dbeta), _p(coef), y.B, y.H, y.W, y.C, y.dt, _p(ws), _stream())


def bn_bwd_apply(dA, y, save_mean, save_invstd, coef, dY):
    call("cmu_bn_bwd_apply", dA.ptr(), dA.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(save_mean), _p(save_invstd),
         _p(coef), dY.ptr(), dY.ld, y.B, y.H, y.W, y.C, y.dt, _stream())


def conv3x3_wgrad(x, dY, dW, ws):
    Cout, Cin = dW.shape[0], dW.shape[1]
    assert x.C == Cin and dY.C == Cout
    call("cmu_conv3x3_wgrad", x.ptr(), x.ld, _p(x.scale), _p(x.shift), x.relu_from, dY.ptr(), dY.ld, _p(_f32c(dW)),
         x.B, x.H, x.W, Cin, Cout, x.dt, _p(ws), _stream(), work=2.0 * 9 * Cin * Cout * x.B * x.H * x.W)


def conv3x3_c1_wgrad(x_bhw, dY, dW, ws, mask=None, mask_per_sample=False):
    B, H, W = x_bhw.shape
    call("cmu_conv3x3_c1_wgrad", _p(_f32c(x_bhw)), _p(mask), int(mask_per_sample), dY.ptr(), dY.ld, _p(_f32c(dW)),
         B, H, W, dW.shape[0], dY.dt, _p(ws), _stream())


def conv3x3_c1_wgrad_bn(x_bhw, dA, yraw, scale, shift, save_mean, save_invstd, coef, dW, ws, mask=None, mask_per_sample=False, w=None):
    """First-layer weight gradient with the layer's BatchNorm+ReLU backward applied in registers (no dY in memory).  ``w``: the
    layer's forward weights -- the raw output is then recomputed from the image instead of read from ``yraw`` (same bits)."""
    B, H, W = x_bhw.shape
    assert dA.dt == yraw.dt
    if w is not None:
        call("cmu_conv3x3_c1_wgrad_bn_w", _p(_f32c(x_bhw)), _p(mask), int(mask_per_sample), dA.ptr(), dA.ld, _p(_f32c(w)), _p(scale), _p(shift),
             _p(save_mean), _p(save_invstd), _p(coef), _p(_f32c(dW)), B, H, W, dW.shape[0], dA.dt, _p(ws), _stream())
        return
    call("cmu_conv3x3_c1_wgrad_bn", _p(_f32c(x_bhw)), _p(mask), int(mask_per_sample), dA.ptr(), dA.ld, yraw.ptr(), yraw.ld,
         _p(scale), _p(shift), _p(save_mean), _p(save_invstd), _p(coef), _p(_f32c(dW)), B, H, W, dW.shape[0], dA.dt, _p(ws),
         _stream())


def maxpool_bwd(dP, dSkip, y, dA, save_mean=None, save_invstd=None, bn_ws=None, dSkip2=None):
    """``dSkip2``: a second gradient of the same skip tensor (two decoders on one encoder), summed inside the pass.
    ``dA`` None (with ``bn_ws``): only the BatchNorm-backward sums are produced -- follow with ``maxpool_bwd_apply``."""
    call("cmu_maxpool_bwd2", dP.ptr(), dP.ld, None if dSkip is None else dSkip.ptr(), 0 if dSkip is None else dSkip.ld,
         None if dSkip2 is None else dSkip2.ptr(), 0 if dSkip2 is None else dSkip2.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift),
         None if dA is None else dA.ptr(), 0 if dA is None else dA.ld, _p(save_mean), _p(save_invstd), _p(bn_ws),
         y.B, y.H, y.W, y.C, y.dt, _stream())


def maxpool_bwd_apply(dP, dSkip, y, save_mean, save_invstd, coef, dY, dSkip2=None):
    """dY of the conv+BN+ReLU layer in front of a max-pool, straight from the pooled gradient and the skip gradient(s): the second
    half of ``maxpool_bwd(..., dA=None, bn_ws=...)`` + ``bn_bwd_finalize`` (the pool's input gradient is never stored)."""
    call("cmu_maxpool_bwd_apply", dP.ptr(), dP.ld, None if dSkip is None else dSkip.ptr(), 0 if dSkip is None else dSkip.ld,
         None if dSkip2 is None else dSkip2.ptr(), 0 if dSkip2 is None else dSkip2.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift),
         _p(save_mean), _p(save_invstd), _p(_f32c(coef)), dY.ptr(), dY.ld, y.B, y.H, y.W, y.C, y.dt, _stream())


def bn_bwd_finalize(bn_ws, count, dgamma, dbeta, coef):
    call("cmu_bn_bwd_finalize", _p(bn_ws), int(count), _p(dgamma), _p(dbeta), _p(coef), coef.shape[1], _stream())


def bn_bwd_finalize_tiles(bstats, count, dgamma, dbeta, coef, ws):
    """Phase 1 of BatchNorm backward from the per-tile slab written by conv3x3_dgrad_bn / convT2x2_dgrad_bn."""
    call("cmu_bn_bwd_finalize_tiles", _p(bstats), bstats.shape[0], int(count), _p(dgamma), _p(dbeta), _p(coef), coef.shape[1], _p(ws),
         _stream())


def conv3x3_dgrad_bn(dY, wpacked_flip, dX, y, save_mean, save_invstd, bstats):
    """dX = data gradient of a 3x3 conv; ``y``: Act of the raw output (+ pending BN transform) of the layer whose activated
    output is the conv's input -- its BatchNorm+ReLU backward partial sums go to ``bstats`` (new_stats shape)."""
    call("cmu_conv3x3_dgrad_bn", dY.ptr(), dY.ld, _p(wpacked_flip), dX.ptr(), dX.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift),
         _p(save_mean), _p(save_invstd), _p(bstats), dX.B, dX.H, dX.W, dY.C, dX.C, dX.dt, _stream(),
         work=2.0 * 9 * dY.C * dX.C * dX.B * dX.H * dX.W)


def convT2x2_dgrad_bn(dOut, wpacked_dgrad, dX, y, save_mean, save_invstd, bstats):
    call("cmu_convT2x2_dgrad_bn", dOut.ptr(), dOut.ld, _p(wpacked_dgrad), dX.ptr(), dX.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift),
         _p(save_mean), _p(save_invstd), _p(bstats), dX.B, dX.H, dX.W, dX.C, dOut.C, dX.dt, _stream(),
         work=2.0 * 4 * dX.C * dOut.C * dX.B * dX.H * dX.W)


def convT2x2_dgrad(dOut, wpacked_dgrad, dX):
    call("cmu_convT2x2_dgrad", dOut.ptr(), dOut.ld, _p(wpacked_dgrad), dX.ptr(), dX.ld, dX.B, dX.H, dX.W, dX.C, dOut.C,
         dX.dt, _stream(), work=2.0 * 4 * dX.C * dOut.C * dX.B * dX.H * dX.W)


def convT2x2_wgrad(x, dOut, dW, dbias, ws):
    Cin, Cout = dW.shape[0], dW.shape[1]
    call("cmu_convT2x2_wgrad", x.ptr(), x.ld, _p(x.scale), _p(x.shift), x.relu_from, dOut.ptr(), dOut.ld, _p(_f32c(dW)),
         _p(_f32c(dbias)), x.B, x.H, x.W, Cin, Cout, x.dt, _p(ws), _stream(), work=2.0 * 4 * Cin * Cout * x.B * x.H * x.W)


def conv1x1_head_bn_apply(dlogits, x, w, save_mean, save_invstd, coef, dY):
    """dY of the conv+BN+ReLU layer that fed the 1x1 head, straight from dlogits (the head's input gradient has rank K and is never
    stored): second half of ``conv1x1_head_bwd(..., dX=None, bn_ws=...)`` + ``bn_bwd_finalize``."""
    K = w.shape[0]
    call("cmu_conv1x1_head_bn_apply", _p(_f32c(dlogits)), x.ptr(), x.ld, _p(x.scale), _p(x.shift), _p(_f32c(w)), _p(save_mean),
         _p(save_invstd), _p(_f32c(coef)), dY.ptr(), dY.ld, x.B, x.H, x.W, x.C, K, x.dt, _stream())


def conv1x1_head_bwd(dlogits, x, w, dX, dW, dbias, ws, save_mean=None, save_invstd=None, bn_ws=None):
    """``dX`` None (with ``bn_ws``): parameter gradients and BatchNorm-backward sums only (see ``conv1x1_head_bn_apply``)."""
    K = w.shape[0]
    if dX is None:
        call("cmu_conv1x1_head_bwd", _p(_f32c(dlogits)), x.ptr(), x.ld, _p(x.scale), _p(x.shift), _p(_f32c(w)), None, 0,
             _p(_f32c(dW)), _p(_f32c(dbias)), _p(save_mean), _p(save_invstd), _p(bn_ws), x.B, x.H, x.W, x.C, K, x.dt, _p(ws),
             _stream())
        return
    call("cmu_conv1x1_head_bwd", _p(_f32c(dlogits)), x.ptr(), x.ld, _p(x.scale), _p(x.shift), _p(_f32c(w)), dX.ptr(), dX.ld,
         _p(_f32c(dW)), _p(_f32c(dbias)), _p(save_mean), _p(save_invstd), _p(bn_ws), x.B, x.H, x.W, x.C, K, x.dt, _p(ws),
         _stream())


# ------------------------------------------------------------------------------------------------
# losses / heads / optimiser
# ------------------------------------------------------------------------------------------------
def masked_mse_fwd_bwd(logits, channel, img, mask, loss, dlogits, loss_scale, ws, amp=None):
    B, K, H, W = logits.shape
    call("cmu_masked_mse_fwd_bwd", _p(_f32c(logits)), K, channel, _p(_f32c(img)), _p(mask), _p(loss), _p(dlogits),
         float(loss_scale), _p(None if amp is None else amp.state), B, H, W, _p(ws), _stream())


def softmax_ce_dice_fwd_bwd(logits, y1h, out, dlogits, loss_scale, ws):
    B, K, H, W = logits.shape
    assert K == 2 and y1h.dtype == torch.float64 and y1h.is_contiguous()
    call("cmu_softmax_ce_dice_fwd_bwd", _p(_f32c(logits)), _p(y1h), _p(out), _p(dlogits), float(loss_scale), B, H, W,
         _p(ws), _stream())


SEG_MAX_K = 8


def _seg_args(logits, y, class_w):
    B, K, H, W = logits.shape
    assert 2 <= K <= SEG_MAX_K and y.shape == logits.shape and y.is_contiguous() and y.dtype in (torch.float32, torch.float64)
    assert class_w is None or (class_w.shape == (K,) and class_w.dtype == torch.float32 and class_w.is_contiguous())
    return B, K, H, W


def seg_stats_fwd(logits, y, class_w, threshold, table, ws):
    """table (1 + 5K fp64) = [ce | tp_soft | spr_soft | tp_hard | spr_hard | sgt] of (B,K,H,W) fp32 logits and fp64 / fp32 targets."""
    B, K, H, W = _seg_args(logits, y, class_w)
    assert table.dtype == torch.float64 and table.numel() == 1 + 5 * K and table.is_contiguous()
    call("cmu_seg_stats_fwd", _p(_f32c(logits)), _p(y), int(y.dtype == torch.float64), _p(class_w), float(threshold), _p(table),
         B, K, H, W, _p(ws), _stream())


def seg_stats_bwd(logits, y, class_w, g_ce, g_tp, g_spr, dlogits):
    """dlogits (fp32) from the device-resident fp64 gradients w.r.t. ce (1) and the soft counters (K each); None = zeros."""
    B, K, H, W = _seg_args(logits, y, class_w)
    for g, n in ((g_ce, 1), (g_tp, K), (g_spr, K)):
        assert g is None or (g.dtype == torch.float64 and g.numel() == n and g.is_contiguous())
    call("cmu_seg_stats_bwd", _p(_f32c(logits)), _p(y), int(y.dtype == torch.float64), _p(class_w), _p(g_ce), _p(g_tp), _p(g_spr),
         _p(_f32c(dlogits)), B, K, H, W, _stream())


PWL_KINDS = {"l1": CONST["CMU_PWL_L1"], "mse": CONST["CMU_PWL_MSE"], "bce": CONST["CMU_PWL_BCE"],
             "bce_with_logits": CONST["CMU_PWL_BCE_WITH_LOGITS"]}
PWL_MAX_C = CONST["CMU_PWL_MAX_C"]


def _pwl_args(kind, x, y, chan_w, chan_pw):
    """(kind code, outer, C, inner) of the (outer, C, inner) view: C = 1 over the whole tensor without per-channel vectors, else the
    vectors' length, which must be x.shape[1] unless it is 1."""
    assert kind in PWL_KINDS, kind
    assert y.shape == x.shape and y.is_cuda and y.is_contiguous() and y.dtype in (torch.float32, torch.float64)
    assert chan_pw is None or kind == "bce_with_logits"
    C = 1
    for v in (chan_w, chan_pw):
        if v is not None:
            assert v.dim() == 1 and v.dtype == torch.float32 and v.is_contiguous() and 1 <= v.shape[0] <= PWL_MAX_C
            assert C in (1, v.shape[0])
            C = v.shape[0]
    if C == 1:                               # no vectors, or one-element vectors: a factor on everything, whatever the shape
        return PWL_KINDS[kind], 1, 1, x.numel()
    assert x.dim() >= 2 and x.shape[1] == C and x.numel() > 0
    return PWL_KINDS[kind], x.shape[0], C, x.numel() // (x.shape[0] * C)


def pointwise_loss_fwd(kind, x, y, chan_w, chan_pw, out, ws):
    """out[0] (fp64) = sum_i w_c term_i of fp32 ``x`` against fp32 / fp64 ``y`` for kind 'l1' / 'mse' / 'bce' / 'bce_with_logits';
    chan_w / chan_pw: fp32 vectors over x.shape[1] or None (cmu_pointwise_loss_fwd)."""
    k, outer, C, inner = _pwl_args(kind, x, y, chan_w, chan_pw)
    assert out.dtype == torch.float64 and out.numel() == 1
    call("cmu_pointwise_loss_fwd", k, _p(_f32c(x)), _p(y), int(y.dtype == torch.float64), _p(chan_w), _p(chan_pw), _p(out), outer, C, inner,
         _p(ws), _stream())


def pointwise_loss_bwd(kind, x, y, chan_w, chan_pw, g, dx):
    """dx (fp32) = g[0] w_c dterm_i with ``g`` one fp64 value on the device (None = zero)."""
    k, outer, C, inner = _pwl_args(kind, x, y, chan_w, chan_pw)
    assert g is None or (g.dtype == torch.float64 and g.numel() == 1)
    assert dx.shape == x.shape
    call("cmu_pointwise_loss_bwd", k, _p(_f32c(x)), _p(y), int(y.dtype == torch.float64), _p(chan_w), _p(chan_pw), _p(g), _p(_f32c(dx)),
         outer, C, inner, _stream())


ICE_LABEL_KINDS = {torch.int64: CONST["CMU_ICE_LABEL_I64"], torch.int32: CONST["CMU_ICE_LABEL_I32"], torch.uint8: CONST["CMU_ICE_LABEL_U8"],
                   torch.float32: CONST["CMU_ICE_LABEL_F32"], torch.float64: CONST["CMU_ICE_LABEL_F64"]}
ICE_ONEHOT_KINDS = {torch.float32: CONST["CMU_ICE_ONEHOT_F32"], torch.float64: CONST["CMU_ICE_ONEHOT_F64"]}


def _ice_args(x, target, onehot, keep, class_w):
    B, K, H, W = x.shape
    assert 2 <= K <= SEG_MAX_K and target.is_cuda and target.is_contiguous()
    if onehot:
        assert target.shape == x.shape and target.dtype in ICE_ONEHOT_KINDS
        kind = ICE_ONEHOT_KINDS[target.dtype]
    else:
        assert target.shape == (B, H, W) and target.dtype in ICE_LABEL_KINDS
        kind = ICE_LABEL_KINDS[target.dtype]
    keep = list(range(K)) if keep is None else list(keep)
    assert keep and keep == sorted(set(keep)) and 0 <= keep[0] and keep[-1] < K
    assert class_w is None or (class_w.shape == (K,) and class_w.dtype == torch.float32 and class_w.is_contiguous())
    return B, K, H, W, kind, sum(1 << c for c in keep)


def index_ce_fwd(x, target, onehot, log_input, keep, class_w, ignore_index, table, ws):
    """table (3 fp64) = [sum w_t (-log p_t) | sum w_t | sum_kept w_c (-log p_c)] of (B,K,H,W) fp32 logits (``log_input``: log-
    probabilities) against a (B,H,W) label plane, or (``onehot``) K planes whose arg-max over ``keep`` is the label (cmu_index_ce_fwd)."""
    B, K, H, W, kind, mask = _ice_args(x, target, onehot, keep, class_w)
    assert table.dtype == torch.float64 and table.numel() == 3 and table.is_contiguous()
    call("cmu_index_ce_fwd", _p(_f32c(x)), _p(target), kind, int(bool(log_input)), mask, _p(class_w), int(ignore_index), _p(table),
         B, K, H, W, _p(ws), _stream())


def index_ce_bwd(x, target, onehot, log_input, keep, class_w, ignore_index, g, dx):
    """dx (fp32) from the device-resident fp64 gradients g = (d/d table[0], d/d table[2]); None = zeros."""
    B, K, H, W, kind, mask = _ice_args(x, target, onehot, keep, class_w)
    assert g is None or (g.dtype == torch.float64 and g.numel() == 2 and g.is_contiguous())
    assert dx.shape == x.shape
    call("cmu_index_ce_bwd", _p(_f32c(x)), _p(target), kind, int(bool(log_input)), mask, _p(class_w), int(ignore_index), _p(g),
         _p(_f32c(dx)), B, K, H, W, _stream())


def infonce_inbatch_fwd_bwd(pred, keys, loss, dpred, rank, temperature, ct_weight):
    B, D = pred.shape
    call("cmu_infonce_inbatch_fwd_bwd", _p(_f32c(pred)), _p(_f32c(keys)), _p(loss), _p(dpred), B, keys.shape[0], D,
         rank, float(temperature), float(ct_weight), _stream())


def moco_infonce_enqueue(q_raw, k_raw, keys_all, queue, queue_ptr, loss, dq, k_norm_out, temperature, ws):
    B, D = q_raw.shape
    K = queue.shape[1]
    Nk = B if keys_all is None else keys_all.shape[0]
    call("cmu_moco_infonce_enqueue", _p(_f32c(q_raw)), _p(_f32c(k_raw)), _p(keys_all), Nk, _p(_f32c(queue)),
         _p(queue_ptr), _p(loss), _p(dq), _p(k_norm_out), B, D, K, float(temperature), _p(ws), _stream())


def l2_normalize_rows(x, out):
    call("cmu_l2_normalize_rows", _p(_f32c(x)), _p(out), x.shape[0], x.shape[1], _stream())


def l2_normalize_rows_bwd(x, dy, dx):
    call("cmu_l2_normalize_rows_bwd", _p(_f32c(x)), _p(_f32c(dy)), _p(dx), x.shape[0], x.shape[1], _stream())


def moco_logits_assemble(q, k, lneg, logits, inv_t):
    B, D = q.shape
    call("cmu_moco_logits_assemble", _p(_f32c(q)), _p(_f32c(k)), _p(_f32c(lneg)), _p(logits), B, D, lneg.shape[1], float(inv_t), _stream())


def moco_logits_split(dlogits, dlneg, inv_t):
    call("cmu_moco_logits_split", _p(_f32c(dlogits)), _p(dlneg), dlneg.shape[0], dlneg.shape[1], float(inv_t), _stream())


def moco_logits_addpos(dlogits, k, dq, inv_t):
    B, D = dq.shape
    call("cmu_moco_logits_addpos", _p(_f32c(dlogits)), _p(_f32c(k)), _p(dq), B, D, dlogits.shape[1] - 1, float(inv_t), _stream())


def row_cross_entropy(logits, target, want_grad=True, want_rank=False):
    """F.cross_entropy(logits, target) (mean) on one kernel: -> (loss (1,), dlogits or None = d mean / d logits, rank (B,) int32 or None)."""
    B, N = logits.shape
    dev = logits.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    rows = torch.empty(B, dtype=torch.float32, device=dev)
    dl = torch.empty((B, N), dtype=torch.float32, device=dev) if want_grad else None
    rank = torch.empty(B, dtype=torch.int32, device=dev) if want_rank else None
    tgt = target if (target.dtype == torch.int64 and target.is_contiguous()) else target.to(torch.int64).contiguous()
    call("cmu_row_cross_entropy", _p(_f32c(logits)), _p(tgt), _p(loss), _p(rows), _p(dl), _p(rank), B, N, _stream())
    return loss, dl, rank


def patchify(x, h, w, p, inverse=False):
    """SparK.patchify (inverse False: (B, C, h*p, w*p) -> (B, h*w, p*p*C)) / unpatchify (inverse True) on cmu_patchify, fp32.
    Contract: CUDA tensors, no autograd (the reference's einsum form is differentiable; here it serves the `vis` path only).
    A shape that does not match (h, w, p) raises, as the reference's reshape does (spark.py:133-149)."""
    if not x.is_cuda:
        raise RuntimeError("ops.patchify: CUDA tensor required (no CPU fallback)")
    if not inverse:
        if x.dim() != 4 or x.shape[2] != h * p or x.shape[3] != w * p:
            raise ValueError(f"patchify: input {tuple(x.shape)} is not (B, C, {h * p}, {w * p}) for h={h}, w={w}, p={p}")
    else:
        if x.dim() != 3 or x.shape[1] != h * w or x.shape[2] % (p * p) != 0 or x.shape[2] == 0:
            raise ValueError(f"unpatchify: input {tuple(x.shape)} is not (B, {h * w}, {p * p}*C) for h={h}, w={w}, p={p}")
    x = x.float().contiguous()
    if not inverse:
        B, C = x.shape[:2]
        out = torch.empty((B, h * w, p * p * C), dtype=torch.float32, device=x.device)
    else:
        B, C = x.shape[0], x.shape[-1] // (p * p)
        out = torch.empty((B, C, h * p, w * p), dtype=torch.float32, device=x.device)
    call("cmu_patchify", _p(x), _p(out), B, C, h, w, p, int(inverse), _stream())
    return out


def scale_by_device_scalar(v, s):
    call("cmu_scale_by_device_scalar", _p(v), _p(_f32c(s.reshape(-1))), v.numel(), _stream())


def softmax2_threshold(logits, threshold, out):
    """out (B,H,W) fp32 = (softmax(logits, 1)[:, 1] > threshold) for (B,2,H,W) fp32 logits."""
    B, K, H, W = logits.shape
    assert K == 2 and out.shape == (B, H, W)
    call("cmu_softmax2_threshold", _p(_f32c(logits)), float(threshold), _p(_f32c(out)), B, H, W, _stream())


def soft_skeleton(img, skel, num_iter, ws=None):
    """skel = the soft skeleton of the fp32 (planes, H, W) stack ``img`` after ``num_iter`` rounds (metrics.py:448-490)."""
    P, H, W = img.shape
    if ws is None:
        ws = workspace("cmu_soft_skeleton_ws_bytes", img.device, img.numel())
    call("cmu_soft_skeleton", _p(_f32c(img)), _p(_f32c(skel)), P, H, W, int(num_iter), _p(ws), _stream())


def keep_mask(keep):
    """Bit k set for every kept channel k (the planes kernels take the channel list as a mask: no device-side index array)."""
    m = 0
    for c in keep:
        m |= 1 << int(c)
    return m


def softmax_planes(logits, target, keep, threshold, p_planes, t_planes):
    """softmax(dim=1) of the channels ``keep`` of (B,K,H,W) fp32 logits as (B*Kk,H,W) fp32 planes (``threshold``: p > threshold as
    0/1), and the same channels of the fp32 / fp64 target (``target`` and ``t_planes`` may both be None)."""
    B, K, H, W = logits.shape
    keep = list(keep)
    assert 2 <= K <= SEG_MAX_K and keep and keep == sorted(set(keep)) and 0 <= keep[0] and keep[-1] < K
    assert p_planes.numel() == B * len(keep) * H * W and (target is None) == (t_planes is None)
    if target is not None:
        assert target.shape == logits.shape and target.is_contiguous() and target.dtype in (torch.float32, torch.float64)
        assert t_planes.numel() == p_planes.numel()
        _f32c(t_planes)
    call("cmu_softmax_planes", _p(_f32c(logits)), _p(target), int(target is not None and target.dtype == torch.float64), keep_mask(keep),
         int(threshold is not None), float(threshold or 0.0), _p(_f32c(p_planes)), _p(t_planes), B, K, H, W, _stream())


def softmax_planes_bwd(logits, g_planes, keep, dlogits):
    """dlogits_k = p_k (G_k - sum_j p_j G_j), G = ``g_planes`` (B*Kk,H,W) on the channels ``keep`` and zero elsewhere."""
    B, K, H, W = logits.shape
    keep = list(keep)
    assert 2 <= K <= SEG_MAX_K and keep and keep == sorted(set(keep)) and 0 <= keep[0] and keep[-1] < K
    assert g_planes.numel() == B * len(keep) * H * W and dlogits.shape == logits.shape
    call("cmu_softmax_planes_bwd", _p(_f32c(logits)), _p(_f32c(g_planes)), keep_mask(keep), _p(_f32c(dlogits)), B, K, H, W, _stream())


def soft_skeleton_save(img, skel, num_iter, kept=None):
    """``soft_skeleton`` (the same bits) that keeps its level images and running skeletons for ``soft_skeleton_bwd``; returns them."""
    P, H, W = img.shape
    if kept is None:
        kept = workspace("cmu_soft_skeleton_save_ws_bytes", img.device, img.numel(), int(num_iter))
    assert kept.numel() >= _lib.lib().cmu_soft_skeleton_save_ws_bytes(img.numel(), int(num_iter)) and skel.shape == img.shape
    call("cmu_soft_skeleton_save", _p(_f32c(img)), _p(_f32c(skel)), P, H, W, int(num_iter), _p(kept), _stream())
    return kept


def soft_skeleton_bwd(img, kept, num_iter, dimg, g_skel=None, g4=None, y_true=None, skel_true=None, ws=None):
    """dimg = gradient of <g, soft_skeleton(img)> w.r.t. ``img`` (P,H,W), g = ``g_skel`` and / or the clDice tail of the device-resident
    fp64 ``g4`` (g4[0] * y_true + g4[1]; ``dimg`` then gains g4[2] * skel_true).  ``kept`` comes from ``soft_skeleton_save``."""
    P, H, W = img.shape
    assert g_skel is not None or g4 is not None
    assert kept.numel() >= _lib.lib().cmu_soft_skeleton_save_ws_bytes(img.numel(), int(num_iter)) and dimg.shape == img.shape
    for t in (g_skel, y_true, skel_true):
        assert t is None or (t.numel() == img.numel() and _f32c(t) is t)
    if g4 is not None:
        assert g4.dtype == torch.float64 and g4.numel() == 4 and g4.is_contiguous() and y_true is not None and skel_true is not None
    if ws is None:
        ws = workspace("cmu_soft_skeleton_bwd_ws_bytes", img.device, img.numel())
    call("cmu_soft_skeleton_bwd", _p(_f32c(img)), _p(kept), _p(g_skel), _p(g4), _p(y_true), _p(skel_true), _p(_f32c(dimg)), P, H, W,
         int(num_iter), _p(ws), _stream())


def cldice_sums(skel_pred, y_true, skel_true, y_pred, out4, ws=None):
    """out4 = (sum skel_pred*y_true, sum skel_pred, sum skel_true*y_pred, sum skel_true) over same-sized fp32 tensors."""
    if ws is None:
        ws = workspace("cmu_cldice_sums_ws_bytes", skel_pred.device)
    call("cmu_cldice_sums", _p(_f32c(skel_pred)), _p(_f32c(y_true)), _p(_f32c(skel_true)), _p(_f32c(y_pred)), skel_pred.numel(),
         _p(out4), _p(ws), _stream())


# ------------------------------------------------------------------------------------------------
# SparK sparse ops
# ------------------------------------------------------------------------------------------------
def masked_channel_stats(x, active, invert=False):
    """-> slab [rows][2][C] fp32 (rows = cmu_masked_stats_rows()) of sums over the selected pixels."""
    rows = _lib.lib().cmu_masked_stats_rows()
    slab = torch.empty((rows, 2, x.C), dtype=torch.float32, device=x.buf.device)
    call("cmu_masked_channel_stats", x.ptr(), x.ld, _p(active), active.shape[-1], int(invert), _p(slab), x.B, x.H, x.W, x.C, x.dt,
         _stream())
    return slab


def rows_channel_stats(x, pixels):
    """masked_channel_stats over a PixelList: the listed pixels only."""
    rows = _lib.lib().cmu_masked_stats_rows()
    slab = torch.empty((rows, 2, x.C), dtype=torch.float32, device=x.buf.device)
    call("cmu_rows_channel_stats", x.ptr(), x.ld, _p(pixels.rows), _p(pixels.count), _p(slab), x.B, x.H, x.W, x.C, x.dt, _stream())
    return slab


def bn_bwd_reduce_rows(dA, y, save_mean, save_invstd, dgamma, dbeta, coef, pixels, count, ws):
    call("cmu_bn_bwd_reduce_rows", dA.ptr(), dA.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(save_mean), _p(save_invstd), _p(dgamma),
         _p(dbeta), _p(coef), _p(pixels.rows), _p(pixels.count), pixels.capacity, int(count), y.B, y.H, y.W, y.C, y.dt, _p(ws), _stream())


_SPARK_CELLS = os.environ.get("CMU_SPARK_CELLS", "1") != "0"      # A/B: the pixel-organised masked kernels


def cells_supported(x, active):
    """Whether the patch-organised element-wise kernels (csrc/sparse_elem.hip) serve this level."""
    if not _SPARK_CELLS:
        return False
    return bool(_lib.lib().cmu_cells_supported(x.B, x.H, x.W, active.shape[-1], x.C, x.dt))


def mask_select(x, active, out, relu=False, invert=False, fill=None, use_transform=True, ring=False, cells=True):
    """out = selected ? relu?(x * scale + shift) : fill.  Without inversion the patch-organised kernel is taken
    (``cells``); ``ring``: only the one-pixel border frame of each masked patch is zeroed -- the caller guarantees that every consumer
    of ``out`` is list-driven (reads active patches and a one-pixel halo only)."""
    sc = x.scale if use_transform else None
    sh = x.shift if use_transform else None
    if cells and not invert and cells_supported(x, active):
        call("cmu_mask_select_cells", x.ptr(), x.ld, _p(sc), _p(sh), int(relu), _p(active), active.shape[-1], int(bool(ring) and fill is None),
             _p(fill), out.ptr(), out.ld, x.B, x.H, x.W, x.C, x.dt, _stream())
        return
    call("cmu_mask_select", x.ptr(), x.ld, _p(sc), _p(sh), int(relu), _p(active), active.shape[-1], int(invert), _p(fill), out.ptr(),
         out.ld, x.B, x.H, x.W, x.C, x.dt, _stream())


def cells_channel_stats(x, active):
    """masked_channel_stats / rows_channel_stats over the active patches, patch-organised -> slab [rows][2][C] fp32."""
    slab = torch.empty((_lib.lib().cmu_cells_stats_rows(), 2, x.C), dtype=torch.float32, device=x.buf.device)
    call("cmu_cells_channel_stats", x.ptr(), x.ld, _p(active), active.shape[-1], _p(slab), x.B, x.H, x.W, x.C, x.dt, _stream())
    return slab


def bn_bwd_reduce_cells(dA, y, save_mean, save_invstd, dgamma, dbeta, coef, active, count, ws):
    """bn_bwd_reduce_masked / bn_bwd_reduce_rows, patch-organised."""
    call("cmu_bn_bwd_reduce_cells", dA.ptr(), dA.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(save_mean), _p(save_invstd), _p(dgamma),
         _p(dbeta), _p(coef), _p(active), active.shape[-1], int(count), y.B, y.H, y.W, y.C, y.dt, _p(ws), _stream())


def cells_channel_sum(x, active, out, invert=False, ws=None):
    """out[c] (fp32, C) = sum of x over the pixels of the active / masked (``invert``) patches: the mask-token gradient."""
    assert out.dtype == torch.float32 and out.numel() == x.C and out.is_contiguous()
    if ws is None:
        ws = workspace("cmu_cells_channel_sum_ws_bytes", x.buf.device, x.C)
    call("cmu_cells_channel_sum", x.ptr(), x.ld, _p(active), active.shape[-1], int(invert), _p(out), _p(ws), x.B, x.H, x.W, x.C, x.dt,
         _stream())


def bnrelu_maxpool_fwd_masked(y, active, out):
    """BN + ReLU + 2x2 max of the raw ``y`` with masked windows pooled to zero (no activated / masked copy of y in memory)."""
    assert y.scale is not None
    call("cmu_bnrelu_maxpool_fwd_masked", y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(active), active.shape[-1], out.ptr(), out.ld,
         y.B, y.H, y.W, y.C, y.dt, _stream())


def maxpool_bwd_masked(dP, dSkip, y, dA, active, cells=True):
    """``maxpool_bwd`` on the raw ``y`` + transform at active windows only; dA of masked windows is left unwritten."""
    name = "cmu_maxpool_bwd_cells" if (cells and y.H // active.shape[-1] >= 2 and cells_supported(y, active)) else "cmu_maxpool_bwd_masked"
    call(name, dP.ptr(), dP.ld, None if dSkip is None else dSkip.ptr(), 0 if dSkip is None else dSkip.ld, y.ptr(), y.ld,
         _p(y.scale), _p(y.shift), _p(active), active.shape[-1], dA.ptr(), dA.ld, y.B, y.H, y.W, y.C, y.dt, _stream())


def bn_bwd_reduce_masked(dA, y, save_mean, save_invstd, dgamma, dbeta, coef, active, count, ws):
    call("cmu_bn_bwd_reduce_masked", dA.ptr(), dA.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(save_mean), _p(save_invstd),
         _p(dgamma), _p(dbeta), _p(coef), _p(active), active.shape[-1], int(count), y.B, y.H, y.W, y.C, y.dt, _p(ws), _stream())


def bn_bwd_apply_masked(dA, y, save_mean, save_invstd, coef, dY, active, ring=False, cells=True):
    """dY = BatchNorm+ReLU backward at active positions, zeros at masked ones (``ring``: see mask_select)."""
    if cells and cells_supported(y, active):
        call("cmu_bn_bwd_apply_cells", dA.ptr(), dA.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(save_mean), _p(save_invstd),
             _p(coef), dY.ptr(), dY.ld, _p(active), active.shape[-1], int(bool(ring)), y.B, y.H, y.W, y.C, y.dt, _stream())
        return
    call("cmu_bn_bwd_apply_masked", dA.ptr(), dA.ld, y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(save_mean), _p(save_invstd),
         _p(coef), dY.ptr(), dY.ld, _p(active), active.shape[-1], y.B, y.H, y.W, y.C, y.dt, _stream())


class TileList:
    """Device-side list of the spatial tiles of one level that overlap an active patch (cmu_sparse_tile_list): ``list`` int32,
    ``count`` int32 (1,) -- both stay on the device.  ``n_dense`` is the dense tile count (the list's capacity).  ``defer``: only
    allocate; ``build_lists`` fills several lists in one launch."""

    def __init__(self, active, H, W, tile_h, tile_w, defer=False):
        B, f = active.shape[0], active.shape[-1]
        self.H, self.W, self.tile_h, self.tile_w = H, W, tile_h, tile_w
        self.n_dense = B * ((H + tile_h - 1) // tile_h) * ((W + tile_w - 1) // tile_w)
        self.list = torch.empty(self.n_dense, dtype=torch.int32, device=active.device)
        self.count = torch.empty(1, dtype=torch.int32, device=active.device)
        if not defer:
            call("cmu_sparse_tile_list", _p(active), f, B, H, W, tile_h, tile_w, _p(self.list), _p(self.count), _stream())


class PixelList:
    """Device-side list of the active pixels of one level (cmu_sparse_pixel_list): ``rows`` int32 dense pixel indices, patch-
    major, padded with -1 to ``capacity``; ``count`` int32 (1,).  ``max_rows``: host-side upper bound of the count (the number
    of active patches x patch area when the caller knows it, else the dense pixel count).  ``defer``: see TileList."""

    def __init__(self, active, H, W, max_rows=None, defer=False):
        B, f = active.shape[0], active.shape[-1]
        dense = B * H * W
        self.H, self.W = H, W
        self.max_rows = dense if max_rows is None else min(int(max_rows), dense)
        self.capacity = max(256, (self.max_rows + 255) // 256 * 256)
        self.rows = torch.empty(self.capacity, dtype=torch.int32, device=active.device)
        self.count = torch.empty(1, dtype=torch.int32, device=active.device)
        if not defer:
            ws = workspace("cmu_sparse_pixel_list_ws_bytes", active.device, B, f)
            call("cmu_sparse_pixel_list", _p(active), f, B, H, W, _p(self.rows), self.capacity, _p(self.count), _p(ws), _stream())


def build_lists(active, tile_lists=(), pixel_lists=()):
    """Fill deferred TileLists / PixelLists of ONE patch map: every tile list (plus the patch list the pixel lists expand) in one launch
    of one workgroup per list, every pixel list in a second launch -- instead of one or two single-workgroup launches per list."""
    B, f = active.shape[0], active.shape[-1]
    lib = _lib.lib()
    tls = list(tile_lists)
    cells = None
    if pixel_lists:
        assert all(pl.H == pl.W for pl in pixel_lists)
        cells = TileList(active, f, f, 1, 1, defer=True)            # tiles of one patch: entries (b*f + fy)*f + fx
        tls = tls + [cells]
    mx = lib.cmu_sparse_tile_lists_max()
    for i in range(0, len(tls), mx):
        part = tls[i:i + mx]
        n = len(part)
        IA, PA = ctypes.c_int * n, ctypes.c_void_p * n
        call("cmu_sparse_tile_lists", _p(active), f, B, n, IA(*[t.H for t in part]), IA(*[t.tile_h for t in part]),
             IA(*[t.tile_w for t in part]), PA(*[t.list.data_ptr() for t in part]), PA(*[t.count.data_ptr() for t in part]), _stream())
    pls = list(pixel_lists)
    for i in range(0, len(pls), mx):
        part = pls[i:i + mx]
        n = len(part)
        IA, PA, LA = ctypes.c_int * n, ctypes.c_void_p * n, ctypes.c_int64 * n
        call("cmu_sparse_pixel_lists", _p(cells.list), _p(cells.count), f, B, n, IA(*[pl.H for pl in part]),
             PA(*[pl.rows.data_ptr() for pl in part]), LA(*[pl.capacity for pl in part]), PA(*[pl.count.data_ptr() for pl in part]), _stream())
    return cells


def conv3x3_rows_supported(B, H, W, Cin, Cout, dt):
    return bool(_lib.lib().cmu_conv3x3_rows_supported(B, H, W, Cin, Cout, dt_code(dt)))


def conv3x3_fwd_rows(x, wpacked, out, pixels):
    """3x3 convolution at the listed pixels only (gather-GEMM, csrc/conv_gather.inc); ``out`` elsewhere untouched.  ``x`` carries no
    pending transform (the sparse encoder's inputs are already activated and masked)."""
    assert x.dt == out.dt and (x.B, x.H, x.W) == (out.B, out.H, out.W) and x.scale is None
    call("cmu_conv3x3_fwd_rows", x.ptr(), x.ld, _p(wpacked), out.ptr(), out.ld, _p(pixels.rows), _p(pixels.count), pixels.capacity,
         x.B, x.H, x.W, x.C, out.C, x.dt, _stream(), work=2.0 * 9 * x.C * out.C * pixels.max_rows)


def conv3x3_tiles_supported(B, H, W, Cin, Cout, dt):
    return bool(_lib.lib().cmu_conv3x3_tiles_supported(B, H, W, Cin, Cout, dt_code(dt)))


def conv3x3_fwd_tiles(x, wpacked, out, tiles, active_fraction=1.0):
    """conv3x3_fwd over the listed 16 x 32 tiles only (``out`` elsewhere untouched).  ``active_fraction``: share of listed
    tiles, for the profiler's algorithmic FLOP count only."""
    assert x.dt == out.dt and (x.B, x.H, x.W) == (out.B, out.H, out.W) and (tiles.tile_h, tiles.tile_w) == (16, 32)
    call("cmu_conv3x3_fwd_tiles", x.ptr(), x.ld, _p(x.scale), _p(x.shift), x.relu_from, _p(wpacked), out.ptr(), out.ld,
         _p(tiles.list), _p(tiles.count), x.B, x.H, x.W, x.C, out.C, x.dt, _stream(),
         work=2.0 * 9 * x.C * out.C * x.B * x.H * x.W * active_fraction)


def conv3x3_wgrad_tile_h(B, H, W, Cin, Cout, dt):
    """Tile height of the list ``conv3x3_wgrad_tiles`` wants for this shape: 8 (8 x 16 tiles, wide kernel) or 16 (16 x 16 tiles)."""
    return int(_lib.lib().cmu_conv3x3_wgrad_tile_h(B, H, W, Cin, Cout, dt_code(dt)))


def conv3x3_wgrad_tiles(x, dY, dW, ws, tiles, active_fraction=1.0):
    """Weight gradient with the contraction restricted to the listed tiles (``dY`` is zero elsewhere): 16 x 16 tiles on the first
    kernel, 8 x 16 tiles on the wide kernel (``conv3x3_wgrad_tile_h`` says which list a shape wants)."""
    Cout, Cin = dW.shape[0], dW.shape[1]
    assert x.C == Cin and dY.C == Cout and tiles.tile_w == 16 and tiles.tile_h in (8, 16)
    call("cmu_conv3x3_wgrad_tiles", x.ptr(), x.ld, _p(x.scale), _p(x.shift), x.relu_from, dY.ptr(), dY.ld, _p(_f32c(dW)),
         _p(tiles.list), _p(tiles.count), tiles.tile_h, x.B, x.H, x.W, Cin, Cout, x.dt, _p(ws), _stream(),
         work=2.0 * 9 * Cin * Cout * x.B * x.H * x.W * active_fraction)


def spark_loss_fwd_bwd(rec, img, active, loss, drec, loss_scale, p, ws):
    B, f = active.shape[0], active.shape[-1]
    call("cmu_spark_loss_fwd_bwd", _p(_f32c(rec)), _p(_f32c(img)), _p(active), _p(loss), _p(drec), float(loss_scale), B, f, p, _p(ws),
         _stream())


def gap_fwd(y, out):
    call("cmu_gap_fwd", y.ptr(), y.ld, _p(y.scale), _p(y.shift), _p(_f32c(out)), y.B, y.H, y.W, y.C, y.dt, _stream())


def gap_bwd(dout, dA):
    call("cmu_gap_bwd", _p(_f32c(dout)), dA.ptr(), dA.ld, dA.B, dA.H, dA.W, dA.C, dA.dt, _stream())


# bumped whenever a raw kernel rewrites parameters in place (PyTorch's version counters do not see it);
# the engine's packed-weight caches compare it together with Tensor._version
PARAM_GENERATION = 0


def bump_param_generation():
    """Call after any raw or bulk write into a parameter arena that PyTorch's version counters do not see (a collective into
    the arena, a checkpoint copied into it): the engine's packed-weight caches key on this counter."""
    global PARAM_GENERATION
    PARAM_GENERATION += 1


def ema_update(target, online, momentum):
    global PARAM_GENERATION
    PARAM_GENERATION += 1
    assert target.numel() == online.numel()
    call("cmu_ema_update", _p(_f32c(target)), _p(_f32c(online)), target.numel(), float(momentum), _stream())


def adam_step(p, g, m, v, wd_mask, lr, beta1, beta2, eps, weight_decay, decoupled, step, grad_scale=1.0, amp=None):
    global PARAM_GENERATION
    PARAM_GENERATION += 1
    call("cmu_adam_step", _p(_f32c(p)), _p(_f32c(g)), _p(_f32c(m)), _p(_f32c(v)), _p(wd_mask), p.numel(), float(lr),
         float(beta1), float(beta2), float(eps), float(weight_decay), int(decoupled), int(step), float(grad_scale),
         _p(None if amp is None else amp.state), _stream())


def adam_ema_step(p, g, m, v, wd_mask, lr, beta1, beta2, eps, weight_decay, decoupled, step, grad_scale, amp, segments, momentum):
    """``adam_step`` + the EMA of the momentum networks in one pass (cmu_adam_ema_step).  ``segments``: up to two
    (lo, hi, target fp32 tensor of hi - lo elements), ascending element ranges of the arena ``p``."""
    global PARAM_GENERATION
    PARAM_GENERATION += 1
    n = len(segments)
    assert 1 <= n <= 2
    lo = (ctypes.c_int64 * n)(*[int(s[0]) for s in segments])
    hi = (ctypes.c_int64 * n)(*[int(s[1]) for s in segments])
    for s in segments:
        assert s[2].numel() == s[1] - s[0] and s[2].device == p.device
    tg = (ctypes.c_void_p * n)(*[_f32c(s[2]).data_ptr() for s in segments])
    call("cmu_adam_ema_step", _p(_f32c(p)), _p(_f32c(g)), _p(_f32c(m)), _p(_f32c(v)), _p(wd_mask), p.numel(), float(lr),
         float(beta1), float(beta2), float(eps), float(weight_decay), int(decoupled), int(step), float(grad_scale),
         _p(None if amp is None else amp.state), n, lo, hi, tg, float(momentum), _stream())


class AmpScaler:
    """Dynamic loss scaler with its state on the device (cmu_amp_*): torch.cuda.amp.GradScaler's protocol -- what mmengine's
    AmpOptimWrapper(loss_scale='dynamic') wraps (cmunet_config.py:76-78) -- without the per-step host read of found_inf."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval
        self.state = torch.zeros(_lib.lib().cmu_amp_state_bytes(), dtype=torch.uint8, device=device)
        call("cmu_amp_init", _p(self.state), float(init_scale), _stream())

    def check(self, grad_arena):
        call("cmu_amp_check_finite", _p(_f32c(grad_arena)), grad_arena.numel(), _p(self.state), _stream())

    def update(self):
        call("cmu_amp_update", _p(self.state), float(self.growth_factor), float(self.backoff_factor), int(self.growth_interval), _stream())

    def read(self):
        """(scale, found_inf, growth_tracker, good_steps, skipped_steps) -- synchronises; for logging and tests."""
        raw = self.state.cpu()
        f = raw[:8].view(torch.float32)
        i = raw[8:20].view(torch.int32)
        return float(f[0]), float(f[1]), int(i[0]), int(i[1]), int(i[2])

    def state_dict(self):
        """GradScaler.state_dict's fields (mmengine's AmpOptimWrapper saves them as ``loss_scaler``) plus the two counters the
        optimiser kernel reads: ``good_steps`` is the step number of Adam's bias corrections, so a resume without it would
        restart them at 1 on steady-state moments (first updates ~2x too large at betas (0.9, 0.95)).  Synchronises."""
        scale, _, tracker, good, skipped = self.read()
        return {"scale": scale, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": tracker, "good_steps": good, "skipped_steps": skipped}

    def load_state_dict(self, sd):
        import struct
        self.growth_factor = sd.get("growth_factor", self.growth_factor)
        self.backoff_factor = sd.get("backoff_factor", self.backoff_factor)
        self.growth_interval = sd.get("growth_interval", self.growth_interval)
        raw = struct.pack("<ffiii", float(sd["scale"]), 0.0, int(sd.get("_growth_tracker", 0)), int(sd.get("good_steps", 0)),
                          int(sd.get("skipped_steps", 0)))
        raw = raw + b"\0" * (self.state.numel() - len(raw))
        self.state.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))


def sgd_step(p, g, buf, wd_mask, lr, momentum, dampening, weight_decay, nesterov, step, grad_scale=1.0):
    global PARAM_GENERATION
    PARAM_GENERATION += 1
    call("cmu_sgd_step", _p(_f32c(p)), _p(_f32c(g)), _p(buf), _p(wd_mask), p.numel(), float(lr), float(momentum), float(dampening),
         float(weight_decay), int(nesterov), int(step), float(grad_scale), _stream())


def sgd_step_amp(p, g, buf, wd_mask, lr, momentum, dampening, weight_decay, nesterov, step, grad_scale, amp):
    """``sgd_step`` skipped / unscaled from the device state of ``amp`` (an ``AmpScaler``)."""
    global PARAM_GENERATION
    PARAM_GENERATION += 1
    call("cmu_sgd_step_amp", _p(_f32c(p)), _p(_f32c(g)), _p(buf), _p(wd_mask), p.numel(), float(lr), float(momentum), float(dampening),
         float(weight_decay), int(nesterov), int(step), float(grad_scale), _p(amp.state), _stream())


def lamb_step(p, g, m, v, u, tables, lr, beta1, beta2, eps, bias_correction, grad_averaging, max_grad_norm, trust_clip,
              always_adapt, step, grad_scale, ws):
    """``tables`` = (blk_start int64, blk_count int32, blk_tensor int32, t_blk0 int32 [T+1], t_wd float32 [T]) on the device."""
    global PARAM_GENERATION
    PARAM_GENERATION += 1
    bs, bc, bt, t0, twd = tables
    call("cmu_lamb_step", _p(_f32c(p)), _p(_f32c(g)), _p(m), _p(v), _p(u), _p(bs), _p(bc), _p(bt), bs.numel(), _p(t0), _p(twd),
         twd.numel(), float(lr), float(beta1), float(beta2), float(eps), int(bias_correction), int(grad_averaging),
         float(max_grad_norm), int(trust_clip), int(always_adapt), int(step), float(grad_scale), _p(ws), _stream())


# ---- input pipeline on the device ---------------------------------------------------------------------
def resize_bicubic(src, out_h, out_w, boxes=None, flip=None):
    """Pillow-convention bicubic resize of per-sample crop windows (+ optional horizontal flip): src (B,H,W) f32 (PIL mode 'F') or
    uint8 (mode 'L': Pillow's 22-bit fixed-point path) cuda, boxes (B,4) int32 (x0, y0, w, h) or None, flip (B,) uint8/bool or
    None -> (B,out_h,out_w) of src's dtype."""
    assert src.dtype in (torch.float32, torch.uint8) and src.dim() == 3 and src.is_contiguous()
    u8 = src.dtype == torch.uint8
    B, H, W = src.shape
    if boxes is not None:
        bh = boxes.detach().cpu().to(torch.int64)
        ok = (bh[:, 0] >= 0) & (bh[:, 1] >= 0) & (bh[:, 2] >= 1) & (bh[:, 3] >= 1) & (bh[:, 0] + bh[:, 2] <= W) & (bh[:, 1] + bh[:, 3] <= H)
        if bh.shape != (B, 4) or not bool(ok.all()):
            raise ValueError("resize_bicubic: crop windows must be (B,4) (x0, y0, w, h) inside the image")
        boxes = boxes.to(device=src.device, dtype=torch.int32).contiguous()
    if flip is not None:
        flip = flip.to(device=src.device, dtype=torch.uint8).contiguous()
    out = torch.empty(B, out_h, out_w, dtype=src.dtype, device=src.device)
    entry = "cmu_resize_bicubic_u8" if u8 else "cmu_resize_bicubic"
    ws = workspace(entry + "_ws_bytes", src.device, B, H, W, out_h, out_w)
    call(entry, _p(src), B, H, W, _p(boxes), _p(flip), _p(out), out_h, out_w, _p(ws), _stream())
    return out


def resize_nearest(src, out_h, out_w):
    """``Image.resize(size, NEAREST)`` of a batch of uint8 label masks (Finetuning/dataset.py:47): src (B,H,W) uint8 cuda ->
    (B,out_h,out_w) uint8."""
    assert src.dtype == torch.uint8 and src.dim() == 3 and src.is_contiguous()
    B, H, W = src.shape
    out = torch.empty(B, out_h, out_w, dtype=torch.uint8, device=src.device)
    ws = workspace("cmu_resize_nearest_u8_ws_bytes", src.device, out_h, out_w)
    call("cmu_resize_nearest_u8", _p(src), B, H, W, _p(out), out_h, out_w, _p(ws), _stream())
    return out


def two_view(src, shifts, out=224, noise=None, seed=0):
    """ShiftPixel crops + GaussNoise: src (B,S,S) f32 cuda, shifts (B,2) int (dy, dx) -> (img, img_t) (B,out,out) f32.
    ``noise``: (B,out,out) float64 standard-normal draws, or None for the in-kernel Philox generator keyed by ``seed``."""
    assert src.dtype == torch.float32 and src.dim() == 3 and src.shape[1] == src.shape[2] and src.is_contiguous()
    B, S = src.shape[0], src.shape[1]
    sh = shifts.detach().cpu().to(torch.int64)
    if sh.shape != (B, 2) or bool((sh < 0).any()) or bool((sh + out > S).any()):
        raise ValueError("two_view: shifts must be (B,2) with 0 <= d and d + out <= S")      # processing.py:112-113 asserts
    shifts = shifts.to(device=src.device, dtype=torch.int32).contiguous()
    if noise is not None:
        assert noise.dtype == torch.float64 and tuple(noise.shape) == (B, out, out) and noise.is_contiguous()
    img = torch.empty(B, out, out, dtype=torch.float32, device=src.device)
    img_t = torch.empty_like(img)
    call("cmu_two_view", _p(src), B, S, _p(shifts), _p(noise), int(seed) & (2 ** 64 - 1), _p(img), _p(img_t), out, _stream())
    return img, img_t


def philox_normal(n, offset=0, seed=0, device="cuda"):
    out = torch.empty(n, dtype=torch.float64, device=device)
    call("cmu_philox_normal", _p(out), n, int(offset), int(seed) & (2 ** 64 - 1), _stream())
    return out


# ---- skinny GEMMs of the necks ----------------------------------------------------------------------------------
SKINNY_MAX_ROWS = 256      # csrc/skinny.hip SK_MAX_M: the reference's own batch size per GPU (cmunet_config.py:55, moco2_module.py:91)


def skinny_eligible(x, weight):
    """nn.Linear on <= SKINNY_MAX_ROWS fp32 rows with K % 8 == 0: what the weight-streaming kernels take (the product path has
    no other GEMM: callers raise on anything else)."""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 2
            and 1 <= x.shape[0] <= SKINNY_MAX_ROWS and x.shape[1] % 8 == 0 and x.shape[1] >= 8)


def _mm16(compute_dt, K, need):
    """16-bit-operand kernels apply for compute_dt f16 / bf16 when K allows; None / f32 -> the exact fp32 kernels."""
    if compute_dt is None:
        return None
    dt = dt_code(compute_dt)
    return dt if (dt in (F16, BF16) and K % need == 0) else None


def skinny_gemm_fwd(x, weight, bias=None, compute_dt=None):
    """``compute_dt`` 'f16' / 'bf16': operands rounded to that type in registers (the AMP arithmetic), fp32 accumulation."""
    x, weight = _f32c(x), _f32c(weight)
    M, K = x.shape
    N = weight.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    dt16 = _mm16(compute_dt, K, 16)
    b = _p(None if bias is None else _f32c(bias))
    if dt16 is not None:
        ws = workspace("cmu_skinny16_gemm_ws_bytes", x.device, M, N, K)
        call("cmu_skinny16_gemm_fwd", _p(x), _p(weight), b, _p(y), M, N, K, dt16, _p(ws), _stream(), work=2.0 * M * N * K)
    else:
        ws = workspace("cmu_skinny_gemm_ws_bytes", x.device, M, N, K)
        call("cmu_skinny_gemm_fwd", _p(x), _p(weight), b, _p(y), M, N, K, _p(ws), _stream(), work=2.0 * M * N * K)
    return y


def skinny_gemm_dgrad(dy, weight, compute_dt=None):
    dy, weight = _f32c(dy), _f32c(weight)
    M, N = dy.shape
    K = weight.shape[1]
    dx = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    dt16 = _mm16(compute_dt, K, 4)
    if dt16 is not None:
        call("cmu_skinny16_gemm_dgrad", _p(dy), _p(weight), _p(dx), M, N, K, dt16, _stream(), work=2.0 * M * N * K)
    else:
        ws = workspace("cmu_skinny_gemm_bwd_ws_bytes", dy.device, M, N)
        call("cmu_skinny_gemm_dgrad", _p(dy), _p(weight), _p(dx), M, N, K, _p(ws), _stream(), work=2.0 * M * N * K)
    return dx


def skinny_gemm_wgrad(dy, x, with_bias=False, compute_dt=None, out=None):
    """``out``: optional preallocated (N, K) fp32 tensor (a view of a trainer's gradient arena)."""
    dy, x = _f32c(dy), _f32c(x)
    M, N = dy.shape
    K = x.shape[1]
    dw = out if out is not None else torch.empty(N, K, dtype=torch.float32, device=dy.device)
    assert dw.shape == (N, K) and dw.dtype == torch.float32 and dw.is_contiguous()
    db = torch.empty(N, dtype=torch.float32, device=dy.device) if with_bias else None
    dt16 = _mm16(compute_dt, K, 4)
    if dt16 is not None:
        call("cmu_skinny16_gemm_wgrad", _p(dy), _p(x), _p(dw), _p(db), M, N, K, dt16, _stream(), work=2.0 * M * N * K)
    else:
        call("cmu_skinny_gemm_wgrad", _p(dy), _p(x), _p(dw), _p(db), M, N, K, _stream(), work=2.0 * M * N * K)
    return dw, db


# ---- BatchNorm1d (+ ReLU) of the necks and the target latent's 1x1 reduction (csrc/necks.hip) ---------------------------------
def bn1d_colsums(x):
    M, N = x.shape
    sums = torch.empty(2, N, dtype=torch.float32, device=x.device)
    call("cmu_bn1d_colsums", _p(_f32c(x)), _p(sums), M, N, _stream())
    return sums


def bn1d_relu_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, training, relu, sums=None, count=0):
    M, N = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(N, dtype=torch.float32, device=x.device)
    invstd = torch.empty(N, dtype=torch.float32, device=x.device)
    call("cmu_bn1d_relu_fwd", _p(_f32c(x)), _p(sums), int(count), _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(momentum),
         float(eps), int(training), int(relu), _p(y), _p(mean), _p(invstd), M, N, _stream())
    return y, mean, invstd


def bn1d_bwd_colsums(dy, x, y, mean, invstd, relu):
    M, N = x.shape
    sums = torch.empty(2, N, dtype=torch.float32, device=x.device)
    call("cmu_bn1d_bwd_colsums", _p(_f32c(dy)), _p(x), _p(y), _p(mean), _p(invstd), int(relu), _p(sums), M, N, _stream())
    return sums


def bn1d_relu_bwd(dy, x, y, mean, invstd, gamma, relu, sums=None, count=0, affine=True):
    M, N = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(N, dtype=torch.float32, device=x.device) if affine else None
    db = torch.empty(N, dtype=torch.float32, device=x.device) if affine else None
    call("cmu_bn1d_relu_bwd", _p(_f32c(dy)), _p(x), _p(y), _p(mean), _p(invstd), _p(gamma), int(relu), _p(sums), int(count), _p(dx), _p(dg),
         _p(db), M, N, _stream())
    return dx, dg, db


def conv1x1_nchw_fwd(x, weight, bias=None):
    """x: Act (NHWC + pending transform); weight (N, K) or (N, K, 1, 1) fp32 -> (B, N, H, W) fp32."""
    w = _f32c(weight.reshape(weight.shape[0], -1))
    N, K = w.shape
    assert K == x.C
    out = torch.empty(x.B, N, x.H, x.W, dtype=torch.float32, device=x.buf.device)
    call("cmu_conv1x1_nchw_fwd", x.ptr(), x.ld, _p(x.scale), _p(x.shift), x.relu_from, _p(w), _p(None if bias is None else _f32c(bias)),
         _p(out), x.B, x.H, x.W, K, N, x.dt, _stream(), work=2.0 * K * N * x.B * x.H * x.W)
    return out


def random_patch_mask(B, H, W, patch_size=16, mask_ratio=0.65, seed=0, offset=0, device="cuda"):
    """UNet_encoder.create_random_patch_mask (UNet_encoder.py:106-139) in one kernel: (B,H,W) uint8, 1 = masked,
    floor(ratio*H*W / patch^2) patches per sample, reproducible from (seed, offset)."""
    n_mask = int(mask_ratio * H * W) // (patch_size * patch_size)
    m = torch.empty(B, H, W, dtype=torch.uint8, device=device)
    call("cmu_random_patch_mask", _p(m), B, H, W, patch_size, n_mask, int(seed) & (2 ** 64 - 1), int(offset), _stream())
    return m


# ---- connected components of label maps (csrc/components.hip) ---------------------------------
CC_MAX_KEEP = 8


def _cc_check(what, t, dtype):
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs on the GPU only; there is no CPU fallback in this package")
    if t.dtype != dtype or t.dim() != 3 or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous (B,H,W) {dtype} tensor, got {tuple(t.shape)} {t.dtype}")
    B, H, W = t.shape
    if B < 1 or H < 1 or W < 1 or H * W >= 2 ** 31 or B > 65535:
        raise ValueError(f"{what}: 1 <= B <= 65535, 1 <= H, W and H * W < 2**31, got {tuple(t.shape)}")
    return B, H, W


def label_components(src, cls=-1, connectivity=8):
    """src (B,H,W) uint8 -> (labels (B,H,W) int32, counts (B,) int32).  Foreground: ``src == cls`` (0..255), ``src != 0`` (-1) or
    ``src != c`` (cls = -2 - c).  labels: 0 on background, else 1 + the smallest row-major index of the pixel's component."""
    B, H, W = _cc_check("label_components", src, torch.uint8)
    if connectivity not in (4, 8):
        raise ValueError(f"label_components: connectivity must be 4 or 8, got {connectivity!r}")
    if not -257 <= int(cls) <= 255:
        raise ValueError(f"label_components: cls in 0..255, -1 or -2 - c, got {cls}")
    labels = torch.empty(B, H, W, dtype=torch.int32, device=src.device)
    counts = torch.empty(B, dtype=torch.int32, device=src.device)
    ws = workspace("cmu_label_components_ws_bytes", src.device, B, H, W)
    call("cmu_label_components", _p(src), int(cls), int(connectivity), _p(labels), _p(counts), B, H, W, _p(ws), _stream())
    return labels, counts


def component_sizes(labels):
    """labels (B,H,W) int32 -> sizes (B,H,W) int32: flat entry r of an image holds the pixel count of label r + 1."""
    B, H, W = _cc_check("component_sizes", labels, torch.int32)
    sizes = torch.empty_like(labels)
    call("cmu_component_sizes", _p(labels), _p(sizes), B, H, W, _stream())
    return sizes


def select_largest(sizes, n):
    """sizes (B,H,W) int32 -> (B,n) int32: labels of the n largest components per image (ties: smaller label), -1 when unused."""
    B, H, W = _cc_check("select_largest", sizes, torch.int32)
    if not 1 <= int(n) <= CC_MAX_KEEP:
        raise ValueError(f"select_largest: n must lie in 1..{CC_MAX_KEEP}, got {n}")
    keep = torch.empty(B, int(n), dtype=torch.int32, device=sizes.device)
    call("cmu_select_largest", _p(sizes), int(n), _p(keep), B, H, W, _stream())
    return keep


def border_components(labels):
    """labels (B,H,W) int32 -> (B,H,W) uint8: flat entry r of an image is 1 iff label r + 1 has a pixel on the image's frame."""
    B, H, W = _cc_check("border_components", labels, torch.int32)
    touches = torch.empty(B, H, W, dtype=torch.uint8, device=labels.device)
    call("cmu_border_components", _p(labels), _p(touches), B, H, W, _stream())
    return touches


def filter_components(src, cls, labels=None, sizes=None, min_size=0, keep_roots=None, removed_value=0, hole_labels=None,
                      hole_touches=None, class_values=None):
    """One pass over src (B,H,W) uint8 -> a new uint8 map: components of ``labels`` below ``min_size`` or missing from ``keep_roots``
    receive ``removed_value``; pixels of ``hole_labels`` components that do not touch the frame receive ``cls``; ``class_values``
    (uint8 device table) maps the result."""
    B, H, W = _cc_check("filter_components", src, torch.uint8)
    if int(min_size) < 0:
        raise ValueError(f"filter_components: min_size must be >= 0, got {min_size}")
    n_keep = 0 if keep_roots is None else int(keep_roots.shape[1])
    out = torch.empty_like(src)
    call("cmu_filter_components", _p(src), int(cls), _p(labels), _p(sizes), min(int(min_size), 2 ** 31 - 1), _p(keep_roots), n_keep,
         int(removed_value), _p(hole_labels), _p(hole_touches), _p(class_values), 0 if class_values is None else class_values.numel(),
         _p(out), B, H, W, _stream())
    return out


# ---- exact Euclidean distance transform, disk morphology, surface distances (csrc/edt.hip) -----
EDT_MAX_SIDE = 4096      # CMU_EDT_MAX_SIDE: 2 * 4095**2 < 2**31


def _edt_check(what, t, dtype, cls=-1):
    B, H, W = _cc_check(what, t, dtype)
    if H > EDT_MAX_SIDE or W > EDT_MAX_SIDE:
        raise ValueError(f"{what}: H, W <= {EDT_MAX_SIDE}, got {tuple(t.shape)}")
    if isinstance(cls, bool) or int(cls) != cls or not -257 <= int(cls) <= 255:
        raise ValueError(f"{what}: cls in 0..255, -1 or -2 - c, got {cls!r}")
    return B, H, W


def _edt_scratch(what, name, t, like, dtype):
    """A caller's scratch / output tensor, or a fresh one: contiguous, ``like``'s shape and device."""
    if t is None:
        return torch.empty(like.shape, dtype=dtype, device=like.device)
    if t.dtype != dtype or t.shape != like.shape or not t.is_contiguous() or t.device != like.device:
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {tuple(like.shape)} on the map's device")
    return t


def edt_columns(src, cls=-1, border=False, g=None):
    """src (B,H,W) uint8 -> g (B,H,W) int32: the vertical distance to the nearest site of the pixel's column, 16384 where the column
    has none.  Sites: the rule ``cls`` (the codes of ``label_components``), or with ``border`` the rule's border pixels."""
    B, H, W = _edt_check("edt_columns", src, torch.uint8, cls)
    g = _edt_scratch("edt_columns", "g", g, src, torch.int32)
    call("cmu_edt_columns", _p(src), int(cls), int(bool(border)), _p(g), B, H, W, _stream())
    return g


def edt_rows(g, want="dist2", base=None, greater=False, t=0, v_hit=-1, v_miss=-1, out=None):
    """The row pass over ``g`` of ``edt_columns``.  ``want``: 'dist2' -> int32 squared distances (-1: the image has no site); 'dist' ->
    float32 roots (inf); 'map' -> uint8: a site keeps ``base``; another pixel with dist2 <= t (``greater``: dist2 > t, -1 infinitely
    far) receives ``v_hit``, else ``v_miss``; -1 keeps ``base``."""
    B, H, W = _edt_check("edt_rows", g, torch.int32)
    if want not in ("dist2", "dist", "map"):
        raise ValueError(f"edt_rows: want must be 'dist2', 'dist' or 'map', got {want!r}")
    if want != "map":
        out = _edt_scratch("edt_rows", "out", out, g, torch.int32 if want == "dist2" else torch.float32)
        call("cmu_edt_rows", _p(g), _p(out if want == "dist2" else None), _p(out if want == "dist" else None), None, None, 0, 0, -1, -1,
             B, H, W, _stream())
        return out
    if base is None or base.dtype != torch.uint8 or base.shape != g.shape or not base.is_contiguous() or base.device != g.device:
        raise ValueError(f"edt_rows: base must be a contiguous uint8 tensor of shape {tuple(g.shape)} on g's device")
    if not (0 <= int(t) < 2 ** 31 and -1 <= int(v_hit) <= 255 and -1 <= int(v_miss) <= 255):
        raise ValueError(f"edt_rows: 0 <= t < 2**31 and v_hit, v_miss in -1..255, got {t}, {v_hit}, {v_miss}")
    out = _edt_scratch("edt_rows", "out", out, g, torch.uint8)
    call("cmu_edt_rows", _p(g), None, None, _p(base), _p(out), int(bool(greater)), int(t), int(v_hit), int(v_miss), B, H, W, _stream())
    return out


def surface_border(src, cls=-1):
    """src (B,H,W) uint8 -> (B,H,W) uint8: 1 on the pixels of the rule's set that have a 4-neighbour outside the set or the image."""
    B, H, W = _edt_check("surface_border", src, torch.uint8, cls)
    out = torch.empty_like(src)
    call("cmu_surface_border", _p(src), int(cls), _p(out), B, H, W, _stream())
    return out


def surface_reduce(src, dist2, tol2=0, cls=-1, masked=None, want_masked=True):
    """Over the border pixels of ``src``'s set, ``dist2`` being the transform to another border -> (sums (B,2) float64 = (sum of the
    roots, root of the largest), counts (B,3) int32 = (n, max dist2, number <= tol2), masked (B,H,W) int32 = dist2 on the border pixels and -2 elsewhere, or None)."""
    B, H, W = _edt_check("surface_reduce", src, torch.uint8, cls)
    if dist2.dtype != torch.int32 or dist2.shape != src.shape or not dist2.is_contiguous() or dist2.device != src.device:
        raise ValueError(f"surface_reduce: dist2 must be a contiguous int32 tensor of shape {tuple(src.shape)} on the map's device")
    if not 0 <= int(tol2) < 2 ** 31:
        raise ValueError(f"surface_reduce: 0 <= tol2 < 2**31, got {tol2}")
    if want_masked or masked is not None:
        masked = _edt_scratch("surface_reduce", "masked", masked, src, torch.int32)
    sums = torch.empty(B, 2, dtype=torch.float64, device=src.device)
    counts = torch.empty(B, 3, dtype=torch.int32, device=src.device)
    call("cmu_surface_reduce", _p(src), int(cls), _p(dist2), int(tol2), _p(masked), _p(sums), _p(counts), B, H, W, _stream())
    return sums, counts, masked


def surface_select(masked_a, masked_b, ranks):
    """The ``ranks[b, r]``-th smallest (from 0) non-negative entry of image b of both masked maps together -> (values (B,R) int32, -1 if
    there are not that many; roots (B,R) float64, inf there).  ``ranks``: (B,R) int32 on the device, R = 1 or 2."""
    B, H, W = _edt_check("surface_select", masked_a, torch.int32)
    if masked_b.dtype != torch.int32 or masked_b.shape != masked_a.shape or not masked_b.is_contiguous() or masked_b.device != masked_a.device:
        raise ValueError("surface_select: both masked maps must be contiguous int32 tensors of one shape on one device")
    if ranks.dtype != torch.int32 or ranks.dim() != 2 or ranks.shape[0] != B or ranks.shape[1] not in (1, 2) or not ranks.is_contiguous() \
            or ranks.device != masked_a.device:
        raise ValueError(f"surface_select: ranks must be a contiguous (B,1) or (B,2) int32 tensor on the maps' device, got {tuple(ranks.shape)} {ranks.dtype}")
    R = int(ranks.shape[1])
    vals = torch.empty(B, R, dtype=torch.int32, device=masked_a.device)
    roots = torch.empty(B, R, dtype=torch.float64, device=masked_a.device)
    call("cmu_surface_select", _p(masked_a), _p(masked_b), _p(ranks), R, _p(vals), _p(roots), B, H, W, _stream())
    return vals, roots


# ---- image preprocessing (csrc/preprocess.hip) ------------------------------------------------
PRE_MAX_RADIUS = CONST["CMU_PRE_MAX_RADIUS"]      # the largest Gaussian radius of the unsharp mask (half-width 64)


def _pre_check(what, t):
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs on the GPU only; there is no CPU fallback in this package")
    if t.dtype not in (torch.uint8, torch.float32) or t.dim() != 3 or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous (B,H,W) uint8 or float32 tensor, got {tuple(t.shape)} {t.dtype}")
    B, H, W = t.shape
    if B < 1 or H < 1 or W < 1 or H * W >= 2 ** 31 or B > 65535:
        raise ValueError(f"{what}: 1 <= B <= 65535, 1 <= H, W and H * W < 2**31, got {tuple(t.shape)}")
    return B, H, W, int(t.dtype == torch.uint8)


def _pre_stats_arg(what, stats, B, device):
    if stats.dtype != torch.float64 or tuple(stats.shape) != (B, 4) or not stats.is_contiguous() or stats.device != device:
        raise ValueError(f"{what}: stats must be a contiguous (B,4) float64 tensor on the image's device, got {tuple(stats.shape)} {stats.dtype}")
    return stats


def pre_stats(x):
    """x (B,H,W) uint8 / float32 -> (B,4) float64: mean, population standard deviation, min, max of every image."""
    B, H, W, u8 = _pre_check("pre_stats", x)
    stats = torch.empty(B, 4, dtype=torch.float64, device=x.device)
    call("cmu_pre_stats", _p(x), u8, _p(stats), B, H, W, _stream())
    return stats


def pre_standardize(x, stats):
    """float32((float64(x) - stats[b,0]) / stats[b,1])."""
    B, H, W, u8 = _pre_check("pre_standardize", x)
    out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    call("cmu_pre_standardize", _p(x), u8, _p(_pre_stats_arg("pre_standardize", stats, B, x.device)), _p(out), B, H, W, _stream())
    return out


def pre_minmax(x, stats):
    """(x - stats[b,2]) / float32(stats[b,3] - stats[b,2]) in the reference's arithmetic (one float32 division)."""
    B, H, W, u8 = _pre_check("pre_minmax", x)
    out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    call("cmu_pre_minmax", _p(x), u8, _p(_pre_stats_arg("pre_minmax", stats, B, x.device)), _p(out), B, H, W, _stream())
    return out


def pre_row_normalize(x):
    """Every row over its Euclidean norm (float64), a zero row unchanged; float32."""
    B, H, W, u8 = _pre_check("pre_row_normalize", x)
    out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    call("cmu_pre_row_normalize", _p(x), u8, _p(out), B, H, W, _stream())
    return out


def pre_unsharp(x, weights, amount, scale_div=1.0, clip=False, stats=None, tmp=None):
    """The two passes of the unsharp mask: ``weights`` (lw + 1,) float32 on the device (tap at distance k), f = x / scale_div,
    out = f + (f - blur(f)) * amount, with ``clip`` clipped to [0,1] ([-1,1] where stats[b,2] < 0).  ``tmp``: the (B,H,W) float32
    plane between the passes (allocated when None)."""
    B, H, W, u8 = _pre_check("pre_unsharp", x)
    lw = int(weights.numel()) - 1
    if weights.dtype != torch.float32 or weights.dim() != 1 or not weights.is_contiguous() or not 0 <= lw <= 4 * PRE_MAX_RADIUS:
        raise ValueError(f"pre_unsharp: weights must be 1..{4 * PRE_MAX_RADIUS + 1} contiguous float32 taps")
    if tmp is None:
        tmp = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    elif tmp.dtype != torch.float32 or tuple(tmp.shape) != (B, H, W) or not tmp.is_contiguous():
        raise ValueError("pre_unsharp: tmp must be a contiguous float32 tensor of the image's shape")
    if stats is not None:
        _pre_stats_arg("pre_unsharp", stats, B, x.device)
    out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    call("cmu_pre_blur_rows", _p(x), u8, float(scale_div), _p(weights), lw, _p(tmp), B, H, W, _stream())
    call("cmu_pre_unsharp_cols", _p(x), u8, float(scale_div), _p(tmp), _p(weights), lw, float(amount), int(bool(clip)), _p(stats), _p(out),
         B, H, W, _stream())
    return out


def pre_crop(x, y0, x0, OH, OW):
    """x[:, y0:y0+OH, x0:x0+OW] as a new contiguous tensor (uint8 or float32)."""
    B, H, W, u8 = _pre_check("pre_crop", x)
    if not (OH >= 1 and OW >= 1 and 0 <= y0 and 0 <= x0 and y0 + OH <= H and x0 + OW <= W):
        raise ValueError(f"pre_crop: the window ({y0}, {x0}) + ({OH}, {OW}) leaves the {H} x {W} image")
    out = torch.empty(B, OH, OW, dtype=x.dtype, device=x.device)
    call("cmu_pre_crop", _p(x), 1 if u8 else 4, _p(out), B, H, W, int(y0), int(x0), int(OH), int(OW), _stream())
    return out


def pre_integrate_masks(masks):
    """masks (B,M,H,W) uint8 -> (B,H,W) uint8: 1 where any of the M masks is non-zero."""
    if not masks.is_cuda:
        raise RuntimeError("pre_integrate_masks runs on the GPU only; there is no CPU fallback in this package")
    if masks.dtype != torch.uint8 or masks.dim() != 4 or not masks.is_contiguous() or min(masks.shape) < 1 or masks.shape[0] > 65535:
        raise ValueError(f"pre_integrate_masks: a contiguous (B,M,H,W) uint8 tensor, got {tuple(masks.shape)} {masks.dtype}")
    B, M, H, W = masks.shape
    out = torch.empty(B, H, W, dtype=torch.uint8, device=masks.device)
    call("cmu_pre_integrate_masks", _p(masks), _p(out), B, M, H * W, _stream())
    return out


# probability histograms, threshold sweeps and calibration (csrc/prob_hist.hip, csrc/hist_curves.h)
HIST_MAX_K = CONST["CMU_HIST_MAX_K"]
HIST_MAX_BINS = CONST["CMU_HIST_MAX_BINS"]
HIST_SELECT = {"dice": 0, "fbeta": 0, "iou": 1, "youden": 2}
_HIST_TARGET_KINDS = {torch.float32: 0, torch.float64: 1, torch.uint8: 2}


def check_bins(what, bins):
    if isinstance(bins, bool) or int(bins) != bins or not 2 <= int(bins) <= HIST_MAX_BINS or int(bins) & (int(bins) - 1):
        raise ValueError(f"{what}: bins must be a power of two in 2..{HIST_MAX_BINS}, got {bins!r}")
    return int(bins)


def hist_buffers(rows_out, K, bins, device):
    """Zeroed (counts (Bout,K,2,bins+1) int64, conf (Bout,K,bins+1) uint64, invalid (Bout,K) int32) of cmu_prob_hist."""
    return (torch.zeros(rows_out, K, 2, bins + 1, dtype=torch.int64, device=device),
            torch.zeros(rows_out, K, bins + 1, dtype=torch.int64, device=device).view(torch.uint64),
            torch.zeros(rows_out, K, dtype=torch.int32, device=device))


def prob_hist(src, target, bins, from_logits, counts, conf, invalid, pooled=True, accumulate=False):
    """One pass of cmu_prob_hist: src (B,K,H,W) float32 logits (``from_logits``: the softmax of cmu_seg_stats_fwd, K = 1: the sigmoid)
    or probability planes; ``target`` float32 / float64 planes of src's shape (positive iff > 0.5) or a (B,H,W) uint8 label map.
    Adds into (``accumulate``) or overwrites counts / conf / invalid (``hist_buffers``'s shapes; Bout = 1 with ``pooled``, else B)."""
    for t in (src, target, counts, conf, invalid):
        if not t.is_cuda:
            raise RuntimeError("prob_hist runs on the GPU only; there is no CPU fallback in this package")
    bins = check_bins("prob_hist", bins)
    if src.dim() != 4 or src.dtype != torch.float32 or not 1 <= src.shape[1] <= HIST_MAX_K or min(src.shape) < 1:
        raise ValueError(f"prob_hist: src must be (B,K,H,W) float32 with 1 <= K <= {HIST_MAX_K}, got {tuple(src.shape)} {src.dtype}")
    if not src.is_contiguous() or not target.is_contiguous():
        raise ValueError("prob_hist: src and target must be contiguous")
    B, K, H, W = src.shape
    kind = _HIST_TARGET_KINDS.get(target.dtype)
    if kind is None or tuple(target.shape) != ((B, H, W) if kind == 2 else (B, K, H, W)):
        raise ValueError(f"prob_hist: the target is float32 / float64 planes of src's shape {tuple(src.shape)} or a (B,H,W) uint8 label "
                         f"map, got {tuple(target.shape)} {target.dtype}")
    Bout = 1 if pooled else B
    for name, t, shape, dt in (("counts", counts, (Bout, K, 2, bins + 1), (torch.int64,)), ("conf", conf, (Bout, K, bins + 1), (torch.uint64, torch.int64)),
                               ("invalid", invalid, (Bout, K), (torch.int32,))):
        if tuple(t.shape) != shape or t.dtype not in dt or not t.is_contiguous():
            raise ValueError(f"prob_hist: {name} must be a contiguous {shape} {dt[0]} tensor, got {tuple(t.shape)} {t.dtype}")
    call("cmu_prob_hist", _p(src), int(bool(from_logits)), _p(target), kind, _p(counts), _p(conf), _p(invalid), B, K, H, W, bins,
         int(bool(pooled)), int(bool(accumulate)), _stream())


def hist_curves(counts, conf=None, eps=1e-7, beta=1.0, select=0):
    """cmu_hist_curves of histogram rows counts (...,2,NB+1) int64 (+ conf (...,NB+1) uint64): (cum (...,4,NB+1) int64 = tp, fp, fn, tn at
    j / NB; scores (...,5,NB+1) float64 = F-beta, IoU, precision, recall, specificity; summary (...,6) float64 = AUROC, average
    precision, ECE, MCE, best j, the selected score there).  ``select``: 0 F-beta, 1 IoU, 2 Youden's J."""
    if not counts.is_cuda or (conf is not None and not conf.is_cuda):
        raise RuntimeError("hist_curves runs on the GPU only; there is no CPU fallback in this package")
    if counts.dtype != torch.int64 or counts.dim() < 2 or counts.shape[-2] != 2 or not counts.is_contiguous() or counts.numel() == 0:
        raise ValueError(f"hist_curves: counts must be a contiguous (...,2,NB+1) int64 tensor, got {tuple(counts.shape)} {counts.dtype}")
    bins = check_bins("hist_curves", counts.shape[-1] - 1)
    lead = tuple(counts.shape[:-2])
    if conf is not None and (tuple(conf.shape) != lead + (bins + 1,) or conf.dtype not in (torch.uint64, torch.int64) or not conf.is_contiguous()):
        raise ValueError(f"hist_curves: conf must be a contiguous {lead + (bins + 1,)} uint64 tensor, got {tuple(conf.shape)} {conf.dtype}")
    if select not in (0, 1, 2) or not eps >= 0 or not beta > 0:
        raise ValueError(f"hist_curves: select in 0..2, eps >= 0 and beta > 0 (got {select!r}, {eps!r}, {beta!r})")
    rows = counts.numel() // (2 * (bins + 1))
    cum = torch.empty(lead + (4, bins + 1), dtype=torch.int64, device=counts.device)
    scores = torch.empty(lead + (5, bins + 1), dtype=torch.float64, device=counts.device)
    summary = torch.empty(lead + (6,), dtype=torch.float64, device=counts.device)
    call("cmu_hist_curves", _p(counts), _p(conf), rows, bins, float(eps), float(beta), int(select), _p(cum), _p(scores), _p(summary), _stream())
    return cum, scores, summary


def threshold_mask(prob, threshold, v_pos=1, v_neg=0, out=None):
    """uint8 mask of prob's shape: ``v_pos`` where prob > threshold, else ``v_neg`` (a NaN: ``v_neg``); prob float32, contiguous."""
    if not prob.is_cuda:
        raise RuntimeError("threshold_mask runs on the GPU only; there is no CPU fallback in this package")
    if prob.dtype != torch.float32 or not prob.is_contiguous() or prob.numel() == 0:
        raise ValueError(f"threshold_mask: a non-empty contiguous float32 tensor, got {tuple(prob.shape)} {prob.dtype}")
    if not (0 <= int(v_pos) <= 255 and 0 <= int(v_neg) <= 255):
        raise ValueError(f"threshold_mask: v_pos and v_neg are bytes, got {v_pos!r}, {v_neg!r}")
    if out is None:
        out = torch.empty(prob.shape, dtype=torch.uint8, device=prob.device)
    elif out.dtype != torch.uint8 or out.shape != prob.shape or not out.is_contiguous() or out.device != prob.device:
        raise ValueError("threshold_mask: out must be a contiguous uint8 tensor of prob's shape on its device")
    call("cmu_threshold_mask", _p(prob), float(threshold), int(v_pos), int(v_neg), _p(out), prob.numel(), _stream())
    return out


# ---- focal cross entropy, map-weighted softmax sums, distance fields (csrc/map_loss.hip) -----
MAP_KINDS = {"linear": 0, "squared": 1}          # cmu_softmax_map_*: sum Wm p | sum Wm (p - y)^2
FIELD_MODES = {"signed": 0, "unsigned": 1}       # cmu_distance_field: Kervadec's signed distance | MONAI's field to the power alpha
MAP_LOSS_MAX_BLOCKS = 1024                       # the grid cap of the passes: ``partials`` holds columns x 1024 doubles


def map_loss_partials(columns, device):
    """The fp64 block-partial tensor of cmu_focal_fwd (3 columns) / cmu_softmax_map_fwd (K columns); needs no initialisation."""
    return torch.empty(columns * MAP_LOSS_MAX_BLOCKS, dtype=torch.float64, device=device)


def _focal_args(x, target, onehot, class_w, gamma):
    B, K, H, W, kind, _ = _ice_args(x, target, onehot, None, class_w)
    assert class_w is None or class_w.is_cuda
    gamma = float(gamma)
    assert 0.0 <= gamma <= 1e6, gamma
    return B, K, H, W, kind, gamma


def focal_fwd(x, target, onehot, class_w, gamma, ignore_index, table, partials=None):
    """table (3 fp64) = [sum alpha_t q^gamma (-log p_t) | sum alpha_t | pixels not ignored], q = 1 - p_t, of (B,K,H,W) fp32 logits
    against a (B,H,W) label plane, or (``onehot``) K planes whose arg-max is the label (cmu_focal_fwd)."""
    B, K, H, W, kind, gamma = _focal_args(x, target, onehot, class_w, gamma)
    assert table.dtype == torch.float64 and table.numel() == 3 and table.is_contiguous()
    if partials is None:
        partials = map_loss_partials(3, x.device)
    assert partials.dtype == torch.float64 and partials.numel() >= 3 * MAP_LOSS_MAX_BLOCKS and partials.is_contiguous()
    call("cmu_focal_fwd", _p(_f32c(x)), _p(target), kind, _p(class_w), gamma, int(ignore_index), _p(table), _p(partials), B, K, H, W,
         _stream())


def focal_bwd(x, target, onehot, class_w, gamma, ignore_index, g, dx):
    """dx (fp32) from the device-resident fp64 gradient g = d / d table[0]; None = zero."""
    B, K, H, W, kind, gamma = _focal_args(x, target, onehot, class_w, gamma)
    assert g is None or (g.dtype == torch.float64 and g.numel() == 1 and g.is_contiguous())
    assert dx.shape == x.shape
    call("cmu_focal_bwd", _p(_f32c(x)), _p(target), kind, _p(class_w), gamma, int(ignore_index), _p(g), _p(_f32c(dx)), B, K, H, W, _stream())


def _map_args(logits, wmap, y, keep, kind):
    B, K, H, W = logits.shape
    assert kind in MAP_KINDS, kind
    assert 2 <= K <= SEG_MAX_K
    keep = list(range(K)) if keep is None else list(keep)
    assert keep and keep == sorted(set(keep)) and 0 <= keep[0] and keep[-1] < K
    assert wmap is None or (wmap.shape == logits.shape and wmap.dtype == torch.float32 and wmap.is_contiguous() and wmap.is_cuda)
    if kind == "squared":
        assert y is not None and y.shape == logits.shape and y.is_contiguous() and y.is_cuda and y.dtype in (torch.float32, torch.float64)
    else:
        y = None
    return B, K, H, W, keep_mask(keep), MAP_KINDS[kind], y


def softmax_map_fwd(logits, wmap, y, keep, kind, table, partials=None):
    """table (K fp64): 'linear' T_c = sum Wm_c p_c, 'squared' T_c = sum Wm_c (p_c - y_c)^2 over the classes ``keep`` (0 for the others);
    Wm (B,K,H,W) fp32 or None = ones, y fp32 / fp64 (cmu_softmax_map_fwd)."""
    B, K, H, W, mask, k, y = _map_args(logits, wmap, y, keep, kind)
    assert table.dtype == torch.float64 and table.numel() == K and table.is_contiguous()
    if partials is None:
        partials = map_loss_partials(K, logits.device)
    assert partials.dtype == torch.float64 and partials.numel() >= K * MAP_LOSS_MAX_BLOCKS and partials.is_contiguous()
    call("cmu_softmax_map_fwd", _p(_f32c(logits)), _p(wmap), _p(y), int(y is not None and y.dtype == torch.float64), mask, k, _p(table),
         _p(partials), B, K, H, W, _stream())


def softmax_map_bwd(logits, wmap, y, keep, kind, g, dlogits):
    """dlogits_j = p_j (G_j - sum_c p_c G_c), G_c = g_c Wm_c ('linear') or 2 g_c Wm_c (p_c - y_c) ('squared'); g: K fp64 on the device."""
    B, K, H, W, mask, k, y = _map_args(logits, wmap, y, keep, kind)
    assert g is None or (g.dtype == torch.float64 and g.numel() == K and g.is_contiguous())
    assert dlogits.shape == logits.shape
    call("cmu_softmax_map_bwd", _p(_f32c(logits)), _p(wmap), _p(y), int(y is not None and y.dtype == torch.float64), mask, k, _p(g),
         _p(_f32c(dlogits)), B, K, H, W, _stream())


def distance_field(d2_to, d2_from, field, plane, mode="signed", alpha=2.0, d2_to_b=None, d2_from_b=None):
    """Plane ``plane`` of the (B,K,H,W) fp32 map ``field`` from the int32 squared distances of ``edt_rows`` to a set (``d2_to``) and to
    its complement (``d2_from``): 'signed' -> sqrt(d2_to) outside the set, 1 - sqrt(d2_from) inside; 'unsigned' -> the distance to the
    boundary to the power ``alpha``, plus that of a second pair when given.  An empty or a full set gives 0 (cmu_distance_field)."""
    if mode not in FIELD_MODES:
        raise ValueError(f"distance_field: mode must be 'signed' or 'unsigned', got {mode!r}")
    B, H, W = _edt_check("distance_field", d2_to, torch.int32)
    pairs = [d2_from] + ([] if d2_to_b is None and d2_from_b is None else [d2_to_b, d2_from_b])
    for t in pairs:
        if t is None or t.dtype != torch.int32 or t.shape != d2_to.shape or not t.is_contiguous() or t.device != d2_to.device:
            raise ValueError(f"distance_field: every distance map must be a contiguous int32 tensor of shape {tuple(d2_to.shape)} on one device")
    if len(pairs) == 3 and mode != "unsigned":
        raise ValueError("distance_field: a second pair of maps belongs to mode 'unsigned'")
    if mode == "unsigned" and not 0.0 < float(alpha) <= 16.0:
        raise ValueError(f"distance_field: 0 < alpha <= 16, got {alpha!r}")
    if (field.dim() != 4 or field.shape[0] != B or field.shape[2:] != (H, W) or field.dtype != torch.float32 or not field.is_contiguous()
            or field.device != d2_to.device):
        raise ValueError(f"distance_field: field must be a contiguous float32 (B,K,H,W) tensor over {(B, H, W)} on the maps' device")
    K = field.shape[1]
    if not 0 <= int(plane) < K:
        raise ValueError(f"distance_field: plane {plane} of {K}")
    call("cmu_distance_field", _p(d2_to), _p(d2_from), _p(d2_to_b), _p(d2_from_b), FIELD_MODES[mode], float(alpha), _p(field), int(plane),
         B, K, H, W, _stream())
    return field


# ---- segmented key sort and the Lovasz-Softmax loss (csrc/key_sort.hip, csrc/lovasz.hip) -----
def sort_tile_keys():
    """Keys per tile of ``sort_u64`` (cmu_sort_tile_keys): segments of up to that many keys need no scratch."""
    return int(_lib.lib().cmu_sort_tile_keys())


def _keys_check(what, name, t, shape, device):
    if t.dtype != torch.int64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{what}: {name} must be a contiguous int64 tensor of shape {tuple(shape)} on the keys' device")
    return t


def sort_u64(keys, out=None, scratch=None):
    """keys (S,n) int64 holding uint64 bit patterns -> ``out`` (S,n): every row sorted ascending AS UNSIGNED 64-bit integers
    (cmu_sort_u64).  ``scratch`` (S,n) is needed when n > ``sort_tile_keys()`` and allocated when not given; it may be ``keys``
    itself, which is then overwritten -- otherwise ``keys`` is left as it was."""
    if not keys.is_cuda:
        raise RuntimeError("sort_u64 runs on the GPU only; there is no CPU fallback in this package")
    if keys.dtype != torch.int64 or keys.dim() != 2 or keys.numel() == 0 or not keys.is_contiguous():
        raise ValueError(f"sort_u64: a non-empty contiguous (S,n) int64 tensor, got {tuple(keys.shape)} {keys.dtype}")
    S, n = keys.shape
    out = torch.empty_like(keys) if out is None else _keys_check("sort_u64", "out", out, keys.shape, keys.device)
    if n > sort_tile_keys():
        scratch = torch.empty_like(keys) if scratch is None else _keys_check("sort_u64", "scratch", scratch, keys.shape, keys.device)
        if scratch.data_ptr() == out.data_ptr():
            raise ValueError("sort_u64: out and scratch are two buffers")
    else:
        scratch = None
    if out.data_ptr() == keys.data_ptr():
        raise ValueError("sort_u64: out is a buffer of its own")
    call("cmu_sort_u64", _p(keys), _p(out), _p(scratch), S, n, _stream())
    return out


def lovasz_sizes(B, K, H, W, keep=None, per_image=False):
    """The tensor sizes of ``lovasz_keys`` / ``lovasz_grad`` in closed form: S segments of n pixels, ``rows`` = S x kept classes sorted
    rows of n keys, ``tiles`` = ceil(n / sort_tile_keys()) per row; counts holds S (K + 1) + 1 int64, out 1 + 2 S + S K fp64,
    tile_fg and partials rows x tiles each."""
    keep = list(range(K)) if keep is None else list(keep)
    S, n = (B, H * W) if per_image else (1, B * H * W)
    rows, tiles = S * len(keep), -(-n // sort_tile_keys())
    return {"S": S, "n": n, "rows": rows, "tiles": tiles, "counts": S * (K + 1) + 1, "out": 1 + 2 * S + S * K, "scratch": rows * tiles}


def _lovasz_args(x, keep, per_image):
    B, K, H, W = x.shape
    assert 2 <= K <= SEG_MAX_K and B <= 65535
    keep = list(range(K)) if keep is None else list(keep)
    assert keep and keep == sorted(set(keep)) and 0 <= keep[0] and keep[-1] < K
    sz = lovasz_sizes(B, K, H, W, keep, per_image)
    assert sz["n"] < 2 ** 31, "a segment holds fewer than 2^31 pixels"
    return B, K, H, W, keep_mask(keep), sz


def lovasz_keys(x, target, onehot, keep, per_image, ignore_index, keys, counts):
    """keys (rows,n) int64 = the sort keys of the Lovasz errors of (B,K,H,W) fp32 logits against a (B,H,W) label plane, or (``onehot``)
    K planes whose arg-max is the label; counts (S (K + 1) + 1 int64) = valid and per-class pixels of every segment, then the labels
    out of range (cmu_lovasz_keys; sizes: ``lovasz_sizes``)."""
    B, K, H, W, mask, sz = _lovasz_args(x, keep, per_image)
    kind = _ice_args(x, target, onehot, None, None)[4]
    assert keys.dtype == torch.int64 and keys.numel() == sz["rows"] * sz["n"] and keys.is_contiguous() and keys.is_cuda
    assert counts.dtype == torch.int64 and counts.numel() == sz["counts"] and counts.is_contiguous() and counts.is_cuda
    call("cmu_lovasz_keys", _p(_f32c(x)), _p(target), kind, mask, int(bool(per_image)), int(ignore_index), _p(keys), _p(counts), B, K, H, W,
         _stream())


def lovasz_grad(sorted_keys, counts, keep, per_image, classes_all, wmap, out, tile_fg=None, partials=None):
    """From the sorted rows of ``lovasz_keys``: wmap (B,K,H,W) fp32 = d loss / d p (-+ coef g at each pixel's rank), out (1 + 2 S + S K
    fp64) = [loss | L_s | coef_s | per-class losses]; ``classes_all``: every kept class counts, else those present in the segment
    (cmu_lovasz_grad).  tile_fg (int64) / partials (fp64): rows x tiles scratch each, allocated when not given."""
    B, K, H, W, mask, sz = _lovasz_args(wmap, keep, per_image)
    assert sorted_keys.dtype == torch.int64 and sorted_keys.numel() == sz["rows"] * sz["n"] and sorted_keys.is_contiguous() and sorted_keys.is_cuda
    assert counts.dtype == torch.int64 and counts.numel() == sz["counts"] and counts.is_contiguous()
    assert out.dtype == torch.float64 and out.numel() == sz["out"] and out.is_contiguous()
    if tile_fg is None:
        tile_fg = torch.empty(sz["scratch"], dtype=torch.int64, device=wmap.device)
    if partials is None:
        partials = torch.empty(sz["scratch"], dtype=torch.float64, device=wmap.device)
    assert tile_fg.dtype == torch.int64 and tile_fg.numel() >= sz["scratch"] and tile_fg.is_contiguous()
    assert partials.dtype == torch.float64 and partials.numel() >= sz["scratch"] and partials.is_contiguous()
    call("cmu_lovasz_grad", _p(sorted_keys), _p(counts), mask, int(bool(per_image)), int(bool(classes_all)), _p(_f32c(wmap)), _p(tile_fg),
         _p(partials), _p(out), B, K, H, W, _stream())
