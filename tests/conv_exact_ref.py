"""Exact float64 references of the MFMA convolution kernels and the list of cases the GPU files run.

Small-integer operands are exact in f16, bf16 and f32, and while every fp32 partial sum stays below 2**24 the MFMA chain, the LDS
folds, the split-K slabs and the epilogues must return the exact result in ANY order.  The helpers below compute that result in
float64 from shifted slices and matrix products (no torch convolution: tests/test_cpu_conv_exact_ref.py proves them against
``F.conv2d`` / ``F.conv_transpose2d`` / ``torch.nn.grad.conv2d_weight`` / autograd), return it as stored (torch's cast: round to
nearest even), and return the statistics slabs of the epilogues.  ``assert_exact_caps`` asserts the 2**24 condition from the
reference alone: a case that violates it is a wrong case, not a tolerance.

Everything is NHWC (the library's layout), works on whatever device its inputs live on, and needs no GPU.
"""
import torch

TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CAP = float(2 ** 24)
TILE = 16          # the statistics slabs keep one row per 16 x 16 pixel tile (ops.new_stats)


# ------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------
def int_operands(shape, lo, hi, density=1.0, seed=0):
    """Integer-valued fp32 tensor, uniform in [lo, hi]; a fraction 1 - density of the entries is zeroed."""
    g = torch.Generator().manual_seed(int(seed))
    t = torch.randint(int(lo), int(hi) + 1, tuple(shape), generator=g).to(torch.float32)
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < density).to(torch.float32)
    return t


def float_operands(shape, seed=0):
    """Random floats with magnitudes in [2**-6, 8): normal numbers in all three storage types (the one-hot cases move them, bit
    for bit; how an MFMA treats a subnormal operand is not what those cases are about)."""
    g = torch.Generator().manual_seed(int(seed))
    mag = torch.exp2(torch.rand(tuple(shape), generator=g) * 9.0 - 6.0)
    sign = torch.randint(0, 2, tuple(shape), generator=g).to(torch.float32) * 2.0 - 1.0
    return mag * sign


def stored(t, dt):
    """float64 -> the storage type with torch's cast (round to nearest even; float64 -> fp32 is exact for every value here)."""
    return t.to(torch.float32).to(TORCH_DT[dt])


def relu_on(c, relu_from):
    """``cmu_relu_on`` of common.h: channels c >= relu_from are activated; a negative value -n activates the channels c < n."""
    return c >= relu_from if relu_from >= 0 else c < -relu_from


def apply_transform(x, transform):
    """Pending transform of an activation view: z = x * scale + shift per channel, ReLU on the channels ``relu_on`` names.
    ``transform``: None or (scale, shift, relu_from)."""
    x = x.double()
    if transform is None:
        return x
    scale, shift, relu_from = transform
    z = x * scale.double().to(x.device) + shift.double().to(x.device)
    c = torch.arange(x.shape[-1], device=x.device)
    return torch.where(relu_on(c, relu_from), z.clamp_min(0.0), z)


def _tiles(t):
    """(B, H, W, C) -> (B * ceil(H/16) * ceil(W/16), C): sums over the valid pixels of each 16 x 16 tile, in ops.new_stats order."""
    B, H, W, C = t.shape
    th, tw = -(-H // TILE), -(-W // TILE)
    p = torch.zeros(B, th * TILE, tw * TILE, C, dtype=t.dtype, device=t.device)
    p[:, :H, :W] = t
    return p.reshape(B, th, TILE, tw, TILE, C).sum((2, 4)).reshape(B * th * tw, C)


def tile_stats(a, b):
    """Slab [tiles][2][C] of (sum a, sum b) per 16 x 16 tile and channel."""
    return torch.stack([_tiles(a), _tiles(b)], 1)


def shift2d(x, dy, dx):
    """out[b, h, w] = x[b, h + dy, w + dx], zero outside the image."""
    B, H, W, C = x.shape
    out = torch.zeros_like(x)
    h0, h1, w0, w1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if h0 < h1 and w0 < w1:
        out[:, h0:h1, w0:w1] = x[:, h0 + dy:h1 + dy, w0 + dx:w1 + dx]
    return out


# ------------------------------------------------------------------------------------------------
# 3x3 convolution, padding 1
# ------------------------------------------------------------------------------------------------
def conv3x3_terms(xa, w):
    """y and sum |terms| of the 3x3 convolution: xa (B,H,W,Cin) float64, already transformed; w (Cout,Cin,3,3)."""
    w = w.double().to(xa.device)
    y = torch.zeros(xa.shape[:3] + (w.shape[0],), dtype=torch.float64, device=xa.device)
    mag = torch.zeros_like(y)
    for ky in range(3):
        for kx in range(3):
            xs = shift2d(xa, ky - 1, kx - 1)
            wt = w[:, :, ky, kx].t()
            y += xs @ wt
            mag += xs.abs() @ wt.abs()
    return y + 0.0, mag          # (+ 0.0: every zero is +0, as a sum that starts from +0 gives)


def conv3x3_exact(x, w, transform=None, dt="f32"):
    """-> dict: ``y`` float64 (B,H,W,Cout), ``stored`` (y in the storage type), ``stats`` fp32 slab [tiles][2][Cout] of sum y and
    sum y^2 of the UNROUNDED values, ``mag`` (sum |terms| per output), ``sumsq`` (float64 slab of sum y^2)."""
    xa = apply_transform(x, transform)
    y, mag = conv3x3_terms(xa, w)
    st = tile_stats(y, y * y)
    return {"y": y, "stored": stored(y, dt), "stats": st.to(torch.float32), "mag": mag, "sumsq": st[:, 1]}


def bn_bwd_sums(dx_stored, yraw, bscale, bshift, mean, invstd):
    """BatchNorm+ReLU backward partial sums on dX AS STORED: per 16 x 16 tile and channel sum(gate * dX) and sum(gate * dX * xhat),
    gate = (yraw * bscale + bshift > 0), xhat = (yraw - mean) * invstd.  -> (fp32 slab, largest intermediate magnitude)."""
    dev = dx_stored.device
    d = dx_stored.double()
    yr = yraw.double().to(dev)
    bs, bh, mu, isd = (t.double().to(dev) for t in (bscale, bshift, mean, invstd))
    dz = torch.where(yr * bs + bh > 0, d, torch.zeros_like(d))
    slab = tile_stats(dz, dz * (yr - mu) * isd)
    # what the kernels hold on the way: sum |dz|, sum |dz * yraw|, |mean| * sum |dz|, all times invstd
    m = tile_stats(dz.abs(), dz.abs() * yr.abs())
    worst = torch.maximum(m[:, 0] * (1.0 + mu.abs()) * isd.clamp_min(1.0), m[:, 1] * isd.clamp_min(1.0)).max()
    return slab.to(torch.float32), float(worst)


def conv3x3_dgrad_bn_exact(dy, w_layer, yraw, bscale, bshift, mean, invstd, dt="f32"):
    """Data gradient of ``conv3x3(., w_layer)`` (w_layer (K, N, 3, 3): K = the layer's output channels = dY's, N = its input
    channels = dX's): the convolution of dY with the flipped, transposed weight, + the BatchNorm-backward sums of the producer."""
    wf = w_layer.flip(2, 3).transpose(0, 1).contiguous()
    r = conv3x3_exact(dy, wf, None, dt)
    r["bstats"], r["bmag"] = bn_bwd_sums(r["stored"], yraw, bscale, bshift, mean, invstd)
    return r


def conv3x3_wgrad_exact(x, dy, transform=None):
    """dW (Cout,Cin,3,3) = sum over pixels of dY[p, co] * xa[p + tap, ci]; -> dict ``dW`` float64, ``mag`` sum |terms|."""
    xa = apply_transform(x, transform)
    d = dy.double().to(xa.device)
    Cin, Cout = xa.shape[-1], d.shape[-1]
    dW = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, device=xa.device)
    mag = torch.zeros_like(dW)
    d2 = d.reshape(-1, Cout)
    for ky in range(3):
        for kx in range(3):
            xs = shift2d(xa, ky - 1, kx - 1).reshape(-1, Cin)
            dW[:, :, ky, kx] = d2.t() @ xs
            mag[:, :, ky, kx] = d2.abs().t() @ xs.abs()
    return {"dW": dW + 0.0, "mag": mag}


# ------------------------------------------------------------------------------------------------
# ConvTranspose 2x2, stride 2
# ------------------------------------------------------------------------------------------------
def convT2x2_exact(x, w, bias, transform=None, dt="f32"):
    """out[b, 2h+i, 2w+j, co] = sum_ci xa[b,h,w,ci] * w[ci,co,i,j] + bias[co]; w (Cin,Cout,2,2)."""
    xa = apply_transform(x, transform)
    w = w.double().to(xa.device)
    bias = bias.double().to(xa.device)
    B, H, W, _ = xa.shape
    Cout = w.shape[1]
    y = torch.zeros(B, 2 * H, 2 * W, Cout, dtype=torch.float64, device=xa.device)
    mag = torch.zeros_like(y)
    for i in range(2):
        for j in range(2):
            y[:, i::2, j::2] = xa @ w[:, :, i, j] + bias
            mag[:, i::2, j::2] = xa.abs() @ w[:, :, i, j].abs() + bias.abs()
    y = y + 0.0
    return {"y": y, "stored": stored(y, dt), "mag": mag}


def convT2x2_dgrad_exact(dout, w, dt="f32"):
    """dX[b,h,w,ci] = sum_{i,j,co} dOut[b,2h+i,2w+j,co] * w[ci,co,i,j]."""
    d = dout.double()
    w = w.double().to(d.device)
    B, H2, W2, _ = d.shape
    y = torch.zeros(B, H2 // 2, W2 // 2, w.shape[0], dtype=torch.float64, device=d.device)
    mag = torch.zeros_like(y)
    for i in range(2):
        for j in range(2):
            y += d[:, i::2, j::2] @ w[:, :, i, j].t()
            mag += d[:, i::2, j::2].abs() @ w[:, :, i, j].abs().t()
    y = y + 0.0
    return {"y": y, "stored": stored(y, dt), "mag": mag}


def convT2x2_dgrad_bn_exact(dout, w, yraw, bscale, bshift, mean, invstd, dt="f32"):
    r = convT2x2_dgrad_exact(dout, w, dt)
    r["bstats"], r["bmag"] = bn_bwd_sums(r["stored"], yraw, bscale, bshift, mean, invstd)
    return r


def convT2x2_wgrad_exact(x, dout, transform=None):
    """dW (Cin,Cout,2,2) = sum over low-res pixels of xa[p, ci] * dOut[2p + (i,j), co]; dbias = sum over all pixels of dOut."""
    xa = apply_transform(x, transform)
    d = dout.double().to(xa.device)
    Cin, Cout = xa.shape[-1], d.shape[-1]
    dW = torch.zeros(Cin, Cout, 2, 2, dtype=torch.float64, device=xa.device)
    mag = torch.zeros_like(dW)
    x2 = xa.reshape(-1, Cin)
    for i in range(2):
        for j in range(2):
            dd = d[:, i::2, j::2].reshape(-1, Cout)
            dW[:, :, i, j] = x2.t() @ dd
            mag[:, :, i, j] = x2.abs().t() @ dd.abs()
    return {"dW": dW + 0.0, "mag": mag, "dbias": d.sum((0, 1, 2)) + 0.0, "dbias_mag": d.abs().sum((0, 1, 2))}


# ------------------------------------------------------------------------------------------------
# the condition that makes a case exact
# ------------------------------------------------------------------------------------------------
def rounding_report(y, dt):
    """(share of outputs that the storage type cannot hold, number of those that are exact round-to-even ties)."""
    if dt == "f32":
        return 0.0, 0
    s = stored(y, dt).double()
    inexact = s != y
    # a tie: y is half-way between two ADJACENT values of the storage type.  s is the nearest value; its mirror image 2 y - s is as far
    # away, and nothing representable lies between them (it would be nearer than s): a tie iff the mirror image is representable
    other = 2.0 * y - s
    tie = inexact & torch.isfinite(s) & (stored(other, dt).double() == other)
    return float(inexact.double().mean()), int(tie.sum())


def assert_exact_caps(ref, dt="f32", stats=False):
    """Asserts, from a reference dict alone, that every fp32 sum a kernel may form for the case is an integer below 2**24 in
    magnitude: sum |terms| per output (``mag`` / ``dbias_mag``), sum y^2 per statistics tile when the case takes statistics, the
    intermediate magnitudes of the BatchNorm-backward sums.  -> dict of the largest figures + the rounding report of ``y``."""
    rep = {}
    rep["terms"] = float(ref["mag"].max())
    assert rep["terms"] < CAP, f"sum |terms| {rep['terms']:.0f} reaches 2^24"
    for k in ("y", "dW"):
        if k in ref:
            assert bool((ref[k] == ref[k].round()).all()), f"{k} is not integer-valued"
    if "dbias_mag" in ref:
        rep["dbias"] = float(ref["dbias_mag"].max())
        assert rep["dbias"] < CAP, f"sum |dOut| {rep['dbias']:.0f} reaches 2^24"
    if stats:
        rep["sumsq"] = float(ref["sumsq"].max())
        assert rep["sumsq"] < CAP, f"sum y^2 per tile {rep['sumsq']:.0f} reaches 2^24"
    if "bmag" in ref:
        rep["bn"] = float(ref["bmag"])
        assert rep["bn"] < CAP, f"BatchNorm-backward sum {rep['bn']:.0f} reaches 2^24"
        assert bool((ref["bstats"].double() * 2 == (ref["bstats"].double() * 2).round()).all())
    if "y" in ref:
        rep["inexact"], rep["ties"] = rounding_report(ref["y"], dt)
    return rep


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
# One dict per case.  Keys:
#   fam     c3f (cmu_conv3x3_fwd) | c3dg (cmu_conv3x3_dgrad_bn, flipped pack) | ctf (cmu_convT2x2_fwd) | ctdg (cmu_convT2x2_dgrad)
#           | ctdgbn (cmu_convT2x2_dgrad_bn) | wg3 (cmu_conv3x3_wgrad) | wgt (cmu_convT2x2_wgrad)
#           | c3rows (cmu_conv3x3_fwd_rows: the convolution read at a list of pixels) | wg3tiles (cmu_conv3x3_wgrad_tiles: the weight
#           gradient of dY restricted to a list of tiles)
#   rows    c3rows: the pixel list (``rows_list``) -- count (a number, or "all": every pixel of the batch), cap ("tight": the count
#           rounded up to 256 | "slack": three more row tiles | "cus": 256 rows per CU of the device), flip (the transpose_flip pack: the
#           data gradient the encoder runs), plist ((f, keep): the list comes from ops.PixelList on a patch map instead)
#   tiles   wg3tiles: the tile list (``tiles_list``) -- th (8 | 16: tiles of th x 16 pixels), cls (the count relative to the split count:
#           zero | below | equal | multiple | remainder | all), order (asc | perm), builder ((f, keep): the list comes from ops.TileList)
#   shape   (B, H, W, K, N): K channels of the operand that is read, N channels written (c3dg / ctdg*: K = dY's, N = dX's; weight
#           gradients: K = Cin, N = Cout).  ConvTranspose: H x W is the LOW resolution.
#   dts     storage types;  rng  operand range of x / dY (and of the weights);  tf  None | relu_from of the pending transform
#   stats   forward statistics taken;  xs / ys  channel offset of the view in a wider input / output buffer
#   knobs   dispatch overrides (CMU_ prefix omitted);  kernel  the tag cmu_last_kernel() must report
#   form    what the launcher's rule, restated in conv_exact_gpu.py, must give for this case (ConvTranspose: the number of 128-byte K
#           steps, and for the data gradients whether a step stays inside one sub-pixel position)
#   wrng    range of the weights when it is not ``rng`` (K = 1024 with statistics: weights in [-2, 2] against activations in {-1, 0, 1}
#           put outputs past 256 -- bf16 ties under the statistics -- while sum y^2 per tile stays below 2**24)
#   spike   statistics cases: input channel 0 is zero except for one 1.0 per 16 x 16 tile (pixel (5, 7) of the tile) and its weights are
#           zero except the centre tap, +-``spike``: ONE output per tile and channel is lifted by +-2048, past what f16 holds exactly (and
#           bf16), while its square (about 2^22) leaves sum y^2 of the tile below 2**24 -- statistics taken from the stored values differ
#   lift    f16 only: the weights of every eighth channel of the contraction are multiplied by this power of two (outputs past 2048:
#           exact ties in f16, which holds every integer below that)
def _c(fam, name, shape, kernel, dts=("f16", "bf16"), rng=(-3, 3), tf=None, stats=False, xs=0, ys=0, knobs=None, form=None, lift=0,
       bias=0, wrng=None, spike=0, rows=None, tiles=None):
    return {"rows": rows, "tiles": tiles, "spike": spike, "wrng": tuple(wrng or rng), "fam": fam, "id": name, "shape": shape, "kernel": kernel, "dts": dts, "rng": rng, "tf": tf, "stats": stats, "xs": xs,
            "ys": ys, "knobs": dict(knobs or {}), "form": dict(form or {}), "lift": lift, "bias": bias}


ALL = ("f32", "f16", "bf16")
H16 = ("f16", "bf16")
# wg3tiles: (count class, list order) pairs -- every class in both orders where it matters, and a shorter walk for the second shape of a kernel
_EVERY = (("zero", "asc"), ("below", "perm"), ("equal", "asc"), ("multiple", "perm"), ("remainder", "perm"), ("remainder", "asc"), ("all", "asc"))
_FEW = (("zero", "asc"), ("below", "asc"), ("equal", "perm"), ("remainder", "perm"), ("all", "asc"))


def _tile_cases(name, shape, kernel, dts, tf, th, knobs, splits, classes, xs=0, ys=0):
    """One wg3tiles case per (count class, list order): the knob gives the launch ``splits`` splits, which the classes are relative to."""
    return [_c("wg3tiles", f"{name} {cls} {order}", shape, kernel, dts, tf=tf, knobs=knobs, xs=xs, ys=ys,
               tiles={"th": th, "cls": cls, "order": order}, form={"splits": splits}) for cls, order in classes]
NN = {"CONV_NARROW": 0}      # keep the 128-channel blocks whatever the CU count (the narrow form is bit-identical and has its own case)

CASES = [
    # ---- conv_igemm_kernel: channel counts that are not whole slices / blocks ---------------------------------------------------
    _c("c3f", "first 8->8 7x9", (1, 7, 9, 8, 8), "conv_igemm_kernel", ALL, tf=0, stats=True, rng=(-1, 1), xs=8, ys=16),
    _c("c3f", "first 24->40 17x33", (1, 17, 33, 24, 40), "conv_igemm_kernel", ALL, tf=-8, stats=True, rng=(-1, 1)),
    _c("c3f", "first 136->256 ragged slice", (2, 5, 18, 136, 256), "conv_igemm_kernel", ALL, ys=8, lift=64),
    _c("c3f", "first spike 24->40 17x33", (1, 17, 33, 24, 40), "conv_igemm_kernel", H16, stats=True, rng=(-1, 1), spike=2048),
    _c("c3f", "first K 1024 (CONV_WIDE 0)", (1, 16, 32, 1024, 128), "conv_igemm_kernel", H16, stats=True, rng=(-1, 1), wrng=(-2, 2),
       knobs={"CONV_WIDE": 0}),
    _c("c3f", "first f32 4->8", (1, 16, 17, 4, 8), "conv_igemm_kernel", ("f32",), tf=0, stats=True),
    _c("c3dg", "first dgrad 24->40", (2, 9, 17, 24, 40), "conv_igemm_kernel", ALL, rng=(-5, 5), lift=64),
    # ---- conv_igemm3_kernel: CONV_PERSIST = 0, and without a knob by a K of fewer than four slices -------------------------------
    _c("c3f", "v3 64->128 16x32 stats", (2, 16, 32, 64, 128), "conv_igemm3_kernel", ALL, stats=True, rng=(-1, 1),
       knobs={"CONV_PERSIST": 0, **NN}, form={"NB": 128, "TW": 32}),
    _c("c3f", "v3 128->64 17x33 tf", (1, 17, 33, 128, 64), "conv_igemm3_kernel", ALL, tf=64, stats=True, rng=(-1, 1), xs=16,
       knobs={"CONV_PERSIST": 0}, form={"NB": 64, "TW": 32}),
    _c("c3f", "v3 slim 64->128 1x16", (3, 1, 16, 64, 128), "conv_igemm3_kernel", ALL, tf=-32, ys=128, lift=256,
       knobs={"CONV_PERSIST": 0, **NN}, form={"NB": 128, "TW": 16}),
    _c("c3f", "v3 slim 128->64 17x9 stats", (2, 17, 9, 128, 64), "conv_igemm3_kernel", ALL, stats=True, rng=(-1, 1),
       knobs={"CONV_PERSIST": 0}, form={"NB": 64, "TW": 16}),
    _c("c3f", "v3 spike 128->64 17x33", (1, 17, 33, 128, 64), "conv_igemm3_kernel", H16, stats=True, rng=(-1, 1), spike=2048,
       knobs={"CONV_PERSIST": 0}, form={"NB": 64, "TW": 32}),
    _c("c3f", "v3 K 1024 17x33", (1, 17, 33, 1024, 128), "conv_igemm3_kernel", H16, stats=True, rng=(-1, 1), wrng=(-2, 2),
       knobs={"CONV_PERSIST": 0, **NN}, form={"NB": 128, "TW": 32}),
    _c("c3f", "v3 narrow 64->128", (1, 16, 32, 64, 128), "conv_igemm3_kernel", H16, lift=64, knobs={"CONV_PERSIST": 0},
       form={"NB": 64, "TW": 32}),
    _c("c3f", "v3 short K 32->64 (no knob)", (1, 16, 33, 32, 64), "conv_igemm3_kernel", H16, tf=8, stats=True, rng=(-1, 1),
       form={"NB": 64, "TW": 32}),
    _c("c3f", "v3 short K f32 16->128 (no knob)", (1, 17, 32, 16, 128), "conv_igemm3_kernel", ("f32",), knobs=NN,
       form={"NB": 128, "TW": 32}),
    _c("c3dg", "v3 dgrad 64->128 17x33", (1, 17, 33, 64, 128), "conv_igemm3_kernel", ALL, ys=64, lift=32,
       knobs={"CONV_PERSIST": 0, **NN}, form={"NB": 128, "TW": 32}),
    # ---- conv_igemm3p_kernel: whole tiles, PART, NB, WRES, BST, the full transform table, several items per workgroup -----------
    _c("c3f", "v3p 64->128 16x32", (2, 16, 32, 64, 128), "conv_igemm3p_kernel", ALL, stats=True, rng=(-1, 1), knobs=NN,
       form={"NB": 128, "PART": False, "WRES": False}),
    _c("c3f", "v3p 64->128 32x64 grid 3", (2, 32, 64, 64, 128), "conv_igemm3p_kernel", H16, tf=32, stats=True, rng=(-1, 1), xs=64, ys=128,
       knobs={"CONV_PERSIST_GRID": 3, "CONV_V5": 0, **NN}, form={"NB": 128, "PART": False, "WRES": False}),
    _c("c3f", "v3p part 64->128 20x33", (2, 20, 33, 64, 128), "conv_igemm3p_kernel", ALL, tf=-16, stats=True, rng=(-1, 1), knobs=NN,
       form={"NB": 128, "PART": True, "WRES": False}),
    _c("c3f", "v3p part 128->64 20x33 grid 1", (2, 20, 33, 128, 64), "conv_igemm3p_kernel", H16, stats=True, rng=(-1, 1),
       knobs={"CONV_PERSIST_GRID": 1}, form={"NB": 64, "PART": True, "WRES": False}),
    _c("c3f", "v3p narrow 128->256 16x32", (1, 16, 32, 128, 256), "conv_igemm3p_kernel", H16, lift=64, knobs={"CONV_V5": 0},
       form={"NB": 64, "PART": False, "WRES": False}),
    _c("c3f", "v3p wres 64->64", (2, 16, 64, 64, 64), "conv_igemm3p_kernel", H16, tf=0, stats=True, rng=(-1, 1),
       knobs={"CONV_PERSIST_GRID": 3}, form={"NB": 64, "PART": False, "WRES": True}),
    _c("c3f", "v3p wres off 64->64", (2, 16, 64, 64, 64), "conv_igemm3p_kernel", H16, tf=0, stats=True, rng=(-1, 1),
       knobs={"CONV_WRES": 0}, form={"NB": 64, "PART": False, "WRES": False}),
    _c("c3f", "v3p f32 64->64", (1, 32, 32, 64, 64), "conv_igemm3p_kernel", ("f32",), stats=True, rng=(-1, 1),
       form={"NB": 64, "PART": False, "WRES": False}),
    _c("c3f", "v3p K 1024 full table", (1, 16, 32, 1024, 128), "conv_igemm3p_kernel", H16, tf=512, stats=True, rng=(-1, 1), wrng=(-2, 2),
       knobs={"CONV_V5": 0, **NN}, form={"NB": 128, "PART": False, "WRES": False}),
    _c("c3f", "v3p part spike 64->128 20x33", (2, 20, 33, 64, 128), "conv_igemm3p_kernel", H16, stats=True, rng=(-1, 1), spike=2048, knobs=NN,
       form={"NB": 128, "PART": True, "WRES": False}),
    _c("c3f", "v3p part K 1024 20x33", (1, 20, 33, 1024, 64), "conv_igemm3p_kernel", H16, stats=True, rng=(-1, 1), wrng=(-2, 2),
       form={"NB": 64, "PART": True, "WRES": False}),
    _c("c3dg", "v3p bst K 128", (2, 16, 32, 128, 128), "conv_igemm3p_kernel", H16, lift=32, knobs=NN,
       form={"NB": 128, "PART": False, "WRES": False, "BST": True}),
    _c("c3dg", "v3p bst part 128->64", (1, 20, 33, 128, 64), "conv_igemm3p_kernel", ALL, rng=(-1, 1), ys=64,
       form={"NB": 64, "PART": True, "WRES": False, "BST": True}),
    # ---- conv_igemm5_kernel -----------------------------------------------------------------------------------------------------
    _c("c3f", "v5 128->128 16x32", (1, 16, 32, 128, 128), "conv_igemm5_kernel", H16, stats=True, rng=(-1, 1), knobs=NN),
    _c("c3f", "v5 spike 128->128", (1, 16, 32, 128, 128), "conv_igemm5_kernel", H16, stats=True, rng=(-1, 1), spike=2048, knobs=NN),
    _c("c3f", "v5 128->128 ties", (1, 16, 32, 128, 128), "conv_igemm5_kernel", H16, knobs=NN, lift=64),
    _c("c3f", "v5 192->384 32x64 B 3 grid 3", (3, 32, 64, 192, 384), "conv_igemm5_kernel", H16, tf=64, stats=True, rng=(-1, 1), xs=64,
       ys=128, knobs={"CONV_PERSIST_GRID": 3, **NN}),
    _c("c3f", "v5 256->128 relu_from -128 grid 1", (3, 16, 32, 256, 128), "conv_igemm5_kernel", H16, tf=-128, stats=True, rng=(-1, 1),
       knobs={"CONV_PERSIST_GRID": 1, **NN}),
    _c("c3f", "v5 K 1024", (1, 16, 32, 1024, 128), "conv_igemm5_kernel", H16, stats=True, rng=(-1, 1), wrng=(-2, 2), knobs=NN),
    _c("c3dg", "v5 dgrad K 256", (2, 16, 32, 256, 128), "conv_igemm5_kernel", H16, ys=128, lift=32, knobs=NN),
    # ---- ConvTranspose ----------------------------------------------------------------------------------------------------------
    _c("ctf", "gemm_s 64->32 5x9 (1 step)", (2, 5, 9, 64, 32), "conv_gemm_s_kernel", H16, tf=0, ys=32, bias=300, lift=256, form={"steps": 1}),
    _c("ctf", "gemm_s 256->64 17x33 (4 steps)", (1, 17, 33, 256, 64), "conv_gemm_s_kernel", H16, xs=64, bias=7, form={"steps": 4}),
    _c("ctf", "gemm 320->64 16x16 (5 steps)", (1, 16, 16, 320, 64), "conv_gemm_kernel", H16, tf=-64, bias=7, lift=256, form={"steps": 5}),
    _c("ctf", "gemm f32 32->64 1x1", (3, 1, 1, 32, 64), "conv_gemm_kernel", ("f32",), bias=7, form={"steps": 1}),
    _c("ctf", "gemm f32 64->128 17x33", (1, 17, 33, 64, 128), "conv_gemm_kernel", ("f32",), tf=32, ys=128, bias=7, form={"steps": 2}),
    _c("ctf", "first 16->8", (2, 5, 9, 16, 8), "conv_igemm_kernel", ALL, tf=8, ys=8, bias=7),
    _c("ctf", "first 64->24 17x33", (1, 17, 33, 64, 24), "conv_igemm_kernel", H16, bias=300, lift=256, form={"steps": 1}),
    _c("ctdg", "gemm_s dgrad 64->128 (Cout 64)", (2, 5, 9, 64, 128), "conv_gemm_s_kernel", H16, rng=(-5, 5), ys=128, lift=64, form={"steps": 4, "inside": True}),
    _c("ctdg", "gemm dgrad 128->256 (Cout 128: 8 steps)", (1, 16, 16, 128, 256), "conv_gemm_kernel", H16, lift=64, form={"steps": 8, "inside": True}),
    _c("ctdg", "first dgrad Cout 32 (K/4 rule)", (1, 17, 33, 32, 256), "conv_igemm_kernel", H16, rng=(-5, 5), lift=64, form={"steps": 2, "inside": False}),
    _c("ctdg", "first dgrad 8->16", (2, 1, 1, 8, 16), "conv_igemm_kernel", ALL),
    _c("ctdgbn", "gemm_s dgrad_bn 64->128", (1, 17, 33, 64, 128), "conv_gemm_s_kernel", H16, rng=(-5, 5), lift=32, form={"steps": 4, "inside": True}),
    _c("ctdgbn", "gemm dgrad_bn 128->256 (inexact dX)", (1, 16, 16, 128, 256), "conv_gemm_kernel", H16, lift=32, form={"steps": 8, "inside": True}),
    _c("ctdgbn", "gemm dgrad_bn f32 32->256", (2, 5, 9, 32, 256), "conv_gemm_kernel", ("f32",), rng=(-2, 2), ys=64, form={"steps": 4, "inside": True}),
    _c("ctdgbn", "first dgrad_bn 16->24", (1, 16, 16, 16, 24), "conv_igemm_kernel", ALL, rng=(-5, 5), lift=64),
    # ---- weight gradients (shapes of WG_CASES in test_gpu_bwd_ops.py); K = Cin, N = Cout ------------------------------------------
    _c("wg3", "first 8->8 7x9", (2, 7, 9, 8, 8), "conv_wgrad_kernel", ALL, tf=0, xs=16, form={"splits": "clamped"}),
    _c("wg3", "first 72->40 33x17 few splits", (1, 33, 17, 72, 40), "conv_wgrad_kernel", ALL, tf=-32, knobs={"WGRAD_BLOCKS1": 8},
       form={"splits": {"f16": "short", "bf16": "short", "f32": "one"}}),
    _c("wg3", "first 32->64 1x1", (3, 1, 1, 32, 64), "conv_wgrad_kernel", H16, form={"splits": "clamped"}),
    _c("wg3", "wide 64->128 20x24", (2, 20, 24, 64, 128), "conv_wgrad2_kernel", H16, tf=32, ys=16, form={"SWAP": False, "splits": "clamped"}),
    _c("wg3", "wide 192->128 33x16 short split", (3, 33, 16, 192, 128), "conv_wgrad2_kernel", H16, tf=-64, xs=16, knobs={"WGRAD_BLOCKS": 24},
       form={"SWAP": False, "splits": "short"}),
    _c("wg3", "wide 64->128 5x3 one tile", (1, 5, 3, 64, 128), "conv_wgrad2_kernel", H16, form={"SWAP": False, "splits": "one"}),
    _c("wg3", "wide 128->256 7x37 scalar reduce", (1, 7, 37, 128, 256), "conv_wgrad2_kernel", H16, knobs={"WGR_VEC": 0, "WGRAD_BLOCKS": 12},
       form={"SWAP": False, "splits": "equal"}),
    _c("wg3", "swap 128->64 20x24", (2, 20, 24, 128, 64), "conv_wgrad2_kernel", H16, tf=64, xs=16, ys=16, form={"SWAP": True, "splits": "clamped"}),
    _c("wg3", "swap 256->64 17x37 short split", (1, 17, 37, 256, 64), "conv_wgrad2_kernel", H16, tf=-8, knobs={"WGRAD_BLOCKS": 8},
       form={"SWAP": True, "splits": "short"}),
    _c("wg3", "swap 128->64 1x1", (2, 1, 1, 128, 64), "conv_wgrad2_kernel", H16, form={"SWAP": True, "splits": "clamped"}),
    _c("wg3", "square 64->64 20x24", (2, 20, 24, 64, 64), "conv_wgrad2s_kernel", H16, tf=8, ys=16, form={"splits": "clamped"}),
    _c("wg3", "square 192->64 33x16 equal", (3, 33, 16, 192, 64), "conv_wgrad2s_kernel", H16, tf=-64, knobs={"WGRAD_BLOCKS": 15},
       form={"splits": "equal"}),
    _c("wg3", "square 64->64 5x3", (1, 5, 3, 64, 64), "conv_wgrad2s_kernel", H16, form={"splits": "one"}),
    _c("wg3", "f32 64->64 20x24", (2, 20, 24, 64, 64), "conv_wgrad2f_kernel", ("f32",), tf=4, xs=16, form={"NAI": 2, "splits": "clamped"}),
    _c("wg3", "f32 64->128 9x37 short", (1, 9, 37, 64, 128), "conv_wgrad2f_kernel", ("f32",), tf=-32, knobs={"WGRAD_BLOCKS": 8},
       form={"NAI": 4, "splits": "short"}),
    _c("wg3", "f32 64->64 5x3 scalar reduce", (1, 5, 3, 64, 64), "conv_wgrad2f_kernel", ("f32",), knobs={"WGR_VEC": 0},
       form={"NAI": 2, "splits": "clamped"}),
    _c("wgt", "T first 32->16 8x8", (2, 8, 8, 32, 16), "conv_wgrad_kernel", ALL, tf=0, form={"splits": "clamped"}),
    _c("wgt", "T first 64->32 17x9", (2, 17, 9, 64, 32), "conv_wgrad_kernel", H16, ys=32, form={"splits": "clamped"}),
    _c("wgt", "T wide 128->64 5x9 NXI 2", (1, 5, 9, 128, 64), "conv_wgradT2_kernel", H16, tf=64, ys=64, form={"NXI": 2, "splits": "clamped"}),
    _c("wgt", "T wide 128->192 4x16 short", (3, 4, 16, 128, 192), "conv_wgradT2_kernel", H16, knobs={"WGRAD_BLOCKS": 8},
       form={"NXI": 2, "splits": "short"}),
    _c("wgt", "T wide 256->64 1x2 NXI 4", (1, 1, 2, 256, 64), "conv_wgradT2_kernel", H16, tf=-128, form={"NXI": 4, "splits": "one"}),
    _c("wgt", "T wide 256->128 7x33 NXI 4 equal", (2, 7, 33, 256, 128), "conv_wgradT2_kernel", H16, knobs={"WGRAD_BLOCKS": 12},
       form={"NXI": 4, "splits": "equal"}),
    _c("wgt", "T wide 256->64 NX256 off", (1, 5, 9, 256, 64), "conv_wgradT2_kernel", H16, knobs={"WGT2_NX256": 0},
       form={"NXI": 2, "splits": "clamped"}),
    _c("wgt", "T f32 128->64 5x9", (1, 5, 9, 128, 64), "conv_wgradT2f_kernel", ("f32",), tf=64, ys=64, form={"splits": "clamped"}),
    _c("wgt", "T f32 256->128 7x33 short", (2, 7, 33, 256, 128), "conv_wgradT2f_kernel", ("f32",), knobs={"WGRAD_BLOCKS": 20},
       form={"splits": "short"}),
    # ---- conv_gather_kernel: the convolution at a hand-built list of pixels (K = Cin: 1, 2, 3 steps of 128 bytes per tap) ---------------
    #      grid = ceil(capacity / 256) * (N / NB): 1, 3, 8, 9, 17 (+ 2, 4, 5 and one workgroup per CU)
    _c("c3rows", "rows 1 step ->128 count 255 grid 1", (2, 12, 13, 64, 128), "conv_gather_kernel", H16, xs=8, ys=16, lift=64,
       rows={"count": 255, "cap": "tight"}, form={"NB": 128, "grid": 1}),
    _c("c3rows", "rows f32 1 step ->128 count 255 grid 1", (2, 12, 13, 32, 128), "conv_gather_kernel", ("f32",), xs=8, ys=16,
       rows={"count": 255, "cap": "tight"}, form={"NB": 128, "grid": 1}),
    _c("c3rows", "rows 2 steps ->384 count 256 grid 3", (1, 17, 16, 128, 384), "conv_gather_kernel", H16, ys=128, lift=32,
       rows={"count": 256, "cap": "tight"}, form={"NB": 128, "grid": 3}),
    _c("c3rows", "rows f32 2 steps ->384 count 256 grid 3", (1, 17, 16, 64, 384), "conv_gather_kernel", ("f32",), ys=128,
       rows={"count": 256, "cap": "tight"}, form={"NB": 128, "grid": 3}),
    _c("c3rows", "rows 3 steps ->256 NB 128 count 1 grid 8", (1, 3, 5, 192, 256), "conv_gather_kernel", H16, xs=64, lift=32,
       knobs={"GATHER_NB": 128}, rows={"count": 1, "cap": "slack"}, form={"NB": 128, "grid": 8}),
    _c("c3rows", "rows f32 3 steps ->256 NB 128 count 1 grid 8", (1, 3, 5, 96, 256), "conv_gather_kernel", ("f32",), xs=32,
       knobs={"GATHER_NB": 128}, rows={"count": 1, "cap": "slack"}, form={"NB": 128, "grid": 8}),
    _c("c3rows", "rows 1 step ->256 NB 256 count 0", (1, 4, 4, 64, 256), "conv_gather_kernel", H16, ys=8,
       knobs={"GATHER_NB": 256}, rows={"count": 0, "cap": "tight"}, form={"NB": 256, "grid": 1}),
    _c("c3rows", "rows 2 steps ->256 NB 256 count 257 grid 5", (2, 12, 13, 128, 256), "conv_gather_kernel", H16, xs=16, ys=256, lift=32,
       knobs={"GATHER_NB": 256}, rows={"count": 257, "cap": "slack"}, form={"NB": 256, "grid": 5}),
    _c("c3rows", "rows f32 1 step ->256 NB 256 count 257 grid 5", (2, 12, 13, 32, 256), "conv_gather_kernel", ("f32",), ys=256,
       knobs={"GATHER_NB": 256}, rows={"count": 257, "cap": "slack"}, form={"NB": 256, "grid": 5}),
    _c("c3rows", "rows 3 steps ->384 count 700 grid 9", (3, 16, 15, 192, 384), "conv_gather_kernel", H16, rng=(-2, 2),
       rows={"count": 700, "cap": "tight"}, form={"NB": 128, "grid": 9}),
    _c("c3rows", "rows 1 step ->128 count 3518 grid 17", (3, 33, 37, 64, 128), "conv_gather_kernel", H16,
       rows={"count": 3518, "cap": "slack"}, form={"NB": 128, "grid": 17}),
    _c("c3rows", "rows ->256 no knob, few row tiles: NB 128 grid 4", (1, 16, 19, 64, 256), "conv_gather_kernel", H16,
       rows={"count": 300, "cap": "tight"}, form={"NB": 128, "grid": 4}),
    _c("c3rows", "rows ->256 no knob, a row tile per CU: NB 256", (1, 16, 19, 64, 256), "conv_gather_kernel", H16, lift=64,
       rows={"count": 300, "cap": "cus"}, form={"NB": 256}),
    _c("c3rows", "rows every pixel of 3 x 5 x 11, flipped pack", (3, 5, 11, 128, 256), "conv_gather_kernel", ALL, xs=32, ys=32, lift=32,
       knobs={"GATHER_NB": 256}, rows={"count": "all", "cap": "tight", "flip": True}, form={"NB": 256, "grid": 1}),
    _c("c3rows", "rows every pixel of 3 x 9 x 7, flipped pack", (3, 9, 7, 64, 128), "conv_gather_kernel", ALL, lift=64,
       rows={"count": "all", "cap": "tight", "flip": True}, form={"NB": 128, "grid": 1}),
    _c("c3rows", "rows builder list 2 x 8 x 8, patches of 2 px", (2, 8, 8, 64, 128), "conv_gather_kernel", ALL,
       rows={"plist": (4, 5), "cap": "tight"}, form={"NB": 128, "grid": 1}),
    _c("c3rows", "rows builder list 3 x 16 x 16, patches of 1 px, flipped", (3, 16, 16, 128, 128), "conv_gather_kernel", H16, lift=32,
       rows={"plist": (16, 100), "cap": "tight", "flip": True}, form={"NB": 128, "grid": 2}),
    # ---- cmu_conv3x3_wgrad_tiles: the three kernels over 16 x 16 and 8 x 16 tile lists, counts relative to the split count -------------
    *_tile_cases("tiles first 72->40 2x20x40", (2, 20, 40, 72, 40), "conv_wgrad_kernel", H16, -32, 16, {"WGRAD_BLOCKS1": 8}, 4, _EVERY, xs=8, ys=8),
    *_tile_cases("tiles first f32 72->40 2x20x40", (2, 20, 40, 72, 40), "conv_wgrad_kernel", ("f32",), -32, 16, {"WGRAD_BLOCKS1": 24}, 4, _FEW, xs=4),
    *_tile_cases("tiles first f32 64->128 2x20x40", (2, 20, 40, 64, 128), "conv_wgrad_kernel", ("f32",), 32, 16, {"WGRAD_BLOCKS1": 32}, 4, _FEW),
    *_tile_cases("tiles wide 64->128 3x20x40", (3, 20, 40, 64, 128), "conv_wgrad2_kernel", H16, 32, 8, {"WGRAD_BLOCKS": 8}, 8, _EVERY, ys=16),
    *_tile_cases("tiles wide 128->256 1x20x40", (1, 20, 40, 128, 256), "conv_wgrad2_kernel", H16, -64, 8, {"WGRAD_BLOCKS": 16}, 4, _FEW, xs=16),
    *_tile_cases("tiles square 64->64 3x20x40", (3, 20, 40, 64, 64), "conv_wgrad2s_kernel", H16, 8, 8, {"WGRAD_BLOCKS": 8}, 8, _EVERY, xs=16),
    *_tile_cases("tiles square 192->64 2x20x40", (2, 20, 40, 192, 64), "conv_wgrad2s_kernel", H16, -64, 8, {"WGRAD_BLOCKS": 12}, 4, _FEW, ys=16),
    _c("wg3tiles", "tiles first builder 2x32x32", (2, 32, 32, 72, 40), "conv_wgrad_kernel", ALL, tf=8, knobs={"WGRAD_BLOCKS1": 8},
       tiles={"th": 16, "builder": (2, 3)}),
    _c("wg3tiles", "tiles wide builder 3x64x64", (3, 64, 64, 64, 128), "conv_wgrad2_kernel", H16, tf=0, knobs={"WGRAD_BLOCKS": 8},
       tiles={"th": 8, "builder": (8, 21)}),
    _c("wg3tiles", "tiles square builder 3x64x64", (3, 64, 64, 64, 64), "conv_wgrad2s_kernel", H16, tf=-32, knobs={"WGRAD_BLOCKS": 8},
       tiles={"th": 8, "builder": (4, 5)}),
]

# every tag cmu_set_kernel_tag can set, apart from conv_igemm6_kernel (opt-in; pinned through its bit-identity test against the dense
# launch).  conv_gather_kernel (the SparK row-list form) is a kernel of its own -- own addressing, K order, staging and scatter -- and has
# its own exact cases (fam c3rows, tests/test_gpu_conv_rows_exact.py); the tile-list forms of the weight-gradient kernels share the dense
# kernels' tags and have theirs in fam wg3tiles (tests/test_gpu_wgrad_tiles_exact.py).  Of the list forms only cmu_conv3x3_fwd_tiles is
# pinned through identity with the dense launch (tests/test_gpu_sparse_tiles.py: torch.equal against it).
PINNED_KERNELS = {"conv_igemm_kernel", "conv_igemm3_kernel", "conv_igemm3p_kernel", "conv_igemm5_kernel", "conv_gemm_kernel",
                  "conv_gemm_s_kernel", "conv_wgrad_kernel", "conv_wgrad2_kernel", "conv_wgrad2s_kernel", "conv_wgrad2f_kernel",
                  "conv_wgradT2_kernel", "conv_wgradT2f_kernel", "conv_gather_kernel"}
# every list-driven C entry of the convolution sources and the file that holds it to an independent reference
LIST_ENTRIES = {"cmu_conv3x3_fwd_rows": "test_gpu_conv_rows_exact.py", "cmu_conv3x3_wgrad_tiles": "test_gpu_wgrad_tiles_exact.py",
                "cmu_conv3x3_fwd_tiles": "test_gpu_sparse_tiles.py", "cmu_conv3x3_c1_fwd_tiles": "test_gpu_elem_fp64.py",
                "cmu_conv3x3_c1_wgrad_bn_tiles": "test_gpu_elem_fp64.py", "cmu_sparse_tile_list": "test_gpu_sparse_lists.py",
                "cmu_sparse_tile_lists": "test_gpu_sparse_lists.py", "cmu_sparse_pixel_list": "test_gpu_sparse_lists.py",
                "cmu_sparse_pixel_lists": "test_gpu_sparse_lists.py"}


# ------------------------------------------------------------------------------------------------
# lists (c3rows, wg3tiles): built by hand, from the case alone
# ------------------------------------------------------------------------------------------------
ROW_TILE = 256     # rows of the list per workgroup of the gather kernel


def patch_map(B, f, keep, seed):
    """(B, f, f) uint8 patch map with ``keep`` active patches per image."""
    g = torch.Generator().manual_seed(int(seed))
    a = torch.zeros(B, f * f, dtype=torch.uint8)
    for b in range(B):
        a[b, torch.randperm(f * f, generator=g)[:keep]] = 1
    return a.view(B, f, f)


def pixel_list_of(active, H):
    """What cmu_sparse_pixel_list(s) must write for a square level of side H = f * s: the pixels of the active patches, patches in
    ascending (b, fy, fx) order, pixels row-major inside a patch.  Written out with loops (a second statement, no index algebra)."""
    B, f = active.shape[0], active.shape[-1]
    s = H // f
    out = []
    for b in range(B):
        for fy in range(f):
            for fx in range(f):
                if int(active[b, fy, fx]):
                    for py in range(s):
                        for px in range(s):
                            out.append((b * H + fy * s + py) * H + fx * s + px)
    return torch.tensor(out, dtype=torch.int32)


def rows_count(case):
    """The list's count, from the case alone."""
    B, H, W = case["shape"][:3]
    r = case["rows"]
    if "plist" in r:
        return B * r["plist"][1] * (H // r["plist"][0]) ** 2
    return B * H * W if r["count"] == "all" else int(r["count"])


def rows_capacity(case, count, cus=256):
    tight = max(ROW_TILE, -(-count // ROW_TILE) * ROW_TILE)
    return {"tight": tight, "slack": tight + 3 * ROW_TILE, "cus": ROW_TILE * cus}[case["rows"]["cap"]]


def rows_list(case, cus=256):
    """-> (rows int32 (capacity,), count).  The first ``count`` entries are a fixed random permutation of distinct pixels of the
    (B, H, W) batch; EVERY entry past the count is a valid pixel too, an unlisted one wherever the batch has one, so that a kernel
    that reads past the count writes a pixel whose previous bits must survive, and never reads out of range."""
    B, H, W = case["shape"][:3]
    r = case["rows"]
    npix = B * H * W
    if "plist" in r:
        f, keep = r["plist"]
        assert H == W and H % f == 0
        listed = pixel_list_of(patch_map(B, f, keep, case_seed(case) + 13), H).long()
    else:
        g = torch.Generator().manual_seed(case_seed(case) + 11)
        perm = torch.randperm(npix, generator=g)
        count = npix if r["count"] == "all" else int(r["count"])
        assert count <= npix
        listed = perm[:count]
    count = len(listed)
    on = torch.zeros(npix, dtype=torch.bool)
    on[listed] = True
    rest = (~on).nonzero()[:, 0]
    if len(rest) == 0:
        rest = torch.arange(npix)
    cap = rows_capacity(case, count, cus)
    pad = rest[torch.arange(cap - count) % len(rest)]
    return torch.cat([listed, pad]).to(torch.int32), count


def rows_expected(stored_y, rows, count, before):
    """The buffer after cmu_conv3x3_fwd_rows: ``stored_y`` (B, H, W, N) at the pixels rows[:count], ``before`` everywhere else."""
    N = stored_y.shape[-1]
    out = before.clone().reshape(-1, N)
    idx = rows[:count].long().to(out.device)
    out[idx] = stored_y.reshape(-1, N)[idx]
    return out.reshape(stored_y.shape)


def layer_weight(w, flip):
    """The tensor to hand to the packer so that the packed weight is ``w`` (N, K, 3, 3): ``w`` itself, or -- transpose_flip=True, the
    data-gradient pack -- the LAYER's weight (K, N, 3, 3), whose flipped transpose is ``w``."""
    return w.flip(2, 3).transpose(0, 1).contiguous() if flip else w


def tiles_geometry(case):
    B, H, W = case["shape"][:3]
    th = case["tiles"]["th"]
    return B, -(-H // th), -(-W // 16), th


def tiles_count(case, splits, ntiles):
    """The list count of a class, relative to the split count of the launch (split s walks the entries s, s + splits, ...)."""
    cls = case["tiles"]["cls"]
    assert splits >= 2 and 2 * splits < ntiles, "the case needs a split count between 2 and half the dense tile count"
    rem = 2 * splits + splits // 2 if 2 * splits + splits // 2 < ntiles else splits + splits // 2
    return {"zero": 0, "below": splits // 2, "equal": splits, "multiple": 2 * splits, "remainder": rem, "all": ntiles}[cls]


def tiles_list(case, splits):
    """-> (list int32 (dense tile count,), count): ``count`` distinct dense tile ids (b * tilesY + ty) * tilesX + tx, ascending or in a
    fixed permutation; the entries past the count hold valid, unlisted tile ids (listed ones only when every tile is listed)."""
    B, tY, tX, th = tiles_geometry(case)
    nt = B * tY * tX
    count = tiles_count(case, splits, nt)
    g = torch.Generator().manual_seed(case_seed(case) + 12)
    perm = torch.randperm(nt, generator=g)
    listed = perm[:count]
    if case["tiles"]["order"] == "asc":
        listed = listed.sort().values
    rest = perm[count:] if count < nt else perm
    pad = rest[torch.arange(nt - count) % len(rest)]
    return torch.cat([listed, pad]).to(torch.int32), count


def tiles_mask(case, tlist, count):
    """(B, H, W, 1) float64: 1 at the pixels of the tiles tlist[:count]."""
    B, H, W = case["shape"][:3]
    _, tY, tX, th = tiles_geometry(case)
    on = torch.zeros(B * tY * tX, dtype=torch.float64)
    on[tlist[:count].long().cpu()] = 1.0
    m = on.view(B, tY, 1, tX, 1).expand(B, tY, th, tX, 16).reshape(B, tY * th, tX * 16)
    return m[:, :H, :W].unsqueeze(-1).contiguous()


def wgrad_tiles_exact(case, x, dy, tlist, count, transform=None):
    """conv3x3_wgrad_exact of dY * [the pixel lies in a listed tile]: x is read wherever the halo of a listed tile reaches."""
    return conv3x3_wgrad_exact(x, dy.double() * tiles_mask(case, tlist, count).to(dy.device), transform)


# ------------------------------------------------------------------------------------------------
# the operands of a case (shared by the CPU walk of CASES and by the GPU files)
# ------------------------------------------------------------------------------------------------
def case_seed(case):
    return sum(ord(ch) for ch in case["id"]) + 17 * sum(case["shape"])


def make_transform(case, C, seed):
    """Integer scale in {-2, -1, 1, 2} (statistics cases: {-1, 1}) and integer shift; None without a transform."""
    if case["tf"] is None:
        return None
    small = case["rng"] == (-1, 1)
    g = torch.Generator().manual_seed(seed + 1)
    mags = torch.randint(1, 2 if small else 3, (C,), generator=g).to(torch.float32)
    scale = mags * (torch.randint(0, 2, (C,), generator=g).to(torch.float32) * 2 - 1)
    shift = torch.randint(-1, 2, (C,), generator=g).to(torch.float32)
    if small:
        shift = shift * (scale > 0)         # keeps the activated operand in {-1, 0, 1, 2} -> most of them in {0, 1}
    return scale, shift, int(case["tf"])


def bn_consts(N, seed):
    """Integer gate transform and integer mean, invstd in {0.5, 1, 2}."""
    g = torch.Generator().manual_seed(seed + 2)
    bscale = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).to(torch.float32)
    bshift = torch.randint(-1, 2, (N,), generator=g).to(torch.float32)
    mean = torch.randint(-2, 3, (N,), generator=g).to(torch.float32)
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
    return bscale, bshift, mean, invstd


def weights_of(case, dt, seed):
    """The case's integer weight in torch's layout: conv (N, K, 3, 3); dgrad of a conv: the LAYER's (K, N, 3, 3); ConvTranspose
    forward (K, N, 2, 2); its data gradients: the layer's (N, K, 2, 2)."""
    B, H, W, K, N = case["shape"]
    lo, hi = case["wrng"]
    fam = case["fam"]
    shape = {"c3f": (N, K, 3, 3), "c3rows": (N, K, 3, 3), "c3dg": (K, N, 3, 3), "ctf": (K, N, 2, 2), "ctdg": (N, K, 2, 2),
             "ctdgbn": (N, K, 2, 2)}[fam]
    w = int_operands(shape, lo, hi, 1.0, seed + 3)
    if case["lift"] and dt == "f16":
        if fam in ("c3f", "c3rows", "ctdg", "ctdgbn"):       # (the contraction runs over the weight's second dimension)
            w[:, ::8] *= float(case["lift"])
        else:
            w[::8] *= float(case["lift"])
    return w


def reference_of(case, dt, device="cpu", splits=None):
    """Integer operands and the exact reference of one case -> (operands dict, reference dict).  ``splits`` (wg3tiles): the split count of
    the launch, which the list classes are relative to (the GPU file passes the restated rule's; default: the case's ``form``)."""
    B, H, W, K, N = case["shape"]
    lo, hi = case["rng"]
    fam, seed = case["fam"], case_seed(case)
    o = {}
    if fam in ("c3f", "ctf"):
        o["x"] = int_operands((B, H, W, K), lo, hi, 1.0, seed).to(device)
        o["tf"] = make_transform(case, K, seed)
        o["w"] = weights_of(case, dt, seed)
        if case["spike"]:
            assert fam == "c3f" and case["tf"] is None
            x0 = torch.zeros(B, H, W)
            x0[:, 5::TILE, 7::TILE] = 1.0
            o["x"][..., 0] = x0.to(device)
            sign = int_operands((N,), 0, 1, 1.0, seed + 7) * 2.0 - 1.0
            o["w"][:, 0] = 0.0
            o["w"][:, 0, 1, 1] = sign * float(case["spike"])
        if fam == "c3f":
            ref = conv3x3_exact(o["x"], o["w"], o["tf"], dt)
        else:
            o["bias"] = int_operands((N,), -case["bias"], case["bias"], 1.0, seed + 4)
            ref = convT2x2_exact(o["x"], o["w"], o["bias"], o["tf"], dt)
    elif fam == "c3dg":
        o["dy"] = int_operands((B, H, W, K), lo, hi, 1.0, seed).to(device)
        o["w"] = weights_of(case, dt, seed)
        o["yraw"] = int_operands((B, H, W, N), -3, 3, 1.0, seed + 5).to(device)
        o["bn"] = bn_consts(N, seed)
        ref = conv3x3_dgrad_bn_exact(o["dy"], o["w"], o["yraw"], *o["bn"], dt=dt)
    elif fam in ("ctdg", "ctdgbn"):
        o["dout"] = int_operands((B, 2 * H, 2 * W, K), lo, hi, 1.0, seed).to(device)
        o["w"] = weights_of(case, dt, seed)
        if fam == "ctdg":
            ref = convT2x2_dgrad_exact(o["dout"], o["w"], dt)
        else:
            o["yraw"] = int_operands((B, H, W, N), -3, 3, 1.0, seed + 5).to(device)
            o["bn"] = bn_consts(N, seed)
            ref = convT2x2_dgrad_bn_exact(o["dout"], o["w"], o["yraw"], *o["bn"], dt=dt)
    elif fam == "wg3":
        o["x"] = int_operands((B, H, W, K), lo, hi, 1.0, seed).to(device)
        o["dy"] = int_operands((B, H, W, N), lo, hi, 1.0, seed + 6).to(device)
        o["tf"] = make_transform(case, K, seed)
        ref = conv3x3_wgrad_exact(o["x"], o["dy"], o["tf"])
    elif fam == "c3rows":
        assert case["tf"] is None and not case["stats"]
        o["x"] = int_operands((B, H, W, K), lo, hi, 1.0, seed).to(device)
        o["w"] = weights_of(case, dt, seed)
        if "plist" not in case["rows"]:        # (a builder-made list is read back from the device by the GPU file)
            o["rows"], o["count"] = rows_list(case)
        ref = conv3x3_exact(o["x"], o["w"], None, dt)
    elif fam == "wg3tiles":
        o["x"] = int_operands((B, H, W, K), lo, hi, 1.0, seed).to(device)
        o["dy"] = int_operands((B, H, W, N), lo, hi, 1.0, seed + 6).to(device)      # non-zero in the unlisted tiles as well
        o["tf"] = make_transform(case, K, seed)
        if "builder" in case["tiles"]:
            ref = conv3x3_wgrad_exact(o["x"], o["dy"], o["tf"])                     # (every tile: an upper bound of the list's terms)
        else:
            o["tiles"], o["count"] = tiles_list(case, splits or case["form"]["splits"])
            ref = wgrad_tiles_exact(case, o["x"], o["dy"], o["tiles"], o["count"], o["tf"])
    elif fam == "wgt":
        o["x"] = int_operands((B, H, W, K), lo, hi, 1.0, seed).to(device)
        o["dout"] = int_operands((B, 2 * H, 2 * W, N), lo, hi, 1.0, seed + 6).to(device)
        o["tf"] = make_transform(case, K, seed)
        ref = convT2x2_wgrad_exact(o["x"], o["dout"], o["tf"])
    else:
        raise ValueError(fam)
    return o, ref
