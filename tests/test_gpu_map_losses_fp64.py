"""The focal cross entropy (cmu_focal_fwd / _bwd), the map-weighted softmax sums (cmu_softmax_map_fwd / _bwd) and the distance fields
(cmu_distance_field) of csrc/map_loss.hip, and FocalLoss / TverskyLoss / BoundaryLoss / HausdorffDTLoss of cmunet_amd/metrics.py on
top of them, against float64 on the CPU from the same fp32 inputs: tests/map_loss_ref.py at the ops level (which
tests/test_cpu_map_losses.py holds to torch autograd and scipy), the hand-written float64 expressions of that CPU test, with distance
maps from scipy, at the class level.

Bounds, with U = 2^-24 and the project's constant C_GRAD = 16 (tests/test_gpu_seg_criterion_fp64.py):

* a sum: 16 U sum |term|.  Every term is a product of fp32 exponentials, one fp32 log1p and fp64 arithmetic in forms without
  cancellation (q and p_c - y_c are sums of the OTHER classes' exponentials over the total), so its error is a few U of itself.
  table[1] of the focal loss is a sum of fp32 weights in fp64 (2 U of the value), table[2] a count (exact).
* a gradient element: (16 + 4 gamma |ln q| [gamma not in {0, 1, 2}]) U magnitude + 2^-150, magnitude = the sum of the absolute
  values of the terms entering the element (tests/map_loss_ref.py); for the focal loss that is |dx| itself.  The bracket is the
  error of the one fp32 exp(gamma log q): the logarithm's 1 ulp is 2 U |ln q| absolute, times gamma, plus the product's rounding,
  taken to the exponent.  2^-150 is half the smallest positive fp32 number (the output is fp32).
* the squared kind is held to these bounds on ONE-HOT targets (what HausdorffDTLoss passes): against a soft target with p_c close
  to y_c the difference cancels in any arithmetic built on fp32 exponentials, and |G_c| -- what the magnitude is built from -- goes
  to zero with it.
* cmu_distance_field: equality of bits with the restatement from the GPU transform's own dist2 for alpha in {1, 2} and the signed
  mode; alpha = 2.5: (4 + 4 (alpha / 2) |ln d2|) U relative (one fp32 exp((alpha / 2) log d2)).
* a class value: the same 16 U carried through the reduction of the sums.

The worst error / bound ratio per kind is printed, and written to the file named by CMU_MAP_LOSS_PARITY_OUT when that is set
(profiles/map_loss_parity.txt holds one such run)."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import map_loss_ref as R
import mem_contract as MC
import test_cpu_map_losses as CT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_GRAD = 16
TINY = 2.0 ** -150
DEV = "cuda"
CAP = 1024                           # the grid cap of the passes, in blocks of 256 lanes
RATIOS = {}
WEIGHTS = [0.5, 2.0, 1.25, 0.75, 1.5, 1.0, 3.0, 0.25]
GAMMAS = (0.0, 0.5, 1.0, 2.0, 3.5)
LABEL_DT = {"i64": torch.int64, "i32": torch.int32, "u8": torch.uint8, "f32": torch.float32, "f64": torch.float64}


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), float(ratio))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    yield o
    lines = [f"{k}: worst error / bound = {r:.4f}" for k, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    out = os.environ.get("CMU_MAP_LOSS_PARITY_OUT")
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tests/test_gpu_map_losses_fp64.py: worst error of cmu_focal_*, cmu_softmax_map_*, cmu_distance_field and the loss classes\n"
                    f"# against float64, as a fraction of the bounds of the test's docstring ({C_GRAD} U sum |term| for a sum; ({C_GRAD} + 4 gamma |ln q|) U\n"
                    f"# magnitude + 2^-150 for a gradient element); worst over the {len(FOCAL_CASES)} focal and {len(MAP_CASES)} map cases\n")
            f.write("\n".join(lines) + "\n")


# Pixels per lane: 4 at K <= 4, 2 above, 1 when H*W is no multiple of that or a pointer is not 16-byte aligned; past the block cap:
#   vec4_stride    (5,2,464,464)  1,076,480 pixels = 269,120 groups: 1,052 blocks' worth
#   vec2_stride    (5,8,328,328)  537,920 pixels = 268,960 groups: 1,051 blocks' worth
#   scalar_stride  (5,2,257,257)  330,245 pixels: 1,291 blocks' worth
SHAPES = {"odd": (2, 9, 13), "vec": (3, 64, 64), "offset": (3, 8, 8), "vec4_stride": (5, 464, 464), "vec2_stride": (5, 328, 328),
          "scalar_stride": (5, 257, 257)}
# (K, shape, target, gammas): target = a label dtype or "oh32" / "oh64" (one-hot planes)
FOCAL_CASES = ([(K, s, "i64" if s == "odd" else "u8", GAMMAS) for K in (2, 3, 4, 5, 8) for s in ("odd", "vec")]
               + [(3, "odd", t, (2.0,)) for t in ("i32", "u8", "f32", "f64", "oh32", "oh64")] + [(8, "vec", "oh64", (0.5,)), (4, "vec", "oh32", (1.0,))]
               + [(2, "offset", "i64", (2.0, 3.5)), (2, "vec4_stride", "u8", (2.0,)), (8, "vec2_stride", "i64", (3.5,)), (2, "scalar_stride", "oh32", (0.5,))])
# (K, shape, kind, ydt, keep, weighted)
MAP_CASES = ([(K, s, kind, ydt, None if K in (3, 4) else tuple(range(1, K)), K != 4)
              for K in (2, 3, 4, 5, 8) for s in ("odd", "vec") for kind, ydt in (("linear", None), ("squared", "f32"), ("squared", "f64"))]
             + [(5, "odd", "linear", None, (1, 3), True), (8, "vec", "squared", "f64", (0, 2, 5, 7), True)]
             + [(2, "offset", "linear", None, (1,), True), (2, "offset", "squared", "f64", None, True),
                (2, "vec4_stride", "linear", None, (1,), True), (2, "scalar_stride", "squared", "f32", (1,), True),
                (8, "vec2_stride", "squared", "f64", (1, 4), True)])


def test_stride_cases_pass_their_grid_cap():
    """The arithmetic behind the *_stride cases (a guard on the case tables, not on the library): more groups than 1,024 blocks of 256
    lanes on the path each one takes -- 4 pixels per lane (2 at K > 4), 1 when the plane is no multiple --, and each path is there."""
    seen = set()
    for K, s in [(c[0], c[1]) for c in FOCAL_CASES] + [(c[0], c[1]) for c in MAP_CASES]:
        B, H, W = SHAPES[s]
        V = 1 if (H * W) % (2 if K > 4 else 4) else (2 if K > 4 else 4)
        if s.endswith("_stride"):
            assert B * H * W // V > CAP * 256 and V == {"vec4_stride": 4, "vec2_stride": 2, "scalar_stride": 1}[s]
            seen.add(s)
        elif s == "odd":
            assert V == 1
        elif s == "vec":
            assert V == (2 if K > 4 else 4) and B * H * W // V > 256
    assert seen == {"vec4_stride", "vec2_stride", "scalar_stride"}


def dev_x(x, offset):
    """x on the device; ``offset``: starting one element past an allocation's (16-byte aligned) start."""
    if not offset:
        return x.to(DEV)
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
    buf[1:].copy_(x.reshape(-1))
    v = buf[1:].view(x.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def held(entry, name, ws_bytes, outs, inputs, run, check):
    """tests/mem_contract.py's harness on the device: guarded buffers, the block partials in four states, every output element
    written (NaN prefill), the inputs untouched, the same bits on every run."""
    case = MC.Case(name, ws_bytes, outs, inputs, device=DEV, min_ws=16)
    return MC.check_call(entry, case, run, check)


def saturate(x, lab):
    """Logits of +-100 on the first pixels of image 0: the label's class at +100 (q underflows to 0), at -100 (p_t underflows), and
    two classes tied at +100."""
    K = x.shape[1]
    v = x[0].reshape(K, -1)
    l0 = lab[0].reshape(-1)
    for i in range(3):
        l0[i] = i % K
    v[:, 0] = -100.0
    v[int(l0[0]), 0] = 100.0
    v[:, 1] = 100.0
    v[int(l0[1]), 1] = -100.0
    v[:, 2] = -100.0
    v[int(l0[2]), 2] = 100.0
    v[(int(l0[2]) + 1) % K, 2] = 100.0


@functools.lru_cache(maxsize=None)
def focal_case(K, shape, target):
    """Logits randn * 2 with saturated pixels at the head; about 10 % of the label pixels ignored (-100; 250 for uint8 labels);
    floating-point labels carry a fraction (k + 0.5 truncates to k).  One-hot targets: the planes of the labels, nothing ignored."""
    B, H, W = SHAPES[shape]
    g = torch.Generator().manual_seed(K * 100 + H + len(target))
    x = torch.randn(B, K, H, W, generator=g) * 2
    lab = torch.randint(0, K, (B, H, W), generator=g)
    saturate(x, lab)
    if target.startswith("oh"):
        tgt = F.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().to(torch.float32 if target == "oh32" else torch.float64)
        return x.contiguous(), tgt, lab, -100
    ign = 250 if target == "u8" else -100
    drop = torch.rand(B, H, W, generator=g) < 0.1
    drop.view(-1)[:3] = False
    lab[drop] = ign
    tgt = lab.to(LABEL_DT[target])
    if tgt.is_floating_point():
        tgt = torch.where(tgt >= 0, tgt + 0.5, tgt)
    return x.contiguous(), tgt.contiguous(), lab, ign


def grad_check(kind, dx, r, gamma, what):
    lnq = r["lnq"] if "lnq" in r and gamma not in (0.0, 1.0, 2.0) else 0.0
    bound = (C_GRAD + 4 * gamma * lnq) * U * r["dx_mag"] + TINY
    err = (dx.double() - r["dx"]).abs()
    ratio = float((err / bound).max())
    note(kind, ratio)
    print(f"{what}: dx worst err/bound {ratio:.4f}")
    assert bool(torch.isfinite(dx).all()) and bool((err <= bound).all()), (what, ratio)


def sum_check(kind, got, want, mag, k, what):
    ratio = abs(float(got) - float(want)) / max(k * U * float(mag), 1e-300)
    note(kind, ratio)
    print(f"{what}: {float(got):.12g} ref {float(want):.12g} err/bound {ratio:.3g}")
    assert math.isfinite(float(got)) and ratio <= 1.0, (what, ratio)


# ---------------------------------------------------------------------------------------------------
# (a) focal cross entropy at the ops level
# ---------------------------------------------------------------------------------------------------
def focal_run(ops, xd, td, onehot, wd, gamma, ign, g):
    def run(ws, outs):
        partials = ws.view(torch.float64) if ws.numel() >= 3 * CAP * 8 else None
        if "table" in outs:
            ops.focal_fwd(xd, td, onehot, wd, gamma, ign, outs["table"], partials)
        if "dx" in outs:
            ops.focal_bwd(xd, td, onehot, wd, gamma, ign, None if g is None else torch.tensor([g], dtype=torch.float64, device=DEV), outs["dx"])
    return run


@pytest.mark.parametrize("K,shape,target,gammas", FOCAL_CASES)
def test_focal_ops(ops, K, shape, target, gammas):
    x, tgt, labels, ign = focal_case(K, shape, target)
    onehot = target.startswith("oh")
    xd, td = dev_x(x, shape == "offset"), tgt.to(DEV)
    got = {}
    for i, gamma in enumerate(gammas):
        w = torch.tensor(WEIGHTS[:K]) if i % 2 == 0 else None
        wd = None if w is None else w.to(DEV)
        g = 0.37 / labels.numel()
        r = R.focal_ref(x, labels, w, gamma, ign, g)
        what = f"focal K={K} {shape} {target} gamma={gamma} alpha={'yes' if w is not None else 'no'}"

        def check(outs):
            T, dx = outs["table"].cpu(), outs["dx"].cpu()
            sum_check("focal_sum", T[0], r["T"][0], r["T_mag"][0], C_GRAD, what + " T0")
            sum_check("focal_sum", T[1], r["T"][1], r["T_mag"][1], 2, what + " T1")
            assert float(T[2]) == float(r["T"][2])
            grad_check("focal_grad" + ("" if gamma in (0.0, 1.0, 2.0) else "_pow"), dx, r, gamma, what)
            assert bool((dx[(labels == ign).unsqueeze(1).expand_as(dx)] == 0).all())
            got[gamma] = (T, dx)
        rec = held("cmu_focal_fwd+bwd", what, 3 * CAP * 8, {"table": MC.Out((3,), torch.float64), "dx": MC.Out(x.shape)},
                   {"x": xd, "target": td}, focal_run(ops, xd, td, onehot, wd, gamma, ign, g), check)
        assert rec["states"][:2] == ["zero", "zero again"]
    if shape == "offset":
        # element by element the one-pixel path computes what the vector path does: the aligned tensor gives the same gradient
        gamma = gammas[-1]
        w = torch.tensor(WEIGHTS[:K]) if (len(gammas) - 1) % 2 == 0 else None
        dx3 = torch.empty(x.shape, device=DEV)
        ops.focal_bwd(x.to(DEV), td, onehot, None if w is None else w.to(DEV), gamma, ign,
                      torch.tensor([0.37 / labels.numel()], dtype=torch.float64, device=DEV), dx3)
        assert torch.equal(dx3.cpu(), got[gamma][1])
    if shape == "vec" and K == 3:
        dx0 = torch.full(x.shape, 7.0, device=DEV)
        ops.focal_bwd(xd, td, onehot, None, 2.0, ign, None, dx0)              # a NULL upstream gradient stands for zero
        assert bool((dx0 == 0).all())


def test_focal_out_of_range_label_is_nan_and_never_an_index(ops):
    K = 3
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, K, 4, 4, generator=g) * 2
    lab = torch.randint(0, K, (1, 4, 4), generator=g)
    lab[0, 1, 2] = K
    lab[0, 3, 3] = -100
    w = torch.tensor(WEIGHTS[:K])
    r = R.focal_ref(x, lab, w, 2.0, -100, 0.4)
    T, dx = torch.empty(3, dtype=torch.float64, device=DEV), torch.full(x.shape, 7.0, device=DEV)
    ops.focal_fwd(x.to(DEV), lab.to(DEV), False, w.to(DEV), 2.0, -100, T)
    ops.focal_bwd(x.to(DEV), lab.to(DEV), False, w.to(DEV), 2.0, -100, torch.tensor([0.4], dtype=torch.float64, device=DEV), dx)
    T, dx = T.cpu(), dx.cpu()
    assert math.isnan(float(T[0])) and math.isnan(float(r["T"][0])) and float(T[2]) == 15.0 == float(r["T"][2])
    assert abs(float(T[1]) - float(r["T"][1])) <= 2 * U * float(r["T_mag"][1])
    assert bool((dx[0, :, 1, 2] == 0).all()) and bool((dx[0, :, 3, 3] == 0).all()) and float(dx.abs().sum()) > 0
    grad_check("focal_grad", dx, r, 2.0, "focal out-of-range label")
    from cmunet_amd import metrics as M
    assert math.isnan(float(M.FocalLoss(alpha=w)(x.to(DEV).requires_grad_(True), lab.to(DEV))))


@pytest.mark.parametrize("K,shape,target", [(2, "odd", "i64"), (3, "vec", "u8"), (8, "vec", "oh64"), (5, "odd", "f32"), (2, "vec4_stride", "u8")])
def test_focal_gamma_zero_is_the_index_cross_entropy(ops, K, shape, target):
    """gamma = 0: table[0] and table[1] are those of cmu_index_ce_fwd BIT FOR BIT (the same -log p_t, the same grid, the same order
    of sums).  The gradient agrees within the two kernels' bounds, not in bits, and the code shows why: the index CE forms
    p_j - [j == t] from p_j = e_j / (1 + rest) in fp32, the focal pass forms -q at j == t from the fp64 sum of the OTHER exponentials
    (the form that keeps its bits when q^(gamma-1) multiplies it) and takes p_j from seg_softmax, whose sum runs in class order."""
    from cmunet_amd import _lib
    x, tgt, labels, ign = focal_case(K, shape, target)
    onehot = target.startswith("oh")
    xd, td, w = x.to(DEV), tgt.to(DEV), torch.tensor(WEIGHTS[:K])
    gup = 0.37 / labels.numel()
    for wd in (None, w.to(DEV)):
        Tf, Ti = torch.empty(3, dtype=torch.float64, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV)
        ws = torch.empty(_lib.lib().cmu_index_ce_ws_bytes(), dtype=torch.uint8, device=DEV)
        ops.focal_fwd(xd, td, onehot, wd, 0.0, ign, Tf)
        ops.index_ce_fwd(xd, td, onehot, False, None, wd, ign, Ti, ws)
        assert torch.equal(Tf[:2], Ti[:2]), (Tf.tolist(), Ti.tolist())
        dxf, dxi = torch.empty(x.shape, device=DEV), torch.empty(x.shape, device=DEV)
        ops.focal_bwd(xd, td, onehot, wd, 0.0, ign, torch.tensor([gup], dtype=torch.float64, device=DEV), dxf)
        ops.index_ce_bwd(xd, td, onehot, False, None, wd, ign, torch.tensor([gup, 0.0], dtype=torch.float64, device=DEV), dxi)
        r = R.focal_ref(x, labels, None if wd is None else w, 0.0, ign, gup)
        # index CE's magnitude |g| w_t (p_j + [j == t]) is at most twice the focal one at j == t (1 + p_t against q ... both bounded by
        # 2 |g| w_t), so the combined bound is written on the larger of the two: 16 U |g| w_t (p_j + [j == t]) + 16 U |dx|
        live = ((labels != ign) & (labels >= 0) & (labels < K)).unsqueeze(1).double()
        oh = F.one_hot(labels.clamp(0, K - 1), K).permute(0, 3, 1, 2).double() * live
        wt = ((torch.ones(K, dtype=torch.float64) if wd is None else w.double()).view(1, K, 1, 1) * oh).sum(1, keepdim=True)
        ice_mag = abs(gup) * wt * (torch.softmax(x.double(), 1) * live + oh)
        bound = C_GRAD * U * (ice_mag + r["dx_mag"]) + 2 * TINY
        err = (dxf.cpu().double() - dxi.cpu().double()).abs()
        note("focal_gamma0_vs_index_ce", float((err / bound).max()))
        assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------------
# (b) map-weighted softmax sums at the ops level
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def map_case(K, shape, ydt):
    """Logits as ``focal_case``; a signed weight map randn * 3 (phi is signed) with exact zeros; a one-hot target."""
    B, H, W = SHAPES[shape]
    g = torch.Generator().manual_seed(K * 77 + H)
    x = torch.randn(B, K, H, W, generator=g) * 2
    lab = torch.randint(0, K, (B, H, W), generator=g)
    saturate(x, lab)
    w = torch.randn(B, K, H, W, generator=g) * 3
    w[torch.rand(B, K, H, W, generator=g) < 0.05] = 0.0
    y = F.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().to(torch.float64 if ydt == "f64" else torch.float32)
    return x.contiguous(), w.contiguous(), y


def map_run(ops, xd, wd, yd, keep, kind, g):
    def run(ws, outs):
        K = xd.shape[1]
        partials = ws.view(torch.float64) if ws.numel() >= K * CAP * 8 else None
        if "table" in outs:
            ops.softmax_map_fwd(xd, wd, yd, keep, kind, outs["table"], partials)
        if "dx" in outs:
            ops.softmax_map_bwd(xd, wd, yd, keep, kind, None if g is None else torch.tensor(g, dtype=torch.float64, device=DEV), outs["dx"])
    return run


@pytest.mark.parametrize("K,shape,kind,ydt,keep,weighted", MAP_CASES)
def test_softmax_map_ops(ops, K, shape, kind, ydt, keep, weighted):
    x, w, y = map_case(K, shape, ydt)
    if not weighted:
        w = None
    keep_l = None if keep is None else list(keep)
    kp = list(range(K)) if keep is None else list(keep)
    xd, yd = dev_x(x, shape == "offset"), y.to(DEV)
    wd = None if w is None else w.to(DEV)
    npix = x.numel() // K
    g = [0.37 * (c + 1) * (-1) ** c / npix for c in range(K)]
    r = R.softmax_map_ref(x, w, y, keep_l, kind, g)
    what = f"map {kind} K={K} {shape} y={ydt} keep={keep} Wm={'yes' if weighted else 'no'}"
    got = {}

    def check(outs):
        T, dx = outs["table"].cpu(), outs["dx"].cpu()
        for c in range(K):
            if c in kp:
                sum_check(f"map_{kind}_sum", T[c], r["T"][c], r["T_mag"][c], C_GRAD, f"{what} T{c}")
            else:
                assert float(T[c]) == 0.0
        grad_check(f"map_{kind}_grad", dx, r, 0.0, what)
        got["dx"] = dx
    held("cmu_softmax_map_fwd+bwd", what, K * CAP * 8, {"table": MC.Out((K,), torch.float64), "dx": MC.Out(x.shape)},
         {"x": xd, "y": yd, **({} if wd is None else {"wmap": wd})}, map_run(ops, xd, wd, yd, keep_l, kind, g), check)
    if shape == "offset":
        dx3 = torch.empty(x.shape, device=DEV)
        ops.softmax_map_bwd(x.to(DEV), wd, yd, keep_l, kind, torch.tensor(g, dtype=torch.float64, device=DEV), dx3)
        assert torch.equal(dx3.cpu(), got["dx"])
    if shape == "vec" and K == 3:
        dx0 = torch.full(x.shape, 7.0, device=DEV)
        ops.softmax_map_bwd(xd, wd, yd, keep_l, kind, None, dx0)
        assert bool((dx0 == 0).all())


def test_unkept_planes_are_not_read(ops):
    """NaN in the weight-map and target planes of the classes outside keep_mask changes nothing: they are not read."""
    K, keep = 4, [1, 3]
    x, w, y = map_case(K, "vec", "f64")
    wn, yn = w.clone(), y.clone()
    wn[:, [0, 2]] = float("nan")
    yn[:, [0, 2]] = float("nan")
    g = torch.tensor([0.1, -0.2, 0.3, 0.4], dtype=torch.float64, device=DEV)
    for kind in ("linear", "squared"):
        res = []
        for ww, yy in ((w, y), (wn, yn)):
            T, dx = torch.empty(K, dtype=torch.float64, device=DEV), torch.empty(x.shape, device=DEV)
            ops.softmax_map_fwd(x.to(DEV), ww.to(DEV), yy.to(DEV), keep, kind, T)
            ops.softmax_map_bwd(x.to(DEV), ww.to(DEV), yy.to(DEV), keep, kind, g, dx)
            res.append((T.cpu(), dx.cpu()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and bool(torch.isfinite(res[1][1]).all())


def test_ops_refuse_bad_arguments(ops):
    from cmunet_amd import _lib
    x = torch.zeros(2, 9, 4, 4, device=DEV)
    lab = torch.zeros(2, 4, 4, dtype=torch.int64, device=DEV)
    t, part = torch.empty(9, dtype=torch.float64, device=DEV), ops.map_loss_partials(9, DEV)
    P, S = ops._p, ops._stream()
    with pytest.raises(_lib.CmuError, match="2 <= K <= 8"):
        _lib.call("cmu_focal_fwd", P(x), P(lab), 0, None, 2.0, -100, P(t), P(part), 2, 9, 4, 4, S)
    with pytest.raises(_lib.CmuError, match="unknown target kind"):
        _lib.call("cmu_focal_bwd", P(x), P(lab), 7, None, 2.0, -100, None, P(x), 2, 3, 4, 4, S)
    with pytest.raises(_lib.CmuError, match="gamma"):
        _lib.call("cmu_focal_fwd", P(x), P(lab), 0, None, -1.0, -100, P(t), P(part), 2, 3, 4, 4, S)
    with pytest.raises(_lib.CmuError, match="keep_mask"):
        _lib.call("cmu_softmax_map_fwd", P(x), None, None, 0, 1 << 3, 0, P(t), P(part), 2, 3, 4, 4, S)
    with pytest.raises(_lib.CmuError, match="unknown kind"):
        _lib.call("cmu_softmax_map_bwd", P(x), None, None, 0, 1, 2, None, P(x), 2, 3, 4, 4, S)
    with pytest.raises(_lib.CmuError, match="bad args"):
        _lib.call("cmu_softmax_map_fwd", P(x), None, None, 0, 1, 1, P(t), P(part), 2, 3, 4, 4, S)      # the squared kind without a target
    d2 = torch.zeros(2, 4, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.CmuError, match="plane"):
        _lib.call("cmu_distance_field", P(d2), P(d2), None, None, 0, 2.0, P(x), 9, 2, 9, 4, 4, S)
    with pytest.raises(_lib.CmuError, match="second pair"):
        _lib.call("cmu_distance_field", P(d2), P(d2), P(d2), P(d2), 0, 2.0, P(x), 0, 2, 9, 4, 4, S)
    with pytest.raises(_lib.CmuError, match="alpha"):
        _lib.call("cmu_distance_field", P(d2), P(d2), None, None, 1, 0.0, P(x), 0, 2, 9, 4, 4, S)


# ---------------------------------------------------------------------------------------------------
# (c) distance fields: equality with the restatement from the GPU transform's own dist2
# ---------------------------------------------------------------------------------------------------
def field_batch(H, W):
    """(B,H,W) uint8 masks that hit each rule: a single pixel, a one-pixel-wide diagonal vessel, a set touching all four borders, an
    empty and a full image between ordinary ones, a vessel-like mask."""
    import edt_cases
    m = np.zeros((6, H, W), np.uint8)
    m[0, H // 2, W // 3] = 1
    i = np.arange(min(H, W))
    m[1, i, i] = 1
    m[2, 0, :] = m[2, -1, :] = m[2, :, 0] = m[2, :, -1] = 1
    m[2, H // 2, 2:W - 2] = 1
    m[4] = 1                                                                 # (3: empty, 4: full)
    m[5] = edt_cases.vessel_like(H, W, strokes=3, steps=40, seed=11)
    return torch.from_numpy(m)


def d2_pair(ops, src, cls_to, cls_from):
    return ops.edt_rows(ops.edt_columns(src, cls_to)), ops.edt_rows(ops.edt_columns(src, cls_from))


@pytest.mark.parametrize("H,W", [(9, 13), (16, 24), (24, 17)])
def test_distance_field_equals_the_restatement(ops, H, W):
    """H != W; (16,24): H*W % 4 == 0, the 4-pixel path; the others the one-pixel path.  The plane goes into the middle class of a
    (B,3,H,W) map whose neighbouring planes are prefilled and must stay untouched."""
    a = field_batch(H, W).to(DEV)
    b = torch.roll(a, shifts=(1, 2, 3), dims=(0, 1, 2)).contiguous()        # a second set per image: the "prediction" of the pair
    to_a, from_a = d2_pair(ops, a, -1, 0)
    to_b, from_b = d2_pair(ops, b, -1, 0)
    na, nb = [t.cpu().numpy() for t in (to_a, from_a)], [t.cpu().numpy() for t in (to_b, from_b)]
    assert (na[0][3] == -1).all() and (na[1][4] == -1).all() and (na[0][0] >= 0).all()
    B = a.shape[0]

    def run_mode(mode, alpha, second):
        def run(ws, outs):
            f = outs["field"]
            f[:, 0] = 5.0
            f[:, 2] = -6.0
            ops.distance_field(to_a, from_a, f, 1, mode, alpha, *((to_b, from_b) if second else (None, None)))
        return run

    def check_for(want, rel=None, d2=None):
        def check(outs):
            f = outs["field"].cpu()
            assert bool((f[:, 0] == 5.0).all()) and bool((f[:, 2] == -6.0).all())
            got = f[:, 1].numpy()
            if rel is None:
                assert got.dtype == np.float32 and np.array_equal(got, want)
                return 0.0
            err = np.abs(got.astype(np.float64) - want)
            bound = rel * np.abs(want)
            assert (err <= bound).all()
            return float((err / np.maximum(bound, 1e-300)).max())
        return check

    out = {"field": MC.Out((B, 3, H, W), marks_unwritten=False, why="the neighbouring planes are the caller's")}
    ins = {"to_a": to_a, "from_a": from_a, "to_b": to_b, "from_b": from_b}
    phi = R.signed_field_ref(*na)
    assert not phi[3].any() and not phi[4].any() and phi[0].min() == 0.0 and phi[1].max() > 1
    held("cmu_distance_field", f"signed {H}x{W}", 0, out, ins, run_mode("signed", 2.0, False), check_for(phi))
    for alpha in (1, 2):
        fa, fb = R.unsigned_field_ref(*na, alpha)[0], R.unsigned_field_ref(*nb, alpha)[0]
        held("cmu_distance_field", f"unsigned alpha={alpha} {H}x{W}", 0, out, ins, run_mode("unsigned", alpha, False), check_for(fa))
        held("cmu_distance_field", f"unsigned pair alpha={alpha} {H}x{W}", 0, out, ins, run_mode("unsigned", alpha, True), check_for(fa + fb))
        assert not fa[3].any() and not fa[4].any() and (fa + fb)[3].any()            # the empty image's addend is 0, its partner's is not
    _, ea, d2a = R.unsigned_field_ref(*na, 2.5)
    _, eb, d2b = R.unsigned_field_ref(*nb, 2.5)
    rel = (4 + 4 * 1.25 * np.log(np.maximum(np.maximum(d2a, d2b), 1))) * U
    rec = held("cmu_distance_field", f"unsigned pair alpha=2.5 {H}x{W}", 0, out, ins, run_mode("unsigned", 2.5, True), check_for(ea + eb, rel + U))
    note("distance_field_alpha_2.5", rec["worst"])


def test_distance_maps_of_the_metrics_layer_against_scipy(ops):
    from cmunet_amd import metrics as M
    K = 3
    lab = CT.vessel_batch(K)
    y1h = F.one_hot(lab, K).permute(0, 3, 1, 2).double()
    want = CT.scipy_signed_maps(lab, K, range(K))
    for tgt, kw in ((lab.to(torch.uint8).to(DEV), dict(classes=K)), (lab.unsqueeze(1).to(DEV), dict(classes=K)), (y1h.to(DEV), {})):
        got = M.signed_distance_maps(tgt, **kw)
        assert got.dtype == torch.float32 and not got.requires_grad and torch.equal(got.cpu(), want)
    masks = np.stack([(lab.numpy() == c) for c in range(K)], 1)                        # (B,K,H,W)
    pr = np.roll(masks, 3, axis=3)
    for alpha in (1.0, 2.0):
        fa, fb = CT.scipy_fields(masks, alpha), CT.scipy_fields(pr, alpha)
        got = M.distance_fields(y1h.to(DEV), alpha=alpha)
        if alpha == 1.0:
            assert torch.equal(got.cpu(), fa)
        else:                                                                          # scipy's root squared again against the integer
            assert bool(((got.cpu() - fa).abs() <= 4 * U * fa).all())
        both = M.distance_fields(torch.from_numpy(pr.astype(np.uint8)).to(DEV), y1h.to(DEV), alpha=alpha)
        assert bool(((both.cpu() - (fa + fb)).abs() <= 4 * U * (fa + fb)).all())
    with pytest.raises(ValueError):
        M.signed_distance_maps(lab.to(DEV))                                            # a label map needs classes=


# ---------------------------------------------------------------------------------------------------
# the classes, on a (2,K,24,40) batch with vessel-like targets
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def class_case(K):
    lab = CT.vessel_batch(K)
    g = torch.Generator().manual_seed(40 + K)
    x = torch.randn(2, K, 24, 40, generator=g) * 2 + 1.5 * F.one_hot(lab, K).permute(0, 3, 1, 2)      # a prediction that has learnt something
    # a pixel with a probability within 1e-3 of the threshold 0.5 gets +-4 logits, so that the thresholded sets are the same in fp32 and fp64
    near = ((torch.softmax(x.double(), 1) - 0.5).abs() < 1e-3).any(1, keepdim=True)
    pix = torch.arange(2 * 24 * 40).view(2, 24, 40)
    x = torch.where(near, torch.where(F.one_hot(pix % K, K).permute(0, 3, 1, 2).bool(), 4.0, -4.0), x)
    p = torch.softmax(x.double(), 1)
    assert bool(((p - 0.5).abs() > 1e-4).all()) and float(near.double().mean()) < 0.02
    y = F.one_hot(lab, K).permute(0, 3, 1, 2).double().contiguous()
    return x.contiguous(), lab, y


def run_class(crit, x, target, *extra):
    from cmunet_amd import metrics as M
    M.clear_seg_cache()
    xd = x.to(DEV).requires_grad_(True)
    v = crit(xd, target, *extra)
    assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda
    v.backward()
    return v.detach().cpu(), xd.grad.cpu()


@pytest.mark.parametrize("K,gamma,red,target", [(2, 2.0, "mean", "i64"), (3, 0.5, "weighted_mean", "u8"), (5, 3.5, "sum", "oh64"), (3, 0.0, "weighted_mean", "i64")])
def test_focal_loss_class(ops, K, gamma, red, target):
    from cmunet_amd import metrics as M
    x, lab, y = class_case(K)
    lab = lab.clone()
    ign = 250 if target == "u8" else -100
    if not target.startswith("oh"):
        lab[torch.rand(lab.shape, generator=torch.Generator().manual_seed(5)) < 0.1] = ign
    alpha = torch.tensor(WEIGHTS[:K])
    tgt = y.to(DEV) if target.startswith("oh") else lab.to(LABEL_DT[target]).unsqueeze(1).to(DEV)
    crit = M.FocalLoss(gamma=gamma, alpha=alpha, ignore_index=ign, reduction=red)
    v, grad = run_class(crit, x, tgt)
    x64 = x.double().requires_grad_(True)
    want = CT.hand_focal(x64, lab, alpha, gamma, ign, red)
    want.backward()
    r0 = R.focal_ref(x, lab, alpha, gamma, ign)
    den = float(r0["T"][2]) if red == "mean" else float(r0["T"][1]) if red == "weighted_mean" else 1.0
    r = R.focal_ref(x, lab, alpha, gamma, ign, 1.0 / den)
    sum_check("focal_loss", v, want.detach(), float(r0["T_mag"][0]) / den, C_GRAD + 2, f"FocalLoss K={K} gamma={gamma} {red}")
    assert bool(((r["dx"] - x64.grad).abs() <= 1e-10 * r["dx_mag"] + 1e-300).all())
    grad_check("focal_loss", grad, r, gamma, f"FocalLoss K={K} gamma={gamma} {red} {target}")
    if gamma == 0.0:
        # the values of RobustCrossEntropyLoss, bit for bit: its 'mean' is the weighted mean (the gradients: the seam test above)
        rv, _ = run_class(M.RobustCrossEntropyLoss(weight=alpha, ignore_index=ign).to(DEV), x, tgt)
        assert torch.equal(rv, v)


def seg_grad_bound(x, y, g_tp, g_spr):
    """The bound of cmu_seg_stats_bwd (tests/test_gpu_seg_criterion_fp64.py's grad_bound with g_ce = 0)."""
    K = x.shape[1]
    L = x.double()
    p, lse = torch.softmax(L, 1), torch.logsumexp(L, 1, keepdim=True)
    G = (g_tp.view(1, K, 1, 1) * y + g_spr.view(1, K, 1, 1)).abs()
    return U * (C_GRAD + 2 * (L - lse).abs()) * p * (G + (p * G).sum(1, keepdim=True))


def counter_grads(x, y, fn):
    """d fn(tp, spr, sgt) / d (tp, spr) at the float64 soft counters."""
    p = torch.softmax(x.double(), 1)
    tp, spr = (y * p).sum((0, 2, 3)).requires_grad_(True), p.sum((0, 2, 3)).requires_grad_(True)
    return torch.autograd.grad(fn(tp, spr, y.sum((0, 2, 3))), (tp, spr))


@pytest.mark.parametrize("K,alpha,beta,gamma,ign", [(2, 0.5, 0.5, 1.0, [0]), (3, 0.3, 0.7, 0.75, [0]), (5, 0.7, 0.3, 1.0, None)])
def test_tversky_loss_class(ops, K, alpha, beta, gamma, ign):
    from cmunet_amd import metrics as M
    x, lab, y = class_case(K)
    keep = [c for c in range(K) if c not in (ign or [])]
    eps = 1e-7
    v, grad = run_class(M.TverskyLoss(alpha, beta, gamma, eps, ignore_channels=ign), x, y.to(DEV))
    x64 = x.double().requires_grad_(True)
    want = CT.hand_tversky(x64, y, alpha, beta, gamma, eps, keep)
    want.backward()
    p = torch.softmax(x.double(), 1)[:, keep]
    tp, spr, sgt = float((p * y[:, keep]).sum()), float(p.sum()), float(y[:, keep].sum())
    N, D = tp + eps, tp + alpha * (spr - tp) + beta * (sgt - tp) + eps
    ti = N / D
    d_ti = ti * C_GRAD * U * (tp / N + (abs(1 - alpha - beta) * tp + alpha * spr + beta * sgt) / D)      # every counter within 16 U of itself
    vb = 1.01 * max(1.0, gamma * (1 - ti) ** (gamma - 1)) * d_ti + 4e-16
    print(f"TverskyLoss K={K}: {float(v):.12g} ref {float(want):.12g} err/bound {abs(float(v) - float(want)) / vb:.3g}")
    assert abs(float(v) - float(want.detach())) <= vb
    g_tp, g_spr = counter_grads(x, y, lambda a, b, c: (1 - M.tversky_from_counters(a, b, c, alpha, beta, eps, ign)) ** gamma)
    bound = seg_grad_bound(x, y, g_tp, g_spr) + TINY
    err = (grad.double() - x64.grad).abs()
    note("tversky_loss", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    if (alpha, beta, gamma) == (0.5, 0.5, 1.0):
        # the Dice loss: (2 tp + 2 eps) / (2 tp + fn + fp + 2 eps) against (2 tp + eps') / (... + eps'): equal at eps' = 2 eps, and the
        # two differ by at most |eps' - 2 eps| / D for any other pair
        d2, _ = run_class(M.DiceLoss(eps=2 * eps, beta=1.0, activation="softmax", ignore_channels=ign, threshold=None), x, y.to(DEV))
        assert abs(float(d2) - float(v)) <= 4e-16
        d1, _ = run_class(M.DiceLoss(eps=1e-5, beta=1.0, activation="softmax", ignore_channels=ign, threshold=None), x, y.to(DEV))
        assert abs(float(d1) - float(v)) <= abs(1e-5 - 2 * eps) / (2 * D) + 4e-16
    # with a threshold the value is detached
    M.clear_seg_cache()
    vt = M.TverskyLoss(alpha, beta, gamma, eps, ignore_channels=ign, threshold=0.5)(x.to(DEV).requires_grad_(True), y.to(DEV))
    assert not vt.requires_grad and 0.0 <= float(vt) <= 1.0


@pytest.mark.parametrize("K,ign", [(2, (0,)), (3, (0,)), (5, None)])
def test_boundary_loss_class(ops, K, ign):
    from cmunet_amd import metrics as M
    x, lab, y = class_case(K)
    keep = [c for c in range(K) if c not in (ign or ())]
    phi = CT.scipy_signed_maps(lab, K, keep)
    crit = M.BoundaryLoss(ignore_channels=ign)
    v, grad = run_class(crit, x, y.to(DEV))
    x64 = x.double().requires_grad_(True)
    want = CT.hand_boundary(x64, phi, keep)
    want.backward()
    N = 2 * len(keep) * 24 * 40
    r = R.softmax_map_ref(x, phi, None, keep, "linear", [1.0 / N] * K)
    sum_check("boundary_loss", v, want.detach(), float(r["T_mag"].sum()) / N, C_GRAD + 2, f"BoundaryLoss K={K}")
    assert bool(((r["dx"] - x64.grad).abs() <= 1e-10 * r["dx_mag"] + 1e-300).all())
    grad_check("boundary_loss", grad, r, 0.0, f"BoundaryLoss K={K}")
    # precomputed maps, and a label-map target: the same bits
    maps = M.signed_distance_maps(y.to(DEV))
    assert torch.equal(maps[:, keep].cpu(), phi[:, keep])
    for args in ((y.to(DEV), maps), (None, maps), (lab.to(DEV),)):
        v2, grad2 = run_class(crit, x, *args)
        assert torch.equal(v2, v) and torch.equal(grad2, grad)
    v3, grad3 = run_class(M.BoundaryLoss(ignore_channels=ign, maps=maps), x, y.to(DEV))
    assert torch.equal(v3, v) and torch.equal(grad3, grad)
    # a prediction that is the target itself: the sum of phi inside the target, a negative value
    perfect = (y * 60 - 30).float()
    vp = crit(perfect.to(DEV), y.to(DEV))
    assert float(vp) < 0 and abs(float(vp) - float((phi.double()[:, keep] * y[:, keep]).sum() / N)) <= 1e-9


@pytest.mark.parametrize("K,alpha,ign,ydt", [(2, 2.0, (0,), torch.float64), (3, 1.0, (0,), torch.float32), (5, 2.0, None, torch.float64)])
def test_hausdorff_dt_loss_class(ops, K, alpha, ign, ydt):
    from cmunet_amd import metrics as M
    x, lab, y = class_case(K)
    keep = [c for c in range(K) if c not in (ign or ())]
    p = torch.softmax(x.double(), 1)
    w = torch.zeros(x.shape)
    w[:, keep] = CT.scipy_fields((p > 0.5).numpy()[:, keep], alpha) + CT.scipy_fields((y > 0.5).numpy()[:, keep], alpha)
    if alpha == 2.0:                                                        # the kernel's field is the integer d2: scipy's root squared is not
        w = torch.round(w)
    v, grad = run_class(M.HausdorffDTLoss(alpha=alpha, ignore_channels=ign), x, y.to(ydt).to(DEV))
    x64 = x.double().requires_grad_(True)
    want = CT.hand_squared(x64, y, w, keep)
    want.backward()
    N = 2 * len(keep) * 24 * 40
    r = R.softmax_map_ref(x, w, y, keep, "squared", [1.0 / N] * K)
    sum_check("hausdorff_dt_loss", v, want.detach(), float(r["T_mag"].sum()) / N, C_GRAD + 2, f"HausdorffDTLoss K={K} alpha={alpha}")
    # (torch's p - y in float64 against the restatement's form without cancellation: 1e-16 of p, not of the difference)
    assert bool(((r["dx"] - x64.grad).abs() <= 1e-10 * r["dx_mag"] + 1e-14 / N * w.double().max()).all())
    grad_check("hausdorff_dt_loss", grad, r, 0.0, f"HausdorffDTLoss K={K} alpha={alpha}")
    assert float(v) > 0


def test_combined_loss_is_the_weighted_sum_of_its_parts(ops, monkeypatch):
    """DiceLoss() + 0.5 * FocalLoss() + 0.01 * BoundaryLoss() forward and backward: the gradient is the weighted sum of the parts'
    gradients within their bounds; and TverskyLoss() + CrossEntropyLoss() runs cmu_seg_stats_fwd once."""
    from cmunet_amd import metrics as M
    K = 3
    x, lab, y = class_case(K)
    parts = [(1.0, M.DiceLoss(activation="softmax", threshold=None)), (0.5, M.FocalLoss()), (0.01, M.BoundaryLoss())]
    crit = parts[0][1] + 0.5 * parts[1][1] + 0.01 * parts[2][1]
    assert crit.__name__ == "dice_loss + 0.5 * focal_loss + 0.01 * boundary_loss"
    v, grad = run_class(crit, x, y.to(DEV))
    vals, grads = zip(*[run_class(c, x, y.to(DEV)) for _, c in parts])
    assert abs(float(v) - sum(a * float(pv) for (a, _), pv in zip(parts, vals))) <= 4e-16 * sum(abs(a * float(pv)) for (a, _), pv in zip(parts, vals))
    g_tp, g_spr = counter_grads(x, y, lambda a, b, c: 1 - M.f_score_from_counters(a, b, c, 1.0, 1e-5, None))
    N = 2 * 2 * 24 * 40
    rf = R.focal_ref(x, lab, None, 2.0, -100, 0.5 / lab.numel())
    rb = R.softmax_map_ref(x, CT.scipy_signed_maps(lab, K, [1, 2]), None, [1, 2], "linear", [0.01 / N] * K)
    # every part's fp32 gradient is within its bound; their fp32 sum adds one rounding per addition
    bound = seg_grad_bound(x, y, g_tp, g_spr) + C_GRAD * U * (rf["dx_mag"] + rb["dx_mag"]) + 3 * TINY
    total = sum(a * gp.double() for (a, _), gp in zip(parts, grads))
    err = (grad.double() - total).abs()
    slack = 3 * U * sum(abs(a) * gp.double().abs() for (a, _), gp in zip(parts, grads)) + TINY
    assert bool((err <= slack).all())
    x64 = x.double().requires_grad_(True)
    p = torch.softmax(x64, 1)
    tp = (p * y).sum()
    dice = 1 - (2 * tp + 1e-5) / (2 * tp + (y.sum() - tp) + (p.sum() - tp) + 1e-5)
    want = dice + 0.5 * CT.hand_focal(x64, lab, None, 2.0, -100, "mean") + 0.01 * CT.hand_boundary(x64, CT.scipy_signed_maps(lab, K, [1, 2]), [1, 2])
    want.backward()
    err = (grad.double() - x64.grad).abs()
    note("dice+focal+boundary", float((err / (bound + slack)).max()))
    assert bool((err <= bound + slack).all()), float((err / (bound + slack)).max())
    # one pass of the counters for TverskyLoss + CrossEntropyLoss
    calls = []
    real = ops.seg_stats_fwd
    monkeypatch.setattr(ops, "seg_stats_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for K2 in (2, 3):
        x2, _, y2 = class_case(K2)
        calls.clear()
        pair = M.TverskyLoss(0.3, 0.7, ignore_channels=[0]) + M.CrossEntropyLoss()
        v2, g2 = run_class(pair, x2, y2.to(DEV))
        assert len(calls) == 1 and math.isfinite(float(v2)) and float(g2.abs().max()) > 0


def test_new_losses_do_not_wait_for_the_device(ops):
    """Forward and backward of every new class issue launches only (torch's sync debug mode on 'error')."""
    from cmunet_amd import metrics as M
    K = 3
    x, lab, y = class_case(K)
    yd, ld = y.to(DEV), lab.to(DEV)
    crits = [(M.FocalLoss(gamma=1.5, alpha=torch.tensor(WEIGHTS[:K])).to(DEV), ld), (M.TverskyLoss(0.3, 0.7, 0.75), yd), (M.BoundaryLoss(), yd),
             (M.HausdorffDTLoss(), yd)]
    xd = x.to(DEV).requires_grad_(True)

    def go():
        M.clear_seg_cache()
        vals = [c(xd, t) for c, t in crits]
        torch.stack(vals).sum().backward()
        return vals

    go()                                                  # first use: library load, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        vals = go()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(torch.stack(vals)).all()) and float(xd.grad.abs().max()) > 0
