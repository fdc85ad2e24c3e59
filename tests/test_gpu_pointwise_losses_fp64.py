"""The element-wise losses (cmu_pointwise_loss_fwd / _bwd) and the class-index cross entropy (cmu_index_ce_fwd / _bwd) of
csrc/pointwise_loss.hip, and the six classes of cmunet_amd/metrics.py on top of them, against float64 on the CPU from the same fp32
inputs: tests/pointwise_loss_ref.py (which tests/test_cpu_pointwise_losses.py holds to torch.nn in float64) at the ops level, the
installed torch.nn losses and their autograd in float64 at the class level.

Bounds, with U = 2^-24 and the project's constant C_GRAD = 16 (tests/test_gpu_seg_criterion_fp64.py):

* a sum S = sum w term: 16 U sum |w term|.  The kernels take one fp32 transcendental per term (logf, log1pf or log1pf(expf): a few
  ulp RELATIVE, also where the result is tiny) and combine and accumulate in fp64, so the error of every term is a few U of itself.
  table[1] of the index CE is a sum of the fp32 weights in fp64: 2 U of the value.
* a gradient element: |dx - fp64| <= 16 U magnitude + 2^-150, the magnitude built from the sizes of the terms entering it:
    l1               |g w| [x != y]                  (exact up to the product g w; exactly 0 at ties)
    mse              |g w| 2 (|x| + |y|)             (x - y in fp64: exact)
    bce              |g w| (|x| + |y|) / max(x (1 - x), 1e-12)
    bce_with_logits  |g w| (|1 - y| + c sigmoid(-x)), c = 1 + (pw - 1) y: sigmoid(-|x|) is an fp32 exp, add and division (4 U)
    index CE         |g0| w_t (p_j + [j == t]) + |g2| (p_j sum_kept w_c + [j kept] w_j); p_j: an fp32 exp, a sum of K <= 8 terms
                     and a division (under 12 U); log-probability input: |g0| w_t [j == t] + |g2| [j kept] w_j
  plus the rounding of the result to fp32 (U of it, inside the 16).  2^-150 is half the smallest positive fp32 number: the output
  is fp32, and g w dterm of a saturated logit against its own label (x = 100, y = 1: 3.7e-44 g w) lies below the fp32 range.
* a class value: the same 16 U carried through torch's reduction of the sums.

The worst error / bound ratio seen per kind is printed, and written to the file named by CMU_PWL_PARITY_OUT when that is set
(profiles/pointwise_loss_parity.txt holds one such run)."""
import functools
import itertools
import math
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pointwise_loss_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_GRAD = 16
TINY = 2.0 ** -150
DEV = "cuda"
RATIOS = {}
WEIGHTS = [0.5, 2.0, 1.25, 0.75, 1.5, 1.0, 3.0, 0.25]
POS_WEIGHTS = [3.0, 0.25, 1.0, 2.0, 0.5, 1.5, 4.0, 0.75]


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), ratio)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    yield o
    lines = [f"{k}: worst |dx - fp64| / bound = {r:.4f}" for k, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    out = os.environ.get("CMU_PWL_PARITY_OUT")
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tests/test_gpu_pointwise_losses_fp64.py: worst per-element error of cmu_pointwise_loss_bwd / cmu_index_ce_bwd against\n"
                    f"# float64, as a fraction of the bound {C_GRAD} U magnitude + 2^-150; worst over the {len(PW_CASES)} element-wise and\n"
                    f"# {len(ICE_CASES)} class-index cases of the test\n")
            f.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------------------------------
# (a) element-wise family at the ops level
# ---------------------------------------------------------------------------------------------------
# The grid is capped at 1,024 blocks of 256 lanes; a lane takes 4 elements when inner % 4 == 0 and the pointers are 16-byte aligned,
# else 1, so a lane runs its grid-stride loop a second time past 1,048,576 / 262,144 elements:
#   odd            (2,C,9,13)     inner = 117: the scalar path (a 4-vector would straddle a channel plane)
#   vec            (3,C,64,64)    inner = 4,096: the 4-element path
#   offset         (3,2,8,8)      inner = 64 but x starts one element past a 16-byte boundary: the scalar path
#   vec_stride     (5,1,464,464)  1,076,480 elements = 269,120 groups of 4: 1,052 blocks' worth
#   scalar_stride  (5,1,257,257)  330,245 elements: 1,291 blocks' worth
PW_SHAPES = {"odd": (2, None, 9, 13), "vec": (3, None, 64, 64), "offset": (3, 2, 8, 8), "vec_stride": (5, 1, 464, 464),
             "scalar_stride": (5, 1, 257, 257)}
PW_CASES = ([(k, s, C, t) for k in R.KINDS for s in ("odd", "vec") for C in (1, 2, 3, 8) for t in ("f32", "f64")]
            + [(k, "offset", 2, "f64") for k in R.KINDS]
            + [(k, s, 1, t) for k in R.KINDS for s, t in (("vec_stride", "f32"), ("scalar_stride", "f64"))])


def test_stride_cases_pass_their_grid_cap():
    """The arithmetic behind the *_stride cases (a guard on the case tables, not on the library): more groups than 1,024 blocks of
    256 lanes on the path each one takes -- 4 elements / pixels per lane (2 pixels at K > 4), 1 when the plane is no multiple."""
    for _, s, C, _ in PW_CASES:
        B, _, H, W = PW_SHAPES[s]
        V = 4 if (H * W) % 4 == 0 else 1
        if s.endswith("_stride"):
            assert B * C * H * W // V > 1024 * 256 and V == {"vec_stride": 4, "scalar_stride": 1}[s]
    for K, s, *_ in ICE_CASES:
        B, H, W = ICE_SHAPES[s]
        V = 1 if (H * W) % (2 if K > 4 else 4) else (2 if K > 4 else 4)
        if s.endswith("_stride"):
            assert B * H * W // V > 1024 * 256 and V == {"vec4_stride": 4, "vec2_stride": 2, "scalar_stride": 1}[s]


@functools.lru_cache(maxsize=None)
def pw_case(kind, shape, C, ydt):
    """Seeded inputs with the values that break naive forms at the head of the tensor: logits 0, +-30, +-100 against labels 0 / 1 /
    0.3; probabilities exactly 0 and 1 against targets 0, 1 and 0.3 (the -100 clamp and the 1e-12 clamp); exact ties for L1 / MSE."""
    B, _, H, W = PW_SHAPES[shape]
    C = PW_SHAPES[shape][1] or C
    ydt = torch.float32 if ydt == "f32" else torch.float64
    g = torch.Generator().manual_seed(len(kind) * 1000 + H * 10 + C)
    s = (B, C, H, W)
    if kind == "bce":
        x, y = torch.rand(s, generator=g), torch.rand(s, generator=g, dtype=ydt)
        x.view(-1)[:6] = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
        y.view(-1)[:6] = torch.tensor([0.0, 1.0, 0.3, 0.0, 1.0, 0.3], dtype=ydt)
    elif kind == "bce_with_logits":
        x = torch.randn(s, generator=g) * 3
        y = (torch.rand(s, generator=g) > 0.5).to(ydt)
        y.view(-1)[15:40] = torch.rand(25, generator=g, dtype=ydt)
        x.view(-1)[:15] = torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0] * 3)
        y.view(-1)[:15] = torch.tensor([0.0] * 5 + [1.0] * 5 + [0.3] * 5, dtype=ydt)
    else:
        x, y = torch.randn(s, generator=g), torch.randn(s, generator=g, dtype=ydt)
        ties = torch.rand(s, generator=g) < 0.05
        y = torch.where(ties, x.to(ydt), y)
    weighted = C > 1 or shape == "vec"                                  # (C = 1 and weights: a one-element vector)
    w = torch.tensor(WEIGHTS[:C]) if weighted else None
    pw = torch.tensor(POS_WEIGHTS[:C]) if weighted and kind == "bce_with_logits" else None
    return x.contiguous(), y.contiguous(), w, pw


def dev_x(x, offset):
    """x on the device; ``offset``: starting one element past an allocation's (16-byte aligned) start."""
    if not offset:
        return x.to(DEV)
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
    buf[1:].copy_(x.reshape(-1))
    v = buf[1:].view(x.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def run_pw(ops, kind, xd, yd, wd, pwd, g):
    from cmunet_amd import _lib
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.lib().cmu_pointwise_loss_ws_bytes(), dtype=torch.uint8, device=DEV)
    ops.pointwise_loss_fwd(kind, xd, yd, wd, pwd, out, ws)
    dx = torch.full(xd.shape, 7.0, device=DEV)
    ops.pointwise_loss_bwd(kind, xd, yd, wd, pwd, None if g is None else torch.tensor([g], dtype=torch.float64, device=DEV), dx)
    return out.cpu()[0], dx.cpu()


@pytest.mark.parametrize("kind,shape,C,ydt", PW_CASES)
def test_pointwise_ops(ops, kind, shape, C, ydt):
    x, y, w, pw = pw_case(kind, shape, C, ydt)
    g = 0.37 / x.numel()
    r = R.pointwise_ref(kind, x, y, w, pw, g)
    xd, yd = dev_x(x, shape == "offset"), y.to(DEV)
    wd, pwd = (None if v is None else v.to(DEV) for v in (w, pw))
    S, dx = run_pw(ops, kind, xd, yd, wd, pwd, g)
    s_ratio = abs(float(S) - float(r["S"])) / (C_GRAD * U * float(r["S_mag"]))
    bound = C_GRAD * U * r["dx_mag"] + TINY
    err = (dx.double() - r["dx"]).abs()
    ratio = float((err / bound).max())
    note(kind, ratio)
    print(f"{kind} {shape} C={C} {ydt}: S {float(S):.12g} ref {float(r['S']):.12g} err/bound {s_ratio:.3g}; dx worst err/bound {ratio:.4f}")
    assert math.isfinite(float(S)) and s_ratio <= 1.0
    assert bool(torch.isfinite(dx).all()) and bool((err <= bound).all())
    if kind == "l1":
        assert bool((dx[x.double() == y.double()] == 0).all())
    # the same bits on a second call (fixed-order sums, no floating-point atomics)
    S2, dx2 = run_pw(ops, kind, xd, yd, wd, pwd, g)
    assert torch.equal(S2, S) and torch.equal(dx2, dx)
    if shape == "offset":
        # element by element the scalar path computes what the vector path does: the aligned tensor gives the same dx
        S3, dx3 = run_pw(ops, kind, x.to(DEV), yd, wd, pwd, g)
        assert torch.equal(dx3, dx) and abs(float(S3) - float(S)) <= 2 * C_GRAD * U * float(r["S_mag"])
    if shape == "vec" and C == 2:
        # NULL upstream gradient stands for zero
        assert bool((run_pw(ops, kind, xd, yd, wd, pwd, None)[1] == 0).all())


def test_bce_outside_the_unit_interval_is_nan_not_an_error(ops):
    x, y, _, _ = pw_case("bce", "odd", 2, "f64")
    x = x.clone()
    x.view(-1)[7] = 1.5
    S, dx = run_pw(ops, "bce", x.to(DEV), y.to(DEV), None, None, 1.0)
    assert math.isnan(float(S)) and int(torch.isnan(dx).sum()) == 0


def test_ops_refuse_bad_arguments(ops):
    from cmunet_amd import _lib
    x = torch.zeros(2, 9, 4, 4, device=DEV)
    out, ws = torch.empty(1, dtype=torch.float64, device=DEV), torch.empty(_lib.lib().cmu_pointwise_loss_ws_bytes(), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.CmuError, match="1 <= C <= 8"):
        _lib.call("cmu_pointwise_loss_fwd", 0, ops._p(x), ops._p(x), 0, None, None, ops._p(out), 2, 9, 16, ops._p(ws), ops._stream())
    with pytest.raises(_lib.CmuError, match="unknown kind"):
        _lib.call("cmu_pointwise_loss_fwd", 4, ops._p(x), ops._p(x), 0, None, None, ops._p(out), 1, 1, 288, ops._p(ws), ops._stream())
    with pytest.raises(_lib.CmuError, match="BCE_WITH_LOGITS only"):
        _lib.call("cmu_pointwise_loss_bwd", 2, ops._p(x), ops._p(x), 0, None, ops._p(x), None, ops._p(x), 2, 8, 18, ops._stream())
    lab = torch.zeros(2, 4, 4, dtype=torch.int64, device=DEV)
    t3, ws3 = torch.empty(3, dtype=torch.float64, device=DEV), torch.empty(_lib.lib().cmu_index_ce_ws_bytes(), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.CmuError, match="2 <= K <= 8"):
        _lib.call("cmu_index_ce_fwd", ops._p(x), ops._p(lab), 0, 0, 1, None, -100, ops._p(t3), 2, 9, 4, 4, ops._p(ws3), ops._stream())
    with pytest.raises(_lib.CmuError, match="keep_mask"):
        _lib.call("cmu_index_ce_fwd", ops._p(x), ops._p(lab), 0, 0, 1 << 3, None, -100, ops._p(t3), 2, 3, 4, 4, ops._p(ws3), ops._stream())
    with pytest.raises(_lib.CmuError, match="unknown target kind"):
        _lib.call("cmu_index_ce_bwd", ops._p(x), ops._p(lab), 7, 0, 7, None, -100, None, ops._p(x), 2, 3, 4, 4, ops._stream())


# ---------------------------------------------------------------------------------------------------
# (b) class-index cross entropy at the ops level
# ---------------------------------------------------------------------------------------------------
# Pixels per lane: 4 at K <= 4, 2 above, 1 when H*W is no multiple of that (or a pointer is not 16-byte aligned); past the block cap:
#   vec4_stride    (5,3,464,464)  1,076,480 pixels = 269,120 groups: 1,052 blocks' worth
#   vec2_stride    (5,8,328,328)  537,920 pixels = 268,960 groups: 1,051 blocks' worth
#   scalar_stride  (5,3,257,257)  330,245 pixels: 1,291 blocks' worth
ICE_SHAPES = {"odd": (2, 9, 13), "vec": (3, 64, 64), "offset": (3, 8, 8), "vec4_stride": (5, 464, 464), "vec2_stride": (5, 328, 328),
              "scalar_stride": (5, 257, 257)}
LABEL_DT = {"i64": torch.int64, "i32": torch.int32, "u8": torch.uint8, "f32": torch.float32, "f64": torch.float64}
# (K, shape, target, log_input, keep): target = a label dtype, or "oh32" / "oh64" (one-hot planes, arg-max over ``keep``)
ICE_CASES = ([(K, s, t, False, None) for K in (2, 3, 5, 8) for s in ("odd", "vec") for t in LABEL_DT]
             + [(3, "odd", "oh64", False, (1, 2)), (4, "vec", "oh32", False, None), (8, "vec", "oh64", False, (1, 2, 3, 4, 5, 6, 7)),
                (2, "odd", "oh32", True, (1,)), (4, "vec", "oh64", True, (1, 2, 3)), (5, "odd", "i64", True, None), (3, "vec", "u8", True, None),
                (3, "offset", "i64", False, None), (8, "offset", "oh64", False, None),
                (3, "vec4_stride", "u8", False, None), (8, "vec2_stride", "i64", False, None), (3, "scalar_stride", "oh32", False, (0, 2)),
                (2, "vec4_stride", "i64", True, None)])


@functools.lru_cache(maxsize=None)
def ice_case(K, shape, target, log_input, keep):
    """Logits randn * 2 (log-probabilities of them for ``log_input``); about 10 % of the label pixels ignored (-100; 250 for uint8
    labels, which cannot hold -100); floating-point labels carry a fraction (k + 0.5 truncates to k).  One-hot targets: the planes
    of random labels, so with ignored channels some pixels have all-zero kept channels (arg-max: the first kept channel)."""
    B, H, W = ICE_SHAPES[shape]
    g = torch.Generator().manual_seed(K * 100 + H + len(target))
    x = torch.randn(B, K, H, W, generator=g) * 2
    if log_input:
        x = torch.log_softmax(x.double(), 1).float()
    lab = torch.randint(0, K, (B, H, W), generator=g)
    if target.startswith("oh"):
        tgt = F.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().to(torch.float32 if target == "oh32" else torch.float64)
        labels, ign = R.labels_of(tgt, True, keep), -100
        if keep is not None and len(keep) < K:
            assert bool((tgt[:, list(keep)].sum(1) == 0).any())
    else:
        ign = 250 if target == "u8" else -100
        lab[torch.rand(B, H, W, generator=g) < 0.1] = ign
        tgt = lab.to(LABEL_DT[target])
        if tgt.is_floating_point():
            tgt = torch.where(tgt >= 0, tgt + 0.5, tgt)
        labels = R.labels_of(tgt)
        assert torch.equal(labels, lab)
    return x.contiguous(), tgt.contiguous(), labels, ign


def run_ice(ops, x, tgt, onehot, log_input, keep, w, ign, g):
    from cmunet_amd import _lib
    table = torch.empty(3, dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.lib().cmu_index_ce_ws_bytes(), dtype=torch.uint8, device=DEV)
    ops.index_ce_fwd(x, tgt, onehot, log_input, keep, w, ign, table, ws)
    dx = torch.full(x.shape, 7.0, device=DEV)
    ops.index_ce_bwd(x, tgt, onehot, log_input, keep, w, ign, None if g is None else torch.tensor(g, dtype=torch.float64, device=DEV), dx)
    return table.cpu(), dx.cpu()


def check_table(T, r, what):
    for i, k in ((0, C_GRAD), (1, 2), (2, C_GRAD)):
        ratio = abs(float(T[i]) - float(r["T"][i])) / max(k * U * float(r["T_mag"][i]), 1e-300)
        print(f"{what}: T{i} {float(T[i]):.12g} ref {float(r['T'][i]):.12g} err/bound {ratio:.3g}")
        assert math.isfinite(float(T[i])) and ratio <= 1.0, (what, i)


@pytest.mark.parametrize("K,shape,target,log_input,keep", ICE_CASES)
def test_index_ce_ops(ops, K, shape, target, log_input, keep):
    x, tgt, labels, ign = ice_case(K, shape, target, log_input, keep)
    onehot = target.startswith("oh")
    npix = labels.numel()
    xd, td = dev_x(x, shape == "offset"), tgt.to(DEV)
    keep_l = None if keep is None else list(keep)
    for w in (None, torch.tensor(WEIGHTS[:K])):
        g = (0.37 / npix, 0.011 / npix)
        r = R.index_ce_ref(x, labels, w, ign, log_input, keep_l, *g)
        T, dx = run_ice(ops, xd, td, onehot, log_input, keep_l, None if w is None else w.to(DEV), ign, g)
        what = f"K={K} {shape} {target} log_input={log_input} keep={keep} w={'yes' if w is not None else 'no'}"
        check_table(T, r, what)
        bound = C_GRAD * U * r["dx_mag"] + TINY
        err = (dx.double() - r["dx"]).abs()
        ratio = float((err / bound).max())
        note("index_ce" + ("_log_input" if log_input else ""), ratio)
        print(f"{what}: dx worst err/bound {ratio:.4f}")
        assert bool((err <= bound).all())
        assert bool((dx[(labels == ign).unsqueeze(1).expand_as(dx)] == 0).all())
        if log_input and keep is not None:
            assert bool((dx[:, [c for c in range(K) if c not in keep]] == 0).all())
    T2, dx2 = run_ice(ops, xd, td, onehot, log_input, keep_l, w.to(DEV), ign, g)
    assert torch.equal(T2, T) and torch.equal(dx2, dx)
    if shape == "offset":
        T3, dx3 = run_ice(ops, x.to(DEV), td, onehot, log_input, keep_l, w.to(DEV), ign, g)
        assert torch.equal(dx3, dx)
    if shape == "vec" and K == 3:
        assert bool((run_ice(ops, xd, td, onehot, log_input, keep_l, None, ign, None)[1] == 0).all())


def test_out_of_range_label_is_nan_and_never_an_index(ops):
    """One pixel labelled K (one past the end) on a tiny tensor, class weights given: NaN loss, a zero gradient at that pixel, the
    other pixels' gradients as if it were not there."""
    K = 3
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, K, 4, 4, generator=g) * 2
    lab = torch.randint(0, K, (1, 4, 4), generator=g)
    lab[0, 1, 2] = K
    w = torch.tensor(WEIGHTS[:K])
    gg = (0.4, 0.1)
    r = R.index_ce_ref(x, lab, w, -100, False, None, *gg)
    T, dx = run_ice(ops, x.to(DEV), lab.to(DEV), False, False, None, w.to(DEV), -100, gg)
    assert math.isnan(float(T[0])) and math.isnan(float(r["T"][0]))
    assert abs(float(T[1]) - float(r["T"][1])) <= 2 * U * float(r["T_mag"][1]) and abs(float(T[2]) - float(r["T"][2])) <= C_GRAD * U * float(r["T_mag"][2])
    assert bool((dx[0, :, 1, 2] == 0).all()) and bool(torch.isfinite(dx).all())
    assert bool(((dx.double() - r["dx"]).abs() <= C_GRAD * U * r["dx_mag"] + TINY).all())
    assert float(dx.abs().sum()) > 0
    from cmunet_amd import metrics as M
    v = M.RobustCrossEntropyLoss(weight=w)(x.to(DEV).requires_grad_(True), lab.to(DEV))
    assert math.isnan(float(v))


# ---------------------------------------------------------------------------------------------------
# the classes: values and autograd against the installed torch.nn in float64
# ---------------------------------------------------------------------------------------------------
def class_pair(kind, C, red, weighted):
    from cmunet_amd import metrics as M
    w = torch.tensor(WEIGHTS[:C]).view(C, 1, 1) if weighted else None
    pw = torch.tensor(POS_WEIGHTS[:C]).view(1, C, 1, 1) if weighted else None
    wd, pwd = (None if v is None else v.double() for v in (w, pw))
    if kind == "l1":
        return M.L1Loss(reduction=red), nn.L1Loss(reduction=red), None, None
    if kind == "mse":
        return M.MSELoss(reduction=red), nn.MSELoss(reduction=red), None, None
    if kind == "bce":
        return M.BCELoss(weight=w, reduction=red), nn.BCELoss(weight=wd, reduction=red), w, None
    return M.BCEWithLogitsLoss(weight=w, reduction=red, pos_weight=pw), nn.BCEWithLogitsLoss(weight=wd, reduction=red, pos_weight=pwd), w, pw


@pytest.mark.parametrize("kind,red,weighted", [(k, r, wt) for k in R.KINDS for r, wt in (("mean", False), ("sum", True))])
def test_pointwise_classes_against_torch_fp64(ops, kind, red, weighted):
    """0.37 * loss + another loss of the same prediction, then .backward(): value and gradient against torch.nn in float64."""
    from cmunet_amd import metrics as M
    C = 3
    x, y, _, _ = pw_case(kind, "odd", C, "f64")
    y2 = torch.randn(x.shape, generator=torch.Generator().manual_seed(9))
    crit, ref, w, pw = class_pair(kind, C, red, weighted)
    crit = crit.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    v = 0.37 * crit(xd, y.to(DEV)) + M.MSELoss()(xd, y2.to(DEV))
    assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda
    v.backward()
    x64 = x.double().requires_grad_(True)
    want = 0.37 * ref(x64, y.double()) + nn.MSELoss()(x64, y2.double())
    want.backward()
    n = x.numel() if red == "mean" else 1
    fw = None if w is None else w.reshape(-1)
    fpw = None if pw is None else pw.reshape(-1)
    r1, r2 = R.pointwise_ref(kind, x, y, fw, fpw, 0.37 / n), R.pointwise_ref("mse", x, y2, None, None, 1.0 / x.numel())
    vb = C_GRAD * U * (0.37 * float(r1["S_mag"]) / n + float(r2["S_mag"]) / x.numel())
    print(f"{kind} {red}: value {float(v):.12g} ref {float(want):.12g} err/bound {abs(float(v) - float(want)) / vb:.3g}")
    assert abs(float(v) - float(want)) <= vb
    bound = C_GRAD * U * (r1["dx_mag"] + r2["dx_mag"]) + 2 * TINY
    err = (xd.grad.cpu().double() - x64.grad).abs()
    note(kind, float((err / bound).max()))
    assert xd.grad.dtype == torch.float32 and bool((err <= bound).all()), float((err / bound).max())
    # the same bits on a second evaluation
    g1 = xd.grad.clone()
    xd.grad = None
    v2 = 0.37 * crit(xd, y.to(DEV)) + M.MSELoss()(xd, y2.to(DEV))
    v2.backward()
    assert torch.equal(v2.detach(), v.detach()) and torch.equal(xd.grad, g1)


def test_bce_classes_take_any_shape_without_weights_and_one_element_weights(ops):
    from cmunet_amd import metrics as M
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(7, 11, generator=g), torch.rand(7, 11, generator=g)
    for crit, ref in ((M.BCEWithLogitsLoss(), nn.BCEWithLogitsLoss()), (M.BCEWithLogitsLoss(weight=torch.tensor([2.0]), pos_weight=torch.tensor(3.0)),
                                                                      nn.BCEWithLogitsLoss(weight=torch.tensor([2.0]).double(), pos_weight=torch.tensor(3.0).double())),
                      (M.L1Loss(), nn.L1Loss())):
        v = crit.to(DEV)(x.to(DEV), y.to(DEV))
        want = ref(x.double(), y.double())
        assert abs(float(v) - float(want)) <= C_GRAD * U * abs(float(want))             # (every term is non-negative)
    with pytest.raises(ValueError):
        M.BCELoss(weight=torch.ones(3, 1, 1))(torch.rand(2, 2, 4, 4, device=DEV), torch.rand(2, 2, 4, 4, device=DEV))
    with pytest.raises(ValueError):
        M.L1Loss()(torch.rand(2, 2, device=DEV), torch.rand(2, 3, device=DEV))


@pytest.mark.parametrize("eps,weighted,red,target", [(e, wt, r, t) for e in (0.0, 0.1) for wt in (False, True)
                                                      for r, t in (("mean", "i64"), ("sum", "u8"), ("mean", "f32"))])
def test_robust_cross_entropy_against_torch_fp64(ops, eps, weighted, red, target):
    from cmunet_amd import metrics as M
    K = 3
    x, tgt, labels, ign = ice_case(K, "odd", target, False, None)
    w = torch.tensor(WEIGHTS[:K]) if weighted else None
    crit = M.RobustCrossEntropyLoss(weight=w, ignore_index=ign, reduction=red, label_smoothing=eps).to(DEV)
    ref = nn.CrossEntropyLoss(weight=None if w is None else w.double(), ignore_index=ign, reduction=red, label_smoothing=eps)
    xd = x.to(DEV).requires_grad_(True)
    other = M.NLLLoss(activation="logsoftmax")
    y1h = F.one_hot(torch.randint(0, K, labels.shape, generator=torch.Generator().manual_seed(1)), K).permute(0, 3, 1, 2).double()
    # (B,1,H,W) targets, as the reference's compatibility layer takes them
    v = 0.37 * crit(xd, tgt.unsqueeze(1).to(DEV)) + other(xd, y1h.to(DEV))
    assert v.dtype == torch.float64 and v.dim() == 0
    v.backward()
    x64 = x.double().requires_grad_(True)
    want = 0.37 * ref(x64, labels) + nn.NLLLoss()(torch.log_softmax(x64, 1), torch.argmax(y1h, 1))
    want.backward()
    r0 = R.index_ce_ref(x, labels, w, ign)
    T1 = float(r0["T"][1]) if red == "mean" else 1.0
    g0, g2 = 0.37 * (1 - eps) / T1, 0.37 * (eps / K) / T1
    r1 = R.index_ce_ref(x, labels, w, ign, False, None, g0, g2)
    npix = labels.numel()
    r2 = R.index_ce_ref(x, torch.argmax(y1h, 1), None, -100, False, None, 1.0 / npix, 0.0)
    vb = C_GRAD * U * (0.37 * float(R.reduce_ce(r0["T_mag"], K, red, eps)) + float(r2["T_mag"][0]) / npix)
    print(f"eps={eps} weighted={weighted} {red} {target}: value {float(v):.12g} ref {float(want):.12g} err/bound {abs(float(v) - float(want)) / vb:.3g}")
    assert abs(float(v) - float(want)) <= vb
    bound = C_GRAD * U * (r1["dx_mag"] + r2["dx_mag"]) + 2 * TINY
    err = (xd.grad.cpu().double() - x64.grad).abs()
    note("robust_cross_entropy_loss", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    g1 = xd.grad.clone()
    xd.grad = None
    (0.37 * crit(xd, tgt.to(DEV)) + other(xd, y1h.to(DEV))).backward()          # (B,H,W) targets: the same bits
    assert torch.equal(xd.grad, g1)


def test_all_pixels_ignored_is_nan_as_in_torch(ops):
    from cmunet_amd import metrics as M
    x = torch.randn(2, 3, 9, 13)
    lab = torch.full((2, 9, 13), -100, dtype=torch.int64)
    xd = x.to(DEV).requires_grad_(True)
    v = M.RobustCrossEntropyLoss()(xd, lab.to(DEV))
    assert math.isnan(float(v)) and math.isnan(float(nn.CrossEntropyLoss()(x.double(), lab)))
    assert float(M.RobustCrossEntropyLoss(reduction="sum")(xd, lab.to(DEV))) == 0.0


@pytest.mark.parametrize("activation,ign", [("logsoftmax", None), ("logsoftmax", [0]), (None, [0]), ("identity", None)])
def test_nll_loss_against_the_reference_composition(ops, activation, ign):
    """metrics.py:523-543 with torch.nn in float64; ignore_channels=[0] leaves pixels whose kept target channels are all zero."""
    from cmunet_amd import metrics as M
    K = 4
    keep = tuple(c for c in range(K) if c not in (ign or []))
    x, tgt, labels, _ = ice_case(K, "odd", "oh64", activation != "logsoftmax", keep if ign else None)
    crit = M.NLLLoss(activation=activation, ignore_channels=ign, threshold=0.5)
    xd = x.to(DEV).requires_grad_(True)
    v = crit(xd, tgt.to(DEV))
    (0.37 * v).backward()
    x64 = x.double().requires_grad_(True)
    pr = torch.log_softmax(x64, 1) if activation == "logsoftmax" else x64
    want = nn.NLLLoss()(pr[:, list(keep)], torch.argmax(tgt[:, list(keep)], dim=1))
    (0.37 * want).backward()
    npix = labels.numel()
    r = R.index_ce_ref(x, labels, None, -100, activation != "logsoftmax", list(keep), 0.37 / npix, 0.0)
    assert v.dtype == torch.float64 and v.dim() == 0
    assert abs(float(v) - float(want)) <= C_GRAD * U * float(r["T_mag"][0]) / npix
    bound = C_GRAD * U * r["dx_mag"] + TINY
    err = (xd.grad.cpu().double() - x64.grad).abs()
    note("nll_loss", float((err / bound).max()))
    assert bool((err <= bound).all())
    with pytest.raises(NotImplementedError):
        crit(torch.zeros(2, K, 4, device=DEV), torch.zeros(2, K, 4, device=DEV))


@pytest.mark.parametrize("second", ["bce_with_logits", "nll"])
def test_dice_plus_new_loss_on_one_hot_targets(ops, second):
    """DiceLoss(softmax, threshold=None) + BCEWithLogitsLoss() / + NLLLoss('logsoftmax') on one-hot targets: the summed logit
    gradient within the sum of the two bounds of float64 autograd (the Dice bound: tests/test_gpu_seg_criterion_fp64.py)."""
    import test_gpu_seg_criterion_fp64 as SC
    from oracle import losses as OL
    from cmunet_amd import metrics as M
    K = 3
    c = SC.make_case(K, "vec", "onehot64")
    new = M.BCEWithLogitsLoss() if second == "bce_with_logits" else M.NLLLoss(activation="logsoftmax")
    crit = M.DiceLoss(activation="softmax", threshold=None) + new
    assert crit.__name__ == "dice_loss + " + new.__name__
    M.clear_seg_cache()
    lo, y = c.logits.to(DEV).requires_grad_(True), c.y_dev.to(DEV)
    v = crit(lo, y)
    v.backward()
    l64 = c.L.clone().requires_grad_(True)
    if second == "bce_with_logits":
        want2 = nn.BCEWithLogitsLoss()(l64, c.y)
        r2 = R.pointwise_ref("bce_with_logits", c.logits, c.y_dev, None, None, 1.0 / c.logits.numel())
        v2b = float(r2["S_mag"]) / c.logits.numel()
    else:
        want2 = nn.NLLLoss()(torch.log_softmax(l64, 1), torch.argmax(c.y, 1))
        r2 = R.index_ce_ref(c.logits, R.labels_of(c.y_dev, True), None, -100, False, None, 1.0 / c.npix, 0.0)
        v2b = float(r2["T_mag"][0]) / c.npix
    want = OL.dice_loss(l64, c.y, eps=1e-5, beta=1.0, threshold=None, ignore_channels=None) + want2
    want.backward()
    assert abs(float(v) - float(want)) <= 32 * U + C_GRAD * U * v2b             # Dice: 1 - N / D with counters within 16 U
    g_tp, g_spr = SC.soft_grads(c, 1.0, 0.0, None, 1.0, 1e-5)
    bound = SC.grad_bound(c, 0.0, g_tp, g_spr, torch.ones(K, dtype=torch.float64)) + C_GRAD * U * r2["dx_mag"] + TINY
    err = (lo.grad.cpu().double() - l64.grad).abs()
    print(f"dice + {second}: worst err / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())


def test_new_losses_do_not_wait_for_the_device(ops):
    """Forward and backward of every new class issue launches only (torch's sync debug mode on 'error')."""
    from cmunet_amd import metrics as M
    K = 3
    x, tgt, labels, ign = ice_case(K, "odd", "i64", False, None)
    y1h = F.one_hot(labels.clamp_min(0), K).permute(0, 3, 1, 2).double().to(DEV)
    prob = torch.rand(x.shape).to(DEV)
    w3 = torch.tensor(WEIGHTS[:K])
    crits = [(M.L1Loss(), y1h), (M.MSELoss(reduction="sum"), y1h), (M.BCEWithLogitsLoss(weight=w3.view(K, 1, 1), pos_weight=w3.view(1, K, 1, 1)).to(DEV), y1h),
             (M.NLLLoss(activation="logsoftmax", ignore_channels=[0]), y1h),
             (M.RobustCrossEntropyLoss(weight=w3, label_smoothing=0.1).to(DEV), tgt.to(DEV))]
    xd = x.to(DEV).requires_grad_(True)
    pd = prob.clone().requires_grad_(True)
    bce = M.BCELoss(weight=torch.tensor([2.0])).to(DEV)

    def go():
        vals = [c(xd, t) for c, t in crits] + [bce(pd, y1h)]
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


# ---------------------------------------------------------------------------------------------------
# end to end: a one-channel binary head
# ---------------------------------------------------------------------------------------------------
def binary_batch(seed, B=2, S=32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, S, generator=g)
    y = (F.avg_pool2d(x.unsqueeze(1), 3, 1, 1) > 0).double()          # (B,1,S,S): a target the network can learn
    return x, y


def test_one_channel_unet_with_bce_with_logits(ops):
    from cmunet_amd import metrics as M, model as Mod
    torch.manual_seed(7)
    net = Mod.UNet(out_classes=1, base_ch=16, depth=3, dtype="f32").cuda().train()
    x, y = binary_batch(1)
    logits = net(x.cuda())
    assert logits.shape == (2, 1, 32, 32) and logits.dtype == torch.float32
    logits.retain_grad()
    loss = M.BCEWithLogitsLoss()(logits, y.cuda())
    loss.backward()
    lg = logits.detach().cpu()
    l64 = lg.double().requires_grad_(True)
    want = nn.BCEWithLogitsLoss()(l64, y)
    want.backward()
    r = R.pointwise_ref("bce_with_logits", lg, y, None, None, 1.0 / lg.numel())
    assert abs(float(loss) - float(want)) <= C_GRAD * U * float(r["S_mag"]) / lg.numel()
    err = (logits.grad.cpu().double() - l64.grad).abs()
    assert bool((err <= C_GRAD * U * r["dx_mag"] + TINY).all())
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)


def test_train_epochs_with_a_one_channel_head(ops):
    from cmunet_amd import metrics as M, model as Mod, train as T
    torch.manual_seed(11)
    net = Mod.UNet(out_classes=1, base_ch=16, depth=3, dtype="f32")
    loader = [binary_batch(s) for s in (21, 22, 23, 24)]
    opt = torch.optim.Adam(net.parameters(), lr=3e-3)
    tr = T.TrainEpoch(net, loss=M.BCEWithLogitsLoss(), metrics=[M.L1Loss()], optimizer=opt, device="cuda", verbose=False)
    first, second = tr.run(loader), tr.run(loader)
    for logs in (first, second):
        assert set(logs) == {"bce_with_logits_loss", "l1_loss"} and all(math.isfinite(v) for v in logs.values()), logs
    assert second["bce_with_logits_loss"] < first["bce_with_logits_loss"], (first, second)
