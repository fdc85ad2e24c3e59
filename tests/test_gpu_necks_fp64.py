"""The neck path of DESIGN 4.8 op by op: the six skinny-GEMM entries (csrc/skinny.hip fp32, csrc/necks.hip 16-bit operands), the
``cmu_bn1d_*`` kernels and ``cmu_conv1x1_nchw_fwd``, against the float64 references of tests/necks_fp64_ref.py (proved on the CPU in
tests/test_cpu_necks_ref.py).  Conventions of test_gpu_elem_fp64.py / test_gpu_heads_optim_fp64.py (U = 2^-24, ``k=`` next to each
counted bound, every comparison recorded in ``PARITY``; profiles/necks_fp64_parity.txt is that table).

  * GEMMs: no tolerance anywhere.  Integer operands in [-3, 3] are exact in f16 / bf16 and every fp32 partial sum stays below 2^24
    whatever the order, so MFMA chain, LDS fold and split-K slab must reproduce the exact product; a one-hot operand moves rows /
    columns of the other one (rounded to the operand type in the 16-bit forms).  "Equal" is value equality of finite floats: the same
    bits up to the sign of a zero.  The launch geometry (``skf_splits``, ``sk16_splits``, the per-wave row partition ``nq``) is
    restated here and every case asserts the branch it is named after.  Outputs are written between guard bands.
  * BatchNorm1d: statistics per output within k U sum |terms| (k from the row chain), then every later stage per element against
    float64 evaluated AT the fp32 values the previous stage returned.  The backward takes ``y`` as data with exact 0.0, -0.0 and
    negative entries: the gate must be ``> 0``.
  * 1x1 convolution: exact-integer data bit for bit (integer scale and shift), the input a channel slice of a wider buffer, both
    signs of ``relu_from``; one float case per storage type at the bar of test_gpu_skinny.py.
"""
import math

import numpy as np
import pytest
import torch

import necks_fp64_ref as R
from elem_fp64_ref import U, D, TORCH_DT, elem_bound, quant  # noqa: F401
from test_gpu_elem_fp64 import PARITY, bits_equal, within  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.0
NAN = float("nan")
FORMS = ["f32", "f16", "bf16"]                     # operand form of the GEMMs / storage type of the convolution
EPC = {"f32": 4, "f16": 8, "bf16": 8}
MOM = float(np.float32(0.1))
EPS = float(np.float32(1e-6))                      # the necks' SyncBN eps


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    return o


def lib():
    from cmunet_amd import _lib
    return _lib.lib()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def exact(got, ref64, what, dt):
    """got == ref64 value for value (finite floats: bit for bit up to the sign of a zero); recorded as ratio 0 in PARITY."""
    got = got.detach().cpu()
    ref = ref64.to(got.dtype)
    assert torch.equal(ref.double(), ref64.double()), f"{what}: the reference is not representable in the output type"
    key = (what.split(":")[0], dt)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ok = bool(torch.isfinite(got).all()) and torch.equal(got, ref)
    PARITY[key] = max(PARITY.get(key, 0.0), 0.0 if ok else math.inf)
    if not ok:
        bad = (got != ref) | ~torch.isfinite(got)
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what} ({dt}): {int(bad.sum())} of {ref.numel()} differ; first at flat index {i}: got "
                             f"{got.flatten()[i].item():.9g}, exact {ref.flatten()[i].item():.9g}")


# ------------------------------------------------------------------------------------------------
# the launchers' geometry, restated (skinny.hip: skf_splits, skinny_dgrad_kernel; necks.hip: sk16_splits, skinny16_dgrad_kernel)
# ------------------------------------------------------------------------------------------------
CHUNK = {"f32": 32, "f16": 64, "bf16": 64}         # k per staged chunk (SKF_KC) / per unrolled trip (16 * SK16_UNROLL)
TARGET = {"f32": 768, "f16": 2048, "bf16": 2048}   # workgroups the split count aims at


def fwd_splits(form, N, K):
    """-> (splits, k per split, k of the last split, clamped): clamped = K / target splits is below one chunk, so the split is
    lifted to one chunk and the split count falls below its target."""
    nblk = -(-N // 128)
    want = -(-TARGET[form] // nblk)
    kc = -(-K // want)
    clamped = kc < CHUNK[form]
    kc = max(-(-kc // CHUNK[form]) * CHUNK[form], CHUNK[form])
    splits = -(-K // kc)
    return splits, kc, K - (splits - 1) * kc, clamped


def fwd_kind(form, N, K):
    splits, kc, last, _ = fwd_splits(form, N, K)
    return "one" if splits == 1 else ("equal" if last == kc else "short")


def dgrad_nq(form, N):
    """Rows of w per wave of the input gradient: an even number (fp32: n pairs), whole 16-row steps (16-bit)."""
    q = (N + 3) // 4
    return ((q + 1) & ~1) if form == "f32" else -(-q // 16) * 16


# ------------------------------------------------------------------------------------------------
# the six entries, called through the C ABI with guard bands around y and dx; dw through ``out=``
# ------------------------------------------------------------------------------------------------
def guarded(n, lead):
    buf = torch.full((lead + n + lead,), SENT, device=DEV)
    buf[lead:lead + n] = NAN                                  # an element the kernel does not write stays NaN
    return buf, buf[lead:lead + n]


def guards_ok(buf, lead, n):
    return bool((buf[:lead] == SENT).all()) and bool((buf[lead + n:] == SENT).all())


def ws_bytes(n):
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=DEV)


def gemm_fwd(ops, x, w, b, form):
    M, K = x.shape
    N = w.shape[0]
    buf, y = guarded(M * N, 5)                                # y needs no alignment: an odd offset
    if form == "f32":
        assert K % 8 == 0
        ops.call("cmu_skinny_gemm_fwd", ops._p(x), ops._p(w), ops._p(b), ops._p(y), M, N, K, ops._p(ws_bytes(lib().cmu_skinny_gemm_ws_bytes(M, N, K))),
                 ops._stream())
    else:
        assert K % 16 == 0
        ops.call("cmu_skinny16_gemm_fwd", ops._p(x), ops._p(w), ops._p(b), ops._p(y), M, N, K, ops.dt_code(form),
                 ops._p(ws_bytes(lib().cmu_skinny16_gemm_ws_bytes(M, N, K))), ops._stream())
    assert guards_ok(buf, 5, M * N), "skinny_gemm_fwd wrote outside y"
    return y.view(M, N)


def gemm_dgrad(ops, dy, w, form):
    M, N = dy.shape
    K = w.shape[1]
    assert K % 4 == 0
    buf, dx = guarded(M * K, 8)                               # dx must stay 16-byte aligned
    if form == "f32":
        ops.call("cmu_skinny_gemm_dgrad", ops._p(dy), ops._p(w), ops._p(dx), M, N, K, ops._p(ws_bytes(lib().cmu_skinny_gemm_bwd_ws_bytes(M, N))), ops._stream())
    else:
        ops.call("cmu_skinny16_gemm_dgrad", ops._p(dy), ops._p(w), ops._p(dx), M, N, K, ops.dt_code(form), ops._stream())
    assert guards_ok(buf, 8, M * K), "skinny_gemm_dgrad wrote outside dx"
    return dx.view(M, K)


def gemm_wgrad(ops, dy, x, bias, form):
    N, K = dy.shape[1], x.shape[1]
    buf, dw = guarded(N * K, 4)
    dw2, db = ops.skinny_gemm_wgrad(dy, x, with_bias=bias, compute_dt=None if form == "f32" else form, out=dw.view(N, K))
    assert dw2.data_ptr() == dw.data_ptr() and guards_ok(buf, 4, N * K), "skinny_gemm_wgrad wrote outside out="
    return dw.view(N, K), db


def ints(shape, g):
    return torch.randint(-3, 4, shape, generator=g).float()


def check_int_products(ops, M, K, N, form, which="fdw"):
    """All requested products of integer operands against the exact product: f = forward (with bias), d = input gradient,
    w = weight gradient (with and without the bias sum)."""
    assert max(K, N, M) * 9 + 3 < 2 ** 24
    g = gen(M * 131 + K * 7 + N)
    x, w, b, dy = ints((M, K), g), ints((N, K), g), ints((N,), g), ints((M, N), g)
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    tag = f"M={M} K={K} N={N}"
    if "f" in which:
        exact(gemm_fwd(ops, xd, wd, bd, form), R.gemm_fwd_ref(x, w, b), f"skinny_fwd exact: y {tag}", form)
        exact(gemm_fwd(ops, xd, wd, None, form), R.gemm_fwd_ref(x, w, None), f"skinny_fwd exact: y (no bias) {tag}", form)
    if "d" in which:
        exact(gemm_dgrad(ops, dyd, wd, form), R.gemm_dgrad_ref(dy, w), f"skinny_dgrad exact: dx {tag}", form)
    if "w" in which:
        rw, rb = R.gemm_wgrad_ref(dy, x)
        dw, db = gemm_wgrad(ops, dyd, xd, True, form)
        exact(dw, rw, f"skinny_wgrad exact: dw {tag}", form)
        exact(db, rb, f"skinny_wgrad exact: db {tag}", form)
        dw, db = gemm_wgrad(ops, dyd, xd, False, form)
        assert db is None
        exact(dw, rw, f"skinny_wgrad exact: dw (no bias) {tag}", form)


KF = {"f32": 80, "f16": 80, "bf16": 80}            # small K of the M / N sweeps: a multiple of 16, more than one split with a short last one


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M", [1, 7, 31, 32, 33, 63, 64, 65, 255, 256])
def test_skinny_exact_rows_axis(ops, form, M):
    """One 32-row group (the one-group weight gradient), whole groups, and a ragged last group of the MULTI forms."""
    K, N = KF[form], 70
    assert fwd_kind(form, N, K) == "short"
    check_int_products(ops, M, K, N, form)


N_AXIS = [1, 2, 3, 5, 8, 9, 31, 32, 33, 63, 64, 65, 68, 127, 128, 129, 130]


def test_n_axis_covers_the_row_partition():
    """Pure arithmetic on the restated partition: the N sweep below holds, for each form, a partition that is exact (4 nq = N), one
    whose last wave is empty, one whose last wave is ragged, and a wave that runs more than one trip with a ragged last trip."""
    for form, trip in (("f32", 16), ("f16", 16)):
        kinds = set()
        for N in N_AXIS:
            nq = dgrad_nq(form, N)
            assert 4 * nq >= N and (nq % 2 == 0 if form == "f32" else nq % 16 == 0)
            kinds.add("exact" if 4 * nq == N else ("empty" if 3 * nq >= N else "ragged"))
            if nq > trip and nq % trip:
                kinds.add("ragged trip")
            if min(nq, N) < trip:
                kinds.add("short trip")
        want = {"exact", "empty", "ragged", "short trip"} | ({"ragged trip"} if form == "f32" else set())
        assert want <= kinds, (form, kinds)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", N_AXIS)
def test_skinny_exact_columns_axis(ops, form, N):
    """N around the 32-row MFMA tile, the 64-row tiles of the weight gradient, the 128-row workgroups of the forward, and the per-wave
    row partition of the input gradient (test_n_axis_covers_the_row_partition); two row groups, the second of one row."""
    check_int_products(ops, 33, 144, N, form)


# forward K: (M, K, N, kind, more than one chunk per split, clamped)
FWD_K = {
    "f32": [(5, 8, 70, "one", False, True), (5, 32, 70, "one", False, True), (5, 64, 70, "equal", False, True), (5, 40, 70, "short", False, True),
            (33, 4096, 70, "equal", False, True), (33, 4096, 1536, "equal", True, False), (33, 4104, 1536, "short", True, False)],
    "f16": [(5, 16, 70, "one", False, True), (5, 64, 70, "one", False, True), (5, 128, 70, "equal", False, True), (5, 80, 70, "short", False, True),
            (33, 4096, 1536, "equal", False, True), (33, 4112, 1536, "short", False, True), (5, 12288, 1536, "equal", True, False)],
}
FWD_K["bf16"] = FWD_K["f16"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(7))
def test_skinny_exact_forward_split_k(ops, form, i):
    """One split, equal splits, a short last split, the split lifted to one chunk (clamped), several chunks per split; N = 1,536
    for many splits.  K = 12,288 is what a second trip per split takes in the 16-bit form at N = 1,536."""
    M, K, N, kind, multi, clamped = FWD_K[form][i]
    splits, kc, last, cl = fwd_splits(form, N, K)
    assert fwd_kind(form, N, K) == kind and (kc > CHUNK[form]) == multi and cl == clamped, (splits, kc, last, cl)
    if N == 1536:
        assert splits >= 43
    check_int_products(ops, M, K, N, form, "f")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", [4, 124, 128, 132, 516])
def test_skinny_exact_dgrad_column_blocks(ops, form, K):
    """The 128-column workgroups of the input gradient: less than one, one short of one, one, one and a 16-byte piece, four and one."""
    check_int_products(ops, 33, K, 70, form, "d")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", [4, 128, 132, 508, 512, 516])
def test_skinny_exact_wgrad_tiles(ops, form, K):
    """The 512-column workgroups (four 128-column waves) and the 64-row blockIdx.y tiles of the weight gradient, one-group and
    MULTI form with a ragged last group, with and without the bias sum."""
    for N in (63, 64, 65):
        for M in (7, 33):
            check_int_products(ops, M, K, N, form, "w")


def round_to(t, form):
    return t if form == "f32" else quant(t, form)


@pytest.mark.parametrize("form", FORMS)
def test_skinny_one_hot_forward(ops, form):
    """x[m, k_m] = 1: y[m, :] = w[:, k_m] (rounded to the operand type).  k_m walks every residue of the staged chunk, in different
    chunks and splits, the first and the last column; 66 rows = two groups and a ragged one."""
    ch = CHUNK[form]
    K, N = 208, 70
    splits, kc, last, _ = fwd_splits(form, N, K)
    assert splits > 1 and last < kc
    ks = [K - 1, 0] + [r + ch * (r % (K // ch)) for r in range(ch)]
    ks = (ks + [K - 2 - r for r in range(66)])[:66]
    assert {k % ch for k in ks} == set(range(ch)) and max(ks) == K - 1 and all(0 <= k < K for k in ks)
    M = len(ks)
    g = gen(11)
    w = torch.randn(N, K, generator=g)
    x = torch.zeros(M, K)
    x[torch.arange(M), torch.tensor(ks)] = 1.0
    y = gemm_fwd(ops, x.to(DEV), w.to(DEV), None, form)
    exact(y, round_to(w, form)[:, ks].t().double(), "skinny_fwd one-hot: y", form)


@pytest.mark.parametrize("form", FORMS)
def test_skinny_one_hot_dgrad(ops, form):
    """dy[m, n_m] = 1: dx[m, :] = w[n_m, :].  n_m walks every row of w: every residue of a trip, both sides of each wave boundary
    of the row partition, the last row."""
    N, K = 70, 132
    M = N
    nq = dgrad_nq(form, N)
    assert nq < N < 4 * nq
    g = gen(12)
    w = torch.randn(N, K, generator=g)
    ns = [N - 1 - m for m in range(M)]
    dy = torch.zeros(M, N)
    dy[torch.arange(M), torch.tensor(ns)] = 1.0
    dx = gemm_dgrad(ops, dy.to(DEV), w.to(DEV), form)
    exact(dx, round_to(w, form)[ns].double(), "skinny_dgrad one-hot: dx", form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M", [20, 66])
def test_skinny_one_hot_wgrad(ops, form, M):
    """dy[m, n_m] = 1 with distinct n_m: dw[n_m, :] = x[m, :], every other row of dw exactly zero, db = the hit count."""
    N, K = 70, 132
    g = gen(13 + M)
    x = torch.randn(M, K, generator=g)
    ns = [(3 * m + 1) % N for m in range(M)]
    assert len(set(ns)) == M
    dy = torch.zeros(M, N)
    dy[torch.arange(M), torch.tensor(ns)] = 1.0
    ref = torch.zeros(N, K, dtype=torch.float64)
    ref[ns] = round_to(x, form).double()
    dw, db = gemm_wgrad(ops, dy.to(DEV), x.to(DEV), True, form)
    exact(dw, ref, "skinny_wgrad one-hot: dw", form)
    exact(db, dy.double().sum(0), "skinny_wgrad one-hot: db", form)


# ------------------------------------------------------------------------------------------------
# BatchNorm1d (+ ReLU)
# ------------------------------------------------------------------------------------------------
def bn_data(M, N, affine, seed):
    g = gen(seed)
    x = torch.randn(M, N, generator=g) * 2 + 0.5
    if N > 2:
        x[:, 2] = 0.625                                       # a constant column: variance 0
    gamma = (1 + 0.3 * torch.randn(N, generator=g)) if affine else None
    if affine and N > 1:
        gamma[1] = -gamma[1]
    beta = 0.2 * torch.randn(N, generator=g) if affine else None
    dy = torch.randn(M, N, generator=g)
    rm, rv = torch.randn(N, generator=g) * 0.1, torch.rand(N, generator=g) + 0.5
    return x, gamma, beta, dy, rm, rv


def c(t):
    return None if t is None else t.to(DEV)


def y_as_data(y, relu):
    """The forward's y with exact 0.0, -0.0 and negative entries put in: the backward reads y as data."""
    y = y.detach().cpu().clone()
    if relu:
        M, N = y.shape
        idx = torch.arange(M).view(-1, 1) + torch.arange(N).view(1, -1)
        y[idx % 5 == 0] = 0.0
        y[idx % 5 == 1] = -0.0
        y[idx % 7 == 3] = -1.5
    return y


def invstd_bound(var, var_b, eps):
    """invstd = 1 / sqrt(var + eps) when the kernel's variance lies within var_b of ``var`` (and is not negative): the exact range of
    1 / sqrt over that interval widened by the addition's rounding (k=1), plus k=4 for the square root and the division (correctly
    rounded takes 2).  Not linearised: in a constant column var_b is a tenth of eps."""
    var = torch.as_tensor(var, dtype=torch.float64)
    inv = R.bn1d_invstd_ref(var, eps)
    lo, hi = (var - var_b).clamp_min(0.0) + eps, var + var_b + eps
    inv_hi, inv_lo = 1.0 / torch.sqrt(lo * (1 - U)), 1.0 / torch.sqrt(hi * (1 + U))
    return torch.maximum(inv_hi - inv, inv - inv_lo) + 4 * U * inv_hi


def check_running(rm_new, rv_new, rm, rv, mean, var, count, mean_b, var_b, what):
    r1, r2, m1, m2 = R.bn1d_running_ref(rm, rv, mean, var, count, MOM)
    unb = count / (count - 1.0) if count > 1 else 1.0
    within(rm_new, r1, MOM * mean_b + 3 * U * m1, f"{what}: running_mean")            # k=3: 1 - momentum, the products, the sum
    within(rv_new, r2, MOM * unb * var_b + 4 * U * m2, f"{what}: running_var")        # k=4: and count / (count - 1)


def bwd_with_sums(ops, dy, x, y, mean, invstd, gamma, relu, sums, count):
    """cmu_bn1d_relu_bwd with dgamma / dbeta buffers whatever ``gamma`` is: the local sums the kernel used for dx."""
    M, N = x.shape
    dx, dg, db = torch.empty_like(x), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    ops.call("cmu_bn1d_relu_bwd", ops._p(dy), ops._p(x), ops._p(y), ops._p(mean), ops._p(invstd), ops._p(gamma), int(relu), ops._p(sums), int(count),
             ops._p(dx), ops._p(dg), ops._p(db), M, N, ops._stream())
    return dx, dg, db


def check_bwd(ops, dy, x, yd, mean, invstd, gamma, relu, affine, sums, count, what):
    """The backward of M rows at (mean, invstd): local sums per output (k = M: the additions; k = M + 2: xhat's two roundings and
    the M fmas), dx per element at the sums the kernel returned (``sums`` None) or the exchanged ones: k=7 -- gamma invstd (1), S / count
    (1 each), xhat (2), xhat c1 (1), the two subtractions (2), the product (1), seven on the longest path."""
    M = x.shape[0]
    args = (c(dy), c(x), c(yd), mean, invstd, c(gamma), relu)
    dx, dg, db = ops.bn1d_relu_bwd(*args, sums, count, affine=affine)
    dx2, dg2, db2 = bwd_with_sums(ops, *args, sums, count)
    assert bits_equal(dx, dx2) and (not affine or (bits_equal(dg, dg2) and bits_equal(db, db2)))
    ref, mags = R.bn1d_bwd_sums_ref(dy, x, yd, mean.cpu(), invstd.cpu(), relu)
    within(db2, ref[0], M * U * mags[0], f"{what}: dbeta")                        # k=M
    within(dg2, ref[1], (M + 2) * U * mags[1], f"{what}: dgamma")                 # k=M+2
    used = torch.stack([db2, dg2]).cpu() if sums is None else sums.cpu()
    rdx, m = R.bn1d_bwd_dx_ref(dy, x, yd, mean.cpu(), invstd.cpu(), gamma, relu, used, count if sums is not None else M)
    within(dx, rdx, elem_bound(rdx, m, 7, "f32"), f"{what}: dx")                  # k=7
    return dx


BN_M = [2, 31, 32, 33, 64, 256]
BN_N = [1, 63, 64, 65, 1536]


@pytest.mark.parametrize("relu,affine", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("N", BN_N)
@pytest.mark.parametrize("M", BN_M)
def test_bn1d_local_and_eval(ops, M, N, relu, affine):
    x, gamma, beta, dy, rm, rv = bn_data(M, N, affine, 1000 + M + N)
    rmc, rvc = c(rm), c(rv)
    y, mean, invstd = ops.bn1d_relu_fwd(c(x), c(gamma), c(beta), rmc, rvc, MOM, EPS, True, relu)
    st = R.bn1d_stats_local_ref(x)
    mean_b = M * U * st["mag_mean"]                            # k=M: M - 1 additions and the division
    var_b = (M + 3) * U * st["var"] + mean_b ** 2              # k=M+3: x - mean rounded and squared (2), M fmas, the division
    within(mean, st["mean"], mean_b, "bn1d_fwd: mean")
    within(invstd, R.bn1d_invstd_ref(st["var"], EPS), invstd_bound(st["var"], var_b, EPS), "bn1d_fwd: invstd")
    check_running(rmc, rvc, rm, rv, st["mean"], st["var"], M, mean_b, var_b, "bn1d_fwd")
    ref, m = R.bn1d_fwd_ref(x, mean.cpu(), invstd.cpu(), gamma, beta, relu)
    within(y, ref, elem_bound(ref, m, 4, "f32"), "bn1d_fwd: y")        # k=4: x - mean, * invstd, * gamma, + beta
    yd = y_as_data(y, relu)
    if relu and M + N > 5:
        assert bool((yd == 0).any()) and bool((yd < 0).any()) and bool((yd > 0).any())
    check_bwd(ops, dy, x, yd, mean, invstd, gamma, relu, affine, None, 0, "bn1d_bwd")
    # eval: the running statistics (as updated above) in, nothing updated; backward with zero sums and count 1
    rm1, rv1 = rmc.clone(), rvc.clone()
    ye, me, ie = ops.bn1d_relu_fwd(c(x), c(gamma), c(beta), rmc, rvc, MOM, EPS, False, relu)
    assert bits_equal(rmc, rm1) and bits_equal(rvc, rv1) and bits_equal(me, rm1)
    rvd = rv1.cpu().double()
    within(ie, R.bn1d_invstd_ref(rvd, EPS), invstd_bound(rvd, 0.0, EPS), "bn1d_fwd eval: invstd")
    ref, m = R.bn1d_fwd_ref(x, me.cpu(), ie.cpu(), gamma, beta, relu)
    within(ye, ref, elem_bound(ref, m, 4, "f32"), "bn1d_fwd eval: y")   # k=4
    check_bwd(ops, dy, x, y_as_data(ye, relu), me, ie, gamma, relu, affine, torch.zeros(2, N, device=DEV), 1, "bn1d_bwd eval")


def exchanged_case(ops, x, gamma, beta, dy, rm, rv, relu, affine, split):
    """Two row blocks [0, split) and [split, M): their column sums added in fp32 are what each block is normalised with, at the
    TOTAL count; the running statistics are updated by the first block's call only."""
    M, N = x.shape
    blocks = [slice(0, split), slice(split, M)]
    parts = []
    for b in blocks:
        s = ops.bn1d_colsums(c(x[b].contiguous()))
        ref, mags = R.bn1d_colsums_ref(x[b])
        mb = x[b].shape[0]
        within(s[0], ref[0], mb * U * mags[0], "bn1d_colsums: sum")                # k=M_b: the additions
        within(s[1], ref[1], mb * U * mags[1], "bn1d_colsums: sum of squares")     # k=M_b: one fma per row
        parts.append(s)
    sums = parts[0] + parts[1]
    st = R.bn1d_stats_exchanged_ref(sums.cpu(), M, split)
    mean_b = U * st["mean"].abs()                              # k=1: the division
    var_b = U * (2 * st["e2"] + 3 * st["mean"] ** 2)           # S1 / count (1), mean^2 (3: mean's rounding twice, the product), the subtraction (1, below e2)
    rmc, rvc = c(rm), c(rv)
    ys, dxs = [], []
    for i, b in enumerate(blocks):
        xb = c(x[b].contiguous())
        y, mean, invstd = ops.bn1d_relu_fwd(xb, c(gamma), c(beta), rmc if i == 0 else None, rvc if i == 0 else None, MOM, EPS, True, relu, sums, M)
        within(mean, st["mean"], mean_b, "bn1d_fwd exchanged: mean")
        within(invstd, R.bn1d_invstd_ref(st["var"], EPS), invstd_bound(st["var"], var_b, EPS), "bn1d_fwd exchanged: invstd")
        ref, m = R.bn1d_fwd_ref(x[b], mean.cpu(), invstd.cpu(), gamma, beta, relu)
        within(y, ref, elem_bound(ref, m, 4, "f32"), "bn1d_fwd exchanged: y")         # k=4
        ys.append((y_as_data(y, relu), mean, invstd))
    check_running(rmc, rvc, rm, rv, st["mean"], st["var"], M, mean_b, var_b, "bn1d_fwd exchanged")
    bparts = []
    for b, (yd, mean, invstd) in zip(blocks, ys):
        s = ops.bn1d_bwd_colsums(c(dy[b].contiguous()), c(x[b].contiguous()), c(yd), mean, invstd, relu)
        ref, mags = R.bn1d_bwd_sums_ref(dy[b], x[b], yd, mean.cpu(), invstd.cpu(), relu)
        mb = x[b].shape[0]
        within(s[0], ref[0], mb * U * mags[0], "bn1d_bwd_colsums: sum dz")            # k=M_b
        within(s[1], ref[1], (mb + 2) * U * mags[1], "bn1d_bwd_colsums: sum dz xhat")  # k=M_b+2
        bparts.append(s)
    bs = bparts[0] + bparts[1]
    for b, (yd, mean, invstd) in zip(blocks, ys):
        check_bwd(ops, dy[b].contiguous(), x[b].contiguous(), yd, mean, invstd, gamma, relu, affine, bs, M, "bn1d_bwd exchanged")


@pytest.mark.parametrize("relu,affine", [(True, True), (False, False)])
@pytest.mark.parametrize("N", BN_N)
@pytest.mark.parametrize("M", BN_M)
def test_bn1d_exchanged_sums_unequal_blocks(ops, M, N, relu, affine):
    """A block of one row with the rest, and (from four rows on) a third with two thirds.  relu and affine both on or both off here;
    the four combinations run in the local and eval forms, whose row loops are the same code."""
    x, gamma, beta, dy, rm, rv = bn_data(M, N, affine, 2000 + M + N)
    for split in sorted({1, M // 3} - {0}):
        assert 0 < split < M and (M == 2 or split != M - split)
        exchanged_case(ops, x, gamma, beta, dy, rm, rv, relu, affine, split)


@pytest.mark.parametrize("N", BN_N)
def test_bn1d_single_row(ops, N):
    """M = 1 has no batch statistics of its own: the eval form, and one row normalised with sums exchanged over four rows."""
    x, gamma, beta, dy, rm, rv = bn_data(4, N, True, 3000 + N)
    exchanged_case(ops, x, gamma, beta, dy, rm, rv, True, True, 1)
    x1, dy1 = x[:1].contiguous(), dy[:1].contiguous()
    rmc, rvc = c(rm), c(rv)
    ye, me, ie = ops.bn1d_relu_fwd(c(x1), c(gamma), c(beta), rmc, rvc, MOM, EPS, False, True)
    assert bits_equal(rmc.cpu(), rm) and bits_equal(rvc.cpu(), rv) and bits_equal(me.cpu(), rm)
    within(ie, R.bn1d_invstd_ref(rv, EPS), invstd_bound(rv.double(), 0.0, EPS), "bn1d_fwd eval: invstd")
    ref, m = R.bn1d_fwd_ref(x1, me.cpu(), ie.cpu(), gamma, beta, True)
    within(ye, ref, elem_bound(ref, m, 4, "f32"), "bn1d_fwd eval: y")   # k=4
    check_bwd(ops, dy1, x1, y_as_data(ye, True), me, ie, gamma, True, True, torch.zeros(2, N, device=DEV), 1, "bn1d_bwd eval")


@pytest.mark.parametrize("M,N", [(2, 1), (33, 65), (256, 1536)])
def test_bn1d_bwd_impulses(ops, M, N):
    """A gradient of one 1.0 at (0, 0) and one at (M - 1, N - 1), the gate open there and decided by y as data everywhere else:
    dbeta counts the impulses exactly, dgamma is xhat at the impulse (k=2, and k=1 more where both share a column), every other
    column of the sums and of dx is exactly zero.  A rounding bound over all rows cannot see one dropped row; this can."""
    x, gamma, beta, _, rm, rv = bn_data(M, N, True, 4000 + M)
    y, mean, invstd = ops.bn1d_relu_fwd(c(x), c(gamma), c(beta), None, None, MOM, EPS, True, True)
    yd = y_as_data(y, True)
    yd[0, 0] = yd[M - 1, N - 1] = 1.0
    dy = torch.zeros(M, N)
    dy[0, 0] = dy[M - 1, N - 1] = 1.0
    dx, dg, db = ops.bn1d_relu_bwd(c(dy), c(x), c(yd), mean, invstd, c(gamma), True)
    ref, mags = R.bn1d_bwd_sums_ref(dy, x, yd, mean.cpu(), invstd.cpu(), True)
    assert float(ref[0].sum()) == 2.0
    exact(db, ref[0], "bn1d_bwd impulse: dbeta", "f32")
    within(dg, ref[1], 3 * U * mags[1], "bn1d_bwd impulse: dgamma")               # k=3
    rdx, m = R.bn1d_bwd_dx_ref(dy, x, yd, mean.cpu(), invstd.cpu(), gamma, True, torch.stack([db, dg]).cpu(), M)
    within(dx, rdx, elem_bound(rdx, m, 7, "f32"), "bn1d_bwd impulse: dx")         # k=7
    if N > 2:
        assert bool((dx[:, 1:N - 1] == 0).all()) and bool((dg[1:N - 1] == 0).all())


# ------------------------------------------------------------------------------------------------
# 1x1 convolution NHWC (dt, pending transform) -> NCHW fp32
# ------------------------------------------------------------------------------------------------
C1_PIX = [(1, 2, 2), (1, 6, 6), (1, 10, 10), (3, 4, 11), (5, 2, 26)]              # B H W = 4, 36, 100, 132, 260 pixels
C1_N = [1, 31, 32, 33, 127, 128, 129, 160]


def conv_act(ops, x, dt, pad, sc, sh, relu_from):
    """NHWC fp32 CPU tensor (already exact in dt) -> Act: channels [pad, pad + K) of a buffer 2 pad wider, a sentinel outside."""
    B, H, W, K = x.shape
    buf = torch.full((B, H, W, K + 2 * pad), SENT, dtype=TORCH_DT[dt])
    buf[..., pad:pad + K] = x.to(buf.dtype)
    return ops.Act(buf.to(DEV), pad, K, c(sc), c(sh), relu_from)


def conv_int_case(ops, dt, B, H, W, K, N, relu_from, pad, transform=True, seed=0):
    g = gen(seed + B * H * W + 3 * N + K)
    x, w, b = ints((B, H, W, K), g), ints((N, K), g), ints((N,), g)
    sc = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (K,), generator=g)] if transform else None
    sh = ints((K,), g) if transform else None
    assert K * 27 + 3 < 2 ** 24                                # |x sc + sh| <= 9, |w| <= 3: every partial sum is an exact integer
    if transform and 0 < abs(relu_from) < K:                   # negative pre-activations on both sides: the data can tell the signs apart
        neg = ((x * sc + sh) < 0).reshape(-1, K).any(0)
        on = R.relu_on(K, relu_from)
        assert bool(neg[on].any()) and bool(neg[~on].any())
    out = ops.conv1x1_nchw_fwd(conv_act(ops, x, dt, pad, sc, sh, relu_from), w.to(DEV), b.to(DEV))
    ref, _ = R.conv1x1_nchw_ref(x, sc, sh, relu_from, w, b, dt)
    exact(out, ref, f"conv1x1_nchw exact: npix={B * H * W} N={N} K={K} relu_from={relu_from}", dt)


@pytest.mark.parametrize("dt,K", [("f32", 8)] + [(dt, K) for dt in FORMS for K in (16, 48, 1024)])
def test_conv1x1_nchw_exact_integers(ops, dt, K):
    """Pixel counts below one 32-pixel wave, a ragged wave, a ragged 128-pixel workgroup and more than one (over several images: the
    (image, pixel) split of the NCHW store); N around the 32-channel MFMA tile and the 128-channel workgroup; K of one k-step, an odd
    number of 16-byte chunks per lane half and the latent's 1,024.  The input is a channel slice with a sentinel outside."""
    assert K % (2 * EPC[dt]) == 0                               # whole 32-byte slices: K = 8 exists at f32 only
    for B, H, W in C1_PIX:
        for N in C1_N:
            conv_int_case(ops, dt, B, H, W, K, N, 0, EPC[dt])
    conv_int_case(ops, dt, 3, 4, 11, K, 33, 0, 0, transform=False)


@pytest.mark.parametrize("dt", FORMS)
@pytest.mark.parametrize("K", [48, 1024])
def test_conv1x1_nchw_relu_from_both_signs(ops, dt, K):
    """relu_from = 0 (every channel), a middle chunk, K (none), and a negative chunk multiple -n: the FIRST n channels (cmu_relu_on)."""
    e = EPC[dt]
    for rf in (0, 2 * e, K, -2 * e, -(K - e)):
        conv_int_case(ops, dt, 3, 4, 11, K, 33, rf, e, seed=5)
        conv_int_case(ops, dt, 1, 10, 10, K, 129, rf, 0, seed=6)


@pytest.mark.parametrize("dt", FORMS)
def test_conv1x1_nchw_float_data(ops, dt):
    """Random data, a sliced input, a negative relu_from: against float64 on the same rounded operands at the bar of
    test_gpu_skinny.py::test_conv1x1_nchw_vs_conv2d."""
    B, H, W, K, N = 2, 6, 10, 1024, 160
    g = gen(77)
    x = quant(torch.randn(B, H, W, K, generator=g), dt)
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    sc, sh = 1 + 0.2 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
    out = ops.conv1x1_nchw_fwd(conv_act(ops, x, dt, EPC[dt], sc, sh, -512), w.to(DEV), b.to(DEV))
    ref, _ = R.conv1x1_nchw_ref(x, sc, sh, -512, w, b, dt)
    tol = {"f32": 2e-5, "f16": 2e-3, "bf16": 1.6e-2}[dt]
    within(out, ref, tol * max(1.0, float(ref.abs().max())), "conv1x1_nchw float", dt)
