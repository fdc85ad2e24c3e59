"""The float64 references of tests/necks_fp64_ref.py against torch on the CPU: BatchNorm1d (+ReLU) against F.batch_norm + relu and
their float64 autograd (local, exchanged-sums and eval forms, with and without affine, running statistics included), the NCHW 1x1
convolution against F.conv2d with both signs of relu_from, mask-select and the masked sums against a per-pixel restatement.  The
exchanged form is checked against the local form on the concatenated rows: that is what the reference's SyncBN computes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import necks_fp64_ref as R

REL = 1e-12
EPS = float(np.float32(1e-6))
MOM = float(np.float32(0.1))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(got, ref, mag, what, rel=REL):
    got, ref, mag = (torch.as_tensor(t, dtype=torch.float64) for t in (got, ref, mag))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > rel * mag + 1e-300
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {ref.numel()} outside {rel:g} of the magnitude, worst {float((err / (mag + 1e-300)).max()):.3g}"


def bn_inputs(M, N, affine, seed):
    g = gen(seed)
    x = torch.randn(M, N, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma = (1 + 0.3 * torch.randn(N, generator=g, dtype=torch.float64)) if affine else None
    if affine and N > 1:
        gamma[1] = -gamma[1]
    beta = 0.2 * torch.randn(N, generator=g, dtype=torch.float64) if affine else None
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(N, generator=g, dtype=torch.float64) * 0.1, torch.rand(N, generator=g, dtype=torch.float64) + 0.5
    return x, gamma, beta, dy, rm, rv


def torch_bn(x, gamma, beta, rm, rv, training, relu, dy):
    """F.batch_norm (+ relu) and its autograd in float64 -> y, dx, dgamma, dbeta, running statistics after the call."""
    xd = x.clone().requires_grad_(True)
    gd = None if gamma is None else gamma.clone().requires_grad_(True)
    bd = None if beta is None else beta.clone().requires_grad_(True)
    rm, rv = rm.clone(), rv.clone()
    y = F.batch_norm(xd, rm, rv, gd, bd, training, MOM, EPS)
    if relu:
        y = F.relu(y)
    y.backward(dy)
    return y.detach(), xd.grad, None if gd is None else gd.grad, None if bd is None else bd.grad, rm, rv


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("M,N", [(2, 5), (7, 3), (33, 4)])
def test_bn1d_local_form_matches_autograd(M, N, affine, relu):
    x, gamma, beta, dy, rm, rv = bn_inputs(M, N, affine, 10 + M + N)
    y_t, dx_t, dg_t, db_t, rm_t, rv_t = torch_bn(x, gamma, beta, rm, rv, True, relu, dy)
    st = R.bn1d_stats_local_ref(x)
    invstd = R.bn1d_invstd_ref(st["var"], EPS)
    y, mag = R.bn1d_fwd_ref(x, st["mean"], invstd, gamma, beta, relu)
    close(y, y_t, mag, "y")
    rm2, rv2, m1, m2 = R.bn1d_running_ref(rm, rv, st["mean"], st["var"], M, MOM)
    close(rm2, rm_t, m1, "running_mean")
    close(rv2, rv_t, m2, "running_var")
    sums, mags = R.bn1d_bwd_sums_ref(dy, x, y, st["mean"], invstd, relu)
    if affine:
        close(sums[0], db_t, mags[0], "dbeta")
        close(sums[1], dg_t, mags[1], "dgamma")
    dx, mdx = R.bn1d_bwd_dx_ref(dy, x, y, st["mean"], invstd, gamma, relu, sums, M)
    close(dx, dx_t, mdx, "dx", 1e-11)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("split", [1, 3, 6])
def test_bn1d_exchanged_form_is_the_local_form_on_the_concatenated_rows(split, relu):
    """Two unequal row blocks (one of a single row): the column sums of the blocks added up give the statistics of all rows, and each
    block's dx at the added backward sums and the TOTAL count is that block's slice of the whole batch's dx."""
    M, N = 7, 4
    x, gamma, beta, dy, rm, rv = bn_inputs(M, N, True, 40 + split)
    y_t, dx_t, dg_t, db_t, rm_t, rv_t = torch_bn(x, gamma, beta, rm, rv, True, relu, dy)
    blocks = [slice(0, split), slice(split, M)]
    sums = sum(R.bn1d_colsums_ref(x[b])[0] for b in blocks)
    st = R.bn1d_stats_exchanged_ref(sums, M, split)
    loc = R.bn1d_stats_local_ref(x)
    close(st["mean"], loc["mean"], loc["mag_mean"], "mean")
    close(st["var"], loc["var"], st["e2"] + loc["mean"] ** 2, "var", 1e-11)
    invstd = R.bn1d_invstd_ref(loc["var"], EPS)
    rm2, rv2, m1, m2 = R.bn1d_running_ref(rm, rv, st["mean"], loc["var"], M, MOM)
    close(rm2, rm_t, m1, "running_mean")
    close(rv2, rv_t, m2, "running_var")
    ys = [R.bn1d_fwd_ref(x[b], loc["mean"], invstd, gamma, beta, relu)[0] for b in blocks]
    close(torch.cat(ys), y_t, y_t.abs() + 1, "y")
    bs = [R.bn1d_bwd_sums_ref(dy[b], x[b], y, loc["mean"], invstd, relu) for b, y in zip(blocks, ys)]
    tot = bs[0][0] + bs[1][0]
    close(tot[0], db_t, bs[0][1][0] + bs[1][1][0], "dbeta")
    close(tot[1], dg_t, bs[0][1][1] + bs[1][1][1], "dgamma")
    for b, y in zip(blocks, ys):
        dx, mdx = R.bn1d_bwd_dx_ref(dy[b], x[b], y, loc["mean"], invstd, gamma, relu, tot, M)
        close(dx, dx_t[b], mdx, "dx", 1e-11)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("M", [1, 5])
def test_bn1d_eval_form_matches_autograd(M, affine, relu):
    """Running statistics in, nothing updated; the backward is that of the fixed affine map: zero sums, count 1."""
    N = 4
    x, gamma, beta, dy, rm, rv = bn_inputs(M, N, affine, 70 + M)
    y_t, dx_t, dg_t, db_t, rm_t, rv_t = torch_bn(x, gamma, beta, rm, rv, False, relu, dy)
    assert torch.equal(rm_t, rm) and torch.equal(rv_t, rv)
    invstd = R.bn1d_invstd_ref(rv, EPS)
    y, mag = R.bn1d_fwd_ref(x, rm, invstd, gamma, beta, relu)
    close(y, y_t, mag, "y")
    sums, mags = R.bn1d_bwd_sums_ref(dy, x, y, rm, invstd, relu)
    if affine:
        close(sums[0], db_t, mags[0], "dbeta")
        close(sums[1], dg_t, mags[1], "dgamma")
    dx, mdx = R.bn1d_bwd_dx_ref(dy, x, y, rm, invstd, gamma, relu, None, 1)
    close(dx, dx_t, mdx, "dx")


def test_bn1d_gate_is_strict_and_unbiased_count_of_one():
    y = torch.tensor([[0.0, -0.0, 1e-30, -1.0]])
    assert R.bn1d_gate(y, True).tolist() == [[False, False, True, False]] and bool(R.bn1d_gate(y, False).all())
    rm2, rv2, _, _ = R.bn1d_running_ref(torch.zeros(1), torch.ones(1), torch.ones(1), torch.full((1,), 2.0), 1, 0.5)
    assert float(rv2) == 0.5 * 1 + 0.5 * 2.0                      # count 1: no count / (count - 1)
    _, rv3, _, _ = R.bn1d_running_ref(torch.zeros(1), torch.ones(1), torch.ones(1), torch.full((1,), 2.0), 3, 0.5)
    assert float(rv3) == 0.5 * 1 + 0.5 * 2.0 * 1.5


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("relu_from", [0, 8, 16, -8])
def test_conv1x1_nchw_matches_conv2d(dt, relu_from):
    g = gen(5)
    B, H, W, K, N = 2, 2, 6, 16, 5
    x = torch.randn(B, H, W, K, generator=g).to(R.TORCH_DT[dt]).float()
    w, b = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    sc, sh = 1 + 0.2 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
    t = x.double() * sc.double() + sh.double()
    on = torch.arange(K) >= relu_from if relu_from >= 0 else torch.arange(K) < -relu_from
    assert 0 < int(on.sum()) < K or relu_from in (0, K)
    a = torch.where(on, t.clamp_min(0), t).to(R.TORCH_DT[dt]).double()
    ref = F.conv2d(a.permute(0, 3, 1, 2), w.to(R.TORCH_DT[dt]).double().view(N, K, 1, 1), b.double())
    out, mag = R.conv1x1_nchw_ref(x, sc, sh, relu_from, w, b, dt)
    close(out, ref, mag, "transformed")
    out, mag = R.conv1x1_nchw_ref(x, None, None, 0, w, None, dt)
    close(out, F.conv2d(x.double().permute(0, 3, 1, 2), w.to(R.TORCH_DT[dt]).double().view(N, K, 1, 1)), mag, "plain")


@pytest.mark.parametrize("invert", [False, True])
def test_mask_select_and_masked_sums_pixel_by_pixel(invert):
    g = gen(9)
    B, f, H, C = 2, 2, 8, 3
    active = torch.tensor([[[1, 0], [0, 0]], [[0, 1], [1, 1]]], dtype=torch.uint8)
    x = torch.randn(B, H, H, C, generator=g).to(torch.float16).float()
    sc, sh, fill = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    sel = R.selection(active, H, H, invert)
    frame = R.ring_frame(active, H)
    for relu, tr, fl in ((True, True, None), (False, True, fill), (False, False, None), (True, False, fill)):
        out, m, moved = R.mask_select_ref(x, sc if tr else None, sh if tr else None, relu, sel, fl, "f16")
        assert moved == (not tr and not relu)
        s1, s2, m1, m2 = R.masked_sums_ref(x, sel)
        e1, e2 = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        for b in range(B):
            for yy in range(H):
                for xx in range(H):
                    on = bool(active[b, yy // 4, xx // 4]) != invert
                    assert bool(sel[b, yy, xx]) == on
                    edge = yy % 4 in (0, 3) or xx % 4 in (0, 3)
                    assert bool(frame[b, yy, xx]) == (not bool(active[b, yy // 4, xx // 4]) and edge)
                    for c in range(C):
                        v = float(x[b, yy, xx, c])
                        if on:
                            t = v * float(sc[c]) + float(sh[c]) if tr else v
                            t = max(t, 0.0) if relu else t
                            e1[c] += v
                            e2[c] += v * v
                        else:
                            t = 0.0 if fl is None else float(fl[c].half())
                            assert float(m[b, yy, xx, c]) == 0.0
                        assert abs(float(out[b, yy, xx, c]) - t) <= 1e-12 * (abs(t) + 1)
        close(s1, e1, m1, "s1")
        close(s2, e2, m2, "s2")


def test_gemm_refs():
    g = gen(3)
    x, w, b, dy = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((5, 8), (3, 8), (3,), (5, 3)))
    xd, wd, bd = (t.clone().requires_grad_(True) for t in (x, w, b))
    F.linear(xd, wd, bd).backward(dy)
    close(R.gemm_fwd_ref(x, w, b), F.linear(x, w, b), 10.0, "y")
    close(R.gemm_dgrad_ref(dy, w), xd.grad, 10.0, "dx")
    dw, db = R.gemm_wgrad_ref(dy, x)
    close(dw, wd.grad, 10.0, "dw")
    close(db, bd.grad, 10.0, "db")
