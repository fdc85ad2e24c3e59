"""The fused MoCo InfoNCE + enqueue kernel (csrc/moco.hip: ``moco_fused_kernel`` behind ``cmu_moco_infonce_enqueue``) per element
against the float64 reference of tests/moco_fused_ref.py (proved on the CPU in tests/test_cpu_moco_fused_ref.py, which also proves
that the bounds used here see single faults).  Conventions of test_gpu_elem_fp64.py / test_gpu_necks_fp64.py: U = 2^-24, bounds
k U sum |terms| with every k counted from the kernel's code (moco_fused_ref's docstring), every comparison recorded in ``PARITY``
and printed as ``[parity] ...``.

Per call: loss (finite, within the loss bound of the float64 mean), dq and k_norm_out element by element, the enqueued columns bit
for bit (the kernel's own k_norm_out, or keys_all), every other queue element's bits kept, the pointer exact, sentinels behind the
queue, dq, loss, k_norm_out and in 256 bytes past cmu_moco_ws_bytes untouched.  Per case: the same bits whatever the workspace held
(NaN, zeros, the leftovers of a call of another shape), on a repeat, and with dq or k_norm_out absent.

The kernel's grid barriers need the device to themselves: every call goes on the current stream between two device
synchronisations, nothing runs beside it, and nothing here goes near the barrier's time-out path.
"""
import math

import pytest
import torch

import moco_fused_ref as R
from test_gpu_elem_fp64 import PARITY, within

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.0
PAD = 64                                          # floats of sentinel behind every output
IDS = [R.case_id(c) for c in R.CASES]
_BUILT = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmunet_amd import ops as o
    return o


def lib():
    from cmunet_amd import _lib
    return _lib.lib()


def built(c):
    """(inputs, float64 reference, bounds) of a case: computed once, shared, never modified."""
    if c not in _BUILT:
        d = R.build_case(c)
        ref = R.reference(d["q_raw"], d["k_raw"], d["keys_all"], d["queue"], d["ptr"], d["T"])
        _BUILT[c] = (d, ref, R.bounds(ref, d["queue"]))
    return _BUILT[c]


def bits_equal(a, b):
    """The same fp32 bit patterns (a NaN equals itself, +0 differs from -0), whatever the strides of the two views."""
    return a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))


def guarded(n, fill):
    buf = torch.full((n + PAD,), SENT, device=DEV)
    buf[:n] = fill
    return buf


class Out:
    """What one call left: loss (1,), dq (B, D) or None, kn (B, D) or None, queue (D, K), ptr (int)."""


def workspace(nbytes, state):
    """cmu_moco_ws_bytes bytes and a 256-byte guard behind them, all filled with NaN bits (0xFF) or zeros."""
    return torch.full((nbytes + 256,), 0xFF if state == "nan" else 0, dtype=torch.uint8, device=DEV)


def run(ops, q_raw, k_raw, keys_all, queue, ptr, T, ws, want_dq=True, want_kn=True):
    """One call on the current stream between two device synchronisations, every output between sentinels."""
    B, D = q_raw.shape
    K = queue.shape[1]
    nws = lib().cmu_moco_ws_bytes(B, D, K)
    assert nws == R.ws_bytes(B, D, K) and ws.numel() >= nws + 256
    qbuf = guarded(D * K, 0.0)
    qbuf[:D * K] = queue.to(DEV).reshape(-1)
    lbuf, dbuf, kbuf = guarded(1, math.nan), guarded(B * D, math.nan), guarded(B * D, math.nan)
    pd = torch.tensor([ptr, 123456789], dtype=torch.long, device=DEV)
    tail = ws[nws:nws + 256].clone()
    qd, kd = q_raw.to(DEV), k_raw.to(DEV)
    ka = None if keys_all is None else keys_all.to(DEV)
    torch.cuda.synchronize()
    ops.moco_infonce_enqueue(qd, kd, ka, qbuf[:D * K].view(D, K), pd, lbuf[:1], dbuf[:B * D].view(B, D) if want_dq else None,
                             kbuf[:B * D].view(B, D) if want_kn else None, T, ws)
    torch.cuda.synchronize()
    for name, buf, n in (("queue", qbuf, D * K), ("dq", dbuf, B * D), ("loss", lbuf, 1), ("k_norm_out", kbuf, B * D)):
        assert bool((buf[n:] == SENT).all()), f"the kernel wrote behind {name}"
    assert torch.equal(ws[nws:nws + 256], tail), "the kernel wrote past cmu_moco_ws_bytes"
    assert int(pd[1]) == 123456789, "the kernel wrote behind queue_ptr"
    if not want_dq:
        assert bool(torch.isnan(dbuf[:B * D]).all())
    if not want_kn:
        assert bool(torch.isnan(kbuf[:B * D]).all())
    o = Out()
    o.loss, o.ptr = lbuf[:1].cpu(), int(pd[0])
    o.dq = dbuf[:B * D].view(B, D).cpu() if want_dq else None
    o.kn = kbuf[:B * D].view(B, D).cpu() if want_kn else None
    o.queue = qbuf[:D * K].view(D, K).cpu()
    assert math.isfinite(float(o.loss)), ("the loss is not finite: the kernel answers NaN when a grid barrier timed out (bar[7] of the "
                                          "workspace, moco.hip) -- was anything else running on the device?  Not retried.")
    return o


def check_against_reference(o, q_raw, keys_all, queue, ptr, ref, b, tag):
    """The per-call assertions of the issue on one result."""
    B, D = q_raw.shape
    K = queue.shape[1]
    Nk = B if keys_all is None else keys_all.shape[0]
    within(o.loss, ref["loss"].reshape(1), b["loss"].reshape(1), f"moco loss: {tag}")
    within(o.dq, ref["dq"], b["dq"], f"moco dq: {tag}")
    within(o.kn, ref["kn"], b["kn"], f"moco k_norm_out: {tag}")
    cols = R.ring_columns(ptr, Nk, K)
    new = o.kn if keys_all is None else keys_all
    assert bits_equal(o.queue[:, cols], new.t()), f"{tag}: the enqueued columns are not the keys bit for bit"
    rest = sorted(set(range(K)) - set(cols))
    assert bits_equal(o.queue[:, rest], queue[:, rest]), f"{tag}: a queue element outside the enqueue changed"
    assert o.ptr == ref["ptr"] == (R.effective_ptr(ptr, K) + Nk) % K, (tag, o.ptr, ref["ptr"])


def same_bits(a, b, what, dq=True, kn=True):
    assert bits_equal(a.loss, b.loss), f"{what}: loss bits differ"
    assert bits_equal(a.queue, b.queue) and a.ptr == b.ptr, f"{what}: queue / pointer differ"
    if dq:
        assert bits_equal(a.dq, b.dq), f"{what}: dq bits differ"
    if kn:
        assert bits_equal(a.kn, b.kn), f"{what}: k_norm_out bits differ"


def other_shape_call(ops, c, d, ws):
    """A call of another shape on the same workspace buffer (2 B rows where the ring allows it, else one row; random rows): what it
    leaves in the workspace is what a later call of the case's shape finds there."""
    B2 = 2 * c.B if c.K % (2 * c.B) == 0 else (1 if c.B > 1 else 2)
    assert B2 != c.B and c.K % B2 == 0
    g = torch.Generator().manual_seed(5)
    run(ops, torch.randn(B2, c.D, generator=g), torch.randn(B2, c.D, generator=g), None, d["queue"], 0, 0.2, ws)


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_moco_fused_against_fp64(ops, c):
    d, ref, b = built(c)
    args = (d["q_raw"], d["k_raw"], d["keys_all"], d["queue"], d["ptr"], d["T"])
    nws = lib().cmu_moco_ws_bytes(c.B, c.D, c.K)
    big = max(nws, lib().cmu_moco_ws_bytes(2 * c.B, c.D, c.K))
    tag = R.case_id(c)
    a = run(ops, *args, workspace(nws, "nan"))                                 # the workspace full of NaN
    check_against_reference(a, d["q_raw"], d["keys_all"], d["queue"], d["ptr"], ref, b, tag)
    same_bits(run(ops, *args, workspace(nws, "zero")), a, f"{tag}: workspace of zeros")
    ws = workspace(big, "zero")
    other_shape_call(ops, c, d, ws)
    same_bits(run(ops, *args, ws), a, f"{tag}: workspace left by another shape")
    same_bits(run(ops, *args, ws), a, f"{tag}: repeat")
    same_bits(run(ops, *args, ws, want_dq=False), a, f"{tag}: dq = None", dq=False)
    same_bits(run(ops, *args, ws, want_kn=False), a, f"{tag}: k_norm_out = None", kn=False)


TWO_STEP = [c for c in R.CASES if (c.B, c.D, c.K, c.Nk, c.ptr) in {(5, 72, 260, None, 255), (5, 72, 260, 10, 255), (33, 130, 396, 66, 330),
                                                                  (3, 5, 12, None, 6), (4, 16, 8, 8, 0)}]


@pytest.mark.parametrize("c", TWO_STEP, ids=[R.case_id(c) for c in TWO_STEP])
def test_second_call_sees_the_first_call_s_keys(ops, c):
    """Two consecutive calls on one queue and pointer, against the reference stepped twice.  The second call's queries are the first
    call's keys: their largest negative logits sit on the columns the first call wrote.  The second reference step starts from the
    queue the device holds after the first call (checked bit for bit against the first call's keys just before)."""
    d, ref, b = built(c)
    nws = lib().cmu_moco_ws_bytes(c.B, c.D, c.K)
    ws = workspace(nws, "nan")
    a = run(ops, d["q_raw"], d["k_raw"], d["keys_all"], d["queue"], d["ptr"], d["T"], ws)
    check_against_reference(a, d["q_raw"], d["keys_all"], d["queue"], d["ptr"], ref, b, R.case_id(c) + " step 1")
    q2, k2 = R.second_step_inputs(d)
    ref2 = R.reference(q2, k2, d["keys_all"], a.queue, a.ptr, d["T"])
    stale = R.reference(q2, k2, d["keys_all"], d["queue"], a.ptr, d["T"])
    b2 = R.bounds(ref2, a.queue)
    # the inputs tell the two queues apart: a second call that saw the first call's OLD queue would be far outside the bounds
    assert abs(float(stale["loss"] - ref2["loss"])) > 100 * float(b2["loss"])
    o = run(ops, q2, k2, d["keys_all"], a.queue, a.ptr, d["T"], ws)
    check_against_reference(o, q2, d["keys_all"], a.queue, a.ptr, ref2, b2, R.case_id(c) + " step 2")
    assert o.ptr == (R.effective_ptr(c.ptr, c.K) + 2 * (c.Nk or c.B)) % c.K


def test_zz_parity_table(ops):
    """Printed record (run with -s): the worst err / bound per output over everything above."""
    keys = [k for k in PARITY if k[0].startswith("moco ")]
    assert {k[0] for k in keys} == {"moco loss", "moco dq", "moco k_norm_out"}
    for k in sorted(keys):
        print(f"[parity] {k[0]} {k[1]}: worst err / bound {PARITY[k]:.3g}")
        assert PARITY[k] <= 1.0
