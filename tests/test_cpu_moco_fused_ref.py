"""CPU proof of tests/moco_fused_ref.py, the float64 reference that tests/test_gpu_moco_fused_fp64.py holds csrc/moco.hip to:

  * the reference equals the oracle (oracle.moco.logits_from_embeddings + F.cross_entropy + autograd + dequeue_and_enqueue) in float64
    to 1e-12 relative on every case; the oracle's enqueue is a slice assignment and refuses a pointer that is no multiple of Nk, so the
    ring rule is also checked against a plain numpy loop, on every case;
  * the designed inputs hold what they promise (unit columns, seam columns with soft-max weight, scaled and all-zero rows);
  * SENSITIVITY: seven single faults put into the float64 reference each move at least one output by more than 4 times its bound, on
    every case -- the bounds would catch a kernel that is wrong in that way (``[sensitivity]`` lines: the smallest ratio per fault);
  * the host restatement of moco_splits and of the workspace layout equals cmu_moco_ws_bytes, and the cases sit on the branches
    they are named for;
  * the entry point refuses K % 4, K % Nk, T <= 0 and a misaligned queue before any HIP call.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import moco_fused_ref as R

IDS = [R.case_id(c) for c in R.CASES]
_BUILT = {}


def built(c):
    """(inputs, reference, bounds) of a case, computed once and never modified."""
    if c not in _BUILT:
        d = R.build_case(c)
        ref = R.reference(d["q_raw"], d["k_raw"], d["keys_all"], d["queue"], d["ptr"], d["T"])
        _BUILT[c] = (d, ref, R.bounds(ref, d["queue"]))
    return _BUILT[c]


def rel_rows(a, b):
    """max over rows of max |a - b| / max |b| of that row (rows differ by 1e8 in scale, the all-zero query row by 1e12)."""
    a, b = a.reshape(a.shape[0], -1) if a.dim() > 1 else a.reshape(1, -1), b.reshape(b.shape[0], -1) if b.dim() > 1 else b.reshape(1, -1)
    den = b.abs().max(1).values
    err = (a - b).abs().max(1).values
    return float((err / den.clamp_min(1e-300)).max()) if bool((den > 0).all()) or bool((err[den == 0] == 0).all()) else math.inf


def test_case_list_is_the_issue_s():
    shapes = {(c.B, c.D, c.K, c.Nk) for c in R.CASES}
    assert shapes == {(1, 8, 4, None), (3, 5, 12, None), (7, 70, 28, None), (5, 72, 260, None), (5, 72, 260, 10), (33, 130, 396, None),
                      (33, 130, 396, 66), (64, 128, 512, None), (8, 64, 16416, None), (32, 1024, 4096, None), (32, 1024, 4096, 64),
                      (4, 16, 8, 8)}
    assert {c.T for c in R.CASES} == set(R.TEMPS)
    kinds = set()
    for c in R.CASES:
        Nk = c.Nk or c.B
        assert c.K % Nk == 0 and c.K % 4 == 0
        if c.ptr == 0:
            kinds.add("zero")
        elif 0 < c.ptr < c.K - Nk and c.ptr % Nk == 0:
            kinds.add("interior")
        elif c.ptr == c.K - Nk:
            kinds.add("wraps to 0")
        elif Nk % 2 == 0 and c.ptr == c.K - Nk // 2:
            kinds.add("split")
        elif c.ptr < 0:
            kinds.add("negative")
        elif c.ptr == c.K:
            kinds.add("K")
        elif c.ptr > c.K:
            kinds.add("past K")
    assert kinds == {"zero", "interior", "wraps to 0", "split", "negative", "K", "past K"}


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_reference_equals_the_oracle(c):
    from oracle import moco as OM
    d, ref, _ = built(c)
    qr = d["q_raw"].double().requires_grad_(True)
    logits, labels, k, q = OM.logits_from_embeddings(qr, d["k_raw"].double(), d["queue"].double(), d["T"])
    per_row = F.cross_entropy(logits, labels, reduction="none")
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    assert rel_rows(ref["kn"], k) <= 1e-12                # (an all-zero row: both exactly zero)
    assert rel_rows(ref["logits"], logits.detach()) <= 1e-12
    assert rel_rows(ref["losses"], per_row.detach()) <= 1e-12
    assert abs(float(ref["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert rel_rows(ref["dq"], qr.grad) <= 1e-12, rel_rows(ref["dq"], qr.grad)
    Nk = c.Nk or c.B
    keys = k.detach() if d["keys_all"] is None else d["keys_all"].double()
    p0 = R.effective_ptr(c.ptr, c.K)                      # the kernel's guard; the oracle has none
    if p0 % Nk == 0:
        oq, optr = d["queue"].double().clone(), torch.tensor([p0])
        OM.dequeue_and_enqueue(keys, oq, optr, c.K)
        assert int(optr) == ref["ptr"]
        if d["keys_all"] is None:
            assert rel_rows(ref["queue"].t(), oq.t()) <= 1e-12
        else:
            assert torch.equal(ref["queue"], oq)
    # the ring rule, in three lines
    want = d["queue"].double().numpy().copy()
    for i in range(Nk):
        want[:, (p0 + i) % c.K] = (ref["kn"] if d["keys_all"] is None else keys).numpy()[i]
    assert np.array_equal(ref["queue"].numpy(), want)
    assert ref["ptr"] == (p0 + Nk) % c.K


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_designed_inputs_hold_their_promises(c):
    d, ref, _ = built(c)
    Q = d["queue"]
    assert Q.dtype == torch.float32 and Q.shape == (c.D, c.K)
    assert float((Q.double().norm(dim=0) - 1).abs().max()) <= 4 * R.U           # unit columns, rounded to fp32
    assert set(d["seams"]) == set(R.seam_columns(c.D, c.K))
    for j, b in d["seams"].items():
        assert float(ref["w"][:, 1 + j].max()) >= R.SEAM_WEIGHT, (j, b, float(ref["w"][:, 1 + j].max()))
    zk, zq = R.zero_rows(c.B)
    if zk is not None:
        assert bool((d["k_raw"][zk] == 0).all()) and bool((ref["kn"][zk] == 0).all())
        assert np.array_equal(ref["queue"][:, R.ring_columns(c.ptr, c.Nk or c.B, c.K)[zk]].numpy(),
                              np.zeros(c.D) if d["keys_all"] is None else d["keys_all"][zk].double().numpy())
    if zq is not None:
        assert zq != zk and bool((d["q_raw"][zq] == 0).all()) and float(ref["nq"][zq]) == 1e-12
        assert bool(torch.isfinite(ref["dq"][zq]).all()) and float(ref["dq"][zq].abs().max()) > 1e6    # g / 1e-12, as autograd gives it
        assert float(ref["dq"][zq].abs().max()) < 1e30                                                   # representable in fp32
    nq = d["q_raw"].double().norm(dim=1)
    if c.B >= 4:
        nk = d["k_raw"].double().norm(dim=1)
        assert float(nq.max()) > 4e3 and float(nq[nq > 0].min()) < 2e-4 and float(nk.max()) > 4e3 and float(nk[nk > 0].min()) < 2e-4
    if d["keys_all"] is not None:
        assert d["keys_all"].shape == (c.Nk, c.D) and torch.equal(d["keys_all"][:c.B], ref["kn"].float())
    assert bool(torch.isfinite(ref["dq"]).all()) and math.isfinite(float(ref["loss"]))


# ------------------------------------------------------------------------------------------------
# sensitivity
# ------------------------------------------------------------------------------------------------
# (fault, case id) pairs where the fault cannot apply -- at most one case per fault.  None is needed: every case has D >= 5
# (drop_last_d), every case writes at least one column whose neighbour holds other values (shift_enqueue), ...
EXCLUDED = {}
SENS = {}


def fault_ratio(c, fault):
    """max over the outputs of max |faulty - reference| / bound; a changed bit of an exact output (queue, pointer) counts as inf."""
    d, ref, b = built(c)
    bad = R.reference(d["q_raw"], d["k_raw"], d["keys_all"], d["queue"], d["ptr"], d["T"], fault=fault)
    if not torch.equal(bad["queue"], ref["queue"]) or bad["ptr"] != ref["ptr"]:
        return math.inf
    r = abs(float(bad["loss"] - ref["loss"])) / float(b["loss"])
    r = max(r, float(((bad["dq"] - ref["dq"]).abs() / b["dq"].clamp_min(1e-300)).max()))
    kd = (bad["kn"] - ref["kn"]).abs()
    return max(r, float((kd / b["kn"].clamp_min(1e-300)).max()) if float(kd.max()) > 0 else 0.0)


def faults_of(c):
    d, _, _ = built(c)
    return [("drop_column", j) for j in d["seams"]] + [(f, None) for f in R.FAULTS if f != "drop_column"]


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_bounds_see_every_single_fault(c):
    assert len(EXCLUDED) <= len(R.FAULTS) and len(set(EXCLUDED)) == len(EXCLUDED)
    for fault in faults_of(c):
        if EXCLUDED.get(fault[0]) == R.case_id(c):
            continue
        r = fault_ratio(c, fault)
        SENS[fault[0]] = min(SENS.get(fault[0], math.inf), r)
        assert r > R.FAULT_FACTOR, f"{R.case_id(c)}: fault {fault} moves no output by more than {R.FAULT_FACTOR} bounds (worst {r:.3g})"


def test_zz_sensitivity_table():
    """Printed record (run with -s): the smallest fault / bound ratio per fault over all cases."""
    assert set(SENS) == set(R.FAULTS)
    for f in R.FAULTS:
        print(f"[sensitivity] {f}: smallest fault / bound {SENS[f]:.3g}")
    finite = [v for v in SENS.values() if math.isfinite(v)]
    print(f"[sensitivity] smallest over all faults and cases: {min(finite):.3g}")
    assert min(SENS.values()) > R.FAULT_FACTOR


def test_bounds_are_small_against_the_outputs():
    """Guards the bounds themselves against growing useless: the loss bound stays below 2e-3 of the loss's own scale (log K + 1 / T),
    and the dq bound of an element below 1e-2 of the largest element of its row, on every case."""
    for c in R.CASES:
        _, ref, b = built(c)
        assert float(b["loss"]) < 2e-3 * (math.log(c.K + 1) + 1 / c.T)
        assert bool((b["dq"].max(1).values < 1e-2 * ref["dq"].abs().max(1).values).all()), R.case_id(c)
        assert bool((b["kn"] <= (R.cdiv(c.D, 256) + 10) * R.U * ref["kn"].abs()).all())


# ------------------------------------------------------------------------------------------------
# the launcher's geometry and workspace
# ------------------------------------------------------------------------------------------------
def lib():
    from cmunet_amd import _lib
    return _lib.lib()


def test_cases_sit_on_the_branches_they_are_named_for():
    assert R.moco_splits(8, 4) == (1, 32) and R.seam_columns(8, 4) == [0, 3]
    dq4 = lambda D: ((D + 3) // 4 + 1) & ~1
    assert dq4(5) == 2 and 3 * dq4(5) >= 5                            # wave 3 gets no rows
    assert 70 % 4 != 0 and 3 * dq4(70) < 70 < 4 * dq4(70) and 28 < 128  # the last wave's quarter is ragged
    assert R.moco_splits(130, 396) == (13, 32) and 396 - 12 * 32 == 12 and 396 - 3 * 128 == 12 and 33 - 32 == 1 and 130 - 128 == 2
    assert R.moco_splits(64, 16416) == (257, 64) and 16416 - 256 * 64 == 32
    assert R.moco_splits(1024, 4096) == (64, 64)
    assert R.seam_columns(64, 16416) == [0, 3, 4, 63, 64, 127, 128, 16412, 16415]
    assert R.seam_columns(72, 260) == [0, 3, 4, 31, 32, 127, 128, 256, 259]


def test_workspace_layout_equals_the_library_s():
    l = lib()
    shapes = {(c.B, c.D, c.K) for c in R.CASES} | {(40, 64, 1024), (8, 128, 512), (2, 1, 4), (256, 2048, 65536), (31, 129, 33)}
    for B, D, K in shapes:
        assert l.cmu_moco_ws_bytes(B, D, K) == R.ws_bytes(B, D, K), (B, D, K)
        sec = R.ws_sections(B, D, K)
        assert [n for n, _ in sec] == ["bar", "qn", "kn", "qnT", "rowst", "L", "slab"] and all(n % 64 == 0 for _, n in sec)
    for bad in ((0, 8, 4), (1, 0, 4), (1, 8, 0), (-1, 8, 4), (1, -8, 4), (1, 8, -4)):
        assert l.cmu_moco_ws_bytes(*bad) == -1


def test_argument_refusals():
    """CMU_CHECK_ARG returns before any HIP call and before any pointer is read: dummy non-null addresses are enough."""
    l = lib()
    ok = 1 << 20                                                       # 16-byte aligned, never dereferenced
    P = ctypes.c_void_p

    def call(B, D, K, T, keys=None, Nk=0, queue=ok, ws=ok):
        return l.cmu_moco_infonce_enqueue(P(ok), P(ok), keys, Nk, P(queue), P(ok), P(ok), P(ok), P(ok), B, D, K, T, P(ws), None)

    def refused(rc, word):
        assert rc == -1, rc                                            # CMU_ERR_ARG
        assert word in l.cmu_last_error().decode(), l.cmu_last_error().decode()

    refused(call(1, 8, 6, 0.2), "K %")                                 # K % 4 != 0
    refused(call(2, 8, 6, 0.2, P(ok), 2), "K %")                       # ... gathered
    refused(call(7, 70, 36, 0.2), "multiple")                          # K % Nk != 0 (the issue's (7, 70, 36))
    refused(call(5, 72, 260, 0.2, P(ok), 8), "multiple")               # ... of the gathered batch
    refused(call(1, 8, 4, 0.0), "bad args")                            # temperature <= 0
    refused(call(1, 8, 4, -0.07), "bad args")
    refused(call(1, 8, 4, 0.2, queue=ok + 4), "aligned")               # a queue that is not 16-byte aligned
    refused(call(1, 8, 4, 0.2, queue=ok + 8), "aligned")
    refused(call(1, 8, 4, 0.2, ws=ok + 4), "aligned")
    refused(call(0, 8, 4, 0.2), "bad args")
