"""The harness of tests/mem_contract.py is proved before it is trusted: ``check_call`` runs on CPU tensors against small torch stand-ins
of a two-pass reduction (each "workgroup" writes one float slot of the workspace, a final pass adds ``nblocks`` of them).  The correct
stand-in passes; every stand-in with ONE fault fails, with the message that names that fault.

The rest needs no GPU either: the table of tests/test_gpu_mem_contract.py accounts for every ``*_ws_bytes`` function of the library
exactly once (a new workspace-taking kernel fails here until it is entered), and every size function is positive at the table's shapes
and does not shrink when one size argument grows to the table's larger shape."""
import pytest
import torch

import mem_contract as MC
from mem_contract import GUARD, Case, Out, check_call

N, NBLOCKS, CAP = 37, 5, 8        # 37 values in blocks of 8 (the last one holds 5); the size function reserves CAP slots


def make_case(fault=None):
    x = torch.randn(N, generator=torch.Generator().manual_seed(1))
    if fault == "slot never written":
        x[24:32] = 0.0        # block 3 has nothing to add (an empty tile, an empty list) and skips its store: right on zeroed memory only
    return x, Case("5 blocks of 8 slots", CAP * 4, {"sums": Out((2,))}, {"x": x})


def reference_check(x):
    def check(outs):
        ref = torch.stack([x.double().sum(), (x.double() ** 2).sum()])
        err = (outs["sums"].double() - ref).abs()
        assert bool(torch.isfinite(outs["sums"]).all()), "sums: non-finite values"
        bound = 64 * 2.0 ** -24 * torch.stack([x.abs().sum(), (x * x).sum()]).double()
        assert bool((err <= bound).all()), f"sums: {outs['sums'].tolist()} against {ref.tolist()}"
        return float((err / bound).max())
    return check


def two_pass(x, fault=None):
    """-> run(ws, outs).  Slots: [0, NBLOCKS) sums, [CAP ... ) unused; the sums of squares are recomputed by the final pass."""
    def raw(t, lo, hi):     # bytes [lo, hi) relative to the payload's start: what a kernel's raw pointer reaches
        return t._mc_parent[GUARD + lo:GUARD + hi]

    def run(ws, outs):
        slot = ws.view(torch.float32)
        for b in range(NBLOCKS):
            part = x[8 * b:8 * b + 8].sum()
            if fault == "slot never written" and b == 3:
                continue
            if fault == "accumulates into its slot" and b == 0:       # "+=" where "=" was meant, behind a NaN guard
                part = part + (slot[0] if bool(torch.isfinite(slot[0])) else 0.0)
            slot[b] = part
        n = NBLOCKS + 1 if fault == "final reads nblocks + 1" else NBLOCKS
        outs["sums"][0] = slot[:n].sum()
        if fault != "last output element never written":
            outs["sums"][1] = (x * x).sum()
        if fault == "float behind the workspace":
            raw(ws, CAP * 4, CAP * 4 + 4).copy_(torch.tensor([1.0]).view(torch.uint8))
        if fault == "byte in front of the workspace":
            raw(ws, -1, 0).fill_(0)
        if fault == "element behind an output":
            raw(outs["sums"], 8, 12).copy_(torch.tensor([1.0]).view(torch.uint8))
        if fault == "input modified":
            x[N - 1] += 1.0
            x[N - 1] -= 1.0
            x[0] = -x[0]
    return run


def test_guarded_layout():
    t = MC.guarded((3, 5), torch.float32, "nan")
    p = t._mc_parent
    assert p.numel() == 2 * GUARD + 60 and t.data_ptr() == p.data_ptr() + GUARD and t.data_ptr() % 16 == 0
    assert bool((p[:GUARD] == 0xA5).all()) and bool((p[GUARD + 60:] == 0xA5).all()) and bool(torch.isnan(t).all())
    assert MC.guards_intact(t) is None
    p[GUARD + 60 + 7] = 0
    assert MC.guards_intact(t) == 7
    t = MC.guarded(13, torch.uint8, 0xFF)
    assert t.numel() == 13 and bool((t == 0xFF).all()) and bool((t.view(torch.int8) == -1).all())
    t._mc_parent[GUARD - 3] = 1
    assert MC.guards_intact(t) == -3
    t = MC.guarded(10, torch.uint8, torch.tensor([1, 2, 3], dtype=torch.uint8))
    assert t.tolist() == [1, 2, 3, 1, 2, 3, 1, 2, 3, 1] and MC.guards_intact(t) is None
    assert bool((MC.guarded((4,), torch.int32, -1) == -1).all())
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        assert bool(torch.isnan(MC.guarded((3,), dt, "nan")).all())


def test_correct_stand_in_passes():
    x, case = make_case()
    rec = check_call("two_pass", case, two_pass(x), reference_check(x))
    assert rec["states"] == ["zero", "zero again", "ff", "leftover"] and 0 < rec["worst"] <= 1
    assert rec["ws_after"].numel() == CAP * 4 and "two_pass" in MC.format_record(rec)


FAULTS = [
    ("slot never written", r"state 'ff'.*depends on what the workspace held|depends on what the workspace held.*state 'ff'"),
    ("final reads nblocks + 1", r"depends on what the workspace held.*state 'ff'"),
    ("float behind the workspace", r"store outside the workspace.*0 bytes behind ws_bytes = 32"),
    ("byte in front of the workspace", r"store outside the workspace.*1 bytes in front"),
    ("element behind an output", r"store outside output 'sums'.*0 bytes behind its end"),
    ("last output element never written", r"output 'sums' never written at 1 of 2 elements, first at flat index 1"),
    ("input modified", r"input 'x' was modified, first at element 0"),
    ("accumulates into its slot", r"depends on what the workspace held.*state 'leftover'"),
]


@pytest.mark.parametrize("fault,message", FAULTS, ids=[f[0] for f in FAULTS])
def test_single_fault_is_caught(fault, message):
    x, case = make_case(fault)
    with pytest.raises(AssertionError, match=message):
        check_call("two_pass", case, two_pass(x, fault), reference_check(x))


def test_unstable_entry_is_named():
    """An entry whose bits change from run to run is reported as that, not as a workspace dependence."""
    x, case = make_case()
    calls = []

    def run(ws, outs):
        two_pass(x)(ws, outs)
        calls.append(1)
        outs["sums"][0] += 1e-3 * len(calls)
    with pytest.raises(AssertionError, match="not bit-stable"):
        check_call("two_pass", case, run, lambda outs: None)


def test_accumulated_output_keeps_a_finite_prefill():
    x, _ = make_case()
    case = Case("dW += ", CAP * 4, {"sums": Out((2,), prefill=0.25, accumulates=True, why="the stand-in adds into it")}, {"x": x})

    def run(ws, outs):
        outs["sums"][0] += x.sum()
    check_call("accumulate", case, run, lambda outs: float(outs["sums"][1] != 0.25))
    with pytest.raises(AssertionError, match="documented condition"):
        Out((2,), prefill=0.0, accumulates=True)


# ---- the table: coverage and size functions ------------------------------------------------------------------------------------------
def table():
    import test_gpu_mem_contract as T
    return T


def test_every_ws_bytes_function_is_accounted_for_once():
    from cmunet_amd import _lib
    T = table()
    names = sorted(n for n in _lib._SIGS if n.endswith("_ws_bytes"))
    assert len(names) == len(set(T.COVERED)) + len(set(T.ELSEWHERE)), (len(names), len(T.COVERED), len(T.ELSEWHERE))
    for n in names:
        where = (n in T.COVERED) + (n in T.ELSEWHERE)
        assert where == 1, f"{n}: entered {where} times in COVERED / ELSEWHERE of tests/test_gpu_mem_contract.py (a workspace-taking kernel is held to the memory contract there)"
    assert not (set(T.COVERED) | set(T.ELSEWHERE)) - set(names)
    assert len(T.COVERED) == 29 and sorted(T.ELSEWHERE) == ["cmu_conv3x3_wgrad_ws_bytes", "cmu_convT2x2_wgrad_ws_bytes", "cmu_moco_ws_bytes"]
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    for n, files in T.ELSEWHERE.items():
        for f in files:
            assert n in open(os.path.join(here, f)).read(), f"{f} does not call {n}"
    for n, c in T.COVERED.items():
        assert c["entries"], n
        for e in c["entries"]:
            assert callable(getattr(T, "test_" + e, None)), f"{n}: no test_{e} in tests/test_gpu_mem_contract.py"


def test_size_functions_are_positive_and_do_not_shrink():
    from cmunet_amd import _lib
    T = table()
    l = _lib.lib()
    for n, c in T.COVERED.items():
        fn = getattr(l, n)
        nargs = len(_lib._SIGS[n][1])
        for small, large in c["sizes"]:
            assert len(small) == len(large) == nargs, (n, small, large)
            a, b = fn(*small), fn(*large)
            assert a > 0 and b > 0, f"{n}{small} = {a}, {n}{large} = {b}"
            assert b >= a, f"{n}: {small} -> {a} bytes, {large} -> {b} bytes"
            for i in range(nargs):
                if i in c.get("not_sizes", ()) or small[i] == large[i]:
                    continue
                grown = tuple(large[j] if j == i else small[j] for j in range(nargs))
                g = fn(*grown)
                assert g >= a, f"{n}: {small} -> {a} bytes, but {grown} -> {g} bytes (argument {i} grew)"
                assert b >= g, f"{n}: {grown} -> {g} bytes, but {large} -> {b} bytes"
    assert l.cmu_contour_points_ws_bytes(1, 1, 1) == 0      # the one documented zero: the 1 x 1 mask (the test passes a 1-byte payload there)
