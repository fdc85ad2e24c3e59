"""The memory contract of a workspace-taking entry point, and the harness that holds a call to it.

A library function that takes a byte workspace of ``cmu_*_ws_bytes`` bytes promises four things:
  1. every workspace byte it reads was written in this call (nothing depends on what the buffer held before);
  2. no store lands behind ``ws_bytes`` (or in front of the buffer);
  3. every element of every output is written;
  4. nothing is written outside the outputs, and no input is modified.

``guarded`` makes buffers whose neighbourhood can be inspected, ``check_call`` runs one call in the three workspace states
``STATES`` and asserts the four rules plus the entry's own reference check.  The module is plain torch: it works on CPU tensors
(tests/test_cpu_mem_contract.py proves, on small torch stand-ins, that each single fault is seen) and on the GPU
(tests/test_gpu_mem_contract.py holds the table of entry points).

Conditions, not measurements: a guard is ``GUARD`` = 4096 bytes of ``GUARD_BYTE`` = 0xA5 on either side of the payload, inside
the same allocation.  A store further than 4 KiB from the payload is outside what this harness sees.  (0xA5A5A5A5 read as a float
is -2.9e-16: a kernel that READS the guard is not seen by its value; over-reads are caught where the workspace is larger than
what the call writes, through rule 1.)
"""
import torch

GUARD = 4096
GUARD_BYTE = 0xA5
STATES = ("zero", "ff", "leftover")

# float outputs start as a NaN with a payload that arithmetic does not produce, so "never written" (these exact bits) can be told
# from "written with a NaN that came out of a stale workspace slot"
_NAN_BITS = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.float64: (torch.int64, 0x7FF80000DEADBEEF),
             torch.float16: (torch.int16, 0x7EAD), torch.bfloat16: (torch.int16, 0x7FED)}


def _nbytes(nbytes_or_shape, dtype):
    if isinstance(nbytes_or_shape, int):
        return nbytes_or_shape, None
    shape = tuple(int(s) for s in nbytes_or_shape)
    n = 1
    for s in shape:
        n *= s
    return n * torch.empty((), dtype=dtype).element_size(), shape


def guarded(nbytes_or_shape, dtype=torch.uint8, fill=0, device="cpu"):
    """One uint8 allocation [GUARD x 0xA5 | payload | GUARD x 0xA5]; -> the payload as a ``dtype`` view (flat for a byte count,
    shaped for a shape).  The payload starts GUARD bytes into a torch allocation (so it is 16-byte aligned) and its last byte
    directly abuts the rear guard: no rounding.  ``fill``: "nan" (the marked NaN of a float dtype), an int 0..255 for uint8
    payloads / a value of ``dtype`` otherwise, or a uint8 tensor of bytes, repeated or cut to the payload's length.
    The view keeps its parent (``guards_intact`` needs it); views OF the view do not."""
    n, shape = _nbytes(nbytes_or_shape, dtype)
    parent = torch.full((GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device)
    raw = parent[GUARD:GUARD + n]
    view = raw.view(dtype) if dtype != torch.uint8 else raw
    if isinstance(fill, torch.Tensor):
        src = fill.reshape(-1).view(torch.uint8).to(device)
        assert src.numel() > 0
        raw.copy_(src.repeat(-(-n // src.numel()))[:n] if src.numel() < n else src[:n])
    elif isinstance(fill, str):
        assert fill == "nan" and dtype in _NAN_BITS, (fill, dtype)
        idt, bits = _NAN_BITS[dtype]
        raw.view(idt).fill_(bits)
    else:
        view.fill_(fill)
    if shape is not None:
        view = view.view(shape)
    view._mc_parent, view._mc_nbytes = parent, n
    return view


def guards_intact(view):
    """None if both guards of a ``guarded`` view hold 0xA5 everywhere; else the offset of the first damaged byte: >= 0 counted from
    the payload's END (0 = the byte directly behind it), < 0 counted from the payload's START (-1 = the byte directly in front)."""
    parent, n = view._mc_parent, view._mc_nbytes
    rear = (parent[GUARD + n:] != GUARD_BYTE).nonzero()
    if rear.numel():
        return int(rear[0])
    front = (parent[:GUARD] != GUARD_BYTE).nonzero()
    if front.numel():
        return int(front[-1]) - GUARD
    return None


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().clone()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a, b)


def _first_diff(a, b, itemsize):
    d = (a != b).nonzero()
    return int(d[0]) // itemsize if d.numel() else -1


class Out:
    """One output of a case.  ``prefill``: "nan" for float outputs (every element must be overwritten), or a value the op cannot
    produce for integer outputs (0xFF for 0 / 1 masks and class maps, -1 for labels and counts) -- an element that still holds it after
    the call was never written.  ``accumulates``: the op documents that it adds into this output (or leaves it alone under a
    condition the case states in ``why``): the prefill is then finite, the "never written" test does not apply and the entry's
    reference is adjusted by the prefill.  ``marks_unwritten`` False (with ``why``): no prefill can mark an unwritten element -- every byte
    value is a legitimate output, or the buffer has padding the op documents as untouched; the guards, the bit comparison across
    states and the reference still apply."""

    def __init__(self, shape, dtype=torch.float32, prefill="nan", accumulates=False, why="", marks_unwritten=True):
        assert not (accumulates or not marks_unwritten) or why, "an accumulated output states the documented condition"
        self.shape, self.dtype, self.prefill, self.accumulates, self.why = tuple(shape), dtype, prefill, accumulates, why
        self.marks_unwritten = marks_unwritten and not accumulates


class Case:
    """What ``check_call`` needs to know about one call: ``ws_bytes`` (what the entry's size function reports: the guard abuts exactly
    that), the outputs (name -> Out), the inputs (name -> tensor; cloned and compared byte for byte), further leftover sources
    (name -> uint8 tensor: the bytes another call left in a workspace this entry shares), and what the record line tells."""

    def __init__(self, name, ws_bytes, outs, inputs, device="cpu", dtype="f32", blocks=0, capped=False, leftovers=None, min_ws=0, aux_ws=None):
        self.name, self.ws_bytes, self.outs, self.inputs, self.device = name, int(ws_bytes), outs, inputs, device
        self.dtype, self.blocks, self.capped, self.leftovers = dtype, blocks, capped, dict(leftovers or {})
        self.min_ws = min_ws      # payload bytes passed where ws_bytes is 0 (a 1-byte payload, as the wrapper passes)
        self.aux_ws = dict(aux_ws or {})    # further workspaces of the call (name -> bytes): guarded, in the same state, handed to run() as outs["ws:<name>"]


RECORDS = []


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _run_once(entry, case, run, state, ws_fill, aux_fill):
    dev = case.device
    ws = guarded(max(case.ws_bytes, case.min_ws), torch.uint8, ws_fill, dev)
    outs = {k: guarded(o.shape, o.dtype, o.prefill, dev) for k, o in case.outs.items()}
    aux = {"ws:" + k: guarded(n, torch.uint8, aux_fill[k] if isinstance(aux_fill, dict) else aux_fill, dev) for k, n in case.aux_ws.items()}
    before = {k: bits(t) for k, t in case.inputs.items()}
    tag = f"{entry} [{case.name}] state '{state}'"
    _sync(dev)
    run(ws, {**outs, **aux})
    _sync(dev)
    for name, t, n in [("workspace", ws, case.ws_bytes)] + [(f"workspace '{k[3:]}'", t, t.numel()) for k, t in aux.items()]:
        bad = guards_intact(t)
        if bad is not None:
            where = f"{bad} bytes behind ws_bytes = {n}" if bad >= 0 else f"{-bad} bytes in front of the workspace"
            raise AssertionError(f"{tag}: store outside the {name}, first damaged guard byte {where}")
    for k, t in outs.items():
        bad = guards_intact(t)
        if bad is not None:
            where = f"{bad} bytes behind its end" if bad >= 0 else f"{-bad} bytes in front of it"
            raise AssertionError(f"{tag}: store outside output '{k}', first damaged guard byte {where}")
    for k, t in case.inputs.items():
        now = bits(t)
        if not same_bits(now, before[k]):
            raise AssertionError(f"{tag}: input '{k}' was modified, first at element {_first_diff(now, before[k], t.element_size())}")
    for k, t in outs.items():
        o = case.outs[k]
        if not o.marks_unwritten:
            continue
        pre = bits(guarded(o.shape, o.dtype, o.prefill, "cpu"))
        es = t.element_size()
        left = (bits(t).view(-1, es) == pre.view(-1, es)).all(dim=1).nonzero()
        if left.numel():
            raise AssertionError(f"{tag}: output '{k}' never written at {left.numel()} of {t.numel()} elements, first at flat index "
                                 f"{int(left[0])} (it still holds its prefill)")
    return ws, outs, aux


def check_call(entry, case, run, reference_check):
    """Runs ``run(ws, outs)`` on fresh guarded buffers with the workspace all zero, all zero again, all 0xFF, and holding leftover
    bytes: those the "zero" run of this very case left, then each of ``case.leftovers``.  After every run: the guards of the workspace
    and of every output are intact, every input has its bytes, no output element holds its prefill, the outputs have the bits of
    the first run (the second "zero" run shows that the entry is bit-stable, so a difference in a later state is the workspace's),
    and ``reference_check(outs)`` passes (it may return its worst err / bound).  -> the record, with ``ws_after``: the bytes this
    case's "zero" run left (the "leftover" source of the entry's smaller cases)."""
    states = [("zero", 0), ("zero again", 0), ("ff", 0xFF), ("leftover", None)] + [(f"leftover:{k}", v) for k, v in case.leftovers.items()]
    first, ws_after, aux_after, worst = None, None, None, 0.0
    for state, fill in states:
        if fill is None:
            fill = ws_after
        if isinstance(fill, torch.Tensor) and fill.numel() == 0:
            fill = 0xFF
        ws, outs, aux = _run_once(entry, case, run, state, fill, aux_after if isinstance(fill, torch.Tensor) else fill)
        now = {k: bits(t) for k, t in outs.items()}
        if first is None:
            first, ws_after, aux_after = now, ws.clone(), {k[3:]: t.clone() for k, t in aux.items()}
        else:
            for k in now:
                if not same_bits(now[k], first[k]):
                    i = _first_diff(now[k], first[k], outs[k].element_size())
                    a, b = outs[k].reshape(-1)[i].item(), None
                    if state == "zero again":
                        raise AssertionError(f"{entry} [{case.name}]: output '{k}' is not bit-stable: two runs on a zeroed workspace differ, "
                                             f"first at flat index {i} (second run {a!r})")
                    raise AssertionError(f"{entry} [{case.name}]: output '{k}' depends on what the workspace held before the call: state "
                                         f"'{state}' differs from 'zero', first at flat index {i} (got {a!r}); a slot the final pass reads "
                                         f"was not written in this call")
        r = reference_check(outs)
        worst = max(worst, float(r) if r is not None else 0.0)
    rec = {"entry": entry, "case": case.name, "dtype": case.dtype, "ws_bytes": case.ws_bytes, "blocks": case.blocks, "capped": case.capped,
           "states": [s for s, _ in states], "worst": worst, "ws_after": ws_after}
    RECORDS.append(rec)
    print(f"[memcontract] {format_record(rec)}")
    return rec


def format_record(r):
    return (f"{r['entry']:<34} {r['case']:<30} {r['dtype']:<5} ws_bytes {r['ws_bytes']:>9}  workgroups {r['blocks']:>6}"
            f"{' (cap)' if r['capped'] else '      '}  states {','.join(r['states'])}  worst err/bound {r['worst']:.3g}")
