"""ctypes binding of libcmunet_hip.so (the C-ABI declared in include/cmunet_hip.h).

The product path has no CPU fallback: if the HIP library is missing (or a call fails) this module
raises.  ``build()`` compiles it in-tree with hipcc for gfx950 (works without a GPU).
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("CMU_LIB_PATH") or os.path.join(CSRC, "libcmunet_hip.so")   # CMU_LIB_PATH: diagnostic builds (tools/)


class CmuError(RuntimeError):
    pass


_SCALAR = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double}
_RETURN = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}


def _ctype(decl, name):
    """The ctypes type of one parameter declaration (``const float* const* ptrs`` -> c_void_p); its name and ``const`` are dropped."""
    tok = decl.replace("*", " * ").split()
    if len(tok) > 1 and re.fullmatch(r"[A-Za-z_]\w*", tok[-1]) and tok[-1] not in _SCALAR:
        tok.pop()                       # the parameter's name
    if "*" in tok:
        return ctypes.c_char_p if tok == ["const", "char", "*"] else ctypes.c_void_p
    t = " ".join(w for w in tok if w != "const")
    if t not in _SCALAR:
        raise CmuError(f"{name}: no ctypes mapping for the parameter {decl.strip()!r}")
    return _SCALAR[t]


def _parse_header(text):
    """``(sigs, consts)`` of a C header: ``sigs`` maps every ``cmu_*`` prototype to ``(restype, [argtypes])``, ``consts`` holds the
    integer ``#define CMU_*`` values and the enumerators.  A prototype whose types are not in the maps above, or a ``cmu_*(`` that is
    not a prototype this parser understands, raises: a function skipped in silence would be called unbound or untyped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    declared = set(re.findall(r"\b(cmu_\w+)\s*\(", text))
    consts = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CMU_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
        consts.update((n, int(v)) for n, v in re.findall(r"(\w+)\s*=\s*(-?\d+)", body))
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    sigs = {}
    for stmt in text.split(";"):
        m = re.search(r"\b(cmu_\w+)\s*\(([^()]*)\)\s*$", stmt)
        if m is None:
            continue
        name, params = m.group(1), m.group(2).strip()
        ret = " ".join(re.split(r"[{}]", stmt[:m.start()])[-1].replace("*", " * ").split())
        if ret not in _RETURN:
            raise CmuError(f"{name}: no ctypes mapping for the return type {ret!r}")
        sigs[name] = (_RETURN[ret], [] if params in ("", "void") else [_ctype(p, name) for p in params.split(",")])
    if declared != set(sigs):
        raise CmuError(f"not parsed as prototypes: {sorted(declared ^ set(sigs))}")
    return sigs, consts


# name -> (restype, argtypes) and the CMU_* constants, read from include/cmunet_hip.h (the header csrc/common.h includes): a new
# entry point needs its prototype there, its definition in csrc/ and its wrapper in ops.py, and nothing here.
with open(os.path.join(_HERE, os.pardir, "include", "cmunet_hip.h")) as _f:
    _SIGS, CONST = _parse_header(_f.read())

EXPORTS = tuple(_SIGS.keys())
F32, F16, BF16 = CONST["CMU_F32"], CONST["CMU_F16"], CONST["CMU_BF16"]


def build(verbose=False):
    """Compile csrc/*.hip into libcmunet_hip.so with hipcc --offload-arch=gfx950 (in-tree)."""
    jobs = str(min(8, os.cpu_count() or 1))
    res = subprocess.run(["make", "-C", CSRC, "-j", jobs], capture_output=not verbose, text=True)
    if res.returncode != 0:
        raise CmuError("building libcmunet_hip.so failed:\n" + (res.stdout or "") + (res.stderr or ""))
    return LIB_PATH


_lib = None


def lib():
    """The loaded library (raises if it has not been built: there is no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CmuError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). The HIP path has no CPU fallback.")
        # PyTorch-ROCm bundles its own libamdhip64: import it FIRST so that this library binds to the same
        # HIP runtime instance as torch's streams/allocator (loading ours first leaves two runtimes in the
        # process and every launch fails with "no ROCm-capable device is detected").
        import torch  # noqa: F401
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name, None)
            if fn is None:      # reported by missing_symbols(); calling it raises below
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def missing_symbols():
    """Entry points declared in include/cmunet_hip.h that the built library does not export."""
    l = lib()
    return [n for n in _SIGS if getattr(l, n, None) is None]


class EventProfiler:
    """Optional per-entry-point timing with HIP events on the launch stream (bench.py's roofline leg).
    ``work`` is the algorithmic FLOP (or byte) count the caller attributes to the launch."""

    def __init__(self, gemm_only=False):
        self.records = []      # (name, start_event, end_event, work, kernel tag)
        self.gemm_only = gemm_only   # time only the GEMM-shaped entries (work > 0): a quarter of the events of a step

    def summary(self):
        import torch
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, work, _ in self.records:
            d = out.setdefault(name, {"ms": 0.0, "calls": 0, "work": 0.0})
            d["ms"] += e0.elapsed_time(e1)
            d["calls"] += 1
            d["work"] += work
        return out

    def by_kernel(self):
        """The MFMA entries (work > 0) grouped by the compute kernel that served them (cmu_last_kernel)."""
        import torch
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, work, tag in self.records:
            if work <= 0 or not tag:
                continue
            d = out.setdefault(tag, {"ms": 0.0, "calls": 0, "work": 0.0, "entries": set()})
            d["ms"] += e0.elapsed_time(e1)
            d["calls"] += 1
            d["work"] += work
            d["entries"].add(name)
        return out


PROFILER = None


class DevPtr(ctypes.c_void_p):
    """A device pointer that remembers which GPU owns it (``dev``): ``call`` binds the launch to that device."""


class _StreamOfArgs:
    """Placeholder for "the current stream of the device that owns this call's tensors" (resolved inside ``call``)."""


STREAM = _StreamOfArgs()


def devptr(addr, dev):
    p = DevPtr(addr)
    p.dev = dev
    return p


def call(name, *args, work=0.0):
    """Call an int-returning entry point; raise CmuError with cmu_last_error() on failure.

    Device binding: every ``DevPtr`` argument must live on ONE device; the launch is issued with that device current and on
    that device's current PyTorch stream (the ``STREAM`` placeholder), whatever the process's current device is -- a model on
    ``cuda:1`` (the reference's own choice, Finetuning/train.py:246,451) runs there, not on device 0's stream."""
    l = lib()
    fn = getattr(l, name, None)
    if fn is None:
        raise CmuError(f"{name} is not exported by {LIB_PATH}")
    import torch
    dev, si = None, -1
    for i, a in enumerate(args):
        if type(a) is DevPtr:
            if dev is None:
                dev = a.dev
            elif a.dev != dev:
                raise CmuError(f"{name}: tensors on different devices (cuda:{dev} and cuda:{a.dev})")
        elif a is STREAM:
            si = i
    cur = torch.cuda.current_device()
    if dev is None:
        dev = cur
    if si >= 0:
        args = list(args)
        args[si] = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if dev != cur:
        with torch.cuda.device(dev):
            return _call_bound(l, fn, name, args, work)
    return _call_bound(l, fn, name, args, work)


def _call_bound(l, fn, name, args, work):
    if PROFILER is not None and (work > 0 or not PROFILER.gemm_only):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        PROFILER.records.append((name, e0, e1, work, l.cmu_last_kernel().decode() if work > 0 else ""))
    else:
        rc = fn(*args)
    if rc != 0:
        raise CmuError(f"{name} failed ({rc}): {l.cmu_last_error().decode()}")
    return rc
