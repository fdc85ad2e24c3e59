"""CPU suite: the C-ABI library builds for gfx950 without a GPU, loads, and exports every symbol that
include/cmunet_hip.h declares with the arity the ctypes binding assumes (no compute calls here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_prototypes():
    src = open(os.path.join(ROOT, "include", "cmunet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"(?:int64_t|int|const char\*)\s+(cmu_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        n = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
        protos[m.group(1)] = n
    return protos


def test_library_builds_loads_and_exports_header():
    from cmunet_amd import _lib
    _lib.build()
    assert os.path.exists(_lib.LIB_PATH)
    protos = header_prototypes()
    assert len(protos) >= 40
    assert _lib.missing_symbols() == []
    assert set(protos) == set(_lib.EXPORTS), set(protos) ^ set(_lib.EXPORTS)
    for name, n in protos.items():
        assert len(_lib._SIGS[name][1]) == n, f"{name}: header has {n} args, binding {len(_lib._SIGS[name][1])}"
    l = _lib.lib()
    assert l.cmu_version() >= 100
    assert [l.cmu_dtype_size(i) for i in (0, 1, 2, 3)] == [4, 2, 2, 0]
    # pure host-side queries (no GPU needed)
    assert l.cmu_conv_ntiles(32, 512, 512) == 32 * 32 * 32
    assert l.cmu_pack_conv3x3_elems(64, 64, 2, 0) == 2 * 9 * 64 * 32
    assert l.cmu_conv3x3_wgrad_ws_bytes(32, 512, 512, 64, 64, 2) > 0


def test_binding_types_of_a_pinned_sample():
    """The binding is parsed from the header; these signatures are written out by hand (they are the rows of the table the parser replaced),
    one for every C type the header uses: an int where the header says int64_t, or a float where it says double, fails here."""
    import ctypes
    from cmunet_amd import _lib
    P, I, L, F, D, U64, S = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_uint64, ctypes.c_char_p)
    pinned = {
        "cmu_adam_step": (I, [P, P, P, P, P, L, F, F, F, F, F, I, L, F, P, P]),
        "cmu_two_view": (I, [P, I, I, P, P, U64, P, P, I, P]),
        "cmu_philox_normal": (I, [P, L, U64, U64, P]),
        "cmu_genesis_sample": (I, [P, P, P, I, I, I, I, I, D, D, D, D, D, U64, U64, P]),
        "cmu_hist_curves": (I, [P, P, I, I, D, D, I, P, P, P, P]),
        "cmu_pack_batch": (I, [P, I, L, I, P]),
        "cmu_set_dispatch_override": (I, [S, I]),
        "cmu_dispatch_knob_name": (S, [I]),
        "cmu_last_error": (S, []),
        "cmu_seg_stats_ws_bytes": (L, [I]),
        "cmu_pointwise_loss_ws_bytes": (L, []),
        "cmu_lamb_step": (I, [P, P, P, P, P, P, P, P, I, P, P, I, F, F, F, F, I, I, F, I, I, L, F, P, P]),
    }
    for name, sig in pinned.items():
        assert _lib._SIGS[name] == sig, (name, _lib._SIGS[name])
    assert all(isinstance(a, list) and (r in (I, L, S)) for r, a in _lib._SIGS.values())


SYNTHETIC_HEADER = """
/* a block comment with int cmu_in_comment(size_t n); over
   two lines */
#ifndef X_H
#define X_H
extern "C" {
typedef enum { CMU_A = 0, CMU_B = 5 } cmu_kind;
#define CMU_NEG (-3)     /* trailing comment */
#define CMU_POS 7        // another
#define CMU_NOT_INT 1.5
int cmu_none(void);
const char* cmu_name();   // int cmu_in_line_comment(unsigned n);
int64_t cmu_many(const float* const* tables, int16_t *q,
                 int64_t n, uint64_t seed,
                 float a, double b, const char* tag, const int flag,
                 void* stream);
}
#endif
"""


def test_header_parser_on_synthetic_text():
    import ctypes
    from cmunet_amd import _lib
    P, I = ctypes.c_void_p, ctypes.c_int
    sigs, consts = _lib._parse_header(SYNTHETIC_HEADER)
    assert sigs == {"cmu_none": (I, []), "cmu_name": (ctypes.c_char_p, []),
                    "cmu_many": (ctypes.c_int64, [P, P, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double, ctypes.c_char_p, I, P])}
    assert consts == {"CMU_A": 0, "CMU_B": 5, "CMU_NEG": -3, "CMU_POS": 7}


@pytest.mark.parametrize("proto", ["int cmu_bad(size_t n);", "int cmu_bad(const float* x, unsigned n);", "int cmu_bad(CmuRec rec);",
                                   "void cmu_bad(int n);", "double cmu_bad(void);", "unsigned cmu_bad(void);",
                                   "int cmu_bad(int (*callback)(int));", "static inline int cmu_ok(void) { return cmu_bad(1); }"])
def test_header_parser_refuses_what_it_cannot_type(proto):
    """An unknown parameter type, an unlisted return type, and a cmu_ function that is no plain prototype all raise, naming the function."""
    from cmunet_amd import _lib
    with pytest.raises(_lib.CmuError, match="cmu_bad"):
        _lib._parse_header("int cmu_ok_before(int n);\n" + proto + "\nint cmu_ok_after(void);\n")


def test_constants_come_from_the_header():
    from cmunet_amd import _lib, ops
    h = open(os.path.join(ROOT, "include", "cmunet_hip.h")).read()
    defines = {n: int(v) for n, v in re.findall(r"^#define (CMU_\w+) \(?(-?\d+)\)?", h, flags=re.M)}
    assert len(defines) == 21
    enum = {"CMU_F32": 0, "CMU_F16": 1, "CMU_BF16": 2}
    assert "typedef enum { CMU_F32 = 0, CMU_F16 = 1, CMU_BF16 = 2 } cmu_dtype;" in h
    assert _lib.CONST == {**defines, **enum}
    C = _lib.CONST
    assert (C["CMU_OK"], C["CMU_ERR_ARG"], C["CMU_ERR_UNSUPPORTED"], C["CMU_ERR_WORKSPACE"], C["CMU_ERR_LAUNCH"]) == (0, -1, -2, -3, -4)
    assert C["CMU_PWL_MAX_C"] == 8 and C["CMU_HIST_MAX_BINS"] == 1024 and C["CMU_HIST_MAX_K"] == 8 and C["CMU_PRE_MAX_RADIUS"] == 16
    assert (_lib.F32, _lib.F16, _lib.BF16) == (0, 1, 2)
    assert ops.PWL_KINDS == {"l1": 0, "mse": 1, "bce": 2, "bce_with_logits": 3} and ops.PWL_MAX_C == 8
    assert (ops.PRE_MAX_RADIUS, ops.HIST_MAX_K, ops.HIST_MAX_BINS) == (16, 8, 1024)


def test_workspace_helper_calls_the_named_size_query():
    import torch
    from cmunet_amd import _lib, ops
    _lib.build()
    ws = ops.workspace("cmu_seg_stats_ws_bytes", "cpu", 3)
    assert ws.dtype == torch.uint8 and ws.device.type == "cpu" and ws.shape == (_lib.lib().cmu_seg_stats_ws_bytes(3),) and ws.numel() > 0
    assert ops.workspace("cmu_soft_skeleton_save_ws_bytes", "cpu", 1000, 3).numel() == _lib.lib().cmu_soft_skeleton_save_ws_bytes(1000, 3)
    for name in ("cmu_version", "cmu_pack_desc_bytes", "cmu_nothing_ws_bytes", "cmu_seg_stats"):
        with pytest.raises(_lib.CmuError, match=name):
            ops.workspace(name, "cpu", 3)


def test_product_has_no_cpu_fallback():
    import torch
    from cmunet_amd import model as M
    m = M.UNet(base_ch=16, depth=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 16, 16))
    # and nothing in the product package imports the oracle
    pkg = os.path.join(ROOT, "cmunet_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, fn)).read().replace("the oracle", ""), fn


def test_state_dict_names_match_reference_layout(golden_dir):
    import numpy as np
    from cmunet_amd import model as M
    f = np.load(f"{golden_dir}/unet_full.npz")
    m = M.UNet()
    assert list(m.state_dict().keys()) == [str(k) for k in f["state_keys"]]
    assert [str(tuple(v.shape)) for v in m.state_dict().values()] == [str(s) for s in f["state_shapes"]]


def test_lr_schedule_and_mask_device_free_logic():
    from cmunet_amd.pretrain import cosine_warmup_lr
    assert abs(cosine_warmup_lr(1.0, 0, 40, 300) - 1e-4) < 1e-12
    assert abs(cosine_warmup_lr(1.0, 40, 40, 300) - 1.0) < 1e-12
    assert cosine_warmup_lr(1.0, 300, 40, 300) < 1e-12


def test_call_refuses_tensors_on_different_devices():
    """Device binding of the C-ABI launches: pointers carry their device; a call mixing two devices is refused
    before anything is launched (checked here without a GPU, with hand-made device pointers)."""
    from cmunet_amd import _lib
    a, b = _lib.devptr(0x1000, 0), _lib.devptr(0x2000, 1)
    with pytest.raises(_lib.CmuError, match="different devices"):
        _lib.call("cmu_ema_update", a, b, 16, 0.5, _lib.STREAM)
    assert isinstance(a, __import__("ctypes").c_void_p) and a.dev == 0 and a.value == 0x1000


def test_bench_self_launch_propagates_rank_failure():
    """`python bench.py --gpus 2` without a launcher starts its own two ranks and never touches the GPU itself; here (no GPU)
    both ranks fail at start-up: the parent must come back promptly with a non-zero status, not hang or re-exec."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert '"metric"' not in r.stdout


def test_bench_refuses_zero_timed_steps():
    """ms_per_step is the time of one of the --steps timed steps: a run without any is refused before anything starts."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, r.stderr
    assert '"metric"' not in r.stdout


def test_conv_igemm5_kernels_use_no_scratch(tmp_path):
    """csrc/conv_igemm5.inc issues its weight / halo loads through inline asm with hand-placed s_waitcnt: hipcc does not know those registers
    are in flight, so a register SPILL right behind such a load would store (and later reload) bytes that have not arrived yet -- it happened
    once in round 5 (21 spilled registers in the data-gradient form: the halo chunks across its epilogue).  The kernels must therefore
    allocate no scratch at all: checked on the code object inside the built library (kernel descriptors' private_segment_fixed_size)."""
    import re
    import shutil
    import subprocess
    lib = os.path.join(ROOT, "cmunet_amd", "csrc", "libcmunet_hip.so")
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(lib) or not all(os.path.exists(t) for t in tools):
        pytest.skip("library or LLVM tools not present")
    fat = str(tmp_path / "fat.bin")
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fat}", lib], check=True)
    blob = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    assert starts, "no offload bundle in .hip_fatbin"
    found = {}
    for i, a in enumerate(starts):
        part = str(tmp_path / f"b{i}.bin")
        open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = str(tmp_path / f"co{i}.o")
        r = subprocess.run([tools[1], "--unbundle", "--type=o", f"--input={part}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                           capture_output=True, text=True)
        if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        notes = subprocess.run([tools[2], "--notes", co], capture_output=True, text=True).stdout
        # AMDGPU metadata (YAML): per kernel a block with .name and .private_segment_fixed_size
        for blk in notes.split("- .agpr_count")[1:]:
            nm = re.search(r"\.name:\s+(\S+)", blk)
            ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if nm and ps and ("conv_igemm5_kernel" in nm.group(1) or "conv_igemm6_kernel" in nm.group(1)):
                found[nm.group(1)] = int(ps.group(1))
    n5 = sum("conv_igemm5_kernel" in k for k in found)
    n6 = sum("conv_igemm6_kernel" in k for k in found)
    assert n5 == 6, f"expected the six conv_igemm5_kernel instantiations (f16 / bf16 x transform / plain / data-gradient), found {sorted(found)}"
    assert n6 == 4, f"expected the four conv_igemm6_kernel instantiations (round 6: f16 / bf16 x transform / plain; same asm-load discipline), found {sorted(found)}"
    assert all(v == 0 for v in found.values()), f"a conv_igemm5 / conv_igemm6 kernel allocates scratch (a spill behind an asm load is a wrong result): {found}"


def test_asm_load_kernels_keep_their_mfma_phase_clean(tmp_path):
    """Advisor, round 5: conv_igemm5 / conv_igemm6 issue weight and halo loads through inline asm and wait for them with hand-placed
    ``s_waitcnt vmcnt(N)`` -- hipcc believes the destination registers are complete when the asm statement ends, so a ``v_mov`` / ``v_accvgpr``
    copy of one of them (or a spill) scheduled in front of the wait would read bytes that have not arrived, and the N of the first wait of a
    position counts the epilogue's 16 stores.  Nothing in the source can assert that; the DISASSEMBLY of the built library can: between
    ``s_setprio 2`` and ``s_setprio 0`` (the MFMA phase) every instantiation holds exactly its MFMAs (288 per position; conv_igemm6 runs a pair:
    576), its weight loads (4 per tap) and LDS fragment reads -- no register copies, no scratch --, and the whole kernel stores its tile with
    exactly 16 ``global_store_dwordx4`` (fewer would make the counted waits too loose)."""
    import re
    import subprocess
    from collections import Counter
    lib = os.path.join(ROOT, "cmunet_amd", "csrc", "libcmunet_hip.so")
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")]
    if not os.path.exists(lib) or not all(os.path.exists(t) for t in tools):
        pytest.skip("library or LLVM tools not present")
    fat = str(tmp_path / "fat.bin")
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fat}", lib], check=True)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    seen = {}
    for i, a in enumerate(starts):
        part = str(tmp_path / f"b{i}.bin")
        open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = str(tmp_path / f"co{i}.o")
        r = subprocess.run([tools[1], "--unbundle", "--type=o", f"--input={part}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                           capture_output=True, text=True)
        if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        syms = subprocess.run([tools[2], "-s", "-W", co], capture_output=True, text=True).stdout
        names = sorted({w for ln in syms.splitlines() for w in ln.split()[-1:] if re.match(r"_Z18conv_igemm[56]_kernel", w) and not w.endswith(".kd")})
        if not names:
            continue
        dis = subprocess.run([tools[3], "-d", "--mcpu=gfx950", "--disassemble-symbols=" + ",".join(names), co], capture_output=True, text=True).stdout
        cur = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
            if m:
                cur = m.group(1)
                seen[cur] = []
            elif cur is not None:
                t = re.sub(r"//.*", "", ln).strip()
                if t and not t.endswith(":"):
                    seen[cur].append(t)
    assert len(seen) == 10, sorted(seen)
    for name, ins in seen.items():
        v6 = "conv_igemm6" in name
        phase, phases = None, []
        for t in ins:
            if t.startswith("s_setprio 2"):
                phase = []
            elif t.startswith("s_setprio 0"):
                if phase is not None:
                    phases.append(phase)
                phase = None
            elif phase is not None:
                phase.append(t.split()[0])
        assert len(phases) == 1, (name, len(phases))
        c = Counter(phases[0])
        assert sum(v for k, v in c.items() if k.startswith("v_mfma")) == (576 if v6 else 288), (name, c)
        assert c.get("buffer_load_dwordx4", 0) == (72 if v6 else 36), (name, c)
        bad = [k for k in c if k.startswith(("v_mov", "v_accvgpr", "v_pk_mov", "scratch_", "v_swap", "v_perm"))]
        assert not bad, f"{name}: register copies / scratch inside the MFMA phase (a copy of an asm-load destination in front of its wait reads stale bytes): {bad}"
        allc = Counter(t.split()[0] for t in ins)
        assert allc.get("global_store_dwordx4", 0) == 16, (name, allc.get("global_store_dwordx4", 0))
        assert not any(k.startswith("scratch_") for k in allc), name


def test_docs_state_the_header_entry_point_count():
    """One number for the C-ABI's size in README / DESIGN / INTEGRATION (round-5 review: 130 / 138 / 131 in three places): the count of functions
    declared in include/cmunet_hip.h -- which test_library_builds_loads_and_exports_header holds equal to the library's exports."""
    import re
    h = open(os.path.join(ROOT, "include", "cmunet_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    h = re.sub(r"//[^\n]*", "", h)
    n = len(set(re.findall(r"\b(cmu_\w+)\s*\(", h)))
    for doc, pat in (("README.md", r"(\d+) entry points"), ("DESIGN.md", r"(\d+) `extern \"C\"` entry points"), ("INTEGRATION.md", r"all (\d+) entry")):
        m = re.search(pat, open(os.path.join(ROOT, doc)).read(), flags=re.S)
        assert m is not None, f"{doc}: no entry-point count found ({pat})"
        assert int(m.group(1)) == n, f"{doc} says {m.group(1)} entry points, include/cmunet_hip.h declares {n}"
