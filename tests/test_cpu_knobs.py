"""CPU suite: the library's dispatch knobs -- every environment variable libcmunet_hip.so reads -- sit in ONE table behind ONE reader
(csrc/common.h CMU_KNOBS, csrc/elementwise.hip cmu_knob).  Checked through the host-only entry points cmu_dispatch_knob_name /
cmu_get_dispatch_knob / cmu_set_dispatch_override on the library that test_cpu_abi builds: names, defaults, how each kind parses its
variable, the override, the single getenv in the sources and the list in tools/README.md.  No GPU call anywhere."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ON = ["CMU_CONV_NARROW", "CMU_CONV_SLIM", "CMU_CONV_PERSIST_PART", "CMU_WGRAD_SQUARE", "CMU_WGRAD_WIDE_F32", "CMU_CONV_V5", "CMU_CONV_PERSIST",
      "CMU_CONV_WRES", "CMU_CONV_BUFLOAD", "CMU_SPARK_GATHER", "CMU_CONVT_SMALL", "CMU_CONVT_GEMM", "CMU_WGR_VEC", "CMU_WGRAD_WIDE",
      "CMU_WGRAD_SWAP", "CMU_WGT2_NX256"]
OPTIN = ["CMU_CONV_V6"]
NUM = {"CMU_CONV_WIDE": 1, "CMU_CONV_PERSIST_GRID": 0, "CMU_GATHER_NB": 0, "CMU_CONVT_SMALL_STEPS": 4, "CMU_V5_MIN_K": 128,
       "CMU_V5_MIN_K_BST": 256, "CMU_V6_MAX_N": 128, "CMU_V6_MAX_N_K128": 64, "CMU_SKF_WGS": 768, "CMU_WGRAD_BLOCKS1": 512,
       "CMU_WGRAD_BLOCKS": 256}
FLOOR8 = ("CMU_WGRAD_BLOCKS1", "CMU_WGRAD_BLOCKS")   # values below 8 fall back to the default
DEFAULTS = {**{k: 1 for k in ON}, **{k: 0 for k in OPTIN}, **NUM}
CMU_ERR_ARG = -1


def expected(name, text):
    """The value of knob `name` when its variable holds `text` (None: unset), by the three rules of the table."""
    if text is None:
        return DEFAULTS[name]
    if name in ON:
        return 0 if text.startswith("0") else 1
    if name in OPTIN:
        return 1 if text.startswith("1") else 0
    n = int(text)
    return DEFAULTS[name] if name in FLOOR8 and n < 8 else n


def knob_names(l):
    names = []
    while l.cmu_dispatch_knob_name(len(names)) is not None:
        names.append(l.cmu_dispatch_knob_name(len(names)).decode())
        assert len(names) < 1000
    return names


def get(l, name):
    v, d = ctypes.c_int(-7), ctypes.c_int(-7)
    assert l.cmu_get_dispatch_knob(name.encode(), ctypes.byref(v), ctypes.byref(d)) == 0, name
    return v.value, d.value


@pytest.fixture(scope="module")
def l():
    from cmunet_amd import _lib
    _lib.build()
    return _lib.lib()


_CHILD = r'''
import ctypes, json, sys
sys.path.insert(0, %r)
from cmunet_amd import _lib
l = _lib.lib()
out, i = {}, 0
while l.cmu_dispatch_knob_name(i) is not None:
    name = l.cmu_dispatch_knob_name(i)
    v, d = ctypes.c_int(-7), ctypes.c_int(-7)
    assert l.cmu_get_dispatch_knob(name, ctypes.byref(v), ctypes.byref(d)) == 0
    out[name.decode()] = [v.value, d.value]
    i += 1
print("KNOBS " + json.dumps(out))
''' % ROOT


def child_values(text):
    """{knob: [value, default]} of a fresh process in which every knob's variable holds `text` (None: no CMU_* variable at all)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CMU_")}
    if text is not None:
        env.update({k: text for k in DEFAULTS})
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("KNOBS ")][-1][6:])


def test_knob_names_are_the_28_documented_ones(l):
    names = knob_names(l)
    assert len(names) == len(set(names)) and len(DEFAULTS) == len(ON) + len(OPTIN) + len(NUM) == 28
    assert sorted(names) == sorted(DEFAULTS)
    assert l.cmu_dispatch_knob_name(-1) is None and l.cmu_dispatch_knob_name(len(names)) is None


def test_defaults_with_the_environment_unset(l):
    got = child_values(None)
    assert got == {k: [d, d] for k, d in DEFAULTS.items()}


@pytest.mark.parametrize("text", ["0", "1", "2", "64"])
def test_each_kind_parses_its_variable(l, text):
    got = child_values(text)
    assert got == {k: [expected(k, text), DEFAULTS[k]] for k in DEFAULTS}


def test_override_reaches_every_kind_and_refuses_bad_values(l):
    s = l.cmu_set_dispatch_override
    for name, forced in (("CMU_WGRAD_WIDE", 0), ("CMU_V5_MIN_K", 64)):   # a formerly lambda-only switch, a number
        before = get(l, name)
        assert s(name.encode(), forced) == 0
        assert get(l, name) == (forced, DEFAULTS[name])
        assert s(name.encode(), -1) == 0
        assert get(l, name) == before
    assert s(b"CMU_WGRAD_WIDE", 2) == CMU_ERR_ARG and get(l, "CMU_WGRAD_WIDE")[0] in (0, 1)
    assert s(b"CMU_CONV_V6", 2) == CMU_ERR_ARG
    assert s(b"CMU_V5_MIN_K", -2) == CMU_ERR_ARG
    assert s(b"CMU_NO_SUCH_KNOB", 0) == CMU_ERR_ARG
    v, d = ctypes.c_int(), ctypes.c_int()
    assert l.cmu_get_dispatch_knob(b"CMU_NO_SUCH_KNOB", ctypes.byref(v), ctypes.byref(d)) == CMU_ERR_ARG


def test_sources_read_the_environment_in_one_place():
    files = [f for ext in ("hip", "inc", "h") for f in glob.glob(os.path.join(ROOT, "cmunet_amd", "csrc", "*." + ext))]
    hits = [(os.path.basename(f), n + 1) for f in files for n, ln in enumerate(open(f)) for _ in range(ln.count("getenv("))]
    assert len(hits) == 1, hits


def test_readme_table_lists_the_library_knobs(l):
    text = open(os.path.join(ROOT, "tools", "README.md")).read()
    section = text.split("## Dispatch knobs of the library", 1)[1].split("\n## ", 1)[0]
    rows = re.findall(r"^\| `(CMU_\w+)` \|", section, flags=re.M)
    assert len(rows) == len(set(rows))
    assert set(rows) == set(knob_names(l))
