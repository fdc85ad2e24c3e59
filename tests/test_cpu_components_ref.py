"""CPU suite for the connected-component clean-up (cmunet_amd/postprocess.py, csrc/components.hip):
  * tests/components_ref.py (the numpy reference of the GPU tests) against scipy.ndimage;
  * the find / union / canonical-label functions of csrc/components_uf.h -- the very code the kernels call -- built into a stand-alone
    host program (tools/components_host_check.cpp) with the host sanitizers and run over the whole case list;
  * the argument validation of infer.Segmenter's clean-up options and the command line's flags, without a GPU.
Everything is an integer: every comparison is exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import components_cases as C
import components_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy_canonical(mask, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, n = ndi.label(mask, structure=np.ones((3, 3), int) if connectivity == 8 else None)
    out = np.zeros(mask.shape, np.int32)
    if n:
        idx = np.arange(mask.size).reshape(mask.shape)
        first = ndi.minimum(idx, lab, np.arange(1, n + 1)).astype(np.int64)      # smallest row-major index per component
        out = np.where(lab > 0, first[np.maximum(lab, 1) - 1] + 1, 0).astype(np.int32)
    return out, n


@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_labelling_is_scipys_relabelled(connectivity):
    pytest.importorskip("scipy")
    for name, mask in C.cases().items():
        lab, n = C.ref_label(name, connectivity)
        want, wn = _scipy_canonical(mask, connectivity)
        assert n == wn, name
        assert np.array_equal(lab, want), name
        sizes = R.component_sizes(lab)
        assert sizes.sum() == int(mask.sum()) and np.array_equal(np.flatnonzero(sizes.ravel()) + 1, np.unique(lab[lab > 0])), name


def test_reference_counts_of_the_designed_cases():
    """What the designed cases are for: the counts a correct labelling must give."""
    n = lambda name, conn: C.ref_label(name, conn)[1]
    assert (n("corner_diag", 8), n("corner_diag", 4)) == (1, 2)
    assert (n("corner_anti", 8), n("corner_anti", 4)) == (1, 2)
    assert (n("corner_both", 8), n("corner_both", 4)) == (1, 1)
    assert (n("checker_66", 8), n("checker_66", 4)) == (1, 66 * 66 // 2)
    for name in ("serpentine_96", "spiral_96", "comb", "all_fg", "ring"):
        assert (n(name, 8), n(name, 4)) == (1, 1), name
    assert n("all_bg", 8) == 0 and n("1x1_fg", 4) == 1 and n("1x1_bg", 4) == 0
    assert C.cases()["spiral_96"].sum() > 96 * 96 // 3 and C.cases()["serpentine_96"].sum() > 96 * 96 // 2


def test_reference_fill_holes_is_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    filled_something = 0
    for name in C.SMALL:
        mask = C.cases()[name]
        got = R.fill_holes(mask)
        assert np.array_equal(got, ndi.binary_fill_holes(mask)), name
        filled_something += int(got.sum() > mask.sum())
    assert filled_something >= 8
    assert np.array_equal(R.fill_holes(C.cases()["open_ring"]), C.cases()["open_ring"] > 0)          # open to the frame: not filled
    d = C.cases()["diag_closed"]
    assert R.fill_holes(d).sum() > d.sum() and R.label(d, 4)[1] > 1 and R.label(d, 8)[1] == 1       # closed only diagonally: filled


def test_reference_largest_ties_min_size_and_clean_mask():
    m = np.zeros((8, 20), np.uint8)
    m[1, 1:5] = 1            # size 4, label 22
    m[3, 10:14] = 1          # size 4, label 71
    m[6, 2:5] = 1            # size 3
    lab, _ = R.label(m, 8)
    sizes = R.component_sizes(lab)
    assert R.select_largest(sizes, 1) == [22] and R.select_largest(sizes, 3) == [22, 71, 123] and R.select_largest(sizes, 5)[3:] == [-1, -1]
    assert R.keep_largest(m, 1).sum() == 4 and R.keep_largest(m, 1)[1, 1]                           # the tie goes to the smaller label
    assert R.remove_small_objects(m, 4).sum() == 8 and R.remove_small_objects(m, 3).sum() == 11 and R.remove_small_objects(m, 5).sum() == 0
    # multi-class: cleaning class 2 leaves class 1 alone; the table is applied at the end
    k3 = np.zeros((12, 12), np.uint8)
    k3[1:4, 1:4] = 1
    k3[6:11, 5:10] = 2
    k3[8, 7] = 1             # a class-1 pixel inside the class-2 square: a hole of class 2
    k3[0, 11] = 2            # a class-2 speck
    out = R.clean_mask(k3, classes=[2], min_size=2, fill_holes=True, class_values=[0, 100, 200])
    assert out[0, 11] == 0 and out[8, 7] == 200 and (out[1:4, 1:4] == 100).all() and (out[6:11, 5:10] == 200).all()
    assert np.array_equal(R.clean_mask(k3), k3) and R.clean_mask(k3, min_size=2, num_classes=3)[8, 7] == 0


def _compiler():
    """(command prefix, flags) of a host C++ compiler with the sanitizers, or None."""
    if shutil.which("g++"):
        return ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if shutil.which("hipcc"):
        return ["hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    return None


def test_host_program_runs_the_kernels_union_find_clean(tmp_path):
    """The stand-alone program labels every case with csrc/components_uf.h (tiles visited serially, pixels in a scrambled order) under
    AddressSanitizer + UBSan: exact labels and counts, no overrun flag, no sanitizer report."""
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "components_host_check")
    r = subprocess.run(cc + [os.path.join(ROOT, "tools", "components_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    jobs = [(name, conn) for name in C.cases() for conn in (4, 8)]
    # the same labelling must come out for a class index and for a complement (cls = 1, cls = -2 - 0) as for cls = -1
    extra = [("rand_0.59_0", 8, 1), ("nested_rings", 4, -2)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(jobs) + len(extra)).tobytes())
        for name, conn, cls in [(n, c, -1) for n, c in jobs] + extra:
            m = C.cases()[name]
            f.write(np.asarray([m.shape[0], m.shape[1], cls, conn], np.int32).tobytes())
            f.write(np.ascontiguousarray(m).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(dst, np.int32)
    o = 0
    for name, conn, cls in [(n, c, -1) for n, c in jobs] + extra:
        m = C.cases()[name]
        want, wn = C.ref_label(name, conn)
        assert raw[o] == wn, (name, conn, cls, int(raw[o]), wn)
        assert np.array_equal(raw[o + 1:o + 1 + m.size].reshape(m.shape), want), (name, conn, cls)
        o += 1 + m.size
    assert o == raw.size


def _tiny_model():
    from cmunet_amd import model as M
    return M.UNet(base_ch=16, depth=3)


def test_segmenter_validates_the_cleanup_options():
    from cmunet_amd.infer import Segmenter
    m = _tiny_model()
    s = Segmenter(m)
    assert (s.min_size, s.keep_largest, s.fill_holes, s.connectivity, s.post) == (None, None, False, 8, False)
    s = Segmenter(m, min_size=50, keep_largest=2, fill_holes=True, connectivity=4, class_values=[0, 255])
    assert (s.min_size, s.keep_largest, s.fill_holes, s.connectivity, s.post) == (50, 2, True, 4, True)
    assert Segmenter(m, min_size=0).post and Segmenter(m, keep_largest=8).post and Segmenter(m, fill_holes=True).post
    for kw in ({"min_size": -1}, {"min_size": 2.5}, {"keep_largest": 0}, {"keep_largest": 9}, {"keep_largest": 1.5}, {"fill_holes": 1},
               {"connectivity": 6}, {"connectivity": None}):
        with pytest.raises(ValueError, match="Segmenter: " + next(iter(kw))):
            Segmenter(m, **kw)


def test_postprocess_has_no_cpu_fallback_and_checks_arguments():
    import torch
    from cmunet_amd import metrics, postprocess as P
    z = torch.zeros(4, 4, dtype=torch.uint8)
    for fn in (lambda: P.label(z), lambda: P.component_sizes(z.int()), lambda: P.remove_small_objects(z, 2), lambda: P.keep_largest(z),
               lambda: P.fill_holes(z), lambda: P.clean_mask(z, min_size=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    for fn in (lambda: P.label(z, connectivity=6), lambda: P.keep_largest(z, n=0), lambda: P.keep_largest(z, n=9),
               lambda: P.remove_small_objects(z, -1), lambda: P.clean_mask(z, keep_largest=0), lambda: P.clean_mask(z, connectivity=5),
               lambda: P.clean_mask(z, class_values=[0, 256]), lambda: metrics.components(connectivity=6)):
        with pytest.raises(ValueError):
            fn()
    assert metrics.components().__name__ == "components"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.components()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))


def test_cli_knows_the_cleanup_flags(tmp_path):
    """The flags parse (the run then stops at the missing GPU or the missing model, after argparse); a bad value is argparse's exit 2."""
    from cmunet_amd import infer
    base = ["--model", str(tmp_path / "none.pth"), "--images", str(tmp_path), "--out", str(tmp_path / "o")]
    with pytest.raises((RuntimeError, FileNotFoundError)):
        infer.main(base + ["--min-size", "50", "--keep-largest", "2", "--fill-holes", "--connectivity", "4"])
    with pytest.raises(SystemExit) as e:
        infer.main(base + ["--connectivity", "6"])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        infer.main(base + ["--min-size", "many"])
