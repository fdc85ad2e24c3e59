"""CPU suite for the exact Euclidean distance transform, the disk morphology and the surface distances (cmunet_amd/postprocess.py,
cmunet_amd/metrics.py, csrc/edt.hip):
  * tests/edt_ref.py (the numpy reference of the GPU tests) against scipy.ndimage: the transform, the disk and border rules of the
    morphology, the border map;
  * the site rule, row-pass search, morphology select and rank selection of csrc/edt_scan.h -- the very code the kernels call -- built
    into a stand-alone host program (tools/edt_host_check.cpp) with the host sanitizers and run over the case list against brute force;
  * the argument validation of infer.Segmenter's opening / closing options and the command line's flags, without a GPU;
  * every new public function refuses a CPU tensor; clean_mask's reference with the new keywords at their defaults is unchanged.
Everything is an integer: every comparison is exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import components_cases as CC
import components_ref as CR
import edt_cases as C
import edt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ndi = pytest.importorskip("scipy.ndimage")


def test_brute_force_is_scipys_transform_squared():
    for name in C.SMALL:
        m = C.cases()[name]
        for sites in (m != 0, m == 0):
            if sites.size * int(sites.sum()) > R.BRUTE_LIMIT:
                continue
            got = R.dist2_brute(sites)
            if not sites.any():
                assert (got == -1).all(), name
                continue
            d = ndi.distance_transform_edt(~sites)
            assert np.array_equal(got, np.rint(d * d).astype(np.int32)), name
            assert np.array_equal(R.edt(got), d.astype(np.float32)), name      # float32(sqrt(float64(d2))) is scipy's root, rounded once
    big = C.cases()["vessel_475"]
    assert 2000 < int(big.sum()) < big.size // 4
    assert np.array_equal(R.squared_distance_transform(big, to="foreground"), R.dist2_scipy(big != 0))


def test_directions_and_rule_codes_of_the_reference():
    lab = C.cases()["labels3"]
    assert np.array_equal(R.squared_distance_transform(lab, -1, "background"), R.dist2_brute(lab == 0))
    assert np.array_equal(R.squared_distance_transform(lab, 2, "foreground"), R.dist2_brute(lab == 2))
    assert np.array_equal(R.squared_distance_transform(lab, 2, "background"), R.dist2_brute(lab != 2))
    assert np.array_equal(R.squared_distance_transform(lab, -2 - 1, "foreground"), R.dist2_brute(lab != 1))
    assert np.array_equal(R.squared_distance_transform(lab, -2 - 1, "background"), R.dist2_brute(lab == 1))
    d = ndi.distance_transform_edt(lab != 0)      # scipy's convention is to="background"
    assert np.array_equal(R.squared_distance_transform(lab), np.rint(d * d).astype(np.int32))


@pytest.mark.parametrize("radius", [r for r in C.RADII if r > 0] + [2.9])
def test_reference_morphology_is_scipys_with_the_disk_and_border_rules(radius):
    se = R.disk(radius)
    assert se[se.shape[0] // 2, se.shape[1] // 2] and se.sum() == sum(1 for y in range(-6, 7) for x in range(-6, 7) if y * y + x * x <= radius * radius)
    for name in C.SMALL:
        m = C.cases()[name]
        if m.size > 2500:
            continue
        fg = m != 0
        dil = ndi.binary_dilation(fg, structure=se, border_value=0)
        ero = ndi.binary_erosion(fg, structure=se, border_value=1)
        assert np.array_equal(R.binary_dilation(m, radius) != 0, dil), name
        assert np.array_equal(R.binary_erosion(m, radius) != 0, ero), name
        opened = ndi.binary_dilation(ero, structure=se, border_value=0)
        closed = ndi.binary_erosion(dil, structure=se, border_value=1)
        assert np.array_equal(R.binary_opening(m, radius) != 0, opened), name
        assert np.array_equal(R.binary_closing(m, radius) != 0, closed), name
        assert not (opened & ~fg).any() and not (fg & ~closed).any(), name      # anti-extensive / extensive
        # away from the frame the border rules do not matter: scipy's own opening / closing of the map in a wide zero margin
        if name not in ("blobs", "labels3", "checker", "ties", "rand_33x65_0.5"):
            continue
        P = 2 * int(radius) + 2
        pad = np.pad(m, P)
        assert np.array_equal((R.binary_opening(pad, radius) != 0), ndi.binary_opening(pad != 0, structure=se)), name
        assert np.array_equal((R.binary_closing(pad, radius) != 0), ndi.binary_closing(pad != 0, structure=se)), name


def test_reference_morphology_values_and_radius_zero():
    m = C.cases()["labels3"] * 7      # values 0, 7, 14
    for fn in (R.binary_dilation, R.binary_erosion, R.binary_opening, R.binary_closing):
        assert np.array_equal(fn(m, 0), m) and np.array_equal(fn(m, 0.9), m)
        out = fn(m, 1.5)
        assert np.array_equal(out[(out != 0) & (m != 0)], m[(out != 0) & (m != 0)])      # kept pixels keep their value
        assert set(np.unique(out[(m == 0)])) <= {0, 1}                                     # added ones become 1


def test_reference_border_and_surface_conventions():
    for name in ("blobs", "rand_33x65_0.5", "checker", "1x1_1", "all_sites"):
        m = C.cases()[name]
        fg = m > 0
        pad = np.pad(fg, 1)
        four = pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
        assert np.array_equal(R.border(m), fg & ~four), name
    a, b = C.cases()["blobs"], np.roll(C.cases()["blobs"], 3, 1)
    z = np.zeros_like(a)
    s = R.surface_distances(a, b)
    assert s["n_pr"] == int(R.border(a).sum()) and 0 < s["nsd"] < 1 and s["hd"] >= s["hd_percentile"] > 0
    pooled = np.sort(np.sqrt(np.hstack((s["d2_ab"], s["d2_ba"])).astype(np.float64)))
    assert s["hd"] == pooled[-1] and pooled[int(0.95 * (pooled.size - 1))] <= s["hd_percentile"] <= pooled[int(0.95 * (pooled.size - 1)) + 1]
    same = R.surface_distances(a, a)
    assert (same["hd"], same["assd"], same["nsd"]) == (0.0, 0.0, 1.0)
    e = R.surface_distances(z, z)
    assert (e["hd"], e["hd_percentile"], e["assd"], e["nsd"]) == (0.0, 0.0, 0.0, 1.0)
    for one in (R.surface_distances(a, z), R.surface_distances(z, a)):
        assert one["hd"] == one["hd_percentile"] == one["assd"] == float("inf") and one["nsd"] == 0.0


def test_reference_clean_mask_defaults_and_gap():
    for name in ("rand_0.59_0", "nested_rings"):
        m = CC.cases()[name]
        for kw in ({}, {"min_size": 4}, {"keep_largest": 2, "fill_holes": True, "connectivity": 4}):
            assert np.array_equal(R.clean_mask(m, **kw), CR.clean_mask(m, **kw)), (name, kw)
    g = C.gap_map()
    split = R.clean_mask(g, num_classes=3, keep_largest=1)
    joined = R.clean_mask(g, num_classes=3, keep_largest=1, closing=1.5)
    assert CR.label(g == 1, 8)[1] == 3 and not split[10, 5] and split[10, 25]              # the shorter half is deleted ...
    assert joined[10, 5] == 1 and joined[10, 25] == 1 and joined[10, 17] == 1 and joined[3, 30] == 0      # ... unless the gap is closed first
    assert (joined[16:19, 14:16] == 2).all() and (split[16:19, 14:16] == 0).all()
    opened = R.clean_mask(g, num_classes=3, opening=1)
    # the cross (radius 1) removes the speck and the two-pixel-wide vessel altogether, and shaves the plate's corners
    assert opened[3, 30] == 0 and not (opened == 1).any() and opened[20, 10] == 2 and opened[22, 5] == 0 and opened[22, 6] == 2


def _compiler():
    """(command prefix, flags) of a host C++ compiler with the sanitizers, or None."""
    if shutil.which("g++"):
        return ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if shutil.which("hipcc"):
        return ["hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    return None


def test_host_program_runs_the_kernels_search_clean(tmp_path):
    """The stand-alone program runs the two passes, the morphology select and the rank selection of csrc/edt_scan.h over the CPU case
    list under AddressSanitizer + UBSan and compares them with its own brute force; the outputs are compared with tests/edt_ref.py."""
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "edt_host_check")
    r = subprocess.run(cc + [os.path.join(ROOT, "tools", "edt_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    jobs = [(name, -1, 0, 2) for name in C.SMALL if C.cases()[name].size <= 6000]
    jobs += [(name, 0, 0, 6) for name in ("rand_33x65_0.5", "checker", "row_band", "1x1_1")]
    jobs += [("labels3", 2, 0, 1), ("labels3", -2 - 1, 0, 4), ("blobs", -1, 1, 2), ("rand_33x65_0.98", -1, 1, 25), ("labels3", 1, 1, 0)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(jobs)).tobytes())
        for name, cls, border, t in jobs:
            m = C.cases()[name]
            f.write(np.asarray([m.shape[0], m.shape[1], cls, border, t], np.int32).tobytes())
            f.write(np.ascontiguousarray(m).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(dst, np.uint8)
    o = 0
    for name, cls, border, t in jobs:
        m = C.cases()[name]
        n = m.size
        d2 = raw[o:o + 4 * n].view(np.int32).reshape(m.shape)
        ref = raw[o + 4 * n:o + 8 * n].view(np.int32).reshape(m.shape)
        dil = raw[o + 8 * n:o + 9 * n].reshape(m.shape)
        ero = raw[o + 9 * n:o + 10 * n].reshape(m.shape)
        o += 10 * n
        cnt = int(raw[o:o + 4].view(np.int32)[0])
        ranks = raw[o + 4:o + 16].view(np.int32)
        o += 16
        sites = R.rule(m, cls)
        if border:
            sites = R.border(sites)
        want = R.dist2_brute(sites)
        assert np.array_equal(d2, want) and np.array_equal(ref, want), (name, cls, border)
        hit = (want > 0) & (want <= t)
        assert np.array_equal(dil, np.where(hit, 1, m)), (name, cls, t)
        assert np.array_equal(ero, np.where((want != 0) & ~((want < 0) | (want > t)), 0, m)), (name, cls, t)
        vals = want.ravel().copy()
        vals[::3] = -2
        srt = np.sort(vals[vals >= 0])
        assert cnt == srt.size
        exp = [int(srt[k]) if 0 <= k < srt.size else -1 for k in (0, srt.size // 2, srt.size - 1)]
        assert list(ranks) == exp, (name, list(ranks), exp)
    assert o == raw.size


def _tiny_model():
    from cmunet_amd import model as M
    return M.UNet(base_ch=16, depth=3)


def test_segmenter_validates_opening_and_closing():
    from cmunet_amd.infer import Segmenter
    m = _tiny_model()
    s = Segmenter(m)
    assert (s.opening, s.closing, s.post) == (None, None, False)
    s = Segmenter(m, opening=1, closing=1.5)
    assert (s.opening, s.closing, s.post) == (1.0, 1.5, True)
    assert Segmenter(m, closing=0).post and Segmenter(m, opening=2.5).post and not Segmenter(m, connectivity=4).post
    for kw in ({"opening": -1}, {"closing": -0.5}, {"opening": "2"}, {"closing": float("nan")}, {"closing": float("inf")}, {"opening": True}):
        with pytest.raises(ValueError, match="Segmenter: " + next(iter(kw))):
            Segmenter(m, **kw)


def test_cli_knows_the_morphology_flags(tmp_path):
    from cmunet_amd import infer
    base = ["--model", str(tmp_path / "none.pth"), "--images", str(tmp_path), "--out", str(tmp_path / "o")]
    args = infer.build_parser().parse_args(base + ["--opening", "1", "--closing", "1.5"])
    assert (args.opening, args.closing) == (1.0, 1.5)
    assert infer.build_parser().parse_args(base).closing is None
    with pytest.raises((RuntimeError, FileNotFoundError)):
        infer.main(base + ["--closing", "1.5", "--keep-largest", "1"])
    with pytest.raises(SystemExit) as e:
        infer.main(base + ["--closing", "wide"])
    assert e.value.code == 2


def test_new_functions_have_no_cpu_fallback_and_check_arguments():
    import torch
    from cmunet_amd import metrics, ops, postprocess as P
    z = torch.zeros(4, 4, dtype=torch.uint8)
    calls = [lambda: P.squared_distance_transform(z), lambda: P.distance_transform_edt(z, to="foreground"), lambda: P.binary_dilation(z, 1),
             lambda: P.binary_erosion(z, 1.5), lambda: P.binary_opening(z, 2), lambda: P.binary_closing(z, 2), lambda: P.binary_closing(z, 0),
             lambda: P.clean_mask(z, closing=1.5), lambda: P.clean_mask(z, opening=1),
             lambda: metrics.surface_distances(z, z), lambda: ops.edt_columns(z[None]), lambda: ops.edt_rows(z[None].int()),
             lambda: ops.surface_border(z[None]), lambda: ops.surface_reduce(z[None], z[None].int()),
             lambda: ops.surface_select(z[None].int(), z[None].int(), torch.zeros(1, 1, dtype=torch.int32))]
    for k, fn in enumerate(calls):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    for cls in (metrics.HausdorffDistance95, metrics.AverageSurfaceDistance, metrics.SurfaceDice):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))
    assert (metrics.HausdorffDistance95().__name__, metrics.AverageSurfaceDistance().__name__, metrics.SurfaceDice(2.0).__name__) == \
        ("hd95", "assd", "surface_dice")
    assert metrics.HausdorffDistance95(percentile=90).percentile == 90 and metrics.SurfaceDice(2.0).tolerance == 2.0
    bad = [lambda: P.binary_dilation(z, -1), lambda: P.binary_closing(z, "2"), lambda: P.binary_opening(z, float("nan")),
           lambda: P.clean_mask(z, closing=-1), lambda: P.clean_mask(z, opening=float("inf")),
           lambda: P.squared_distance_transform(z, to="edge"), lambda: metrics.surface_distances(z, z, tolerance=-1),
           lambda: metrics.surface_distances(z, z, percentile=101), lambda: metrics.SurfaceDice(-1.0), lambda: metrics.HausdorffDistance95(percentile=120)]
    for fn in bad:
        with pytest.raises(ValueError):
            fn()
