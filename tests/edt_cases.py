"""The case list of the distance-transform tests (tests/test_cpu_edt_ref.py, tests/test_gpu_edt.py): uint8 maps, built once.
Binary cases hold 0 / 1; ``labels3`` holds the classes 0..2."""
import functools

import numpy as np

# every tile / workgroup span of csrc/edt.hip, with the sizes one below, at and one above it
SPANS = {
    # the column pass runs 64 columns per workgroup; the row pass sizes its workgroup to the width rounded up to 64, 256 at the most,
    # and a thread then takes pixels x, x + 256, ...
    "W": {63: "64 (column workgroup, one-wave row workgroup)", 64: "64", 65: "64",
          127: "128 (row workgroup of two waves)", 128: "128", 129: "128",
          191: "192 (row workgroup of three waves)", 192: "192", 193: "192",
          255: "256 (the largest row workgroup: beyond it a thread takes a second pixel)", 256: "256", 257: "256",
          513: "512 (a third pixel per thread)"},
    # the column sweeps are unrolled by 8 rows
    "H": {7: "8 (unrolled column sweep)", 8: "8", 9: "8", 17: "16"},
    # the surface reductions run 1024 threads per image over the H * W pixels
    "HW": {(31, 33): "1024 (reduction workgroup)", (32, 32): "1024", (25, 41): "1024", (33, 63): "2048"},
}


def _rand(shape, density, seed):
    return (np.random.RandomState(seed).rand(*shape) < density).astype(np.uint8)


def vessel_like(H=475, W=475, strokes=14, steps=420, seed=7):
    """Random-walk strokes of width 1..3: thin, branching, gapped -- the shape of a vessel mask."""
    rs = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    for _ in range(strokes):
        y, x = rs.randint(0, H), rs.randint(0, W)
        ang, w = rs.rand() * 2 * np.pi, rs.randint(1, 4)
        for _ in range(steps):
            ang += rs.randn() * 0.25
            y, x = y + np.sin(ang) * 1.2, x + np.cos(ang) * 1.2
            iy, ix = int(round(y)), int(round(x))
            if not (0 <= iy < H and 0 <= ix < W):
                break
            if rs.rand() < 0.97:      # (a gap now and then)
                m[max(iy - w // 2, 0):iy + (w + 1) // 2, max(ix - w // 2, 0):ix + (w + 1) // 2] = 1
    return m


CORNERS_SHAPE = (70, 131)
CORNER_SITES = ((0, 0), (0, 130), (69, 0), (69, 130), (35, 65))


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["1x1_0"] = np.zeros((1, 1), np.uint8)
    c["1x1_1"] = np.ones((1, 1), np.uint8)
    c["strip_1x37"] = _rand((1, 37), 0.2, 1)
    c["strip_41x1"] = _rand((41, 1), 0.2, 2)
    for k, (y, x) in enumerate(CORNER_SITES):
        m = np.zeros(CORNERS_SHAPE, np.uint8)
        m[y, x] = 1
        c[f"one_site_{k}"] = m
    c["all_sites"] = np.ones(CORNERS_SHAPE, np.uint8)
    c["no_sites"] = np.zeros(CORNERS_SHAPE, np.uint8)
    m = np.zeros((20, 9), np.uint8)
    m[7, 3] = m[15, 3] = 1
    c["one_column"] = m                    # every column but one holds the sentinel
    m = np.zeros((40, 30), np.uint8)
    m[:5] = _rand((5, 30), 0.3, 3)
    c["row_band"] = m                      # rows 5..39 hold no site
    m = np.zeros((9, 9), np.uint8)
    m[4, 1] = m[4, 7] = m[0, 4] = 1
    c["ties"] = m                          # (4,4) is 9 from two sites, (2,4) is 4 from ... several equal minima
    yy, xx = np.mgrid[0:17, 0:19]
    c["checker"] = ((yy + xx) % 2).astype(np.uint8)
    for shape in ((33, 65), (64, 64), (65, 257)):
        for d in (0.02, 0.5, 0.98):
            c[f"rand_{shape[0]}x{shape[1]}_{d}"] = _rand(shape, d, 10 + int(d * 100) + shape[1])
    for W in SPANS["W"]:
        c[f"w{W}"] = _rand((5, W), 0.03, 100 + W)
    for H in SPANS["H"]:
        c[f"h{H}"] = _rand((H, 21), 0.1, 200 + H)
    for H, W in SPANS["HW"]:
        c[f"hw{H}x{W}"] = _rand((H, W), 0.3, 300 + W)
    c["labels3"] = np.random.RandomState(5).randint(0, 3, (40, 52)).astype(np.uint8)
    blob = np.zeros((48, 61), np.uint8)      # solid shapes: borders with an inside, one of them leaving the frame
    blob[5:20, 6:30] = 1
    blob[30:48, 40:61] = 1
    yy, xx = np.mgrid[0:48, 0:61]
    blob[(yy - 30) ** 2 + (xx - 15) ** 2 <= 64] = 1
    c["blobs"] = blob
    c["vessel_475"] = vessel_like()
    return c


LARGE = ("vessel_475",)
SMALL = tuple(k for k in cases() if k not in LARGE)
RADII = (0, 1, 1.5, 2, 2.5, 5)


def gap_map():
    """A three-class map: class 1 is a vessel broken by a gap of two pixels, with a speck; class 2 a plate with a notch."""
    m = np.zeros((24, 40), np.uint8)
    m[10:12, 2:17] = 1
    m[10:12, 19:36] = 1          # the gap: columns 17, 18
    m[3, 30] = 1                 # a speck an opening of radius 1 removes
    m[16:23, 5:30] = 2
    m[16:19, 14:16] = 0          # a notch of width 2 that a closing of radius 1.5 fills
    return m
