#!/usr/bin/env python3
"""HIP-event timing of the exact Euclidean distance transform, the disk morphology and the surface distances (csrc/edt.hip,
cmunet_amd.postprocess, cmunet_amd.metrics).

(a) Pass level, --images masks of --side x --side (the reference's centre crop, 475):

      squared_distance_transform(mask, to="foreground") on four inputs, each the worst case of one shape of row pass:
        vessel_like   random-walk strokes: what the network predicts
        random_0.5    every scan ends after a step or two
        corner_site   one site in a corner: the outward scan of the far pixels runs nearly the whole row
        no_site       every scan runs the whole row and finds nothing
      binary_closing at radius 1.5 and at radius 8 on the vessel-like masks: the same launches, the radius is only a threshold
      surface_distances(mask, shifted mask)

    with the effective TB/s against each call's own byte model (bytes per pixel; reads served by a cache are counted once):
      squared_distance_transform  column pass: 1 read + 4 written going down, 4 read (+ up to 4 rewritten) coming up; row pass: 4 read
                                  + 4 written = 17 .. 21.  (A column pass that kept its column on chip would make it 13.)
      binary_closing              two transforms whose row pass writes a byte instead: 2 x (1 + 4 + 4 + 4 + 1 + 1) = 30 .. 38
      surface_distances           two transforms (17 .. 21 each) + two reductions (1 + 4 read, 4 written) + the rank selection, which
                                  re-reads both masked maps (8) once per bisection step: not a streaming pass, no byte model

(b) Whole call: Segmenter(UNet(out_classes=2, base 64, depth 5, f16), size=None, tile=256, stride=128).segment on --images images
    with closing=1.5 against the same call without it.

(c) With --host: scipy.ndimage.distance_transform_edt of ONE vessel-like mask on one host thread, for comparison.

Every figure is the median (with min and max) of --rounds windows after a warm-up; inside a round the cases are timed one after the
other (alternating), so drift of the card hits all of them alike.  Prints one JSON line per case.
    python tools/edt_bench.py [--rounds 7] [--out profiles/edt.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from predict_bench import stats, timed  # noqa: E402

BYTES = {"squared_distance_transform": (17, 21), "binary_closing": (30, 38)}


def vessel_like(n, side, seed=0, strokes=14, steps=420):
    """Random-walk strokes of width 1..3 with a gap now and then: thin, branching, broken -- the shape of a vessel mask."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, side, side), np.uint8)
    for m in out:
        for _ in range(strokes):
            y, x = rs.randint(0, side), rs.randint(0, side)
            ang, w = rs.rand() * 2 * np.pi, rs.randint(1, 4)
            for _ in range(steps):
                ang += rs.randn() * 0.25
                y, x = y + np.sin(ang) * 1.2, x + np.cos(ang) * 1.2
                iy, ix = int(round(y)), int(round(x))
                if not (0 <= iy < side and 0 <= ix < side):
                    break
                if rs.rand() < 0.97:
                    m[max(iy - w // 2, 0):iy + (w + 1) // 2, max(ix - w // 2, 0):ix + (w + 1) // 2] = 1
    return torch.from_numpy(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="windows per figure (at least 5)")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--side", type=int, default=475)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--host", action="store_true", help="also time scipy's transform of one mask on the host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    from cmunet_amd import infer, metrics, postprocess as P
    from cmunet_amd.model import UNet
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    lines = []
    n, s = a.images, a.side
    npix = n * s * s

    vessel = vessel_like(n, s).to(dev)
    corner = torch.zeros(n, s, s, dtype=torch.uint8)
    corner[:, 0, 0] = 1
    inputs = {"vessel_like": vessel, "random_0.5": (torch.rand(n, s, s, generator=g) < 0.5).to(torch.uint8).to(dev), "corner_site": corner.to(dev),
              "no_site": torch.zeros(n, s, s, dtype=torch.uint8, device=dev)}
    shifted = torch.roll(vessel, (2, -3), (1, 2)).contiguous()
    fns = {f"squared_distance_transform[{k}]": (lambda m=m: P.squared_distance_transform(m, to="foreground")) for k, m in inputs.items()}
    fns["binary_closing[r=1.5]"] = lambda: P.binary_closing(vessel, 1.5)
    fns["binary_closing[r=8]"] = lambda: P.binary_closing(vessel, 8)
    fns["surface_distances"] = lambda: metrics.surface_distances(vessel, shifted)
    for fn in fns.values():
        timed(fn, 3)
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, a.iters))
    st = {k: stats(v) for k, v in ms.items()}
    tbps = {}
    for k in fns:
        model = BYTES.get(k.split("[")[0])
        if model:
            tbps[k] = [round(b * npix / (st[k]["median"] * 1e-3) / 1e12, 3) for b in model]
    lines.append({"level": "pass", "shape": [n, s, s], "vessel_density": round(float(vessel.float().mean()), 4), "rounds": a.rounds, "iters": a.iters,
                  "launch": "eager", "ms": st, "ms_per_image": {k: round(v["median"] / n, 5) for k, v in st.items()},
                  "model_bytes_per_pixel": {k: list(v) for k, v in BYTES.items()}, "TBps_low_high": tbps,
                  "closing_r8_over_r1.5": stats([x / y for x, y in zip(ms["binary_closing[r=8]"], ms["binary_closing[r=1.5]"])])})
    print(json.dumps(lines[-1]), flush=True)

    if a.host:
        from scipy import ndimage as ndi
        m = vessel[0].cpu().numpy() == 0
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            ndi.distance_transform_edt(m)
            ts.append((time.perf_counter() - t0) * 1e3)
        lines.append({"level": "host", "what": "scipy.ndimage.distance_transform_edt, one mask, one thread", "shape": [s, s], "ms": stats(ts)})
        print(json.dumps(lines[-1]), flush=True)

    if not a.no_model:
        torch.manual_seed(2)
        net = UNet(out_classes=2, base_ch=64, depth=5, dtype="f16").to(dev).eval()
        images = torch.randn(n, s, s, generator=g).to(dev)
        with torch.no_grad():      # re-centre the random head on these images (it would put every pixel in one class): medians aligned
            flat = net(images[:4, :256, :256].contiguous()).transpose(0, 1).reshape(2, -1)
            sc = 2.0 / flat.std(1).clamp_min(1e-6)
            net.conv_last.weight.mul_(sc.view(2, 1, 1, 1))
            net.conv_last.bias.copy_((net.conv_last.bias - flat.median(1).values) * sc)
        kw = dict(size=None, batch=32, tile=256, stride=128)
        off = infer.Segmenter(net, **kw)
        on = infer.Segmenter(net, closing=1.5, **kw)
        masks = torch.stack(off.segment(images))
        fns = {"off": lambda: off.segment(images), "on": lambda: on.segment(images), "clean_mask_alone": lambda: P.clean_mask(masks, closing=1.5)}
        for fn in fns.values():
            timed(fn, 2)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, 3))
        lines.append({"level": "segmenter", "model": "UNet(out_classes=2, base_ch=64, depth=5)", "dtype": "f16", "images": [n, s, s],
                      "tile": 256, "stride": 128, "options": {"closing": 1.5}, "mask_density": round(float(masks.float().mean()), 4),
                      "rounds": a.rounds, "launch": "eager", "ms": {k: stats(v) for k, v in ms.items()},
                      "on_over_off": stats([x / y for x, y in zip(ms["on"], ms["off"])])})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
