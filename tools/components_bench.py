#!/usr/bin/env python3
"""HIP-event timing of the connected-component clean-up (csrc/components.hip, cmunet_amd.postprocess).

(a) Pass level, --images masks of 256 x 256 and of 475 x 475 (the reference's centre crop): a vessel-like mask (thresholded low-pass
    noise: a few large blobs and many specks) and, at 475 x 475, a random mask of density 0.59 (the 4-connected percolation
    threshold: large ragged components, the longest union chains) as the worst case:

      label            postprocess.label(mask, 8)
      component_sizes  postprocess.component_sizes(labels)
      clean_mask       postprocess.clean_mask(mask, min_size=50, keep_largest=2, fill_holes=True)

    with the effective TB/s against each pass's own byte model (bytes per pixel; atomics and pointer chasing not counted):
      label            18 = tile pass 1 read + 4 parent written; seam pass 1 read; flatten 4 parent read + 4 compressed parent written
                       + 4 label written.  (The floor of ANY labelling is 5: 1 read, 4 written.)
      component_sizes  8 = 4 cleared + 4 read
      clean_mask       label 18 + sizes 8 + select 2 x 4 + filter 10 (1 + 4 + 4 gathered + 1) + hole label 18 + border 1 + filter 7
                       (1 + 4 + 1 gathered + 1) = 70

(b) Whole call: Segmenter(UNet(out_classes=2, base 64, depth 5, f16), size=None, tile=256, stride=128).segment on --images images of
    --side x --side with the clean-up options on (min_size=50, keep_largest=2, fill_holes=True) against the same call with them off.

Every figure is the median (with min and max) of --rounds windows after a warm-up; inside a round the sides are timed one after the
other (alternating), so drift of the card hits all of them alike.  Prints one JSON line per case.
    python tools/components_bench.py [--rounds 7] [--out profiles/components.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from predict_bench import stats, timed  # noqa: E402

BYTES = {"label": 18, "component_sizes": 8, "clean_mask": 70}


def vessel_like(n, side, g):
    """Thresholded low-pass noise plus 0.3 % specks: a handful of large blobs with holes and many small components."""
    x = torch.randn(n, 1, side, side, generator=g)
    for _ in range(3):
        x = torch.nn.functional.avg_pool2d(x, 9, 1, 4)
    x = x[:, 0]
    m = x > x.flatten(1).quantile(0.85, dim=1).view(n, 1, 1)
    return (m | (torch.rand(n, side, side, generator=g) < 0.003)).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="windows per figure (at least 5)")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--side", type=int, default=475)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    from cmunet_amd import infer, postprocess as P
    from cmunet_amd.model import UNet
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    lines = []

    cases = [("vessel_like", 256, vessel_like(a.images, 256, g)), ("vessel_like", a.side, vessel_like(a.images, a.side, g)),
             ("random_0.59", a.side, (torch.rand(a.images, a.side, a.side, generator=g) < 0.59).to(torch.uint8))]
    for kind, side, mask in cases:
        m = mask.to(dev)
        labels, counts = P.label(m, 8)
        fns = {"label": lambda m=m: P.label(m, 8), "component_sizes": lambda labels=labels: P.component_sizes(labels),
               "clean_mask": lambda m=m: P.clean_mask(m, min_size=50, keep_largest=2, fill_holes=True)}
        for fn in fns.values():
            timed(fn, 3)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, a.iters))
        npix = a.images * side * side
        st = {k: stats(v) for k, v in ms.items()}
        lines.append({"level": "pass", "mask": kind, "shape": [a.images, side, side], "density": round(float(mask.float().mean()), 4),
                      "components_per_image": round(float(counts.float().mean()), 1), "overrun": bool((counts < 0).any()),
                      "rounds": a.rounds, "iters": a.iters, "launch": "eager", "ms": st, "model_bytes_per_pixel": BYTES,
                      "TBps": {k: round(BYTES[k] * npix / (st[k]["median"] * 1e-3) / 1e12, 3) for k in fns},
                      "label_TBps_at_the_5_byte_floor": round(5 * npix / (st["label"]["median"] * 1e-3) / 1e12, 3)})
        print(json.dumps(lines[-1]), flush=True)

    if not a.no_model:
        torch.manual_seed(2)
        net = UNet(out_classes=2, base_ch=64, depth=5, dtype="f16").to(dev).eval()
        images = torch.randn(a.images, a.side, a.side, generator=g).to(dev)
        with torch.no_grad():      # re-centre the random head on these images (it would put every pixel in one class): medians aligned
            flat = net(images[:4, :256, :256].contiguous()).transpose(0, 1).reshape(2, -1)
            s = 2.0 / flat.std(1).clamp_min(1e-6)
            net.conv_last.weight.mul_(s.view(2, 1, 1, 1))
            net.conv_last.bias.copy_((net.conv_last.bias - flat.median(1).values) * s)
        kw = dict(size=None, batch=32, tile=256, stride=128)
        off = infer.Segmenter(net, **kw)
        on = infer.Segmenter(net, min_size=50, keep_largest=2, fill_holes=True, **kw)
        masks = torch.stack(off.segment(images))
        fns = {"off": lambda: off.segment(images), "on": lambda: on.segment(images),
               "clean_mask_alone": lambda: P.clean_mask(masks, min_size=50, keep_largest=2, fill_holes=True)}
        for fn in fns.values():
            timed(fn, 2)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, 3))
        lines.append({"level": "segmenter", "model": "UNet(out_classes=2, base_ch=64, depth=5)", "dtype": "f16", "images": [a.images, a.side, a.side],
                      "tile": 256, "stride": 128, "options": {"min_size": 50, "keep_largest": 2, "fill_holes": True, "connectivity": 8},
                      "mask_density": round(float(masks.float().mean()), 4), "components_per_image": round(float(P.label(masks, 8)[1].float().mean()), 1),
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
