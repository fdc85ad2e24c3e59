#!/usr/bin/env python3
"""HIP-event timing of the image preprocessing (csrc/preprocess.hip, cmunet_amd.preprocess).

(a) Kernel level, --images raw images of --side x --side (512), uint8 and float32, and their centre crop to --crop (475):

      stats, standardize, minmax, row_normalize, crop           on the raw / cropped batch
      blur_rows + unsharp_cols (= unsharp_mask, preserve_range)  at radius 1, 5 and 16 (half-width 4, 20, 64) on the cropped batch
      pipeline                                                   crop -> unsharp(radius, 1.0) -> intensity, raw -> cropped float32

    with the effective TB/s against each pass's own byte model, bytes per OUTPUT pixel with s = 1 (uint8) or 4 (float32) per input
    pixel (halo re-reads and the statistics' second pass are counted as memory traffic only once where noted):
      stats          2 s   (two passes over the image; the second one is served by the caches at these sizes)
      standardize    s + 4          minmax  s + 4          row_normalize  2 s + 4          crop  2 s
      unsharp        (s + 4) for the row pass + (4 + s + 4) for the column pass = 2 s + 12 (halo rows / columns come from the caches)
      pipeline       crop 2 s + unsharp 2 s + 12 [+ stats 2 s for float32 without preserve_range: not in this pipeline's uint8 leg]
                     + stats 8 + standardize 8
    and the tap count per output pixel, 2 (2 lw + 1), from which the report says whether a radius is byte- or instruction-bound.

(b) Whole call: Segmenter(UNet(out_classes=2, base 64, depth 5, f16), size=None, tile=256, stride=128).segment on the raw uint8 images
    with preprocess = crop -> unsharp(radius) -> intensity, against the same call without it on the images preprocessed beforehand.

(c) Host comparison where scipy is importable: the same pipeline with scipy.ndimage.gaussian_filter in float64 (what skimage runs),
    per image on one host thread.

Every figure is the median (with min and max) of --rounds windows after a warm-up; inside a round the cases are timed one after the
other (alternating), so drift of the card hits all of them alike.  Prints one JSON line per case.
    python tools/preprocess_bench.py [--rounds 7] [--out profiles/preprocess.jsonl]"""
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

RADII = (1, 5, 16)


def host_pipeline(img, size, radius, amount):
    """crop -> skimage's unsharp mask (scipy's Gaussian, float64) -> (x - mean) / std on the host."""
    from scipy.ndimage import gaussian_filter
    H, W = img.shape
    y0, x0 = (H - size) // 2, (W - size) // 2
    f = img[y0:y0 + size, x0:x0 + size].astype(np.float64)
    if img.dtype == np.uint8:
        f = f / 255.0
    res = f + (f - gaussian_filter(f, sigma=radius, mode="reflect", truncate=4.0)) * amount
    res = np.clip(res, -1.0 if (f < 0).any() else 0.0, 1.0)
    return ((res - np.mean(res)) / np.std(res)).astype("float32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="windows per figure (at least 5)")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--crop", type=int, default=475)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    from cmunet_amd import infer, ops, preprocess as P
    from cmunet_amd.model import UNet
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    lines = []
    n, S, C = a.images, a.side, a.crop
    raw8 = torch.randint(0, 256, (n, S, S), generator=g, dtype=torch.uint8)
    raws = {"uint8": raw8.to(dev), "float32": (raw8.float() / 255.0 + 0.05 * torch.randn(n, S, S, generator=g)).to(dev)}

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for dt, raw in raws.items():
        s = raw.element_size()
        crop = P.center_crop(raw, C)
        st_c = P.image_stats(crop)
        wts = {r: P._device_weights(r, raw.device) for r in RADII}
        tmp = torch.empty(n, C, C, dtype=torch.float32, device=dev)
        pipes = {r: P.from_options(crop=C, unsharp=(r, 1.0), normalize="intensity") for r in RADII}
        fns = {"stats": lambda: ops.pre_stats(crop), "standardize": lambda: ops.pre_standardize(crop, st_c),
               "minmax": lambda: ops.pre_minmax(crop, st_c), "row_normalize": lambda: ops.pre_row_normalize(crop),
               "crop": lambda: P.center_crop(raw, C)}
        bytes_pp = {"stats": 2 * s, "standardize": s + 4, "minmax": s + 4, "row_normalize": 2 * s + 4, "crop": 2 * s}
        for r in RADII:
            fns[f"unsharp_r{r}"] = lambda r=r: ops.pre_unsharp(crop, wts[r], 1.0, 1.0, False, None, tmp)
            fns[f"pipeline_r{r}"] = lambda r=r: pipes[r](raw)
            bytes_pp[f"unsharp_r{r}"] = 2 * s + 12
            bytes_pp[f"pipeline_r{r}"] = 2 * s + (2 * s + 12) + 8 + 8
        for fn in fns.values():
            timed(fn, 3)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, a.iters))
        st = {k: stats(v) for k, v in ms.items()}
        npix = n * C * C
        emit({"level": "kernel", "dtype": dt, "raw": [n, S, S], "cropped": [n, C, C], "rounds": a.rounds, "iters": a.iters, "launch": "eager",
              "ms": st, "model_bytes_per_output_pixel": bytes_pp,
              "TBps": {k: round(bytes_pp[k] * npix / (st[k]["median"] * 1e-3) / 1e12, 3) for k in fns},
              "taps_per_pixel": {f"unsharp_r{r}": 2 * (2 * int(4 * r + 0.5) + 1) for r in RADII},
              "Gtaps_per_s": {f"unsharp_r{r}": round(2 * (2 * int(4 * r + 0.5) + 1) * npix / (st[f'unsharp_r{r}']["median"] * 1e-3) / 1e9, 1)
                              for r in RADII}})

    if not a.no_model:
        torch.manual_seed(2)
        net = UNet(out_classes=2, base_ch=64, depth=5, dtype="f16").to(dev).eval()
        raw = raws["uint8"]
        pipes = {r: P.from_options(crop=C, unsharp=(r, 1.0), normalize="intensity") for r in RADII}
        pre = pipes[5](raw)
        with torch.no_grad():      # re-centre the random head on these images (it would put every pixel in one class): medians aligned
            flat = net(pre[:4, :256, :256].contiguous()).transpose(0, 1).reshape(2, -1)
            sc = 2.0 / flat.std(1).clamp_min(1e-6)
            net.conv_last.weight.mul_(sc.view(2, 1, 1, 1))
            net.conv_last.bias.copy_((net.conv_last.bias - flat.median(1).values) * sc)
        kw = dict(size=None, batch=32, tile=256, stride=128)
        off = infer.Segmenter(net, **kw)
        fns = {"off": lambda: off.segment(pre)}
        for r in RADII:
            fns[f"on_r{r}"] = lambda seg=infer.Segmenter(net, preprocess=pipes[r], **kw): seg.segment(raw)
            fns[f"pipeline_alone_r{r}"] = lambda r=r: pipes[r](raw)
        same = all(torch.equal(x, y) for x, y in zip(fns["on_r5"](), fns["off"]()))
        for fn in fns.values():
            timed(fn, 2)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, 3))
        emit({"level": "segmenter", "model": "UNet(out_classes=2, base_ch=64, depth=5)", "dtype": "f16", "raw": [n, S, S], "crop": C, "tile": 256,
              "stride": 128, "pipeline": "crop -> unsharp(radius, 1.0) -> intensity", "masks_equal_preprocessing_by_hand": bool(same),
              "rounds": a.rounds, "launch": "eager", "ms": {k: stats(v) for k, v in ms.items()},
              "on_over_off": {f"r{r}": stats([x / y for x, y in zip(ms[f"on_r{r}"], ms["off"])]) for r in RADII}})

    if not a.no_host:
        try:
            import scipy      # noqa: F401
        except ImportError:
            emit({"level": "host", "scipy": None, "note": "scipy is not importable here: no host figure"})
        else:
            for dt, raw in raws.items():
                imgs = raw[:3].cpu().numpy()
                rec = {"level": "host", "dtype": dt, "scipy": scipy.__version__, "threads": 1, "images_timed": int(imgs.shape[0]),
                       "pipeline": "crop -> unsharp (scipy gaussian_filter, float64) -> intensity", "ms_per_image": {}}
                for r in RADII:
                    host_pipeline(imgs[0], C, r, 1.0)
                    t = []
                    for im in imgs:
                        t0 = time.perf_counter()
                        host_pipeline(im, C, r, 1.0)
                        t.append((time.perf_counter() - t0) * 1e3)
                    rec["ms_per_image"][f"r{r}"] = {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
                emit(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
