#!/usr/bin/env python3
"""HIP-event timing of the probability histogram (csrc/prob_hist.hip) against cmu_seg_stats_fwd, the existing kernel that reads the same bytes
(logits + target), of the 255-point threshold sweep against 255 DiceMetric(threshold=) calls, and of Segmenter.segment with
threshold_class=1 against the same call without it.

(a) Pass level, --batch x K x --size^2 logits for K = 2, 4, 8, fp64 one-hot targets (what cmu_seg_stats_fwd reads) and uint8 label maps (the
    histogram only: 8K - 1 fewer bytes per pixel), 256 bins, pooled, on two inputs:
      random       randn * 3 logits: the pixels of a class spread over every bin
      vessel_like  95 % background pixels with logits (+8, -8, ...): more than 90 % of every class's pixels fall into ONE bin -- the case
                   in which a plain LDS atomic serialises 64 lanes on one address and the per-lane run aggregation has to pay
    with the ratio histogram / seg_stats per round (both timed in the same round, alternating) and the effective TB/s against the byte
    model 4K (logits) + 8K (fp64 planes) or + 1 (labels) bytes per pixel.
(b) The sweep: prob_histogram + threshold_sweep (256 bins: every threshold j / 256 at once) against 255 DiceMetric(threshold=j / 256)
    calls on the same (batch, 2, size, size) pair.
(c) Whole call: Segmenter(UNet(out_classes=2, base 64, depth 5, f16), size=None, tile=256, stride=128).segment on --images images of
    --side^2 with threshold_class=1 against the same call without it.

Every figure is the median (with min and max) of --rounds windows after a warm-up; inside a round the cases are timed one after the other
(alternating), so drift of the card hits all of them alike.  Prints one JSON line per case.
    python tools/prob_hist_bench.py [--rounds 5] [--out profiles/prob_hist.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from predict_bench import stats, timed  # noqa: E402


def make_inputs(kind, B, K, S, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, K, S, S, generator=g) * 3
    lab = torch.randint(0, K, (B, S, S), generator=g)
    if kind == "vessel_like":
        bg = torch.rand(B, S, S, generator=g) < 0.95
        flat = torch.full((B, K, S, S), -8.0)
        flat[:, 0] = 8.0
        logits = torch.where(bg[:, None], flat, logits)
        lab = torch.where(bg, torch.zeros_like(lab), lab)
    y = torch.nn.functional.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().double()
    return logits.cuda(), y.cuda(), lab.to(torch.uint8).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="windows per figure (at least 5)")
    ap.add_argument("--iters", type=int, default=200, help="kernel-level calls per timed window")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--side", type=int, default=475)
    ap.add_argument("--model-iters", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("prob_hist_bench needs a ROCm GPU: a timing on the host says nothing about the kernels")
    from cmunet_amd import _lib, infer, metrics, ops
    from cmunet_amd.model import UNet
    B, S, NB = a.batch, a.size, a.bins
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # (a) pass level
    worst = {}
    for K in (2, 4, 8):
        for kind in ("random", "vessel_like"):
            logits, y, lab = make_inputs(kind, B, K, S, seed=K)
            table = torch.empty(1 + 5 * K, dtype=torch.float64, device="cuda")
            ws = torch.empty(_lib.lib().cmu_seg_stats_ws_bytes(K), dtype=torch.uint8, device="cuda")
            bufs = ops.hist_buffers(1, K, NB, "cuda")
            fns = {"seg_stats_f64": lambda: ops.seg_stats_fwd(logits, y, None, 0.5, table, ws),
                   "prob_hist_f64": lambda: ops.prob_hist(logits, y, NB, True, *bufs),
                   "prob_hist_u8": lambda: ops.prob_hist(logits, lab, NB, True, *bufs)}
            for fn in fns.values():
                timed(fn, 20)
            ms = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    ms[k].append(timed(fn, a.iters))
            counts = bufs[0].cpu()
            share = float((counts.sum(2).max(-1).values.double() / counts.sum((2, 3)).double()).min())
            npix = B * S * S
            byt = {"seg_stats_f64": 12 * K, "prob_hist_f64": 12 * K, "prob_hist_u8": 4 * K + 1}
            rec = {"level": "pass", "input": kind, "shape": [B, K, S, S], "bins": NB, "rounds": a.rounds, "iters": a.iters,
                   "least_share_of_a_class_in_its_fullest_bin": round(share, 4), "ms": {k: stats(v) for k, v in ms.items()},
                   "TBps": {k: round(npix * byt[k] / (stats(v)["median"] * 1e-3) / 1e12, 3) for k, v in ms.items()},
                   "hist_over_seg_stats": {"f64": stats([h / s for h, s in zip(ms["prob_hist_f64"], ms["seg_stats_f64"])]),
                                           "u8": stats([h / s for h, s in zip(ms["prob_hist_u8"], ms["seg_stats_f64"])])}}
            worst[(K, kind)] = stats(ms["prob_hist_f64"])["median"]
            emit(rec)
    emit({"level": "pass", "what": "vessel_like over random, prob_hist_f64 medians",
          "ratio": {str(K): round(worst[(K, "vessel_like")] / worst[(K, "random")], 3) for K in (2, 4, 8)}})

    # (b) the 255-point sweep
    logits, y, _ = make_inputs("random", B, 2, S, seed=1)
    dice = [metrics.DiceMetric(threshold=j / NB) for j in range(1, NB)]

    def sweep():
        return metrics.threshold_sweep(metrics.prob_histogram(logits, y, bins=NB))

    def calls():
        metrics.clear_seg_cache()
        return [m(logits, y) for m in dice]
    ref = 1.0 - torch.stack(calls()).cpu()      # DiceMetric: eps 1e-5, class 0 ignored -> the F-score of class 1
    sw = metrics.threshold_sweep(metrics.prob_histogram(logits, y, bins=NB), eps=1e-5).dice[0, 1, 1:NB].cpu()
    ms = {"sweep": [], "dice_calls": []}
    for _ in range(a.rounds):
        ms["sweep"].append(timed(sweep, 20))
        ms["dice_calls"].append(timed(calls, 2))
    emit({"level": "sweep", "shape": [B, 2, S, S], "thresholds": NB - 1, "rounds": a.rounds,
          "max_abs_difference_of_the_dice_values": float((sw - ref).abs().max()), "ms": {k: stats(v) for k, v in ms.items()},
          "dice_calls_over_sweep": stats([d / s for d, s in zip(ms["dice_calls"], ms["sweep"])])})

    # (c) the whole call
    if not a.no_model:
        torch.manual_seed(0)
        model = UNet(out_classes=2, base_ch=64, depth=5, dtype="f16").cuda().eval()
        imgs = torch.rand(a.images, a.side, a.side, generator=torch.Generator().manual_seed(2)).cuda()
        base = dict(size=None, tile=256, stride=128, batch=32)
        segs = {"off": infer.Segmenter(model, **base), "on": infer.Segmenter(model, threshold=0.375, threshold_class=1, **base)}
        for s in segs.values():
            s.segment(imgs)
        torch.cuda.synchronize()
        ms = {k: [] for k in segs}
        for _ in range(a.rounds):
            for k, s in segs.items():
                ms[k].append(timed(lambda: s.segment(imgs), a.model_iters))
        emit({"level": "segmenter", "model": "UNet(out_classes=2, base_ch=64, depth=5)", "dtype": "f16", "images": [a.images, a.side, a.side],
              "tile": 256, "stride": 128, "options": {"threshold": 0.375, "threshold_class": 1}, "rounds": a.rounds, "launch": "eager",
              "ms": {k: stats(v) for k, v in ms.items()}, "on_over_off": stats([x / y for x, y in zip(ms["on"], ms["off"])])})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
