#!/usr/bin/env python3
"""HIP-event timing of the finetuning driver's two geometry metrics (metrics.hausdorff + metrics.radius_arteries, one batch each
call, csrc/geometry.hip) at batch 32, 256^2 and 512^2, in three regimes:
  vessels  vessel-like ground truth, prediction = ground truth with 2 % of the pixels flipped;
  noisy    first-epoch-like prediction: 45 % of the pixels flipped (~6e4 crossings per 256^2 image);
  full     all-foreground prediction and target (the longest thinning loop).
Prints one JSON line per (size, regime) with the mean ms of the pair of metric calls and, from one profiled call, the ms per C-ABI
entry point.  Budget (issue): <= 3.6 ms per batch at 256^2 (5 % of the fp32 finetuning step).
    python tools/geometry_metrics_bench.py [--iters 20] [--out profiles/geometry_metrics.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def batch(regime, B, S, rs):
    import gen_geometry_metrics as G
    if regime == "full":
        gt = np.ones((B, S, S), bool)
        pr = gt.copy()
    else:
        gt = np.stack([G.vessels(rs, S, S, n_trees=4 if S == 256 else 6) for _ in range(B)])
        pr = gt ^ (rs.rand(B, S, S) < (0.45 if regime == "noisy" else 0.02))
    l1 = torch.from_numpy(np.where(pr, 1.5, -1.5).astype(np.float32))
    y_pr = torch.stack([-l1, l1], 1).contiguous().cuda()
    g = torch.from_numpy(gt.astype(np.float64))
    y_gt = torch.stack([1 - g, g], 1).contiguous().cuda()
    return y_pr, y_gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmunet_amd import _lib, metrics as M
    h = M.hausdorff(threshold=0.5, activation="softmax", ignore_channels=[0])
    r = M.radius_arteries()
    rs = np.random.RandomState(0)
    lines = []
    for S in (256, 512):
        for regime in ("vessels", "noisy", "full"):
            y_pr, y_gt = batch(regime, a.batch, S, rs)
            for _ in range(2):
                h(y_pr, y_gt), r(y_pr, y_gt)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                hv, rv = h(y_pr, y_gt), r(y_pr, y_gt)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            _lib.PROFILER = _lib.EventProfiler()
            h(y_pr, y_gt), r(y_pr, y_gt)
            prof = {k: round(v["ms"], 4) for k, v in _lib.PROFILER.summary().items()}
            _lib.PROFILER = None
            rec = {"size": S, "batch": a.batch, "regime": regime, "ms_both_metrics": round(ms, 4), "hausdorff": float(hv),
                   "radius_arteries": float(rv), "ms_by_entry_point_one_call": prof}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
