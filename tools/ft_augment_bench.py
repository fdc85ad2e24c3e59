#!/usr/bin/env python3
"""HIP-event timing of the finetuning training augmentation (csrc/ft_augment.hip, cmunet_amd/ft_augment.py): one
DeviceTrainingAugmentation batch of --batch float32 images + uint8 masks at --side^2 -> 256^2 image + float64 one-hot, from the device
sampler, with the default probabilities ("default") and with every transform forced on ("all_on", OneOf's choice still drawn).  Mean ms
over --iters batches after --warmup, plus the ms per C-ABI entry point of one profiled batch; then tools/finetune_step.py's bs-32 256^2
training-batch time on the same device for the share.  Appends one JSON line per measurement to --out.  Goal (issue): <= 0.2 ms per batch of 32.
    python tools/ft_augment_bench.py [--iters 100] [--warmup 10] [--dtypes f16,f32] [--out profiles/ft_augment.jsonl]"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--side", type=int, default=475)
    ap.add_argument("--dtypes", default="f16,f32", help="finetune_step.py dtypes to time for the share ('' skips)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmunet_amd import _lib, ft_augment as FA
    B, side = a.batch, a.side
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.standard_normal((B, side, side)).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.uniform(size=(B, side, side)) < 0.1).astype(np.uint8)).cuda()
    lines = []
    forced = dict(p_noise=1.0, p_blur=1.0, p_brightness_contrast=1.0, p_downscale=1.0, p_oneof=1.0)
    for what, cfg in (("default", {}), ("all_on", forced)):
        aug = FA.DeviceTrainingAugmentation(FA.FinetuneAugmentConfig(**cfg), seed=1)
        ms = timed(lambda: aug(x, y), a.iters, a.warmup)
        _lib.PROFILER = _lib.EventProfiler()
        aug(x, y)
        prof = {k: round(v["ms"], 4) for k, v in _lib.PROFILER.summary().items()}
        _lib.PROFILER = None
        rec = {"what": f"ft_augment_{what}", "batch": B, "side": side, "out": 256, "ms": round(ms, 4), "iters": a.iters,
               "ms_by_entry_point_one_batch": prof}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    for dt in [d for d in a.dtypes.split(",") if d]:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "finetune_step.py"), dt, str(B)], capture_output=True, text=True,
                           timeout=600)
        m = re.search(r"train epoch of 10 batches: ([0-9.]+) ms/batch", r.stdout)
        ms = float(m.group(1)) if m else None
        rec = {"what": f"finetune_step_{dt}", "batch": B, "size": 256, "ms": ms,
               "augment_share_default": (round(lines[0]["ms"] / ms, 5) if ms else None), "rc": r.returncode}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
