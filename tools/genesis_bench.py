#!/usr/bin/env python3
"""HIP-event timing of the Models Genesis / MAE baseline (csrc/genesis.hip, cmunet_amd/genesis.py) at batch 64, 256^2:
  genesis_pairs  one GenesisPairGenerator batch from the device sampler (sample, gather + shuffle, Bezier tables, interp + paint);
  mae_pairs      one MAE batch (sample, patch mask, masked gather);
  step_<dtype>   one GenesisPretrainer step (reference UNet, base 64, depth 5, out_classes 1, MSE, SGD momentum 0.9).
Mean ms over --iters repetitions after --warmup, plus (pairs) the ms per C-ABI entry point of one profiled batch.  Appends one JSON line
per measurement to --out.  Goal (issue): Genesis generation <= 1 ms per batch of 64, under 1 % of the step.
    python tools/genesis_bench.py [--iters 50] [--warmup 5] [--dtypes f32,f16] [--out profiles/genesis.jsonl]"""
import argparse
import json
import os
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmunet_amd import _lib, genesis as G, model as M
    S, B = a.size, a.batch
    src = (np.random.RandomState(0).standard_normal((4 * B, S, S)) * 0.8).astype(np.float32)
    lines = []
    for model in ("Model Genesis", "MAE"):
        gen = G.GenesisPairGenerator(src, B, G.GenesisConfig(model=model), seed=1, device="cuda")
        ms = timed(lambda: next(gen), a.iters, a.warmup)
        _lib.PROFILER = _lib.EventProfiler()
        next(gen)
        prof = {k: round(v["ms"], 4) for k, v in _lib.PROFILER.summary().items()}
        _lib.PROFILER = None
        gen.check()
        rec = {"what": "genesis_pairs" if model != "MAE" else "mae_pairs", "batch": B, "size": S, "ms": round(ms, 4),
               "iters": a.iters, "ms_by_entry_point_one_batch": prof}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    gen = G.GenesisPairGenerator(src, B, G.GenesisConfig(), seed=2, device="cuda")
    x, y = next(gen)
    for dt in [d for d in a.dtypes.split(",") if d]:
        net = M.UNet(out_classes=1, dtype=dt).cuda()
        tr = G.GenesisPretrainer(net)
        ms = timed(lambda: tr.step(x, y), a.iters, a.warmup)
        rec = {"what": f"step_{dt}", "batch": B, "size": S, "ms": round(ms, 3), "iters": a.iters, "images_per_s": round(B / ms * 1e3, 1),
               "loss": float(tr.loss.item())}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del tr, net
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
