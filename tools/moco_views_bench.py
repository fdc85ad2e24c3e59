#!/usr/bin/env python3
"""HIP-event timing of MoCo's two augmented views (csrc/moco_views.hip, cmunet_amd/moco_views.py): one DeviceMocoViews batch of --batches
float32 images at 256^2 -> 2 x 224^2 from the device sampler, with the reference's probabilities ("default") and with every transform
forced on ("all_on"), antialias off and on.  Mean ms over --iters batches after --warmup, plus the ms per C-ABI entry point of one profiled
batch; then -- in the same run -- one MocoPretrainer.step at 224^2 on the same batch size (--dtypes) for the share: the views should cost a
few per cent of the step they feed.  Appends one JSON line per measurement to --out.
    python tools/moco_views_bench.py [--iters 100] [--warmup 10] [--batches 64,128] [--dtypes f32,f16] [--out profiles/moco_views.jsonl]"""
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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="64,128")
    ap.add_argument("--dtypes", default="f32,f16", help="MocoPretrainer.step dtypes to time for the share ('' skips)")
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmunet_amd import _lib, moco as MO, moco_views as MV, pretrain as P
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    forced = dict(p_rotation=1.0, p_blur=1.0, p_hflip=1.0, p_vflip=1.0, p_noise=1.0)
    for B in [int(b) for b in a.batches.split(",") if b]:
        x = torch.from_numpy(np.random.RandomState(0).standard_normal((B, 256, 256)).astype(np.float32)).cuda()
        ms_default = None
        for what, cfg in (("default", {}), ("all_on", forced), ("default_antialias", dict(antialias=True)),
                          ("all_on_antialias", dict(antialias=True, **forced))):
            views = MV.DeviceMocoViews(MV.MocoViewConfig(**cfg), seed=1)
            ms = timed(lambda: views.views(x), a.iters, a.warmup)
            _lib.PROFILER = _lib.EventProfiler()
            views.views(x)
            prof = {k: round(v["ms"], 4) for k, v in _lib.PROFILER.summary().items()}
            _lib.PROFILER = None
            if what == "default":
                ms_default = ms
            emit({"what": f"moco_views_{what}", "batch": B, "side": 256, "out": 224, "ms": round(ms, 4), "iters": a.iters,
                  "ms_by_entry_point_one_batch": prof})
        q, k = MV.DeviceMocoViews(seed=2).views(x)
        for dt in [d for d in a.dtypes.split(",") if d]:
            m = MO.Moco_v2(emb_dim=1024, num_negatives=4096, softmax_temperature=0.2, encoder_momentum=0.999, dtype=dt, batch_size=B).cuda()
            tr = P.MocoPretrainer(m)
            scale = 1.0 if dt == "f32" else 1024.0
            ms = timed(lambda: tr.step(q, k, loss_scale=scale), a.step_iters, 3)
            emit({"what": f"moco_step_{dt}", "batch": B, "size": 224, "ms": round(ms, 3), "iters": a.step_iters,
                  "views_share_default": round(ms_default / ms, 5)})
            del m, tr
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
