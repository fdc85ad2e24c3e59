#!/usr/bin/env python3
"""HIP-event timing of the K-class segmentation criterion kernels (cmu_seg_stats_fwd / cmu_seg_stats_bwd, csrc/heads.hip) at
32 x K x 256 x 256 for K = 2, 4, 8 with fp64 targets: forward, backward and the pair, with the effective bandwidth from the bytes
each must move (4K + 8K per pixel in, 4K more out backward).  In the same process, the parent's fused two-class kernel
(cmu_softmax_ce_dice_fwd_bwd, 32 B per pixel) at 32 x 2 x 256 x 256: the yardstick for the K = 2 pair (budget: <= 2.0 x).
Every figure is the median (with min and max) of --rounds windows of --iters calls each (0.1 s or more per window at the defaults),
the calls replayed as captured graphs of --chunk calls so that a window measures the device, not the host's launch rate;
inside a round the old kernel and the new ones are timed one after the other, and the K = 2 ratio is taken per round.
Prints one JSON line per configuration.
    python tools/seg_criterion_bench.py [--iters 5000] [--rounds 5] [--out profiles/seg_criterion.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def graph_of(fn, chunk):
    """``chunk`` calls as one captured graph (a linear chain on one stream), so that a window measures the device and not the
    host's launch rate (a Python call costs about as much as one of these kernels runs)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(chunk):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g.replay


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 5), "min": round(xs[0], 5), "max": round(xs[-1], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5000, help="calls per timed window (5000 calls of ~20 us: a 0.1 s window)")
    ap.add_argument("--rounds", type=int, default=5, help="windows per figure; old and new kernels are timed alternately in every round")
    ap.add_argument("--chunk", type=int, default=100, help="calls per captured graph")
    ap.add_argument("--eager", action="store_true", help="time plain calls instead of captured graphs (host-bound at these sizes)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmunet_amd import _lib, ops
    B, S = a.batch, a.size
    npix = B * S * S
    g = torch.Generator().manual_seed(0)

    def gbs(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / 1e9, 1)

    # the parent's fused two-class kernel (CE + its gradient + thresholded counters in one pass): 8 + 16 B in, 8 B out per pixel
    lo2 = (torch.randn(B, 2, S, S, generator=g) * 2).cuda()
    fg = (torch.rand(B, S, S, generator=g) > 0.6).double()
    y2 = torch.stack([1 - fg, fg], 1).contiguous().cuda()
    out, dl2 = torch.empty(6, device="cuda"), torch.empty_like(lo2)
    ws2 = torch.empty(_lib.lib().cmu_softmax_ce_dice_ws_bytes(B, S, S), dtype=torch.uint8, device="cuda")
    fns = {"old": lambda: ops.softmax_ce_dice_fwd_bwd(lo2, y2, out, dl2, 1.0, ws2)}
    keep = []
    for K in (2, 4, 8):
        lo = (torch.randn(B, K, S, S, generator=g) * 2).cuda()
        y = torch.nn.functional.one_hot(torch.randint(0, K, (B, S, S), generator=g), K).permute(0, 3, 1, 2).contiguous().double().cuda()
        table = torch.empty(1 + 5 * K, dtype=torch.float64, device="cuda")
        ws = torch.empty(_lib.lib().cmu_seg_stats_ws_bytes(K), dtype=torch.uint8, device="cuda")
        gr = torch.randn(1 + 2 * K, generator=g, dtype=torch.float64).cuda()
        dl = torch.empty_like(lo)
        keep.append((lo, y, table, ws, gr, dl))
        fwd = (lambda lo=lo, y=y, table=table, ws=ws: ops.seg_stats_fwd(lo, y, None, 0.5, table, ws))
        bwd = (lambda lo=lo, y=y, gr=gr, dl=dl, K=K: ops.seg_stats_bwd(lo, y, None, gr[0:1], gr[1:1 + K], gr[1 + K:], dl))
        fns[f"fwd{K}"], fns[f"bwd{K}"] = fwd, bwd
        fns[f"pair{K}"] = (lambda fwd=fwd, bwd=bwd: (fwd(), bwd()))
    for fn in fns.values():                     # warm-up
        timed(fn, 20)
    # one launch mode for every figure (a ratio of a graph figure to an eager one would mean nothing); --eager times plain calls,
    # which at these kernel times measures the host's launch rate as much as the device
    mode = "eager" if a.eager else "graph"
    run = {k: (fn, 1) if a.eager else (graph_of(fn, a.chunk), a.chunk) for k, fn in fns.items()}
    ms = {k: [] for k in fns}
    ratios = []
    for _ in range(a.rounds):                   # every round: old, then each new figure, so that clock drift hits all alike
        for k, (go, n) in run.items():
            ms[k].append(timed(go, max(1, a.iters // n)) / n)
        ratios.append(ms["pair2"][-1] / ms["old"][-1])
    lines = [{"kernel": "cmu_softmax_ce_dice_fwd_bwd", "shape": [B, 2, S, S], "targets": "f64", "iters": a.iters, "rounds": a.rounds, "launch": mode,
              "ms": stats(ms["old"]), "GBps": gbs(32 * npix, stats(ms["old"])["median"])}]
    for K in (2, 4, 8):
        f, b, p = stats(ms[f"fwd{K}"]), stats(ms[f"bwd{K}"]), stats(ms[f"pair{K}"])
        rec = {"kernel": "cmu_seg_stats_fwd + cmu_seg_stats_bwd", "shape": [B, K, S, S], "targets": "f64", "iters": a.iters, "rounds": a.rounds, "launch": mode,
               "ms_fwd": f, "ms_bwd": b, "ms_pair": p, "GBps_fwd": gbs(12 * K * npix, f["median"]), "GBps_bwd": gbs(16 * K * npix, b["median"]),
               "GBps_pair": gbs(28 * K * npix, p["median"])}
        if K == 2:
            rec["pair_over_softmax_ce_dice"] = {k: round(v, 3) for k, v in stats(ratios).items()}      # per round, same round's old kernel
        lines.append(rec)
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
