#!/usr/bin/env python3
"""HIP-event timing of the element-wise loss kernels (cmu_pointwise_loss_fwd / _bwd) and the class-index cross entropy
(cmu_index_ce_fwd / _bwd) of csrc/pointwise_loss.hip: forward, and forward + backward,

  * every kind (l1, mse, bce, bce_with_logits) at 32 x 1 x 256 x 256 and 32 x 2 x 256 x 256, fp32 targets
    (4 + 4 bytes in per element, 4 more in and 4 out backward);
  * the index CE at 32 x K x 256 x 256 for K = 2, 4, 8 with uint8 and int64 labels (4K + 1 or 4K + 8 bytes in per pixel, the same
    again plus 4K out backward);

with the effective bandwidth from the bytes each must move.  In the same process and the same alternating rounds, the yardstick: the
cmu_seg_stats_fwd / _bwd pair at the same K with fp64 one-hot targets (12K bytes in per pixel, 16K more backward), which the index CE
replaces when the data set stores a label map.  Every figure is the median (with min and max) of --rounds windows of --iters calls
each, the calls replayed as captured graphs of --chunk calls so that a window measures the device and not the host's launch rate;
inside a round every configuration is timed once, one after the other, so that clock drift hits all alike.
Prints one JSON line per configuration.
    python tools/pointwise_loss_bench.py [--iters 2000] [--rounds 5] [--out profiles/pointwise_loss.jsonl]"""
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
    """``chunk`` calls as one captured graph (a linear chain on one stream)."""
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
    ap.add_argument("--iters", type=int, default=2000, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per figure; every configuration is timed once per round")
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
    dev = "cuda"
    fns, meta, keep = {}, {}, []

    def add(name, fwd, bwd, rec, bytes_fwd, bytes_bwd):
        fns[name + ":fwd"] = fwd
        fns[name + ":pair"] = lambda: (fwd(), bwd())
        meta[name] = (rec, bytes_fwd, bytes_fwd + bytes_bwd)

    gd = torch.tensor([0.37 / npix], dtype=torch.float64, device=dev)
    for C in (1, 2):
        n = npix * C
        for kind in ops.PWL_KINDS:
            x = (torch.rand(B, C, S, S, generator=g) if kind == "bce" else torch.randn(B, C, S, S, generator=g) * 2).to(dev)
            y = torch.rand(B, C, S, S, generator=g).to(dev)
            out = torch.empty(1, dtype=torch.float64, device=dev)
            ws = torch.empty(_lib.lib().cmu_pointwise_loss_ws_bytes(), dtype=torch.uint8, device=dev)
            dx = torch.empty_like(x)
            keep.append((x, y, out, ws, dx))
            add(f"{kind}/C{C}", (lambda kind=kind, x=x, y=y, out=out, ws=ws: ops.pointwise_loss_fwd(kind, x, y, None, None, out, ws)),
                (lambda kind=kind, x=x, y=y, dx=dx: ops.pointwise_loss_bwd(kind, x, y, None, None, gd, dx)),
                {"kernel": "cmu_pointwise_loss_fwd / _bwd", "kind": kind, "shape": [B, C, S, S], "targets": "f32"}, 8 * n, 12 * n)
    g2 = torch.tensor([0.37 / npix, 0.01 / npix], dtype=torch.float64, device=dev)
    for K in (2, 4, 8):
        lo = (torch.randn(B, K, S, S, generator=g) * 2).to(dev)
        lab = torch.randint(0, K, (B, S, S), generator=g)
        dl = torch.empty_like(lo)
        for name, dt, nb in (("u8", torch.uint8, 1), ("i64", torch.int64, 8)):
            t = lab.to(dt).to(dev)
            table = torch.empty(3, dtype=torch.float64, device=dev)
            ws = torch.empty(_lib.lib().cmu_index_ce_ws_bytes(), dtype=torch.uint8, device=dev)
            keep.append((lo, t, table, ws, dl))
            add(f"index_ce/K{K}/{name}", (lambda lo=lo, t=t, table=table, ws=ws: ops.index_ce_fwd(lo, t, False, False, None, None, -100, table, ws)),
                (lambda lo=lo, t=t, dl=dl: ops.index_ce_bwd(lo, t, False, False, None, None, -100, g2, dl)),
                {"kernel": "cmu_index_ce_fwd / _bwd", "shape": [B, K, S, S], "labels": name}, (4 * K + nb) * npix, (8 * K + nb) * npix)
        # the yardstick: the one-hot probability-target pass at the same K
        y = torch.nn.functional.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().double().to(dev)
        table = torch.empty(1 + 5 * K, dtype=torch.float64, device=dev)
        ws = torch.empty(_lib.lib().cmu_seg_stats_ws_bytes(K), dtype=torch.uint8, device=dev)
        gr = torch.randn(1 + 2 * K, generator=g, dtype=torch.float64).to(dev)
        keep.append((y, table, ws, gr))
        add(f"seg_stats/K{K}", (lambda lo=lo, y=y, table=table, ws=ws: ops.seg_stats_fwd(lo, y, None, 0.5, table, ws)),
            (lambda lo=lo, y=y, gr=gr, dl=dl, K=K: ops.seg_stats_bwd(lo, y, None, gr[0:1], gr[1:1 + K], gr[1 + K:], dl)),
            {"kernel": "cmu_seg_stats_fwd / _bwd (yardstick)", "shape": [B, K, S, S], "targets": "f64 one-hot"}, 12 * K * npix, 16 * K * npix)
    for fn in fns.values():                     # warm-up: code objects, allocator
        timed(fn, 20)
    mode = "eager" if a.eager else "graph"
    run = {k: (fn, 1) if a.eager else (graph_of(fn, a.chunk), a.chunk) for k, fn in fns.items()}
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, (go, n) in run.items():
            ms[k].append(timed(go, max(1, a.iters // n)) / n)

    def tbs(nbytes, m):
        return round(nbytes / (m * 1e-3) / 1e12, 3)

    lines = []
    for name, (rec, bf, bp) in meta.items():
        f, p = stats(ms[name + ":fwd"]), stats(ms[name + ":pair"])
        lines.append(dict(rec, iters=a.iters, rounds=a.rounds, launch=mode, ms_fwd=f, ms_pair=p, bytes_fwd=bf, bytes_pair=bp,
                          TBps_fwd=tbs(bf, f["median"]), TBps_pair=tbs(bp, p["median"])))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
