#!/usr/bin/env python3
"""HIP-event timing of the Lovasz-Softmax loss (csrc/lovasz.hip on the key sort of csrc/key_sort.hip) at 32 x K x 256 x 256, K = 2, 4, 8,
batch-wide (one segment of 2,097,152 pixels per class) and per image (32 segments of 65,536), against two yardsticks of the SAME run:

  * the same loss composed from torch ops on the device (softmax, torch.sort, gather, cumsum; backward by autograd), and torch.sort on
    the very keys cmu_sort_u64 sorts -- the yardstick lives in this tool only, nothing of it is in the product path;
  * the cmu_seg_stats_fwd + _bwd pair on the same logits with fp64 one-hot targets, for time per byte (the streaming passes the step
    already runs).

Timed per configuration: cmu_lovasz_keys, cmu_sort_u64 and cmu_lovasz_grad each on its own, the forward (the three in a row), and
forward + backward (cmu_softmax_map_bwd behind them), each next to its byte model; the forward + backward also as a share of --step-ms
(README's 10.7 ms f16 finetuning step).  Every figure is the median (with min and max) of --rounds windows of --iters calls; inside a
round every configuration is timed once, one after the other, so that clock drift hits all alike.  The calls are a few milliseconds
each, so they are launched eagerly.  Prints one JSON line per configuration.
    python tools/lovasz_bench.py [--iters 5] [--rounds 5] [--out profiles/lovasz.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from map_loss_bench import stats, timed, vessel_labels      # noqa: E402


def torch_lovasz(x, lab, per_image):
    """Berman's lovasz_softmax (classes='all', nothing ignored) as batched torch ops: x (B,K,H,W) logits, lab (B,H,W) int64."""
    B, K, H, W = x.shape
    p = torch.softmax(x, 1)
    fg = torch.nn.functional.one_hot(lab, K).permute(0, 3, 1, 2).to(p.dtype)
    e = (fg - p).abs()
    if per_image:
        e, fg = e.reshape(B, K, H * W), fg.reshape(B, K, H * W)
    else:
        e, fg = e.permute(1, 0, 2, 3).reshape(1, K, -1), fg.permute(1, 0, 2, 3).reshape(1, K, -1)
    es, perm = torch.sort(e, dim=2, descending=True)
    fs = torch.gather(fg, 2, perm)
    G = fs.sum(2, keepdim=True)
    inter = G - fs.cumsum(2)
    union = G + (1.0 - fs).cumsum(2)
    J = 1.0 - inter / union
    g = torch.cat((J[..., :1], J[..., 1:] - J[..., :-1]), 2)
    return (es * g).sum(2).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per figure; every configuration is timed once per round")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--step-ms", type=float, default=10.7, help="the training step the loss's share is quoted against")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmunet_amd import _lib, ops
    B, S = a.batch, a.size
    npix = B * S * S
    T = ops.sort_tile_keys()
    gen = torch.Generator().manual_seed(0)
    dev = "cuda"
    run, meta, hold = {}, {}, []

    def add(name, fn, rec, nbytes=None, yard=None):
        run[name] = fn
        meta[name] = (rec, nbytes, yard)

    for K in (2, 4, 8):
        lo = (torch.randn(B, K, S, S, generator=gen) * 2).to(dev)
        lab = vessel_labels(B, S, K, K)
        t8, t64 = lab.to(torch.uint8).to(dev), lab.to(dev)
        dl = torch.empty_like(lo)
        y = torch.nn.functional.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().double().to(dev)
        tseg = torch.empty(1 + 5 * K, dtype=torch.float64, device=dev)
        wseg = torch.empty(_lib.lib().cmu_seg_stats_ws_bytes(K), dtype=torch.uint8, device=dev)
        gr = torch.randn(1 + 2 * K, generator=gen, dtype=torch.float64).to(dev)
        hold.append((lo, t8, t64, dl, y, tseg, wseg, gr))
        add(f"seg_stats/K{K}", lambda lo=lo, y=y, T_=tseg, ws=wseg, gr=gr, dl=dl, K=K: (
            ops.seg_stats_fwd(lo, y, None, 0.5, T_, ws), ops.seg_stats_bwd(lo, y, None, gr[0:1], gr[1:1 + K], gr[1 + K:], dl)),
            {"kernel": "cmu_seg_stats_fwd + _bwd (yardstick)", "shape": [B, K, S, S], "targets": "f64 one-hot"}, (12 * K * 2 + 4 * K) * npix)
        for per_image in (False, True):
            tag = f"K{K}/{'per_image' if per_image else 'batch'}"
            sz = ops.lovasz_sizes(B, K, S, S, None, per_image)
            rows, n = sz["rows"], sz["n"]
            passes = max(0, (sz["tiles"] - 1).bit_length())
            keys = torch.empty((rows, n), dtype=torch.int64, device=dev)
            ranked, scratch = torch.empty_like(keys), torch.empty_like(keys)
            counts = torch.empty(sz["counts"], dtype=torch.int64, device=dev)
            wmap, out = torch.empty_like(lo), torch.empty(sz["out"], dtype=torch.float64, device=dev)
            tile_fg = torch.empty(sz["scratch"], dtype=torch.int64, device=dev)
            partials = torch.empty(sz["scratch"], dtype=torch.float64, device=dev)
            gk = torch.full((K,), 1.0, dtype=torch.float64, device=dev)
            hold.append((keys, ranked, scratch, counts, wmap, out, tile_fg, partials, gk))

            def f_keys(lo=lo, t8=t8, per_image=per_image, keys=keys, counts=counts):
                ops.lovasz_keys(lo, t8, False, None, per_image, -100, keys, counts)

            def f_sort(keys=keys, ranked=ranked, scratch=scratch):
                ops.sort_u64(keys, ranked, scratch)

            def f_grad(ranked=ranked, counts=counts, per_image=per_image, wmap=wmap, out=out, tile_fg=tile_fg, partials=partials):
                ops.lovasz_grad(ranked, counts, None, per_image, True, wmap, out, tile_fg, partials)

            def f_fwd(f_keys=f_keys, f_sort=f_sort, f_grad=f_grad):
                f_keys(), f_sort(), f_grad()

            def f_fwd_bwd(f_fwd=f_fwd, lo=lo, wmap=wmap, gk=gk, dl=dl):
                f_fwd()
                ops.softmax_map_bwd(lo, wmap, None, None, "linear", gk, dl)

            def t_sort(keys=keys):
                torch.sort(keys, dim=1)

            def t_fwd(lo=lo, t64=t64, per_image=per_image):
                with torch.no_grad():
                    torch_lovasz(lo, t64, per_image)

            def t_fwd_bwd(lo=lo, t64=t64, per_image=per_image):
                x = lo.detach().requires_grad_(True)
                torch_lovasz(x, t64, per_image).backward()

            nk = rows * n
            b_keys, b_sort, b_grad = (4 * K + 1) * npix + 8 * nk, 16 * nk * (1 + passes), (8 + 8 + 4) * nk
            b_bwd = 12 * K * npix
            shape = {"shape": [B, K, S, S], "per_image": per_image, "segments": rows, "keys_per_segment": n, "merge_passes": passes, "tile_keys": T}
            add(f"lovasz_keys/{tag}", f_keys, dict(shape, kernel="cmu_lovasz_keys", labels="u8"), b_keys)
            add(f"sort_u64/{tag}", f_sort, dict(shape, kernel="cmu_sort_u64"), b_sort, f"torch_sort/{tag}")
            add(f"lovasz_grad/{tag}", f_grad, dict(shape, kernel="cmu_lovasz_grad"), b_grad)
            add(f"lovasz_fwd/{tag}", f_fwd, dict(shape, kernel="cmu_lovasz_keys + cmu_sort_u64 + cmu_lovasz_grad"), b_keys + b_sort + b_grad, f"torch_fwd/{tag}")
            add(f"lovasz_fwd_bwd/{tag}", f_fwd_bwd, dict(shape, kernel="forward + cmu_softmax_map_bwd"), b_keys + b_sort + b_grad + b_bwd, f"torch_fwd_bwd/{tag}")
            add(f"torch_sort/{tag}", t_sort, dict(shape, kernel="torch.sort on the same keys (yardstick)"))
            add(f"torch_fwd/{tag}", t_fwd, dict(shape, kernel="torch ops: softmax, sort, gather, cumsum (yardstick)"))
            add(f"torch_fwd_bwd/{tag}", t_fwd_bwd, dict(shape, kernel="torch ops + autograd (yardstick)"))
    for name, fn in run.items():                               # real keys in every buffer before a sort is timed on its own
        if name.startswith("lovasz_fwd/"):
            fn()
    for fn in run.values():
        timed(fn, 2)
    ms = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, fn in run.items():
            ms[k].append(timed(fn, a.iters))

    lines = []
    for name, (rec, nbytes, yard) in meta.items():
        p = stats(ms[name])
        line = dict(rec, name=name, iters=a.iters, rounds=a.rounds, launch="eager", ms=p)
        if nbytes is not None:
            line.update(bytes=nbytes, TBps=round(nbytes / (p["median"] * 1e-3) / 1e12, 3))
        if yard is not None:
            line.update(yardstick=yard, time_ratio=round(p["median"] / stats(ms[yard])["median"], 4))
        if name.startswith(("lovasz_", "sort_u64")):
            K = rec["shape"][1]
            ym, yb = stats(ms[f"seg_stats/K{K}"])["median"], meta[f"seg_stats/K{K}"][1]
            line.update(time_per_byte_vs_seg_stats=round((p["median"] / nbytes) / (ym / yb), 4))
        if name.startswith("lovasz_fwd_bwd"):
            line.update(share_of_step=round(p["median"] / a.step_ms, 4), step_ms=a.step_ms)
        lines.append(line)
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
