#!/usr/bin/env python3
"""HIP-event timing of csrc/map_loss.hip at 32 x K x 256 x 256, K = 2, 4, 8, each against its yardstick of the SAME run:

  * cmu_focal_fwd + _bwd at gamma = 0, 2 and 1.5 with uint8 labels against cmu_index_ce_fwd + _bwd on the same tensors -- the same
    bytes (4K + 1 in per pixel, the same again plus 4K out backward), so the expectation is parity;
  * cmu_softmax_map_fwd + _bwd, kind 'linear' (4K logits + 4K map in, the same again plus 4K out backward) and kind 'squared' with
    fp64 targets (8K more each way), against the cmu_seg_stats_fwd + _bwd pair with fp64 one-hot targets (12K in, 12K + 4K backward),
    each next to its byte model: the expectation is no slower per byte;
  * BoundaryLoss and HausdorffDTLoss at 32 x 2 x 256 x 256, the distance maps and the loss pass (forward + backward) timed
    separately, each as a share of --step-ms (README's 10.7 ms f16 finetuning step).

Every figure is the median (with min and max) of --rounds windows; inside a round every configuration is timed once, one after the
other, so that clock drift hits all alike.  The kernel pairs are replayed as captured graphs of --chunk calls, so that a window
measures the device and not the host's launch rate; the map construction (a dozen launches with their allocations) runs eagerly.
Prints one JSON line per configuration.
    python tools/map_loss_bench.py [--iters 2000] [--rounds 5] [--out profiles/map_loss.jsonl]"""
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


def vessel_labels(B, S, K, seed):
    """(B,S,S) int64: random-walk strokes of classes 1..K-1 on background 0 -- thin foregrounds, as the losses are meant for."""
    import numpy as np
    rs = np.random.RandomState(seed)
    lab = np.zeros((B, S, S), np.int64)
    for b in range(B):
        for c in range(1, K):
            for _ in range(4):
                y, x = rs.randint(0, S, 2)
                for _ in range(3 * S):
                    y, x = int(np.clip(y + rs.randint(-1, 2), 0, S - 1)), int(np.clip(x + rs.randint(-1, 2), 0, S - 1))
                    lab[b, max(y - 1, 0):y + 1, max(x - 1, 0):x + 1] = c
    return torch.from_numpy(lab)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000, help="calls per timed window of a kernel pair")
    ap.add_argument("--class-iters", type=int, default=100, help="calls per timed window of a map construction")
    ap.add_argument("--rounds", type=int, default=5, help="windows per figure; every configuration is timed once per round")
    ap.add_argument("--chunk", type=int, default=100, help="calls per captured graph")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--step-ms", type=float, default=10.7, help="the training step the loss shares are quoted against")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmunet_amd import _lib, metrics as M, ops
    B, S = a.batch, a.size
    npix = B * S * S
    g = torch.Generator().manual_seed(0)
    dev = "cuda"
    pairs, meta, keep = {}, {}, []

    def add(name, fwd, bwd, rec, nbytes, yard):
        pairs[name] = lambda: (fwd(), bwd())
        meta[name] = (rec, nbytes, yard)

    for K in (2, 4, 8):
        lo = (torch.randn(B, K, S, S, generator=g) * 2).to(dev)
        lab = vessel_labels(B, S, K, K)
        t8 = lab.to(torch.uint8).to(dev)
        dl = torch.empty_like(lo)
        g1 = torch.tensor([0.37 / npix], dtype=torch.float64, device=dev)
        g2 = torch.tensor([0.37 / npix, 0.0], dtype=torch.float64, device=dev)
        table3 = torch.empty(3, dtype=torch.float64, device=dev)
        ws = torch.empty(_lib.lib().cmu_index_ce_ws_bytes(), dtype=torch.uint8, device=dev)
        part = ops.map_loss_partials(K + 3, dev)
        ice_bytes = (4 * K + 1) * npix * 2 + 4 * K * npix
        add(f"index_ce/K{K}", (lambda lo=lo, t=t8, T=table3, ws=ws: ops.index_ce_fwd(lo, t, False, False, None, None, -100, T, ws)),
            (lambda lo=lo, t=t8, dl=dl, g2=g2: ops.index_ce_bwd(lo, t, False, False, None, None, -100, g2, dl)),
            {"kernel": "cmu_index_ce_fwd + _bwd (yardstick)", "shape": [B, K, S, S], "labels": "u8"}, ice_bytes, None)
        for gamma in (0.0, 2.0, 1.5):
            add(f"focal/K{K}/gamma{gamma:g}", (lambda lo=lo, t=t8, T=table3, p=part, gamma=gamma: ops.focal_fwd(lo, t, False, None, gamma, -100, T, p)),
                (lambda lo=lo, t=t8, dl=dl, g1=g1, gamma=gamma: ops.focal_bwd(lo, t, False, None, gamma, -100, g1, dl)),
                {"kernel": "cmu_focal_fwd + _bwd", "shape": [B, K, S, S], "labels": "u8", "gamma": gamma}, ice_bytes, f"index_ce/K{K}")
        y = torch.nn.functional.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().double().to(dev)
        wm = (torch.randn(B, K, S, S, generator=g) * 3).to(dev)
        tseg = torch.empty(1 + 5 * K, dtype=torch.float64, device=dev)
        wseg = torch.empty(_lib.lib().cmu_seg_stats_ws_bytes(K), dtype=torch.uint8, device=dev)
        gr = torch.randn(1 + 2 * K, generator=g, dtype=torch.float64).to(dev)
        gk = torch.randn(K, generator=g, dtype=torch.float64).to(dev) / npix
        tk = torch.empty(K, dtype=torch.float64, device=dev)
        keep.append((lo, t8, dl, y, wm, tseg, wseg, gr, gk, tk, part, table3, ws))
        add(f"seg_stats/K{K}", (lambda lo=lo, y=y, T=tseg, ws=wseg: ops.seg_stats_fwd(lo, y, None, 0.5, T, ws)),
            (lambda lo=lo, y=y, gr=gr, dl=dl, K=K: ops.seg_stats_bwd(lo, y, None, gr[0:1], gr[1:1 + K], gr[1 + K:], dl)),
            {"kernel": "cmu_seg_stats_fwd + _bwd (yardstick)", "shape": [B, K, S, S], "targets": "f64 one-hot"}, (12 * K * 2 + 4 * K) * npix, None)
        for kind, per_pass in (("linear", 8 * K), ("squared", 16 * K)):
            add(f"softmax_map/{kind}/K{K}", (lambda lo=lo, wm=wm, y=y, T=tk, p=part, kind=kind: ops.softmax_map_fwd(lo, wm, y, None, kind, T, p)),
                (lambda lo=lo, wm=wm, y=y, gk=gk, dl=dl, kind=kind: ops.softmax_map_bwd(lo, wm, y, None, kind, gk, dl)),
                {"kernel": "cmu_softmax_map_fwd + _bwd", "kind": kind, "shape": [B, K, S, S], "map": "f32", "targets": "f64 one-hot" if kind == "squared" else None},
                (per_pass * 2 + 4 * K) * npix, f"seg_stats/K{K}")

    # the two map losses at K = 2, ignore_channels = (0,): maps and loss pass separately
    K = 2
    lo = (torch.randn(B, K, S, S, generator=g) * 2).to(dev)
    lab = vessel_labels(B, S, K, 9)
    lab8 = lab.to(torch.uint8).to(dev)
    y = torch.nn.functional.one_hot(lab, K).permute(0, 3, 1, 2).contiguous().double().to(dev)
    hd = M.HausdorffDTLoss()
    phi, fields = M._signed_maps(lab8, K, [1]), hd._fields(lo, lab8, [1])
    dl, tk, part = torch.empty_like(lo), torch.empty(K, dtype=torch.float64, device=dev), ops.map_loss_partials(K, dev)
    gk = torch.full((K,), 1.0 / npix, dtype=torch.float64, device=dev)
    eager = {"boundary/maps": lambda: M._signed_maps(lab8, K, [1]), "hausdorff_dt/maps": lambda: hd._fields(lo, lab8, [1])}
    add("boundary/loss_pass", lambda: ops.softmax_map_fwd(lo, phi, None, [1], "linear", tk, part), lambda: ops.softmax_map_bwd(lo, phi, None, [1], "linear", gk, dl),
        {"kernel": "BoundaryLoss: cmu_softmax_map_fwd + _bwd, keep = [1]", "shape": [B, K, S, S]}, (2 * (4 * K + 4) + 4 * K) * npix, None)
    add("hausdorff_dt/loss_pass", lambda: ops.softmax_map_fwd(lo, fields, y, [1], "squared", tk, part), lambda: ops.softmax_map_bwd(lo, fields, y, [1], "squared", gk, dl),
        {"kernel": "HausdorffDTLoss: cmu_softmax_map_fwd + _bwd, keep = [1], f64 targets", "shape": [B, K, S, S]}, (2 * (4 * K + 4 + 8) + 4 * K) * npix, None)

    for fn in list(pairs.values()) + list(eager.values()):                     # warm-up: code objects, allocator
        timed(fn, 10)
    run = {k: (graph_of(fn, a.chunk), a.chunk, a.iters) for k, fn in pairs.items()}
    run.update({k: (fn, 1, a.class_iters) for k, fn in eager.items()})
    ms = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, (go, n, iters) in run.items():
            ms[k].append(timed(go, max(1, iters // n)) / n)

    lines = []
    for name, (rec, nbytes, yard) in meta.items():
        p = stats(ms[name])
        line = dict(rec, name=name, iters=a.iters, rounds=a.rounds, launch="graph", ms_pair=p, bytes_pair=nbytes,
                    TBps_pair=round(nbytes / (p["median"] * 1e-3) / 1e12, 3))
        if yard is not None:
            ym, yb = stats(ms[yard])["median"], meta[yard][1]
            line.update(yardstick=yard, time_ratio=round(p["median"] / ym, 4), time_per_byte_ratio=round((p["median"] / nbytes) / (ym / yb), 4))
        if name.endswith("loss_pass"):
            line.update(share_of_step=round(p["median"] / a.step_ms, 4), step_ms=a.step_ms)
        lines.append(line)
    for name in eager:
        p = stats(ms[name])
        lines.append({"name": name, "what": "distance maps of one class for the batch (transforms + cmu_distance_field"
                      + ("; softmax plane + threshold mask for the prediction" if name.startswith("hausdorff") else "") + ")",
                      "shape": [B, K, S, S], "iters": a.class_iters, "rounds": a.rounds, "launch": "eager", "ms": p,
                      "share_of_step": round(p["median"] / a.step_ms, 4), "step_ms": a.step_ms})
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
