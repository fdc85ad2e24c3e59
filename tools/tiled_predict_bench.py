#!/usr/bin/env python3
"""HIP-event timing of tiled prediction (csrc/tiled_predict.hip, cmunet_amd.infer.Segmenter) against the untiled code it sits beside.

(a) Whole call, at sizes a user runs: --images images of --side x --side (475: the reference's centre crop), tile 256, stride 128,
    UNet(out_classes=K, base 64, depth 5), f32 and f16, K = 1, 2, 8, tta None and 'd4':

      tiled     Segmenter(size=None, tile, stride, tta).segment(images, prob_class): extract_tiles + predict_probs per network batch +
                blend_tiles
      predict   UNet.predict(prob_class=...) over the same (tiles x copies, tile, tile) stack in the same network batches: the same
                network work ending in the label + one-probability head, without the three passes

    The three passes move about 8 + 8 K' + 1 bytes per tile pixel (extract: 4 read + 4 written; head_probs writes 4 K' that blend
    reads back; 1 label) beside the network's own traffic; the expected ratio is at most 1.05.

(b) Kernel level, 32 x 256 x 256 pixels of C = 64 channels with a pending BatchNorm + ReLU transform: cmu_head_probs (all codes 0, and
    the eight codes in turn) against cmu_head_predict with one probability.  Allowance: the ratio of their bytes per pixel,
    (C es + 4 K') / (C es + 5), plus 10 %.  Replayed as captured graphs of --chunk calls like tools/predict_bench.py.

Every figure is the median (with min and max) of --rounds windows; inside a round the two sides of every comparison are timed one
after the other.  Prints one JSON line per configuration.
    python tools/tiled_predict_bench.py [--rounds 5] [--out profiles/tiled_predict.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from predict_bench import graph_of, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="windows per figure (at least 5)")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--side", type=int, default=475)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--stride", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32, help="tiles per network call")
    ap.add_argument("--iters", type=int, default=1000, help="kernel-level calls per timed window")
    ap.add_argument("--chunk", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    from cmunet_amd import infer, ops
    from cmunet_amd.model import UNet
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    lines = []

    # (a) whole call
    if not a.no_model:
        images = torch.randn(a.images, a.side, a.side, generator=g).to(dev)
        for dt in ("f32", "f16"):
            for K in (1, 2, 8):
                torch.manual_seed(K)
                net = UNet(out_classes=K, base_ch=64, depth=5, dtype=dt).to(dev).eval()
                for tta in (None, "d4"):
                    seg = infer.Segmenter(net, size=None, batch=a.batch, tile=a.tile, stride=a.stride, tta=tta)
                    grid, _, _ = seg._grid(a.side, a.side, images.device)
                    stack = ops.extract_tiles(images, grid, "reflect")
                    pc = max(K, 1) - 1

                    def tiled(seg=seg, pc=pc):
                        return seg.segment(images, prob_class=pc)

                    def predict(net=net, stack=stack, pc=pc):
                        return [net.predict(stack[c0:c0 + a.batch], prob_class=pc) for c0 in range(0, stack.shape[0], a.batch)]

                    timed(tiled, 1)
                    timed(predict, 1)
                    ms = {"tiled": [], "predict": []}
                    for _ in range(a.rounds):
                        ms["predict"].append(timed(predict, 1))
                        ms["tiled"].append(timed(tiled, 1))
                    KP = max(K, 1)
                    lines.append({"level": "model", "model": f"UNet(out_classes={K}, base_ch=64, depth=5)", "dtype": dt, "K": K, "tta": tta or "none",
                                  "images": [a.images, a.side, a.side], "tile": a.tile, "stride": a.stride, "tiles": int(stack.shape[0]),
                                  "batch": a.batch, "rounds": a.rounds, "launch": "eager",
                                  "pass_bytes_per_tile_pixel": 8 + 8 * KP + 1,
                                  "ms": {k: stats(v) for k, v in ms.items()},
                                  "tiled_over_predict": stats([t / p for t, p in zip(ms["tiled"], ms["predict"])]), "expected_at_most": 1.05})
                    print(json.dumps(lines[-1]), flush=True)
                    del stack, seg
                del net
                torch.cuda.empty_cache()

    # (b) kernel level
    if not a.no_kernel:
        B, S, C = 32, 256, 64
        npix = B * S * S
        fns, meta = {}, {}
        for dt, tdt, es in (("f32", torch.float32, 4), ("f16", torch.float16, 2)):
            x = torch.randn(B, S, S, C, generator=g).to(tdt).to(dev)
            act = ops.Act(x, 0, C, (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.3).to(dev))
            codes = (torch.arange(B) % 8).to(torch.uint8).to(dev)
            for K in (1, 2, 8):
                KP = max(K, 1)
                w, b = (torch.randn(K, C, generator=g) / 8).to(dev), (torch.randn(K, generator=g) * 0.2).to(dev)
                labels = torch.empty(B, S, S, dtype=torch.uint8, device=dev)
                prob = torch.empty(B, S, S, device=dev)
                probs = torch.empty(B, KP, S, S, device=dev)
                name = f"{dt}/K{K}"
                fns[name + ":predict_prob"] = lambda act=act, w=w, b=b, labels=labels, prob=prob, K=K: ops.head_predict(act, w, b, labels, prob, K - 1)
                fns[name + ":probs"] = lambda act=act, w=w, b=b, probs=probs: ops.head_probs(act, w, b, probs)
                fns[name + ":probs_d4"] = lambda act=act, w=w, b=b, probs=probs, codes=codes: ops.head_probs(act, w, b, probs, codes, True)
                rd = C * es
                meta[name] = ({"level": "kernel", "dtype": dt, "K": K, "shape": [B, S, S, C]},
                              {"predict_prob": (rd + 5) * npix, "probs": (rd + 4 * KP) * npix, "probs_d4": (rd + 4 * KP + 1.0 / (S * S)) * npix},
                              (rd + 4 * KP) / (rd + 5) + 0.10)
        for fn in fns.values():
            timed(fn, 10)
        run = {k: graph_of(fn, a.chunk) for k, fn in fns.items()}
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, go in run.items():
                ms[k].append(timed(go, max(1, a.iters // a.chunk)) / a.chunk)
        for name, (rec, nbytes, allow) in meta.items():
            st = {k: stats(ms[f"{name}:{k}"]) for k in nbytes}
            lines.append(dict(rec, iters=a.iters, rounds=a.rounds, launch="graph", ms=st, bytes={k: int(v) for k, v in nbytes.items()},
                              TBps={k: round(nbytes[k] / (st[k]["median"] * 1e-3) / 1e12, 3) for k in nbytes},
                              probs_over_predict_prob=stats([p / h for p, h in zip(ms[name + ":probs"], ms[name + ":predict_prob"])]),
                              probs_d4_over_predict_prob=stats([p / h for p, h in zip(ms[name + ":probs_d4"], ms[name + ":predict_prob"])]),
                              allowance=round(allow, 4)))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
