#!/usr/bin/env python3
"""HIP-event timing of the fused prediction head (cmu_head_predict, csrc/predict.hip) against the route it replaces.

Kernel level, at B x S x S pixels of C = 64 channels with a pending BatchNorm + ReLU transform (what the last decoder layer hands the
head), for K = 1, 2, 8 and f32 / f16 activations:

  (a) head       cmu_conv1x1_head_fwd alone: fp32 NCHW logits (reads C sizeof(dt) bytes per pixel, writes 4 K)
  (b) head+argmax  (a) + logits.argmax(1).to(torch.uint8) (K = 1: (logits[:, 0] > t).to(torch.uint8)): what a user of the logits runs
  (c) predict    cmu_head_predict: uint8 labels (reads the same bytes, writes 1)
  (d) predict+prob  cmu_head_predict with the probability of one class (writes 5)

Model level: UNet.predict against model.eval()(x) + argmax + cast at base 64, depth 5 (--model-batch images of S x S).

Every figure is the median (with min and max) of --rounds windows; inside a round every configuration is timed once, one after the
other, so that clock drift hits all alike.  The kernel-level calls are replayed as captured graphs of --chunk calls (a linear chain on
one stream), so that a window measures the device and not the host's launch rate; every shape is warmed up first.
Prints one JSON line per configuration.
    python tools/predict_bench.py [--iters 1000] [--rounds 5] [--out profiles/predict.jsonl]"""
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
    ap.add_argument("--iters", type=int, default=1000, help="kernel-level calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per figure (at least 5); every configuration is timed once per round")
    ap.add_argument("--chunk", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--eager", action="store_true", help="time plain calls instead of captured graphs")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--model-batch", type=int, default=32)
    ap.add_argument("--model-iters", type=int, default=5, help="whole-model calls per timed window")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    from cmunet_amd import ops
    from cmunet_amd.model import UNet
    B, S, C = a.batch, a.size, 64
    npix = B * S * S
    g = torch.Generator().manual_seed(0)
    dev = "cuda"
    fns, meta = {}, {}
    for dt, tdt, es in (("f32", torch.float32, 4), ("f16", torch.float16, 2)):
        x = torch.randn(B, S, S, C, generator=g).to(tdt).to(dev)
        act = ops.Act(x, 0, C, (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.3).to(dev))
        for K in (1, 2, 8):
            w, b = (torch.randn(K, C, generator=g) / 8).to(dev), (torch.randn(K, generator=g) * 0.2).to(dev)
            logits = torch.empty(B, K, S, S, device=dev)
            labels = torch.empty(B, S, S, dtype=torch.uint8, device=dev)
            prob = torch.empty(B, S, S, device=dev)
            name = f"{dt}/K{K}"

            def head(act=act, w=w, b=b, logits=logits):
                ops.conv1x1_head_fwd(act, w, b, logits)

            def head_argmax(act=act, w=w, b=b, logits=logits, K=K):
                ops.conv1x1_head_fwd(act, w, b, logits)
                return (logits[:, 0] > 0.0).to(torch.uint8) if K == 1 else logits.argmax(1).to(torch.uint8)

            fns[name + ":head"] = head
            fns[name + ":head_argmax"] = head_argmax
            fns[name + ":predict"] = lambda act=act, w=w, b=b, labels=labels: ops.head_predict(act, w, b, labels)
            fns[name + ":predict_prob"] = lambda act=act, w=w, b=b, labels=labels, prob=prob, K=K: ops.head_predict(act, w, b, labels, prob, K - 1)
            rd = C * es
            meta[name] = ({"level": "kernel", "dtype": dt, "K": K, "shape": [B, S, S, C]},
                          {"head": (rd + 4 * K) * npix, "head_argmax": (rd + 4 * K + (4 * K + 8) + (8 + 1) if K > 1 else rd + 4 + (4 + 1) + (1 + 1)) * npix,
                           "predict": (rd + 1) * npix, "predict_prob": (rd + 5) * npix})
    for fn in fns.values():                     # warm-up of every shape: code objects, allocator
        timed(fn, 10)
    run = {k: (fn, 1) if a.eager else (graph_of(fn, a.chunk), a.chunk) for k, fn in fns.items()}
    ms = {k: [] for k in fns}
    # whole model: eager calls (tens of launches each; milliseconds per call)
    mfns = {}
    if not a.no_model:
        xm = torch.randn(a.model_batch, S, S, generator=g).to(dev)
        for dt in ("f32", "f16"):
            torch.manual_seed(1)
            net = UNet(out_classes=2, base_ch=64, depth=5, dtype=dt).to(dev).eval()

            def logits_route(net=net):
                with torch.no_grad():
                    return net(xm).argmax(1).to(torch.uint8)

            mfns[f"{dt}:eval_argmax"] = logits_route
            mfns[f"{dt}:predict"] = lambda net=net: net.predict(xm)
        for fn in mfns.values():
            timed(fn, 3)
        ms.update({k: [] for k in mfns})
    for _ in range(a.rounds):
        for k, (go, n) in run.items():
            ms[k].append(timed(go, max(1, a.iters // n)) / n)
        for k, fn in mfns.items():
            ms[k].append(timed(fn, a.model_iters))

    def tbs(nbytes, m):
        return round(nbytes / (m * 1e-3) / 1e12, 3)

    lines = []
    for name, (rec, nbytes) in meta.items():
        st = {k: stats(ms[f"{name}:{k}"]) for k in nbytes}
        # per round: the fused kernel over the logits kernel of the same round
        ratio = stats([p / h for p, h in zip(ms[name + ":predict"], ms[name + ":head"])])
        ratio_prob = stats([p / h for p, h in zip(ms[name + ":predict_prob"], ms[name + ":head"])])
        ratio_route = stats([p / h for p, h in zip(ms[name + ":predict"], ms[name + ":head_argmax"])])
        lines.append(dict(rec, iters=a.iters, rounds=a.rounds, launch="eager" if a.eager else "graph",
                          ms={k: v for k, v in st.items()}, bytes=nbytes, TBps={k: tbs(nbytes[k], st[k]["median"]) for k in nbytes},
                          predict_over_head=ratio, predict_prob_over_head=ratio_prob, predict_over_head_argmax=ratio_route))
    if mfns:
        for dt in ("f32", "f16"):
            e, p = stats(ms[f"{dt}:eval_argmax"]), stats(ms[f"{dt}:predict"])
            lines.append({"level": "model", "model": "UNet(out_classes=2, base_ch=64, depth=5)", "dtype": dt, "shape": [a.model_batch, S, S],
                          "iters": a.model_iters, "rounds": a.rounds, "launch": "eager", "ms": {"eval_argmax": e, "predict": p},
                          "predict_over_eval_argmax": stats([x / y for x, y in zip(ms[f"{dt}:predict"], ms[f"{dt}:eval_argmax"])])})
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
