#!/usr/bin/env python3
"""HIP-event timing of soft-clDice at 32 x K x 256 x 256, K = 2 / 4 / 8 with ignore_channels=[0] and fp64 one-hot targets
(csrc/cldice_grad.hip, the clDice kernels of csrc/heads.hip):
  thr_old       the thresholded metric on the driver's kernel sequence (cmu_softmax2_threshold -> cmu_soft_skeleton x 2 -> sums; K = 2)
  thr_new       the thresholded metric through the planes kernel (any K)
  soft_fwd      the differentiable forward (planes, the saving skeleton, the target's skeleton, sums)
  soft_fwd_bwd  the same plus cmu_soft_skeleton_bwd and cmu_softmax_planes_bwd
  module_*      metrics.soft_cldice(threshold=None) called as training calls it (autograd, allocator, Python), plain launches
The kernel-level figures replay captured graphs of --chunk calls (a linear chain on one stream) unless --eager, so that they measure
the device and not the host's launch rate; every round times all figures one after the other (old and new alternate), and each
figure is reported as min / median / max over --rounds rounds.  Next to each time: the bytes its passes must move (every array of
n = B Kk H W floats read or written once per kernel that touches it), the rate that implies, the kernel launches, and -- with
--step-ms-f16 / --step-ms-f32, the times of one finetuning step from tools/finetune_step.py in the same run -- the share of a step.
    python tools/cldice_bench.py [--rounds 5] [--iters 200] [--out profiles/cldice_grad.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.seg_criterion_bench import graph_of, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=10, help="calls per captured graph")
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--step-ms-f16", type=float, default=None)
    ap.add_argument("--step-ms-f32", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmunet_amd import _lib, metrics as M, ops
    B, S, N = a.batch, a.size, 10
    npix = B * S * S
    g = torch.Generator().manual_seed(0)
    L = _lib.lib()
    fns, info, hold = {}, {}, []
    for K in (2, 4, 8):
        keep = list(range(1, K))
        n = npix * len(keep)
        lo = (torch.randn(B, K, S, S, generator=g) * 2).cuda()
        y = torch.nn.functional.one_hot(torch.randint(0, K, (B, S, S), generator=g), K).permute(0, 3, 1, 2).contiguous().double().cuda()
        yp, yt, sp, st, G = (torch.empty(B * len(keep), S, S, device="cuda") for _ in range(5))
        ws = torch.empty(L.cmu_soft_skeleton_ws_bytes(n), dtype=torch.uint8, device="cuda")
        kept = torch.empty(L.cmu_soft_skeleton_save_ws_bytes(n, N), dtype=torch.uint8, device="cuda")
        bws = torch.empty(L.cmu_soft_skeleton_bwd_ws_bytes(n), dtype=torch.uint8, device="cuda")
        sws = torch.empty(L.cmu_cldice_sums_ws_bytes(), dtype=torch.uint8, device="cuda")
        out4, dl = torch.empty(4, device="cuda"), torch.empty_like(lo)
        g4 = torch.tensor([-1e-6, 2e-7, -1.5e-6, 3e-7], dtype=torch.float64, device="cuda")
        hold.append((lo, y, yp, yt, sp, st, G, ws, kept, bws, sws, out4, dl, g4))

        def thr_new(lo=lo, y=y, keep=keep, yp=yp, yt=yt, sp=sp, st=st, ws=ws, sws=sws, out4=out4):
            ops.softmax_planes(lo, y, keep, 0.5, yp, yt)
            ops.soft_skeleton(yp, sp, N, ws)
            ops.soft_skeleton(yt, st, N, ws)
            ops.cldice_sums(sp, yt, st, yp, out4, sws)

        def soft_fwd(lo=lo, y=y, keep=keep, yp=yp, yt=yt, sp=sp, st=st, ws=ws, sws=sws, out4=out4, kept=kept):
            ops.softmax_planes(lo, y, keep, None, yp, yt)
            ops.soft_skeleton_save(yp, sp, N, kept)
            ops.soft_skeleton(yt, st, N, ws)
            ops.cldice_sums(sp, yt, st, yp, out4, sws)

        def soft_fwd_bwd(f=soft_fwd, lo=lo, keep=keep, yp=yp, yt=yt, st=st, kept=kept, G=G, g4=g4, bws=bws, dl=dl):
            f()
            ops.soft_skeleton_bwd(yp, kept, N, G, g4=g4, y_true=yt, skel_true=st, ws=bws)
            ops.softmax_planes_bwd(lo, G, keep, dl)

        if K == 2:
            y1 = y[:, 1].float().contiguous()
            hold.append(y1)

            def thr_old(lo=lo, y1=y1, yp=yp, sp=sp, st=st, ws=ws, sws=sws, out4=out4):
                ops.softmax2_threshold(lo, 0.5, yp)
                ops.soft_skeleton(yp, sp, N, ws)
                ops.soft_skeleton(y1, st, N, ws)
                ops.cldice_sums(sp, y1, st, yp, out4, sws)
            fns["thr_old2"] = thr_old
            info["thr_old2"] = (4 * 2 * npix + 4 * n + 2 * 24 * (N + 1) * n + 16 * n, 1 + 4 * (N + 1) + 2)
        fns[f"thr_new{K}"], fns[f"soft_fwd{K}"], fns[f"soft_fwd_bwd{K}"] = thr_new, soft_fwd, soft_fwd_bwd
        # bytes: planes (logits 4K + fp64 target 8K per pixel in, 8n out); a skeleton: erode 8n + update 16n per level (the saving one
        # 2n more: its selection codes); sums 16n; backward: ten float arrays and three code bytes per level kernel (43n), T_1's gather
        # 18n, the final kernel 17n; planes backward 8K per pixel + 4n
        fwd_bytes = 12 * K * npix + 8 * n + 2 * 24 * (N + 1) * n + 16 * n
        save_bytes = 2 * (N + 1) * n
        bwd_bytes = 43 * (N + 1) * n + 35 * n + 8 * K * npix + 4 * n
        fwd_launches = 1 + 4 * (N + 1) + 2
        info[f"thr_new{K}"] = (fwd_bytes, fwd_launches)
        info[f"soft_fwd{K}"] = (fwd_bytes + save_bytes, fwd_launches)
        info[f"soft_fwd_bwd{K}"] = (fwd_bytes + save_bytes + bwd_bytes, fwd_launches + (N + 2) + 1 + 1)
        crit = M.soft_cldice(threshold=None, activation="softmax", ignore_channels=[0])
        lor = lo.clone().requires_grad_(True)
        hold.append(lor)
        fns[f"module_fwd{K}"] = (lambda crit=crit, lor=lor, y=y: crit(lor, y))
        fns[f"module_fwd_bwd{K}"] = (lambda crit=crit, lor=lor, y=y: crit(lor, y).backward())
        info[f"module_fwd{K}"], info[f"module_fwd_bwd{K}"] = info[f"soft_fwd{K}"], info[f"soft_fwd_bwd{K}"]
    for fn in fns.values():
        timed(fn, 3)
    run = {}
    for k, fn in fns.items():
        run[k] = (fn, 1) if (a.eager or k.startswith("module")) else (graph_of(fn, a.chunk), a.chunk)
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, (go, n) in run.items():
            ms[k].append(timed(go, max(1, a.iters // n)) / n)
    kept_bytes = L.cmu_soft_skeleton_save_ws_bytes(npix, N)
    lines = []
    for k in fns:
        st_ = stats(ms[k])
        nbytes, launches = info[k]
        rec = {"what": k.rstrip("0123456789"), "K": int(k[-1]), "shape": [B, int(k[-1]), S, S], "num_iter": N, "rounds": a.rounds, "iters": a.iters,
               "launch": "eager" if (a.eager or k.startswith("module")) else "graph", "ms": st_, "bytes": nbytes,
               "GBps": round(nbytes / (st_["median"] * 1e-3) / 1e9, 1), "kernel_launches": launches}
        if "soft" in k or "module" in k:
            rec["kept_bytes_per_plane_stack"] = kept_bytes
        for name, step in (("share_of_f16_step", a.step_ms_f16), ("share_of_f32_step", a.step_ms_f32)):
            if step:
                rec[name] = round(st_["median"] / step, 4)
                rec[name.replace("share_of", "ms").replace("_step", "_finetune_step")] = step
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
