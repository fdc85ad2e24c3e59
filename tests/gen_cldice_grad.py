#!/usr/bin/env python3
"""Writes tests/golden/cldice_grad.npz: the reference's own ``soft_cldice(threshold=None, activation='softmax', ...)``
(Finetuning/metrics.py:401-431) run in fp64 with autograd -- loss and d loss / d logits -- for tests/test_cpu_cldice_grad.py (the
restatements) and tests/test_gpu_cldice_grad_fp64.py (the HIP kernels).

Needs torch and numpy and the reference tree:   python3 tests/gen_cldice_grad.py /path/to/reference
(``metrics.py`` imports scikit-image at module level; it is imported behind a stub created in a temp dir, as oracle/gen_golden.py does.)

Cases at B 2, 12 x 20: (K, ignore_channels, exclude_background) of CASES, each once with random logits and random one-hot targets
("soft") and once with logits scaled until plateaus of exact 0 / 1 probabilities appear ("sat").
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "cldice_grad.npz")
B, H, W = 2, 12, 20
CASES = ((2, [0], False), (3, None, False), (3, [0], False), (4, None, True), (4, [1], True))


def import_reference(ref):
    stub = tempfile.mkdtemp(prefix="skimage_stub_")
    os.makedirs(os.path.join(stub, "skimage"))
    with open(os.path.join(stub, "skimage", "__init__.py"), "w") as f:
        f.write("from . import morphology, measure\n")
    with open(os.path.join(stub, "skimage", "morphology.py"), "w") as f:
        f.write("def skeletonize(*a, **k):\n    raise NotImplementedError\ndef skeletonize_3d(*a, **k):\n    raise NotImplementedError\n")
    with open(os.path.join(stub, "skimage", "measure.py"), "w") as f:
        f.write("def find_contours(*a, **k):\n    raise NotImplementedError\n")
    sys.path.insert(0, stub)
    sys.path.insert(0, os.path.join(ref, "Finetuning"))
    import metrics as ref_metrics  # noqa
    return ref_metrics


def make_inputs(K, regime, seed):
    """fp32-representable logits (so that the device sees the very same numbers) and a random one-hot target."""
    rs = np.random.RandomState(seed)
    cls = rs.randint(0, K, (B, H, W))
    y = np.eye(K)[cls].transpose(0, 3, 1, 2).copy()
    logits = rs.standard_normal((B, K, H, W)) + 1.5 * y * (rs.rand(B, 1, H, W) < 0.7)
    if regime == "sat":
        # blocks of one winning class 800 above the rest (softmax gives exact 1 and exact 0 in fp64 and in fp32), soft elsewhere
        win = np.repeat(np.repeat(rs.randint(0, K, (B, H // 4, W // 4)), 4, 1), 4, 2)
        hard = np.repeat(np.repeat(rs.rand(B, H // 4, W // 4) < 0.6, 4, 1), 4, 2)
        logits = logits + 800.0 * np.eye(K)[win].transpose(0, 3, 1, 2) * hard[:, None]
    return logits.astype(np.float32).astype(np.float64), y


def main(ref):
    import torch
    M = import_reference(ref)
    out = {"cases": np.array([f"{K}|{'' if ign is None else ','.join(map(str, ign))}|{int(eb)}" for K, ign, eb in CASES]),
           "versions": np.array([f"torch {torch.__version__}", f"numpy {np.__version__}"])}
    for ci, (K, ign, eb) in enumerate(CASES):
        for regime in ("soft", "sat"):
            lg, y = make_inputs(K, regime, 4200 + 10 * ci + (regime == "sat"))
            x = torch.from_numpy(lg).requires_grad_(True)
            m = M.soft_cldice(threshold=None, activation="softmax", ignore_channels=ign, exclude_background=eb)
            loss = m(x, torch.from_numpy(y))
            loss.backward()
            p = torch.softmax(x.detach(), 1)
            exact = float(((p == 0) | (p == 1)).double().mean())
            key = f"c{ci}_{regime}"
            out[key + "_logits"], out[key + "_target"] = lg.astype(np.float32), y.astype(np.float32)
            out[key + "_loss"], out[key + "_dlogits"] = np.float64(loss.item()), x.grad.numpy()
            print(f"{key}: K {K} ignore {ign} exclude_background {eb}: loss {loss.item():.15f}  max|g| {x.grad.abs().max().item():.3e}  "
                  f"exact 0/1 probabilities {100 * exact:.1f} %", flush=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


def load(path=OUT):
    """[(name, K, ignore_channels, exclude_background, regime, logits, target, loss, dlogits)] with fp64 arrays."""
    z = np.load(path)
    rows = []
    for ci, c in enumerate(z["cases"]):
        K, ign, eb = str(c).split("|")
        ign = None if ign == "" else [int(v) for v in ign.split(",")]
        for regime in ("soft", "sat"):
            key = f"c{ci}_{regime}"
            rows.append((key, int(K), ign, bool(int(eb)), regime, z[key + "_logits"].astype(np.float64), z[key + "_target"].astype(np.float64),
                         float(z[key + "_loss"]), z[key + "_dlogits"]))
    return rows


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
