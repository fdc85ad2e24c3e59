"""numpy restatement of the probability histogram and its curves (csrc/prob_hist.hip, csrc/hist_curves.h): the bin rule in float32, counts by
np.add.at, the fixed-point sums with Python integers, suffix sums, the reference's score formulas (Finetuning/metrics.py:135-198) in Python
floats, and AUROC / average precision / ECE / MCE as exact rationals (fractions.Fraction).  tests/test_cpu_prob_hist_ref.py pins it to
brute-force (p > j / NB) & y counts and to scikit-learn on the bin indices."""
from fractions import Fraction

import numpy as np

SCORE_NAMES = ("dice", "iou", "precision", "recall", "specificity")
SELECT = {"dice": 0, "iou": 1, "youden": 2}


def clamp(p):
    """(float32 probabilities with NaN / negatives -> 0 and values above 1 -> 1, the mask of the elements that were changed)."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (p >= 0) & (p <= 1)
        q = np.where(ok, p, np.where(p > 1, np.float32(1), np.float32(0))).astype(np.float32)
    return q, ~ok


def bins_of(p, NB):
    """ceil(p * NB) in float32 for clamped probabilities: bin b holds (b - 1) / NB < p <= b / NB, bin 0 holds p == 0."""
    return np.ceil(np.asarray(p, np.float32) * np.float32(NB)).astype(np.int64)


def positives(target, K):
    """(B,K,H,W) bool from one-hot planes (> 0.5) or a (B,H,W) uint8 label map (class c for plane c; one plane: label != 0)."""
    target = np.asarray(target)
    if target.dtype == np.uint8:
        if K == 1:
            return (target != 0)[:, None]
        return np.stack([target == c for c in range(K)], axis=1)
    return target > 0.5


def histogram(p, target, NB, pooled=True):
    """p (B,K,H,W) probabilities -> counts (Bout,K,2,NB+1) int64, conf (Bout,K,NB+1) of Python ints (object), invalid (Bout,K) int32."""
    p = np.asarray(p, np.float32)
    B, K = p.shape[:2]
    q, bad = clamp(p)
    b = bins_of(q, NB)
    y = positives(target, K).astype(np.int64)
    Bout = 1 if pooled else B
    img = np.zeros_like(b) if pooled else np.broadcast_to(np.arange(B)[:, None, None, None], b.shape)
    cls = np.broadcast_to(np.arange(K)[None, :, None, None], b.shape)
    counts = np.zeros((Bout, K, 2, NB + 1), np.int64)
    np.add.at(counts, (img, cls, y, b), 1)
    fixed = np.floor(q.astype(np.float64) * 2.0 ** 32).astype(np.int64)      # exact: a float32 times 2^32, at most 2^32
    assert p.size < 2 ** 30      # a bin's sum stays below 2^62: int64 adds are exact; handed out as Python integers
    conf64 = np.zeros((Bout, K, NB + 1), np.int64)
    np.add.at(conf64, (img, cls, b), fixed)
    conf = conf64.astype(object)
    invalid = np.zeros((Bout, K), np.int32)
    np.add.at(invalid, (img[bad], cls[bad]), 1)
    return counts, conf, invalid


def softmax32(logits):
    """Float64 softmax of float32 logits (for data whose probabilities stay away from the bin edges)."""
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def cum_counts(row):
    """row (2,NB+1) counts -> (4,NB+1) int64: tp, fp, fn, tn at threshold j / NB (predicted positive: bin > j)."""
    neg, pos = np.asarray(row[0], np.int64), np.asarray(row[1], np.int64)
    tp = np.concatenate([np.cumsum(pos[::-1])[::-1][1:], [0]])
    fp = np.concatenate([np.cumsum(neg[::-1])[::-1][1:], [0]])
    return np.stack([tp, fp, pos.sum() - tp, neg.sum() - fp])


def scores_at(tp, fp, fn, tn, eps=1e-7, beta=1.0):
    """The five formulas in Python floats, operation by operation as the reference writes them."""
    tp, fp, fn, tn = float(tp), float(fp), float(fn), float(tn)
    b2 = beta * beta
    return (((1.0 + b2) * tp + eps) / ((1.0 + b2) * tp + b2 * fn + fp + eps),
            (tp + eps) / (tp + fp + fn + eps),
            (tp + eps) / (tp + fp + eps),
            (tp + eps) / (tp + fn + eps),
            (tn + eps) / (tn + fp + eps))


def scores(cum, eps=1e-7, beta=1.0):
    return np.array([scores_at(*cum[:, j], eps=eps, beta=beta) for j in range(cum.shape[1])], np.float64).T


def selected(cum, j, select, eps=1e-7, beta=1.0):
    tp, fp, fn, tn = (float(v) for v in cum[:, j])
    if select == 2:
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(np.float64(tp) / np.float64(tp + fn) + np.float64(tn) / np.float64(tn + fp) - 1.0)
    return scores_at(tp, fp, fn, tn, eps, beta)[select]


def best(cum, select, eps=1e-7, beta=1.0):
    """(j, value): the first argmax over j = 1..NB-1; a NaN never replaces anything."""
    NB = cum.shape[1] - 1
    bj, bs = 1, selected(cum, 1, select, eps, beta)
    for j in range(2, NB):
        s = selected(cum, j, select, eps, beta)
        if s > bs:
            bj, bs = j, s
    return bj, bs


def summary_exact(row, conf_row=None):
    """(AUROC, AP, ECE, MCE) as Fractions, None where undefined (AUROC: an empty class; AP: no positive; ECE / MCE: no conf or no pixel)."""
    neg, pos = [int(v) for v in row[0]], [int(v) for v in row[1]]
    n = len(pos)
    P, N = sum(pos), sum(neg)
    above = [sum(pos[b + 1:]) for b in range(n)]
    auc = Fraction(sum(2 * neg[b] * above[b] + neg[b] * pos[b] for b in range(n)), 2 * P * N) if P and N else None
    ap = None
    if P:
        ap = Fraction(0)
        for b in range(n):
            if pos[b]:
                tp, fp = above[b] + pos[b], sum(neg[b:])
                ap += Fraction(pos[b], P) * Fraction(tp, tp + fp)
    ece = mce = None
    if conf_row is not None and P + N:
        gaps = [abs(Fraction(pos[b]) - Fraction(int(conf_row[b]), 2 ** 32)) for b in range(n)]
        ece = sum(gaps, Fraction(0)) / (P + N)
        mce = max([g / (pos[b] + neg[b]) for b, g in enumerate(gaps) if pos[b] + neg[b]], default=Fraction(0))
    return auc, ap, ece, mce
