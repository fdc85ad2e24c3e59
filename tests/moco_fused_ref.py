"""Float64 reference, error bounds and designed inputs of the fused MoCo InfoNCE + enqueue kernel (csrc/moco.hip:
``moco_fused_kernel`` behind ``cmu_moco_infonce_enqueue``).  Plain torch / numpy on the CPU, no GPU import; the conventions are those
of tests/elem_fp64_ref.py and tests/necks_fp64_ref.py: the reference takes what the kernel takes (the fp32 inputs as the kernel
receives them, the temperature as the fp32 value the C ABI passes), computes in float64 and returns next to each result the
MAGNITUDES its error bound is built from (for a sum: sum |terms|).  tests/test_cpu_moco_fused_ref.py proves the reference against
the oracle's float64 autograd and proves that the bounds are tight enough to see single faults; tests/test_gpu_moco_fused_fp64.py
holds the kernel to them.

The arithmetic restates moco2_module.py:160-175 and :256-285 as the header of moco.hip cites them:
  qn = q / max(|q|, 1e-12), kn likewise (F.normalize)          logits = [qn.kn, qn @ queue_old] / T, label 0
  loss = mean_b (logsumexp(logits_b) - logits_b0)              dq = (I - qn qn^T)(gpos kn + p @ queue_old^T) / max(|q|, 1e-12)
  with w = softmax(logits), gpos = (w_0 - 1) / (B T), p = w_1.. / (B T)
  queue[:, (ptr0 + i) mod K] = keys[i], ptr0 := 0 when it lies outside [0, K) (the kernel's documented guard), ptr' = (ptr0 + Nk) % K

BOUNDS (``bounds``).  U = 2^-24.  Every k below is the number of fp32 roundings on the kernel's own chain for that value, counted from
csrc/moco.hip (line numbers of that file) and csrc/common.h (block_sum4 = wave_sum + pairwise fold); none was fitted to an output.
  ns = ceil(D / 256) + 8      a block sum over D: the per-thread fma chain (moco.hip:93-96, 100-107, 247-252), six shuffle additions
                              (wave_sum) and the pairwise fold of four waves (block_sum4: 2)
  kn, qn        k = ns + 2    the sum of squares (ns), sqrtf (1), the division (1)                          moco.hip:93-103
  positive      k = 2 (ns + 2) + ns + 1   both normalised operands, the fma chain and its fold, / T         moco.hip:100-108
  logit         k = D + ns + 10           the issue's form (D + c): a wave's MFMA chain over its dq4 rows rounds at most twice per row
                              (product, accumulate) and 2 dq4 <= D + 4 (moco.hip:125, 138-151); c = 4 + the rounded qn operand (ns + 2) +
                              the three additions of the LDS fold + the division by T (moco.hip:165)
  exp           (|L - m| + 6) U relative: the subtraction's rounding enters the exponent, expf within 3 ulp  moco.hip:181, 184, 186
  se            nK = ceil(K / 256) + 9: per-thread chain, wave_sum (6), fold (2), + exp(pos - m)             moco.hip:181-182
  p, gpos       4 more: se * B, * T, the reciprocal, the product (moco.hip:183-184); gpos: the subtraction, B * T, the division (:186)
  G             k = 2 kchunk + splits: the MFMA chain of one K-split (product, accumulate: moco.hip:208-220) and the slab additions in
                split order on top of gpos kn (moco.hip:248-249)
  dq            the dot product (ns, moco.hip:251-253), qn * dot and the subtraction (2), the division by |q| (1) and |q| itself
                (ns + 2: its own chain and the fp32 form of the 1e-12 clamp)                                moco.hip:254
  loss          logf within 3 ulp (6), m + log se and - pos (2), / B (1), the float of the double total (1)  moco.hip:187, 272-274
The logit error is propagated exactly, not linearised: with e_j the bound of logit j and w the float64 softmax,
|logsumexp(l + d) - logsumexp(l)| <= log sum_j w_j exp(e_j) =: lse_err for every |d_j| <= e_j (Jensen for the lower side), and a
softmax weight moves by a factor within exp(+-(e_j + lse_err)).
"""
import math
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-12                                    # F.normalize's clamp (the kernel's 1e-12f differs from it by less than U, counted in dq)
TEMPS = (0.2, 0.07)
BETA = 0.6                                     # cosine between a query row and its positive key
SEAM_WEIGHT = 0.05                             # softmax weight every seam column must carry in some row (the builder aims at 0.08)
FAULT_FACTOR = 4.0

Case = namedtuple("Case", "B D K Nk ptr T")    # Nk None: ungathered (the kernel enqueues its own B keys)


def f32(x):
    return float(np.float32(x))


def cdiv(a, b):
    return -(-a // b)


def case_id(c):
    return f"B{c.B}-D{c.D}-K{c.K}-{'own' if c.Nk is None else 'Nk%d' % c.Nk}-ptr{c.ptr}-T{c.T}"


# ------------------------------------------------------------------------------------------------
# the launcher's geometry, restated (moco.hip: moco_splits, moco_align, cmu_moco_ws_bytes)
# ------------------------------------------------------------------------------------------------
def moco_splits(D, K):
    """-> (splits, kchunk): the K ranges of P3.  ~512 work items over the 128-row blocks of D, whole 32-column trips, at least one."""
    nblk = cdiv(D, 128)
    want = cdiv(512, nblk)
    kc = max(cdiv(cdiv(K, want), 32) * 32, 32)
    return cdiv(K, kc), kc


def _align(n):
    return cdiv(n, 64) * 64                    # floats -> 256-byte sections


def ws_sections(B, D, K):
    """The seven sections of the workspace in order, in floats: the barrier counters, qn, kn, qnT, rowst, L, the split-K slabs."""
    splits, _ = moco_splits(D, K)
    RT = cdiv(B, 32)
    return [("bar", 64), ("qn", _align(B * D)), ("kn", _align(B * D)), ("qnT", _align(RT * D * 32)), ("rowst", _align(B * 4)),
            ("L", _align(B * K)), ("slab", _align(splits * B * D))]


def ws_bytes(B, D, K):
    return 4 * sum(n for _, n in ws_sections(B, D, K))


def seam_columns(D, K):
    """Queue columns at the seams of the kernel's tilings: the 16-byte load (0, 3, 4), the 128-column block of P1 (127, 128), the
    K-split of P3 (kchunk - 1, kchunk), the last 16-byte piece and the last column -- where they exist."""
    _, kc = moco_splits(D, K)
    return sorted({j for j in (0, 3, 4, 127, 128, kc - 1, kc, K - 4, K - 1) if 0 <= j < K})


def effective_ptr(ptr, K):
    return ptr if 0 <= ptr < K else 0


def ring_columns(ptr, Nk, K):
    p0 = effective_ptr(ptr, K)
    return [(p0 + i) % K for i in range(Nk)]


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
FAULTS = ("drop_column", "drop_last_d", "late_queue", "no_pos_in_lse", "no_projection", "one_T_less", "shift_enqueue")


def reference(q_raw, k_raw, keys_all, queue, ptr, T, fault=None):
    """What cmu_moco_infonce_enqueue computes, in float64 -> dict: kn, losses (per row), loss, dq, queue (after the enqueue), ptr (new),
    and qn, nq, nk, logits ((B, 1 + K), positive first), w, p, gpos, g, dot, mag_pos, mag_L for the bounds.
    ``fault`` = (name, arg) puts ONE deliberate mistake into the arithmetic (tests/test_cpu_moco_fused_ref.py: the bounds must see it):
    drop_column j: column j missing from p @ queue^T; drop_last_d: the last d missing from q @ queue; late_queue: logits and p @ queue^T
    on the queue AFTER the enqueue; no_pos_in_lse: the positive logit missing from the log-sum-exp; no_projection: (I - qn qn^T) left
    out; one_T_less: d loss / d logit without its 1 / T; shift_enqueue: the ring written one column further."""
    fname, farg = fault if fault is not None else (None, None)
    assert fname is None or fname in FAULTS
    q, k, Q = q_raw.double(), k_raw.double(), queue.double()
    T = f32(T)
    B, D = q.shape
    K = Q.shape[1]
    nq = q.norm(dim=1).clamp_min(EPS)
    nk = k.norm(dim=1).clamp_min(EPS)
    qn, kn = q / nq[:, None], k / nk[:, None]
    keys = kn if keys_all is None else keys_all.double()
    Nk = keys.shape[0]
    cols = ring_columns(ptr, Nk, K)
    if fname == "shift_enqueue":
        cols = [(j + 1) % K for j in cols]
    Qnew = Q.clone()
    Qnew[:, cols] = keys.t()
    Qu = Qnew if fname == "late_queue" else Q
    lneg = qn[:, :-1] @ Qu[:-1] if fname == "drop_last_d" else qn @ Qu
    logits = torch.cat([(qn * kn).sum(1, keepdim=True), lneg], 1) / T
    lse = torch.logsumexp(logits[:, 1:] if fname == "no_pos_in_lse" else logits, 1)
    w = torch.exp(logits - lse[:, None])
    losses = lse - logits[:, 0]
    scale = 1.0 / B if fname == "one_T_less" else 1.0 / (B * T)
    gpos, p = (w[:, 0] - 1.0) * scale, w[:, 1:] * scale
    pg = p
    if fname == "drop_column":
        pg = p.clone()
        pg[:, farg] = 0.0
    g = gpos[:, None] * kn + pg @ Qu.t()
    dot = (g * qn).sum(1)
    dq = (g if fname == "no_projection" else g - qn * dot[:, None]) / nq[:, None]
    return {"kn": kn, "qn": qn, "nq": nq, "nk": nk, "losses": losses, "loss": losses.mean(), "dq": dq, "queue": Qnew,
            "ptr": (effective_ptr(ptr, K) + Nk) % K, "logits": logits, "w": w, "p": p, "gpos": gpos, "g": g, "dot": dot, "T": T,
            "mag_pos": (qn * kn).abs().sum(1) / T, "mag_L": qn.abs() @ Q.abs() / T}


def bounds(ref, queue):
    """Elementwise error bounds of the kernel's kn, loss and dq around ``ref`` (module docstring: every k and where it was counted)
    -> dict kn (B, D), loss (scalar), dq (B, D), and the intermediate ones (logit, p_rel, g) for the record."""
    Qa = queue.double().abs()
    qn, kn, nq, w, p, gpos, g, dot, T = (ref[n] for n in ("qn", "kn", "nq", "w", "p", "gpos", "g", "dot", "T"))
    B, D = qn.shape
    K = Qa.shape[1]
    splits, kchunk = moco_splits(D, K)
    ns = cdiv(D, 256) + 8
    e_n = (ns + 2) * U                                                      # k=ns+2: relative error of an element of qn / kn
    b_kn = e_n * kn.abs()
    e_pos = (2 * (ns + 2) + ns + 1) * U * ref["mag_pos"]                   # k=2(ns+2)+ns+1
    e_L = (D + ns + 10) * U * ref["mag_L"]                                  # k=D+ns+10
    e = torch.cat([e_pos[:, None], e_L], 1)
    lse_err = torch.log1p((w * torch.expm1(e)).sum(1))                      # the logit errors through the log-sum-exp, exactly
    logits = ref["logits"]
    m = logits.max(1).values
    rng = (m[:, None] - logits).max(1).values + 2 * e.max(1).values         # |L - m| of the kernel's own logits
    r_exp = (rng + 6) * U                                                   # the subtraction into the exponent, expf within 3 ulp
    r_se = r_exp + (cdiv(K, 256) + 9) * U                                   # k=nK on a sum of positive terms: relative
    logse = (torch.logsumexp(logits, 1) - m).abs()
    # loss: row term (m + logf(se) - pos) / B, summed in double, rounded to float
    row = (lse_err + e_pos - torch.log1p(-r_se) + 6 * U * logse + 2 * U * (m.abs() + logse + logits[:, 0].abs())
           + U * ref["losses"].abs()) / B
    b_loss = row.sum() + U * ref["loss"].abs()
    # softmax weights: relative error of w_j as the kernel forms it from its own logits, times the propagated logit error
    own = r_exp + r_se + 4 * U                                              # se * B, * T, the reciprocal, the product
    rho = torch.exp(e + lse_err[:, None]) * (1 + own[:, None]) - 1          # (B, 1 + K)
    b_gpos = (w[:, 0] * rho[:, 0] + U * (1 - w[:, 0]).abs()) / (B * T) + 2 * U * gpos.abs()
    G_mag = p @ Qa.t()
    mag_g = (gpos[:, None] * kn).abs() + G_mag
    b_g = (kn.abs() * b_gpos[:, None] + (gpos[:, None] * kn).abs() * (e_n + U) + (p * rho[:, 1:]) @ Qa.t()
           + 2 * kchunk * U * G_mag + splits * U * mag_g)                   # k=2 kchunk + splits
    b_dot = (b_g * qn.abs() + (g * qn).abs() * (e_n + ns * U)).sum(1)       # k=ns on the dot's own chain
    qd = (qn * dot[:, None]).abs()
    b_dq = ((b_g + qn.abs() * b_dot[:, None] + qd * (e_n + U) + U * (g.abs() + qd)) / nq[:, None]
            + ref["dq"].abs() * (1 + ns + 2) * U)                           # the division, |q| (ns + 1) and its fp32 clamp (1)
    return {"kn": b_kn, "loss": b_loss, "dq": b_dq, "logit": e, "p_rel": rho, "g": b_g,
            "k": {"ns": ns, "kn": ns + 2, "pos": 2 * (ns + 2) + ns + 1, "logit": D + ns + 10, "se": cdiv(K, 256) + 9,
                  "G": 2 * kchunk + splits, "dot": ns}}


# ------------------------------------------------------------------------------------------------
# designed inputs
# ------------------------------------------------------------------------------------------------
def _unit(t, dim):
    return t / t.norm(dim=dim, keepdim=True)


def zero_rows(B):
    """(all-zero key row, all-zero query row): distinct rows, present from two / three rows on; from four rows on they are rows of
    scale 1, so that both scaled rows of q_raw and of k_raw stay."""
    if B >= 4:
        return 1, 3
    return (B - 1 if B >= 2 else None), (B - 2 if B >= 3 else None)


def build_case(c):
    """Designed fp32 inputs of a Case -> dict q_raw, k_raw, keys_all (None: ungathered), queue (D, K) with unit columns, ptr, T, seams
    (column -> the row whose qn it was mixed towards).  Every key is mixed towards its query (cosine BETA) so that no row's soft-max is
    saturated by the queue alone; rows are scaled by 1, 1e4 and 1e-4 in turn; one key row and one query row are all zero
    (``zero_rows``); every seam column is turned towards a row's qn until it carries at least 0.08 of that row's soft-max."""
    B, D, K = c.B, c.D, c.K
    g = torch.Generator().manual_seed(1000003 * B + 1009 * D + 7 * K + 31 * (c.Nk or 0) + 3 * (c.ptr + 11) + int(round(c.T * 100)))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    qdir = _unit(rn(B, D), 1)
    kdir = _unit(BETA * qdir + math.sqrt(1 - BETA * BETA) * _unit(rn(B, D), 1), 1)
    rows = torch.arange(B)
    sq = torch.tensor([1.0, 1e4, 1e-4], dtype=torch.float64)[rows % 3] * (0.5 + torch.rand(B, generator=g, dtype=torch.float64))
    sk = torch.tensor([1e-4, 1.0, 1e4], dtype=torch.float64)[rows % 3] * (0.5 + torch.rand(B, generator=g, dtype=torch.float64))
    q_raw, k_raw = (qdir * sq[:, None]).float(), (kdir * sk[:, None]).float()
    zk, zq = zero_rows(B)
    if zk is not None:
        k_raw[zk] = 0.0
    if zq is not None:
        q_raw[zq] = 0.0
    base = _unit(rn(D, K), 0)
    qn = q_raw.double() / q_raw.double().norm(dim=1, keepdim=True).clamp_min(EPS)
    live = [b for b in range(B) if b != zq]
    seams = {j: live[i % len(live)] for i, j in enumerate(seam_columns(D, K))}
    alpha = {j: 0.3 for j in seams}
    T = f32(c.T)
    for _ in range(16):
        queue = base.clone()
        for j, b in seams.items():
            perp = base[:, j] - (base[:, j] @ qn[b]) * qn[b]
            queue[:, j] = alpha[j] * qn[b] + math.sqrt(1 - alpha[j] ** 2) * perp / perp.norm()
        queue = queue.float()
        kn = k_raw.double() / k_raw.double().norm(dim=1, keepdim=True).clamp_min(EPS)
        w = torch.softmax(torch.cat([(qn * kn).sum(1, keepdim=True), qn @ queue.double()], 1) / T, 1)
        lag = [j for j, b in seams.items() if float(w[b, 1 + j]) < 0.08]
        if not lag:
            break
        for j in lag:
            alpha[j] = min(alpha[j] + 0.05, 0.98)
    else:
        raise AssertionError(f"{case_id(c)}: seam columns {lag} cannot reach a soft-max weight of 0.08")
    keys_all = None
    if c.Nk is not None:
        assert c.Nk >= B
        keys_all = torch.cat([kn.float(), _unit(rn(c.Nk - B, D), 1).float()])
    return {"case": c, "q_raw": q_raw, "k_raw": k_raw, "keys_all": keys_all, "queue": queue, "ptr": c.ptr, "T": T, "seams": seams}


def second_step_inputs(data):
    """Rows for a second call on the queue the first one left: the queries are the first call's keys (their logits on the freshly
    enqueued columns are the largest of the row), the keys the first call's queries."""
    q2, k2 = data["k_raw"].clone(), data["q_raw"].clone()
    return q2, k2


# ------------------------------------------------------------------------------------------------
# the cases: (B, D, K) of the issue, each with the pointers and temperatures it runs
# ------------------------------------------------------------------------------------------------
def _cases():
    out = []

    def add(B, D, K, Nk, runs):
        out.extend(Case(B, D, K, Nk, ptr, T) for ptr, T in runs)

    # the smallest legal shape: one 16-byte queue load, Nk = 1, a grid of 1; every pointer rule
    add(1, 8, 4, None, [(0, 0.2), (2, 0.07), (3, 0.07), (-5, 0.2), (4, 0.07), (7, 0.2)])
    # D odd and below the wave quarters: dq4 = 2, wave 3 gets no rows
    add(3, 5, 12, None, [(0, 0.07), (6, 0.2), (9, 0.2)])
    # D % 4 != 0, the last wave's quarter ragged, K < 128.  (The issue wrote K = 36; 36 % 7 != 0 is refused by the entry point and by
    # moco2_module.py:169, see test_cpu_moco_fused_ref.py::test_argument_refusals; 28 keeps every property the case is named for.)
    add(7, 70, 28, None, [(0, 0.2), (14, 0.07), (21, 0.07)])
    # the existing ragged case
    add(5, 72, 260, None, [(0, 0.07), (255, 0.2)])
    add(5, 72, 260, 10, [(250, 0.2), (255, 0.07), (100, 0.07)])           # 255 = K - Nk / 2: the enqueue splits across the ring's end
    # second row tile of one row, second 128-block of P3 of two rows, last P1 block and last K-split chunk of 12 columns
    add(33, 130, 396, None, [(363, 0.07), (33, 0.2)])
    add(33, 130, 396, 66, [(330, 0.07), (363, 0.2)])                      # 363 = K - Nk / 2
    # two whole row tiles
    add(64, 128, 512, None, [(0, 0.2), (448, 0.07)])
    # kchunk = 64 > 32, 257 splits, the last chunk half a chunk, a 4 MB queue
    add(8, 64, 16416, None, [(16408, 0.07), (16419, 0.07)])               # 16419 = K + 3: treated as 0
    # the benchmark's own shape, once each
    add(32, 1024, 4096, None, [(4064, 0.07)])
    add(32, 1024, 4096, 64, [(1024, 0.07)])
    # the whole queue replaced
    add(4, 16, 8, 8, [(0, 0.2), (4, 0.07), (-5, 0.07), (8, 0.2)])         # 4 = K - Nk / 2; 8 = K: treated as 0
    return out


CASES = _cases()
