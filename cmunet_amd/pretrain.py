"""Fused CM-UNet masked-reconstruction pretraining step (BASELINE config 2).

What the reference spreads over mmengine's Runner (Pretraining/CM-UNet/training/train.py:51-94 ->
CM_UNet.forward_train cmunet.py:108-135 -> CMUNetPretrainHead.forward cmunet_head.py:47-70 ->
AmpOptimWrapper.update_params -> AdamW.step, cmunet_config.py:76-91) is ONE kernel schedule here:

    patch mask (UNet_encoder.py:106-158)  fused into the first conv's load (x * (1 - mask[0]))
    online encoder + pixel decoder        engine.unet_forward   (raw conv outputs, BN+ReLU applied on load)
    masked MSE on logits[:,1]             cmu_masked_mse_fwd_bwd (per-row normalised target, A-3)
    backward                              engine.unet_backward  (gradients written into the flat arena)
    gradient exchange                     one RCCL all-reduce over the arena (data parallel, C1)
    AdamW                                 cmu_adam_step over the arena (biases exempt from decay; BatchNorm weights decay: cmunet_config.py:84-91)

``ct_weight = 0`` drops the contrastive branch (target encoder, feature decoder, projector, predictor),
exactly the "masked-recon only" configuration SURVEY 8(d)-(2) names; the joint step lives in cmunet.py.
"""
import math
import os
from time import perf_counter as _host_clock

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .optim import FlatParams, FusedAdam, FusedLAMB, FusedSGD, cmunet_paramwise_decay, dp_exchanges, dp_world


def create_random_patch_mask(batch_size, img_size, patch_size=16, mask_ratio=0.65, rng=None):
    """Host mask generator with the reference's exact RNG consumption (UNet_encoder.py:106-139): per sample,
    shuffle the patch indices and mask patches until floor(mask_ratio*H*W) pixels are covered."""
    rng = np.random if rng is None else rng
    per_side = img_size // patch_size
    n_mask = int(mask_ratio * img_size * img_size) // (patch_size * patch_size)
    mask = np.zeros((batch_size, per_side * per_side), dtype=np.uint8)
    for i in range(batch_size):
        idx = np.arange(per_side * per_side)
        rng.shuffle(idx)
        mask[i, idx[:n_mask]] = 1
    mask = mask.reshape(batch_size, per_side, per_side)
    return np.repeat(np.repeat(mask, patch_size, axis=1), patch_size, axis=2)


def random_patch_mask_device(batch_size, H, W, patch_size=16, mask_ratio=0.65, generator=None, device="cuda", seed=None, offset=0):
    """Same distribution, generated on the device: a random permutation of the patches per
    sample, the first floor(ratio*H*W/patch^2) masked.  Returns uint8 (B,H,W), 1 = masked.
    ``seed`` given: one launch of the counter-based kernel (``ops.random_patch_mask``; the caller advances ``offset`` by
    B * patches per call); else torch's generator (rand + double argsort)."""
    if seed is not None:
        from . import ops
        return ops.random_patch_mask(batch_size, H, W, patch_size, mask_ratio, seed, offset, device)
    ph, pw = H // patch_size, W // patch_size
    n_mask = int(mask_ratio * H * W) // (patch_size * patch_size)
    r = torch.rand(batch_size, ph * pw, generator=generator, device=device)
    rank = r.argsort(dim=1).argsort(dim=1)
    m = (rank < n_mask).to(torch.uint8).view(batch_size, ph, pw)
    return m.repeat_interleave(patch_size, 1).repeat_interleave(patch_size, 2).contiguous()


def default_amp(model, amp):
    """``amp=None`` resolves by the model's storage type: f16 activations need the loss scaler (a masked-MSE gradient is ~1e-7 per
    pixel at bs 32 x 512 x 512, below f16's smallest normal: without scaling it is flushed, silently), so the default for an
    f16 model is the reference's own AmpOptimWrapper(loss_scale='dynamic') (cmunet_config.py:76-78); f32 / bf16 models default to no
    scaler.  ``amp=False`` switches it off explicitly (advisor, round 3: the defaults did not compose)."""
    if amp is None:
        return ops.dt_code(getattr(model, "dtype", "f32")) == ops.F16
    return amp


# ---- one step's data-parallel gradient exchange over a ``FlatParams`` gradient arena ---------------------------------------------------
# What DDP's bucketed all-reduce gives the reference (Spark/main.py:102, dist_train.sh:9-17 + cmunet_config.py:120, Lightning's DDP): a
# bucket's SUM all-reduce starts while the backward pass is still running, all of them are waited for before the inf / nan check, and the
# step reports what was hidden under the backward and what was not.  The trainers below (and genesis.py) decide WHEN a range of the arena
# is final; everything about the collectives themselves -- work handles, the late-write snapshots, the timed wait, the report -- lives in
# ``GradExchange`` and nowhere else.
_TEST_AFTER_LAUNCH = None      # test hook: callable(flat, lo, hi) run right after a bucket's exchange was started (tests/dp_child.py)

# how a bucket was started -> the report's byte counter: from inside a fused node ("early"), from autograd's hooks ("in_backward") or only
# after the backward pass ("flushed": nothing left to hide it under, so its bytes are the exposed ones)
_BYTES = {"early": "bytes_early", "in_backward": "bytes_in_backward", "flushed": "exposed_bytes"}


class GradExchange:
    """``begin(n)``, then ``start(lo, hi, how)`` per bucket as its gradients become final, then ``finish()`` -- or ``abort()`` when the
    step raised in between.  ``starter(lo, hi) -> work or None`` replaces the plain all-reduce of a range (``flat.all_reduce_range_async``);
    ``timed`` (the trainers' ``time_exchange``) brackets the waits of ``finish()`` with clocks; ``last`` is the step's report.

    CMU_DDP_OVERLAP=0 (``overlap``): the owner exchanges the whole arena as one bucket behind the backward pass (A/B and fallback switch).

    Debug mode CMU_DP_CHECK_LATE_WRITES=1 (``late_check``; meant for one-rank groups -- CMU_DP_REHEARSE=1 -- where the SUM all-reduce is an
    identity): a bucket's collective runs on a COPY of its range taken when it STARTS, the arena keeps the producer's values, and the two
    are compared after all exchanges were waited for -- a gradient written into a bucket after its all-reduce was launched (what the
    in-forward announcements of SparK's fused node and the fused nodes' ``notify_ready`` must never allow) shows, whichever side of the
    collective's own read / write-back it would have landed on, and raises instead of silently exchanging a stale value (advisor, round 4)."""

    def __init__(self, flat, group=None, starter=None):
        self.flat, self.group, self.starter = flat, group, starter
        self.overlap = os.environ.get("CMU_DDP_OVERLAP", "1") != "0"
        self.late_check = os.environ.get("CMU_DP_CHECK_LATE_WRITES", "0") == "1"
        self.timed = False
        self.active = False
        self.works, self.snapshots, self.events, self.last = [], [], None, {}

    def begin(self, n_buckets):
        self.active = dp_exchanges(self.group)
        self.works, self.snapshots, self.events = [], [], None
        self.last = {"buckets": n_buckets, "early": 0, "in_backward": 0, "flushed": 0, "bytes_early": 0, "bytes_in_backward": 0,
                     "exposed_bytes": 0}

    def start(self, lo, hi, how):
        """Start the SUM all-reduce of arena gradient elements [lo, hi) (async, on the group's stream) and count it under ``how``."""
        if not self.active:
            return
        if self.late_check and hi > lo:
            snap = self.flat.grad[lo:hi].clone()
            self.snapshots.append((lo, hi, snap))
            w = dist.all_reduce(snap, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        elif self.starter is not None:
            w = self.starter(lo, hi)
        else:
            w = self.flat.all_reduce_range_async(lo, hi, self.group)
        if w is not None:
            self.works.append(w)
            if _TEST_AFTER_LAUNCH is not None:
                _TEST_AFTER_LAUNCH(self.flat, lo, hi)
        self.last[how] += 1
        self.last[_BYTES[how]] += 4 * int(hi - lo)

    def finish(self):
        """Wait for every exchange in flight, then compare the late-write snapshots.  TIMED when ``timed`` is set (bench.py, tests):
        ``wait_ms`` is the host clock around the waits (what a blocking backend -- gloo -- costs the step), ``exposed_ms`` the time the
        COMPUTE stream stood still for them (events on the current stream around the waits: on RCCL ``work.wait()`` only makes the stream
        wait, the host runs on) -- resolved lazily by ``report()``, never by a synchronisation inside the step."""
        timed = self.timed and self.works and self.flat.grad.is_cuda
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = _host_clock()
        for w in self.works:
            w.wait()
        if timed:
            self.last["wait_ms"] = (_host_clock() - t0) * 1e3
            e1.record()
            self.events = (e0, e1)
        self.works = []
        snaps, self.snapshots = self.snapshots, []
        if not snaps:
            return
        if dp_world(self.group) != 1:
            raise RuntimeError("CMU_DP_CHECK_LATE_WRITES=1 compares a bucket with a copy taken at the launch of an IDENTITY all-reduce: use it on a one-rank group")
        for lo, hi, snap in snaps:
            now = self.flat.grad[lo:hi]
            if not torch.equal(snap.view(torch.int32), now.view(torch.int32)):         # bit for bit (NaNs included)
                bad = (snap.view(torch.int32) != now.view(torch.int32)).nonzero()
                first = int(bad[0]) + int(lo)
                owner = next((n for n, (off, cnt) in self.flat.offsets.items() if off <= first < off + cnt), "?")
                raise RuntimeError(f"gradient exchange: {int(bad.numel())} element(s) of the bucket [{lo}, {hi}) were written after its all-reduce had "
                                   f"started (first: arena index {first}, parameter {owner})")

    def abort(self):
        """The step raised while exchanges were in flight: wait for them before the exception travels on (the next step's arena writes
        would race the un-waited collectives), then forget them (advisor, round 4)."""
        try:
            for w in self.works:
                w.wait()
        finally:
            self.works, self.snapshots = [], []

    def report(self):
        """``last`` with the timed fields resolved (synchronises: call it outside the timed region)."""
        rep = dict(self.last)
        if self.events is not None:
            self.events[1].synchronize()
            rep["exposed_ms"] = float(self.events[0].elapsed_time(self.events[1]))
        return rep


# ---- sharded exchange of one big parameter (round 6; the joint step's projector.fc0.weight: 262,144 x 1,536 fp32 = 1.61 GB at 512 x 512) --------
# The reference exchanges it like everything else (DDP's all-reduce: dist_train.sh:9-17 + cmunet_config.py:18-26,120).  A ring all-reduce IS a
# reduce-scatter followed by an all-gather; splitting the two lets (i) every rank run AdamW (+ the EMA of the momentum projector) on 1/world of the
# 403 M elements instead of all of them and (ii) the all-gather -- of the UPDATED parameters instead of the gradients -- run under the next step's
# encoder / decoder forward, where nothing needs the projector yet.  Element for element the arithmetic is the all-reduce path's (a SUM over the
# ranks, then the same optimiser kernel on the same operands): bit-identical on two ranks (a + b commutes; tests/test_cpu_distributed.py,
# tests/test_gpu_dataparallel.py), equal to reduction order beyond.
class _Works:
    """Several async collectives (and what has to follow them on the host side) behind one ``wait()``."""

    def __init__(self, works=(), after=None):
        self.works, self.after = [w for w in works if w is not None], after

    def wait(self):
        for w in self.works:
            w.wait()
        if self.after is not None:
            self.after()
            self.after = None


def _group_backend(group):
    return dist.get_backend(group) if dist.is_available() and dist.is_initialized() else "none"


def shard_bounds(n, world, rank):
    """Element range [lo, hi) of ``rank``'s share of ``n`` elements (``n % world == 0``)."""
    chunk = n // world
    return rank * chunk, (rank + 1) * chunk


def reduce_scatter_sum_async(t, group=None):
    """SUM over the ranks of the 1-D tensor ``t`` (``t.numel() % world == 0``), each rank ending with ITS share summed in place
    (``t[shard_bounds(...)]``); the rest of ``t`` keeps unspecified (local or partly reduced) values.  RCCL: one reduce-scatter into a scratch
    share, copied home behind the wait; other backends (gloo has no reduce-scatter): one in-place reduce per share to its owner."""
    world, rank = dp_world(group), (dist.get_rank(group) if dist.is_initialized() else 0)
    lo, hi = shard_bounds(t.numel(), world, rank)
    if _group_backend(group) == "nccl":
        out = torch.empty(hi - lo, dtype=t.dtype, device=t.device)
        w = dist.reduce_scatter_tensor(out, t, op=dist.ReduceOp.SUM, group=group, async_op=True)
        return _Works([w], after=lambda: t[lo:hi].copy_(out))
    works = []
    for k in range(world):
        a, b = shard_bounds(t.numel(), world, k)
        dst = dist.get_global_rank(group, k) if group is not None else k
        works.append(dist.reduce(t[a:b], dst=dst, op=dist.ReduceOp.SUM, group=group, async_op=True))
    return _Works(works)


def all_gather_shares_async(t, group=None):
    """Every rank's share of the 1-D tensor ``t`` to every rank, in place."""
    world, rank = dp_world(group), (dist.get_rank(group) if dist.is_initialized() else 0)
    lo, hi = shard_bounds(t.numel(), world, rank)
    if _group_backend(group) == "nccl":
        mine = t[lo:hi].clone()                      # (a separate send buffer: no aliasing of the collective's input and output)
        return _Works([dist.all_gather_into_tensor(t, mine, group=group, async_op=True)])
    works = []
    for k in range(world):
        a, b = shard_bounds(t.numel(), world, k)
        src = dist.get_global_rank(group, k) if group is not None else k
        works.append(dist.broadcast(t[a:b], src=src, group=group, async_op=True))
    return _Works(works)


class _ExchangingTrainer:
    """What both trainer families share: the step's gradient exchange (``self.exchange``, a ``GradExchange``) as bench.py and the tests
    see it, and the optimiser step behind it."""

    last_exchange = property(lambda self: self.exchange.last)
    time_exchange = property(lambda self: self.exchange.timed, lambda self, on: setattr(self.exchange, "timed", on))

    def exchange_report(self):
        return self.exchange.report()

    def _checked_step(self, amp, **kw):
        """The optimiser step behind the exchange.  ``amp``: an ``ops.AmpScaler`` or None -- the inf / nan check runs on the EXCHANGED
        gradients (every rank sees the same ones and takes the same decision), the optimiser kernel unscales or skips from the same
        device state, the scale is updated afterwards."""
        if amp is not None:
            amp.check(self.flat.grad)
            self._amp_agree(amp)
            kw["amp"] = amp
        self._opt_step(**kw)
        if amp is not None:
            amp.update()

    # (hooks of the sharded exchange, JointPretrainer)
    def _amp_agree(self, amp):
        pass

    def _opt_step(self, **kw):
        self.opt.step(**kw)


class MaskedReconPretrainer(_ExchangingTrainer):
    """One object = model + flat arenas + fused AdamW + (optional) data-parallel group."""

    def __init__(self, model, lr=1.5e-4, betas=(0.9, 0.95), weight_decay=0.05, eps=1e-8, rc_weight=1.0,
                 ref_compat=True, pred_channel=1, process_group=None, loss_scale=1.0, amp=None):
        """``amp``: True (or an ``ops.AmpScaler``) turns on the dynamic loss scaling of the reference's AmpOptimWrapper
        (cmunet_config.py:76-78; needed with f16 activations: a masked-MSE gradient is ~1e-7 per pixel at bs 32 x 512 x 512,
        below f16's smallest normal) -- state and decisions stay on the device.  None (default): on for an f16 model, off
        otherwise (``default_amp``); False: off."""
        assert next(model.parameters()).is_cuda, "move the model to the GPU first"
        self.model = model.train()
        self.device = next(model.parameters()).device
        self.flat = FlatParams(model)
        self.opt = FusedAdam(self.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=True,
                             decay_filter=cmunet_paramwise_decay)
        self.engine = model._engine(self.device)
        self.sd = dict(model.named_parameters())
        self.sd.update(dict(model.named_buffers()))
        self.rc_weight, self.ref_compat, self.pred_channel = rc_weight, ref_compat, pred_channel
        self.group = process_group
        self.loss_scale = loss_scale
        amp = default_amp(model, amp)
        self.amp = ops.AmpScaler(self.device) if amp is True else (amp or None)
        self.opt.amp = self.amp
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._dlogits = None
        self._ws = None
        # gradient exchange in three buckets, in the order the backward pass completes them: the decoder (the tail of the
        # arena, 12.2 M parameters) half-way through; the bottleneck (``double_conv.*``, 14.2 M of the encoder's 18.8 M) as soon
        # as the encoder backward has passed it; the four down blocks (4.7 M) at the end -- only that last 19 MB all-reduce is
        # not hidden under kernels.  (CMU_DDP_OVERLAP=0: one all-reduce of the whole arena after the backward pass -- A/B and
        # fallback switch)
        self.exchange = GradExchange(self.flat, self.group)
        n = int(self.flat.grad.numel())
        dec_off = self.flat.tail_offset(("up_conv", "conv_last")) if self.exchange.overlap else None
        self._dec = (dec_off, n) if dec_off is not None else None
        self._bott = self.flat.prefix_range("double_conv.") if self._dec is not None else None
        if self._bott is not None and self._bott[1] != dec_off:
            self._bott = None                       # (the bottleneck is expected right in front of the decoder)
        self._rest = (0, (self._bott or self._dec or (n, n))[0])

    def broadcast_parameters(self, src=0):
        if dp_exchanges(self.group):
            dist.broadcast(self.flat.arena, src=src, group=self.group)
            ops.bump_param_generation()          # a raw write into the arena: packed-weight caches must not survive it
            for n, b in self.model.named_buffers():
                if b.is_floating_point():
                    dist.broadcast(b, src=src, group=self.group)

    def state_dict(self):
        """Optimiser moments + step + the loss scaler's state (``optimizer``), next to the model's own ``state_dict()``."""
        return {"optimizer": self.opt.state_dict()}

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd["optimizer"], amp=self.amp)
        ops.bump_param_generation()

    def forward_backward(self, img, mask):
        """img (B,H,W) fp32 cuda, mask (B,H,W) uint8 cuda (1 = masked).  Leaves gradients in the arena and
        returns the loss tensor (1,) on the device (no host sync)."""
        eng = self.engine
        B, H, W = img.shape
        eng.prepack(self.sd)      # all weight packs of the step in one launch
        logits, ctx = eng.unet_forward(self.sd, img, True, mask, mask_per_sample=not self.ref_compat)
        if self._dlogits is None or self._dlogits.shape != logits.shape:
            self._dlogits = torch.empty_like(logits)
            self._ws = ops.workspace("cmu_masked_mse_ws_bytes", self.device, B, H)
        ops.masked_mse_fwd_bwd(logits, self.pred_channel, img, mask, self.loss, self._dlogits,
                               self.rc_weight * self.loss_scale, self._ws, self.amp)
        eng.grad_target, eng.grad_prefix = self.flat.grad_views, ""
        # what the exchange of this step looks like (bench.py prints it next to the RCCL world size): the decoder and the bottleneck
        # start from inside the backward pass ("early"), the down blocks behind it ("flushed": the bytes left for after it)
        self.exchange.begin(1 + (self._dec is not None) + (self._bott is not None))
        try:
            eng.unet_backward(self.sd, ctx, self._dlogits, after_decoder=self._decoder_done, after_bottleneck=self._bottleneck_done)
        except BaseException:
            self.exchange.abort()       # (in-flight all-reduces are waited for before the exception travels on, as in ArenaTrainer)
            raise
        finally:
            eng.grad_target = None
        return self.loss

    def _decoder_done(self):
        if self._dec is not None:
            self.exchange.start(*self._dec, "early")

    def _bottleneck_done(self):
        if self._bott is not None:
            self.exchange.start(*self._bott, "early")

    def exchange_gradients(self):
        """Finish the data-parallel gradient SUM (the decoder and bottleneck buckets may already be in flight) and return 1/world."""
        if not dp_exchanges(self.group):
            return 1.0
        self.exchange.start(*self._rest, "flushed")
        self.exchange.finish()
        return 1.0 / dp_world(self.group)

    def step(self, img, mask):
        loss = self.forward_backward(img, mask)
        self._checked_step(self.amp, grad_scale=self.exchange_gradients() / self.loss_scale)
        return loss


class ArenaTrainer(_ExchangingTrainer):
    """Data-parallel trainer for the autograd-wrapped pretraining models (``CM_UNet``, ``Moco_v2``, ``SparK``): what the
    reference gets from DistributedDataParallel + an optimiser object (Spark/main.py:102,130-140; dist_train.sh:9-17 with
    cmunet_config.py:76-91,120; Lightning's DDP for moco2_module.py:339-344) is here

        trainable parameters re-homed into ONE fp32 arena (frozen momentum / target networks stay outside)
        loss.backward() through the module's fused autograd node(s)
        gradients gathered into the gradient arena; parameters that received no gradient (SparK's ``densify_projs`` of
            the full UNet, SURVEY A-10 -- they would trip the reference's own DDP(find_unused_parameters=False)) count as zero
        ONE RCCL all-reduce (SUM) over the arena, 1/world folded into the optimiser kernel's gradient load
        ONE fused optimiser launch (AdamW / SGD-momentum / LAMB, csrc/heads.hip + optim.hip).

    Embedding all-gathers and SyncBN exchanges stay inside the models (cmunet.py, moco.py, spark.py); all of them use the
    default process group, as the reference's do."""

    _ov_active = False         # True from ``_begin_overlap`` to ``_end_overlap``: hooks and ``notify_ready`` start buckets only then

    def __init__(self, model, optimizer, process_group=None, starter=None):
        self.model = model
        self.group = process_group
        self.flat = optimizer.flat
        self.opt = optimizer
        self.device = self.flat.arena.device
        # Backward-overlapped gradient exchange (what DDP's bucketed all-reduce gives the reference: Spark/main.py:102,
        # dist_train.sh:9-17 + cmunet_config.py:120, Lightning's DDP): the arena is cut into buckets along the top-level modules
        # (an encoder's bottleneck apart from its down blocks); a bucket's all-reduce starts as soon as its last gradient has
        # landed -- told either by autograd's post-accumulate hooks or, earlier, by the fused autograd nodes themselves
        # (``notify_ready`` from inside _CMUNetFn / _EncoderGapFn.backward, which finish a decoder or the bottleneck long before
        # the node returns) -- and runs under the rest of the backward pass; everything is waited for before the inf check.
        # For the joint model the 1.6 GB projector gradient, produced first, is exchanged under the whole conv backward.
        # CMU_DDP_OVERLAP=0: one all-reduce of the whole arena after loss.backward() (A/B and fallback switch).
        self.exchange = GradExchange(self.flat, self.group, starter)
        self._buckets = [dict(lo=lo, hi=hi, names=names, pending=0, launched=False) for lo, hi, names in self.flat.buckets()]
        self._bucket_of = {n: b for b in self._buckets for n in b["names"]}
        # (hooks hold the trainer weakly: a model that outlives its trainer keeps no arena alive, and a dead trainer's hooks are no-ops)
        import weakref
        me = weakref.ref(self)

        def hook(name):
            def fire(_p):
                t = me()
                if t is not None:
                    t._on_grad(name)
            return fire
        self._hook_handles = [p.register_post_accumulate_grad_hook(hook(n)) for n, p in self.flat.params.items()]

    def close(self):
        """Detach from the model: remove the gradient hooks (a second trainer on the same model starts clean)."""
        for h in getattr(self, "_hook_handles", []):
            h.remove()
        self._hook_handles = []
        if getattr(self.model, "_grads_ready", None) is not None and getattr(self.model._grads_ready, "__self__", None) is self:
            object.__setattr__(self.model, "_grads_ready", None)

    # ---- overlapped exchange ----------------------------------------------------------------------------------------------
    def _begin_overlap(self):
        for b in self._buckets:
            b["pending"], b["launched"] = len(b["names"]), False
        self.exchange.begin(len(self._buckets))
        self._ov_active = True

    def _end_overlap(self):
        """Forget this step's bucket state and give the claimed gradient sinks back."""
        from .optim import _SINKS_CLAIMED
        self._ov_active = False
        _SINKS_CLAIMED.difference_update(id(p) for p in self.flat.params.values())

    def _launch(self, b, how):
        """Gradients of bucket ``b`` are final: bring stragglers into the arena, start its all-reduce (async, on the group's stream)."""
        b["launched"] = True
        self.flat.gather_names(b["names"])
        self.exchange.start(b["lo"], b["hi"], how)

    def _on_grad(self, name):
        if not self._ov_active:
            return
        b = self._bucket_of[name]
        b["pending"] -= 1
        if b["pending"] == 0 and not b["launched"]:
            self._launch(b, "in_backward")

    def notify_ready(self, prefix, grads):
        """Called from inside a fused autograd node: every parameter gradient under ``prefix`` is final and sits in ``grads``.  Buckets
        made only of such parameters whose gradients were all written straight into the arena start their exchange now."""
        if not self._ov_active:
            return
        for b in self._buckets:
            if b["launched"] or not all(n.startswith(prefix) for n in b["names"]):
                continue
            ok = True
            for n in b["names"]:
                g = grads.get(n)
                if g is None or g.data_ptr() != self.flat.grad_views[n].data_ptr():
                    ok = False
                    break
            if ok:
                b["launched"] = True          # (their hooks fire when the node returns: nothing left to do then)
                self.exchange.start(b["lo"], b["hi"], "early")

    def _finish_overlap(self):
        """After loss.backward(): buckets that never completed (parameters without a gradient: SparK's ``densify_projs``) in arena
        order -- the same order on every rank --, then wait for everything."""
        for b in self._buckets:
            if not b["launched"]:
                self._launch(b, "flushed")
        self._end_overlap()
        self.exchange.finish()

    def _abort_overlap(self):
        """A forward / backward raised while exchanges were in flight: wait for them (the next step's arena writes would race the
        un-waited collectives), give the claimed gradient sinks back, forget the bucket state (advisor, round 4)."""
        try:
            self.exchange.abort()
        finally:
            self._end_overlap()

    def _exchange_whole_arena(self):
        """One exchange behind the backward pass: the whole arena as a single flushed bucket."""
        self.exchange.begin(1)
        self.exchange.start(0, int(self.flat.grad.numel()), "flushed")
        self.exchange.finish()

    @staticmethod
    def trainable(model):
        want = {n for n, p in model.named_parameters() if p.requires_grad}
        return FlatParams(model, names=lambda n: n in want)

    def world(self):
        return dp_world(self.group)

    def broadcast_parameters(self, src=0):
        """Rank ``src``'s parameters and floating-point buffers to every rank (DDP does this at construction)."""
        if not dp_exchanges(self.group):
            return
        dist.broadcast(self.flat.arena, src=src, group=self.group)
        ops.bump_param_generation()              # raw write into the arena (advisor, round 2): stale packed weights otherwise
        held = {id(p) for p in self.flat.params.values()}
        for p in self.model.parameters():
            if id(p) not in held:
                dist.broadcast(p.data, src=src, group=self.group)
        for b in self.model.buffers():
            if b.is_floating_point():
                dist.broadcast(b, src=src, group=self.group)

    def backward_and_step(self, loss, loss_scale=1.0, amp=None, ema=None, overlap_begun=False):
        """``loss``: scalar tensor from the model's forward (already multiplied by ``loss_scale`` if one is used).
        ``overlap_begun``: the caller opened the overlapped exchange before the FORWARD (SparK: its fused node produces the gradients
        there) -- buckets may already be in flight.
        ``ema``: (segments, momentum) handed to the optimiser kernel (``FusedAdam.step``): the momentum networks' EMA in the same pass.
        ``amp``: an ``ops.AmpScaler`` -- dynamic loss scaling as mmengine's AmpOptimWrapper does it (cmunet_config.py:76-78): the loss
        is multiplied by the scale held ON THE DEVICE (no host read), the inf / nan check runs on the exchanged gradients, the
        optimiser kernel unscales or skips from the same state, the scale is updated afterwards."""
        for p in self.flat.params.values():
            p.grad = None
        if amp is not None:
            loss = loss * amp.state[:4].view(torch.float32)          # the current scale, a one-element device tensor
        exch = dp_exchanges(self.group)
        if exch and self.exchange.overlap:
            if not overlap_begun:
                self._begin_overlap()
            # (a raise in the backward pass or in the waits: every arena trainer gets the cleanup SparKPretrainer.step has -- in-flight
            # all-reduces waited for, gradient sinks released, buckets reset -- before the exception travels on)
            try:
                loss.backward()
                self._finish_overlap()
            except BaseException:
                self._abort_overlap()
                raise
        else:
            loss.backward()
            self.flat.gather_autograd_grads()
            if exch:
                self._exchange_whole_arena()
        scale = 1.0 / self.world() if exch else 1.0
        self._checked_step(amp, grad_scale=scale / loss_scale, **({} if ema is None else {"ema": ema}))
        for p in self.flat.params.values():       # the arena holds them; drop the per-tensor copies autograd made
            p.grad = None


class JointPretrainer(ArenaTrainer):
    """Joint contrastive + masked-reconstruction step of CM-UNet (BASELINE config 4; cmunet.py:108-135 under
    cmunet_config.py:76-114): AdamW(lr, betas (0.9, 0.95), wd 0.05; exempt from decay: names containing 'ln' / 'bias' / ... --
    the BatchNorm weights decay, ``optim.cmunet_paramwise_decay``), then the EMA of the
    target backbone + projector (MomentumUpdateHook.after_train_iter) as two launches between two arenas."""

    def __init__(self, model, lr=1.5e-4, betas=(0.9, 0.95), weight_decay=0.05, eps=1e-8, process_group=None, amp=None):
        """``amp``: True (or an ``ops.AmpScaler``): the dynamic loss scaling of the reference's AmpOptimWrapper (cmunet_config.py:76-78);
        needed with f16 activations (the masked-MSE gradient per pixel is far below f16's normals).  None (default): on for an f16
        model -- what ``cmunet_config()`` / ``CM_UNet`` default to --, off otherwise (``default_amp``); False: off."""
        model.train()
        flat = self.trainable(model)
        opt = FusedAdam(flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=True, decay_filter=cmunet_paramwise_decay)
        super().__init__(model, opt, process_group, starter=self._start_sharded)
        amp = default_amp(model, amp)
        self.amp = ops.AmpScaler(self.device) if amp is True else (amp or None)
        self.opt.amp = self.amp
        tnames = {n for n, _ in model.named_parameters() if n.startswith(("target_backbone.", "target_projector."))}
        self.tflat = FlatParams(model, names=lambda n: n in tnames)
        # identical layouts: (backbone, projector) inside the online arena <-> (target_backbone, target_projector)
        self._ema = []
        for src, dst in (("backbone.", "target_backbone."), ("projector.", "target_projector.")):
            a, b = self.flat.prefix_range(src), self.tflat.prefix_range(dst)
            assert a is not None and b is not None and a[1] - a[0] == b[1] - b[0], "online / target layouts differ"
            self._ema.append((a, b))
        self._ema.sort()
        object.__setattr__(model, "_grads_ready", self.notify_ready)     # fused node -> trainer: "these gradients are final"
        # the EMA rides in the AdamW kernel (cmu_adam_ema_step: one pass over the 1.7 GB of parameters instead of two);
        # CMU_EMA_FUSE=0 keeps the two stand-alone EMA launches behind the optimiser (A/B switch, bit-identical)
        self._fuse_ema = os.environ.get("CMU_EMA_FUSE", "1") != "0"
        self._shard, self._pending_gather, self._shard_hooks = None, None, []
        self._setup_shard()

    # ---- sharded exchange of projector.fc0.weight (see reduce_scatter_sum_async above) -------------------------------------------------------
    def _setup_shard(self):
        """On when gradients are exchanged at all, the parameter is big enough to matter (CMU_DP_SHARD_MIN elements, default 2^24 = 64 MB: the
        reference geometry's 77 M and the bench's 403 M both qualify) and divides into whole 16-byte pieces per rank.  CMU_DP_SHARD_PROJECTOR=0:
        the all-reduce path (A/B switch).  Between the optimiser step and the next forward's projector call a rank's copy of the parameter is
        only valid on its own share: ``finish_pending()`` (called by a forward pre-hook of the two projectors, by ``state_dict`` and by
        ``close``) completes it."""
        name, tname = "projector.fc0.weight", "target_projector.fc0.weight"
        if os.environ.get("CMU_DP_SHARD_PROJECTOR", "1") == "0" or not dp_exchanges(self.group) or self.exchange.late_check:
            return
        if name not in self.flat.offsets or tname not in self.tflat.offsets:
            return
        (off, cnt), (toff, tcnt) = self.flat.offsets[name], self.tflat.offsets[tname]
        world = self.world()
        if cnt != tcnt or cnt < int(os.environ.get("CMU_DP_SHARD_MIN", str(1 << 24))) or cnt % (4 * world) != 0 or off % 4 != 0:
            return
        rank = dist.get_rank(self.group) if (dist.is_available() and dist.is_initialized()) else 0
        a, b = shard_bounds(cnt, world, rank)
        self._shard = dict(lo=off, hi=off + cnt, own=(off + a, off + b), t_lo=toff)
        import weakref
        me = weakref.ref(self)

        def pre(_m, _inp):
            t = me()
            if t is not None:
                t.finish_pending()
        self._shard_hooks = [self.model.projector.register_forward_pre_hook(pre), self.model.target_projector.register_forward_pre_hook(pre)]

    def close(self):
        self.finish_pending()
        for h in self._shard_hooks:
            h.remove()
        self._shard_hooks = []
        super().close()

    def _start_sharded(self, lo, hi):
        """The exchange's starter: the bucket that holds the big parameter is all-reduced in front of and behind it, the parameter itself
        reduce-scattered; every other range is all-reduced as usual."""
        sh = self._shard
        if sh is None or not (lo <= sh["lo"] and sh["hi"] <= hi):
            return self.flat.all_reduce_range_async(lo, hi, self.group)
        self.exchange.last["reduce_scatter_bytes"] = 4 * int(sh["hi"] - sh["lo"])
        return _Works([self.flat.all_reduce_range_async(lo, sh["lo"], self.group),
                       reduce_scatter_sum_async(self.flat.grad[sh["lo"]:sh["hi"]], self.group),
                       self.flat.all_reduce_range_async(sh["hi"], hi, self.group)])

    def _amp_agree(self, amp):
        """With a sharded gradient a rank sees the SUMMED gradient only on its own share (elsewhere its local one): the inf / nan flags are
        combined (MAX) so that every rank skips or steps together, as it does when all of them check the same all-reduced arena."""
        if self._shard is not None:
            dist.all_reduce(amp.state[4:8].view(torch.float32), op=dist.ReduceOp.MAX, group=self.group)

    def _opt_step(self, grad_scale=1.0, amp=None, ema=None):
        sh = self._shard
        if sh is None:
            return self.opt.step(grad_scale=grad_scale, amp=amp, **({} if ema is None else {"ema": ema}))
        self.finish_pending()
        n = int(self.flat.arena.numel())
        ranges = [r for r in ((0, sh["lo"]), sh["own"], (sh["hi"], n)) if r[1] > r[0]]
        self.opt.step_ranges(ranges, grad_scale=grad_scale, amp=amp, ema=ema)
        # the updated share to every rank -- under whatever the compute stream does next (the next forward's encoders and decoders); the EMA of
        # the momentum projector rode in the optimiser kernel on the own share only: the other shares follow once their parameters are here
        w = all_gather_shares_async(self.flat.arena[sh["lo"]:sh["hi"]], self.group)
        self._pending_gather = (w, None if ema is None else float(ema[1]))

    def finish_pending(self):
        """Complete the parameter all-gather started by the last optimiser step (no-op when there is none)."""
        pg, self._pending_gather = self._pending_gather, None
        if pg is None:
            return
        w, mom = pg
        w.wait()
        sh = self._shard
        if mom is not None:
            for c0, c1 in ((sh["lo"], sh["own"][0]), (sh["own"][1], sh["hi"])):
                if c1 > c0:
                    t0 = sh["t_lo"] + (c0 - sh["lo"])
                    ops.ema_update(self.tflat.arena[t0:t0 + (c1 - c0)], self.flat.arena[c0:c1], mom)
        ops.bump_param_generation()      # raw writes into the arena: packed / converted copies of the parameter are stale

    def momentum_update(self):
        self.finish_pending()            # (sharded exchange: the whole parameter first)
        for (a0, a1), (b0, b1) in self._ema:
            ops.ema_update(self.tflat.arena[b0:b1], self.flat.arena[a0:a1], self.model.momentum)

    def state_dict(self):
        self.finish_pending()
        if self._shard is not None:      # the moments of the sharded parameter live on their owners: bring them together for the checkpoint
            sh = self._shard
            for t in (self.opt.m, self.opt.v):
                all_gather_shares_async(t[sh["lo"]:sh["hi"]], self.group).wait()
        return {"optimizer": self.opt.state_dict()}

    def load_state_dict(self, sd):
        self.finish_pending()            # (a parameter all-gather still in flight would land on top of what the caller loads next)
        self.opt.load_state_dict(sd["optimizer"], amp=self.amp)
        ops.bump_param_generation()

    def broadcast_parameters(self, src=0):
        self.finish_pending()
        super().broadcast_parameters(src)

    def step(self, img, img_t, mask=None, cur_iter=None, max_iter=None, **kw):
        if cur_iter is not None and max_iter:
            from .cmunet import momentum_schedule
            self.model.momentum = momentum_schedule(cur_iter, max_iter, self.model.base_momentum, getattr(self.model, "end_momentum", self.model.base_momentum))
        losses = self.model(img, mode="loss", img_t=img_t, mask=mask, **kw)
        if self._fuse_ema:
            segs = [(a0, a1, self.tflat.arena[b0:b1]) for (a0, a1), (b0, b1) in self._ema]
            self.backward_and_step(losses["loss_ct"] + losses["loss_rc"], amp=self.amp, ema=(segs, self.model.momentum))
        else:
            self.backward_and_step(losses["loss_ct"] + losses["loss_rc"], amp=self.amp)
            self.momentum_update()
        return {k: v.detach() for k, v in losses.items()}


class MocoPretrainer(ArenaTrainer):
    """MoCo-v2 step (BASELINE config 3; moco2_module.py:287-309,339-344): SGD(lr, momentum 0.9, weight decay 1e-4) on the
    query encoder; the key encoder's EMA (before the forward, A-8) is one launch between two arenas."""

    def __init__(self, model, lr=None, momentum=None, weight_decay=None, process_group=None):
        model.train()
        hp = model.hparams
        flat = self.trainable(model)
        opt = FusedSGD(flat, lr=hp["learning_rate"] if lr is None else lr, momentum=hp["momentum"] if momentum is None else momentum,
                       weight_decay=hp["weight_decay"] if weight_decay is None else weight_decay)
        super().__init__(model, opt, process_group)
        knames = {n for n, _ in model.named_parameters() if n.startswith("encoder_k.")}
        self.kflat = FlatParams(model, names=lambda n: n in knames)
        a, b = self.flat.prefix_range("encoder_q."), self.kflat.prefix_range("encoder_k.")
        assert a is not None and b is not None and a[1] - a[0] == b[1] - b[0]
        model._ema_arenas = (self.kflat.arena[b[0]:b[1]], self.flat.arena[a[0]:a[1]])     # used by _momentum_update_key_encoder
        # the query encoder's fused node names its parameters without the "encoder_q." prefix
        object.__setattr__(model.encoder_q, "_grads_ready",
                           lambda prefix, grads: self.notify_ready("encoder_q." + prefix, {"encoder_q." + k: v for k, v in grads.items()}))

    def set_epoch(self, epoch, max_epochs):
        """moco2_module.py:345-348: the cosine learning rate of ``epoch`` (0-based: CosineAnnealingLR after ``epoch`` scheduler steps)."""
        if not hasattr(self, "_base_lr"):
            self._base_lr = self.opt.lr
        self.opt.lr = moco_cosine_lr(self._base_lr, epoch, max_epochs)
        return self.opt.lr

    def step(self, img_q, img_k, loss_scale=1.0):
        """``loss_scale``: static scale on the loss before backward (16-bit activations store their gradients in the model's dtype:
        the InfoNCE gradient reaches the first layers at ~1e-6 per element), divided out again by the SGD kernel."""
        # the PREVIOUS step's loss is checked here (its kernels have finished long before the host gets back: no stall of the launch
        # queue): the fused InfoNCE kernel ends with a NaN loss, a zero query gradient and an untouched queue when one of its
        # grid barriers timed out (csrc/moco.hip) -- SGD has no inf / nan skip of its own, so that must not pass silently
        prev = getattr(self, "_prev_loss", None)
        if prev is not None and not bool(torch.isfinite(prev)):
            self._prev_loss = None
            raise RuntimeError("MocoPretrainer: the previous step's loss is not finite (a timed-out grid barrier of "
                               "cmu_moco_infonce_enqueue -- was another kernel resident beside it? -- or an overflow)")
        loss = self.model.training_step((img_q, img_k))
        self.backward_and_step(loss * float(loss_scale) if loss_scale != 1.0 else loss, loss_scale)
        self._prev_loss = loss.detach()
        return self._prev_loss


class SparKPretrainer(ArenaTrainer):
    """SparK step (BASELINE config 5; Spark/main.py:178-227 with utils/lamb.py): LAMB (betas (0.9, 0.95), wd 0.04, global
    gradient-norm clip) over every parameter, the unused ``densify_projs`` included (zero gradient)."""

    def __init__(self, model, lr=2e-4, betas=(0.9, 0.95), weight_decay=0.04, clip=5.0, process_group=None):
        model.train()
        flat = self.trainable(model)
        # lr_control.get_param_groups (lr_control.py:32-53) with main.py:107's nowd_keys
        nowd = ("cls_token", "pos_embed", "mask_token", "gamma")
        opt = FusedLAMB(flat, lr=lr, betas=betas, weight_decay=weight_decay, max_grad_norm=clip,
                        decay_filter=lambda n, p: not (p.dim() == 1 or n.endswith(".bias") or any(k in n for k in nowd)))
        super().__init__(model, opt, process_group)
        # round 4: SparK's fused node computes its gradients inside its FORWARD (spark._SparKFn) -- it announces the decoder, the
        # bottleneck and each encoder level as their gradients land in the arena, so their all-reduces run under the rest of the
        # step instead of back to back behind it (137 MB were exposed; now the down blocks' 19 MB + the mask tokens, as in the other trainers)
        object.__setattr__(model, "_grads_ready", self.notify_ready)

    def anneal(self, peak_lr, wd, wd_end, cur_it, wp_it, max_it):
        """main.py:192: set this iteration's learning rate and weight decay (``spark_lr_wd``); returns them."""
        lr, cur_wd = spark_lr_wd(peak_lr, wd, wd_end, cur_it, wp_it, max_it)
        self.opt.set_lr_wd(lr, cur_wd)
        return lr, cur_wd

    def step(self, inp_bchw, active_b1ff=None, loss_scale=1.0):
        """``loss_scale``: static scale applied to the loss gradient INSIDE the fused step (the activations' gradients are
        stored in the model's dtype) and divided out again by the optimiser kernel."""
        self.model.grad_scale = float(loss_scale)
        begun = self.exchange.overlap and dp_exchanges(self.group)
        try:
            if begun:
                for p in self.flat.params.values():
                    p.grad = None
                self._begin_overlap()                      # before the forward: that is where this model's gradients are produced
                self.model._unit_backward = True           # loss.backward() below hands the node a gradient of exactly 1: no in-place
                #                                            rescale of gradients whose all-reduce may be in flight
            loss = self.model(inp_bchw, active_b1ff=active_b1ff)
            self.backward_and_step(loss, loss_scale, overlap_begun=begun)
        except BaseException:
            if begun:
                self._abort_overlap()
            raise
        finally:
            self.model.grad_scale = 1.0
            self.model._unit_backward = False
        return loss.detach()


def spark_lr_wd(peak_lr, wd, wd_end, cur_it, wp_it, max_it):
    """SparK's per-iteration schedule (Spark/utils/lr_control.py:11-22, called at main.py:192 with cur_it = it + ep * iters,
    wp_it = wp_ep * iters, max_it = ep * iters): linear warm-up from 0.5 % of the peak learning rate, then a cosine to 0.1 % of it;
    the weight decay follows a cosine from ``wd`` to ``wd_end`` over the whole run.  Returns (lr, weight_decay)."""
    wp_it = round(wp_it)
    if cur_it < wp_it:
        lr = peak_lr * (0.005 + 0.995 * cur_it / wp_it)
    else:
        lr = peak_lr * (0.001 + 0.999 * 0.5 * (1.0 + math.cos(math.pi * (cur_it - wp_it) / (max_it - 1 - wp_it))))
    return lr, wd_end + (wd - wd_end) * 0.5 * (1.0 + math.cos(math.pi * cur_it / (max_it - 1)))


def moco_cosine_lr(base_lr, epoch, max_epochs, eta_min=0.0):
    """MoCo's schedule (moco2_module.py:345-348: CosineAnnealingLR(optimizer, trainer.max_epochs), stepped once per epoch)."""
    return eta_min + (base_lr - eta_min) * 0.5 * (1.0 + math.cos(math.pi * epoch / max_epochs))


def cosine_warmup_lr(base_lr, it, warmup_iters, total_iters, start_factor=1e-4):
    """cmunet_config.py:94-109: LinearLR(start_factor 1e-4) for the warm-up, then CosineAnnealingLR to 0."""
    if it < warmup_iters:
        return base_lr * (start_factor + (1 - start_factor) * it / max(1, warmup_iters))
    t = (it - warmup_iters) / max(1, total_iters - warmup_iters)
    return 0.5 * base_lr * (1 + math.cos(math.pi * min(1.0, t)))
