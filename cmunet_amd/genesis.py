"""Models Genesis and MAE baseline pretraining (Pretraining/Transformation_based/: Genesis_Chest_CT.py, utils.py, config.py) on the GPU.

The reference builds every batch with single-threaded numpy inside its training loop (about 78 ms per 256 x 256 image).  Here a batch
is four launches of csrc/genesis.hip, driven by one PER-IMAGE RECORD (``REC_DTYPE``) that holds every random decision of the image:

    records       cmu_genesis_sample (Philox keyed by (seed, offset): the production path) or ``replay_records`` -- Python's ``random``
                  and a numpy ``RandomState`` called in exactly the reference's order (parity path, as slow as the reference)
    y, x          cmu_genesis_gather_shuffle: y = flip(src[idx]), x = local pixel shuffle of y
    Bezier        cmu_genesis_bezier: the two 100,000-point cubics of nonlinear_transformation and their sorted copies
    x             cmu_genesis_intensity_paint: np.interp through them, then in- / out-painting
    (MAE)         cmu_genesis_mae: x = y * (1 - mask[0])

``GenesisPretrainer`` is the reference's step (UNet(out_classes=1), nn.MSELoss, SGD(1e-2, momentum 0.9)), ``pretrain_genesis`` its driver
(epochs, validation on corrupted pairs, early stopping, best checkpoint, losses pickle, resume).  No host synchronisation inside an epoch:
losses stay on the device and are read back once per epoch together with the Bezier error word.
"""
import os
import pickle

import numpy as np
import torch

from . import _lib, ops
from ._lib import call
from .dataset import apply_overrides
from .optim import FlatParams, FusedSGD
from .pretrain import ArenaTrainer, create_random_patch_mask, default_amp, dp_exchanges

NBLOCKS = 10000            # local_pixel_shuffling's num_block
NT = 100000                # bezier_curve's nTimes
GF_FLIP0, GF_FLIP1, GF_LOCAL, GF_NONLIN, GF_SORTY = 1, 2, 4, 8, 16

# csrc/genesis.hip GenesisRec (112 bytes)
REC_DTYPE = np.dtype({
    "names": ["src", "flags", "paint", "nrect", "rect", "nblocks", "slot", "block_off", "perm_off", "bez"],
    "formats": ["<i4", "<i4", "<i4", "<i4", ("<i2", (5, 4)), "<i4", "<i4", "<i8", "<i8", ("<f8", (4,))],
    "offsets": [0, 4, 8, 12, 16, 56, 60, 64, 72, 80],
    "itemsize": 112})

_MASK_SEED_SALT = 0x9E3779B97F4A7C15     # the MAE mask's Philox key differs from the sampler's


class GenesisConfig:
    """config.py's ``models_genesis_config`` (the values this driver reads).  ``model``: "Model Genesis" or "MAE"."""

    def __init__(self, model="Model Genesis", **kw):
        self.model = model
        self.suffix = "genesis_chest_ct"
        self.ratio = 0.1
        self.input_rows = 64
        self.input_cols = 64
        self.nb_class = 1
        self.weights = None
        self.batch_size = 64
        self.optimizer = "sgd"
        self.nb_epoch = 256
        self.patience = 50
        self.lr = 1
        self.nonlinear_rate = 0.9
        self.paint_rate = 0.9
        self.outpaint_rate = 0.8
        self.local_rate = 0.5
        self.flip_rate = 0.4
        self.model_path = "pretrained_weights"
        exp_name = kw.pop("exp_name", None)
        apply_overrides(self, kw)
        self.inpaint_rate = 1.0 - self.outpaint_rate
        self.exp_name = exp_name or f"{self.model}-{self.suffix}"
        if self.model not in ("Model Genesis", "MAE"):
            raise ValueError(f"Unsupported method: {self.model}. Supported methods are 'MAE' and 'Model Genesis'.")
        if self.optimizer != "sgd":
            raise ValueError("only optimizer='sgd' is supported (the reference's 'adam' branch passes conf.lr as its betas)")


def step_lr(epoch, base_lr=1e-2, patience=50, gamma=0.5):
    """StepLR(step_size=int(0.8 * patience), gamma) stepped with ``scheduler.step(epoch)`` before each epoch: its closed form."""
    return base_lr * gamma ** (epoch // int(patience * 0.8))


# ------------------------------------------------------------------------------------------------
# host replay of the reference's random stream
# ------------------------------------------------------------------------------------------------
def replay_records(n_images, batch_size, H, W, config, py_random, np_rng):
    """One batch of generate_pair (Genesis) or generate_pair_mae (MAE), drawing from ``py_random`` (a ``random.Random`` or the
    ``random`` module) and ``np_rng`` (a ``np.random.RandomState`` or ``np.random``) exactly as the reference does.
    -> dict(recs, blocks (B,10000,4) int16, perms (B,10000,slot) uint8, noise (B,H,W) f32) for Genesis, dict(recs, mask (H,W) uint8)
    for MAE.  The block permutations come from shuffling arange(bx*by): the same draws as shuffling the window itself."""
    index = list(range(n_images))
    py_random.shuffle(index)
    idx = index[:batch_size]
    B = len(idx)
    recs = np.zeros(B, REC_DTYPE)
    recs["src"] = idx
    if config.model == "MAE":
        mask = create_random_patch_mask(B, H, 16, 0.5, np_rng)
        return {"recs": recs, "mask": np.ascontiguousarray(mask[0])}
    slot = (H // 25) * (W // 25)
    blocks = np.zeros((B, NBLOCKS, 4), np.int16)
    perms = np.zeros((B, NBLOCKS, slot), np.uint8)
    noise = np.zeros((B, H, W), np.float32)
    for n in range(B):
        r = recs[n]
        r["slot"] = slot
        r["block_off"] = n * NBLOCKS
        r["perm_off"] = n * NBLOCKS * slot
        flags = 0
        cnt = 3                                                   # data_augmentation
        while py_random.random() < config.flip_rate and cnt > 0:
            flags ^= GF_FLIP1 if py_random.choice([0, 1]) else GF_FLIP0
            cnt -= 1
        if not py_random.random() >= config.local_rate:           # local_pixel_shuffling
            flags |= GF_LOCAL
            r["nblocks"] = NBLOCKS
            for k in range(NBLOCKS):
                bx = py_random.randint(1, H // 25)
                by = py_random.randint(1, W // 25)
                x0 = py_random.randint(0, H - bx)
                y0 = py_random.randint(0, W - by)
                perm = np.arange(bx * by)
                np_rng.shuffle(perm)
                blocks[n, k] = (x0, y0, bx, by)
                perms[n, k, :bx * by] = perm
        if not py_random.random() >= config.nonlinear_rate:       # nonlinear_transformation
            flags |= GF_NONLIN
            r["bez"] = [py_random.random() for _ in range(4)]
            if not py_random.random() < 0.5:
                flags |= GF_SORTY
        if py_random.random() < config.paint_rate:
            rects = []
            if py_random.random() < config.inpaint_rate:         # image_in_painting
                r["paint"] = 1
                cnt = 5
                while cnt > 0 and py_random.random() < 0.95:
                    sx = py_random.randint(H // 6, H // 3)
                    sy = py_random.randint(W // 6, W // 3)
                    x0 = py_random.randint(3, H - sx - 3)
                    y0 = py_random.randint(3, W - sy - 3)
                    noise[n, x0:x0 + sx, y0:y0 + sy] = np_rng.rand(sx, sy)
                    rects.append((x0, y0, sx, sy))
                    cnt -= 1
            else:                                                 # image_out_painting
                r["paint"] = 2
                noise[n] = np_rng.rand(H, W)
                sx = H - py_random.randint(2 * H // 7, 4 * H // 7)
                sy = W - py_random.randint(2 * W // 7, 4 * W // 7)
                rects.append((py_random.randint(3, H - sx - 3), py_random.randint(3, W - sy - 3), sx, sy))
                cnt = 4
                while cnt > 0 and py_random.random() < 0.95:
                    sx = H - py_random.randint(3 * H // 7, 4 * H // 7)
                    sy = W - py_random.randint(3 * W // 7, 4 * W // 7)
                    rects.append((py_random.randint(3, H - sx - 3), py_random.randint(3, W - sy - 3), sx, sy))
                    cnt -= 1
            r["nrect"] = len(rects)
            for q, rc in enumerate(rects):
                r["rect"][q] = rc
        r["flags"] = flags
    return {"recs": recs, "blocks": blocks, "perms": perms, "noise": noise}


# ------------------------------------------------------------------------------------------------
# pair generator
# ------------------------------------------------------------------------------------------------
class GenesisPairGenerator:
    """generate_pair / generate_pair_mae (utils.py:196-253) as an iterator of device tensors ``(x, y)``, both (B, H, W) float32.

    ``images``: (N, H, W) float32 (numpy or tensor), kept on the device.  Batches are drawn with replacement across steps (the
    reference shuffles all indices per batch and takes the first B; B = min(batch_size, N)).  Default: the device sampler keyed by
    ``(seed, offset)``; ``offset`` advances by one per batch, so the same (seed, offset) gives the same bits.  ``reference_stream =
    (py_random, np_rng)``: the records come from the host replay of the reference's own random stream instead."""

    def __init__(self, images, batch_size, config=None, seed=0, offset=0, reference_stream=None, device=None):
        self.config = config or GenesisConfig()
        dev = torch.device(device) if device is not None else (images.device if torch.is_tensor(images) and images.is_cuda
                                                               else torch.device("cuda", torch.cuda.current_device()))
        src = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images))
        if src.dtype != torch.float32 or src.dim() != 3:
            raise ValueError(f"images must be (N, H, W) float32, got {tuple(src.shape)} {src.dtype}")
        self.src = src.to(dev).contiguous()
        self.N, self.H, self.W = self.src.shape
        self.B = min(int(batch_size), self.N)
        self.mae = self.config.model == "MAE"
        self.seed, self.offset = int(seed) & (2 ** 64 - 1), int(offset)
        self.reference_stream = reference_stream
        self.device = dev
        H, W, B = self.H, self.W, self.B
        l = _lib.lib()
        assert l.cmu_genesis_rec_bytes() == REC_DTYPE.itemsize, "GenesisRec layout differs from REC_DTYPE"
        self.recs = torch.zeros(B * REC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.mae:
            if H % 16 or W % 16:
                raise ValueError("MAE pairs need sides that are multiples of the 16-pixel patch")
        else:
            if H < 42 or W < 42 or (H // 25) * (W // 25) > 256:
                raise ValueError(f"Genesis pairs need 42 <= H, W and (H//25)*(W//25) <= 256 (got {H}x{W})")
            self.slot = (H // 25) * (W // 25)
            self.blocks = torch.zeros(B * NBLOCKS * 4, dtype=torch.int16, device=dev)
            self.perms = torch.zeros(B * NBLOCKS * self.slot, dtype=torch.uint8, device=dev)
            self.minmax = torch.zeros(B * l.cmu_genesis_segments(H, W) * 2, dtype=torch.float32, device=dev)
            self.ws = ops.workspace("cmu_genesis_bezier_ws_bytes", dev, B)
        self.last_noise = None

    def __iter__(self):
        return self

    def _put(self, dst, arr):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(arr)).view(-1).view(dst.dtype))

    def __next__(self):
        B, H, W, p = self.B, self.H, self.W, ops._p
        with torch.cuda.device(self.device):
            x = torch.empty(B, H, W, dtype=torch.float32, device=self.device)
            y = torch.empty_like(x)
            cfg = self.config
            noise = None
            if self.reference_stream is not None:
                rep = replay_records(self.N, B, H, W, cfg, *self.reference_stream)
                self._put(self.recs, rep["recs"].view(np.uint8))
                if self.mae:
                    mask = torch.from_numpy(rep["mask"]).to(self.device)
                else:
                    self._put(self.blocks, rep["blocks"])
                    self._put(self.perms, rep["perms"])
                    noise = torch.from_numpy(rep["noise"]).to(self.device)
            else:
                call("cmu_genesis_sample", p(self.recs), p(getattr(self, "blocks", None)), p(getattr(self, "perms", None)), self.N, B, H, W,
                     int(self.mae), float(cfg.flip_rate), float(cfg.local_rate), float(cfg.nonlinear_rate), float(cfg.paint_rate),
                     float(cfg.inpaint_rate), self.seed, self.offset, ops._stream())
                if self.mae:
                    mask = ops.random_patch_mask(1, H, W, 16, 0.5, self.seed ^ _MASK_SEED_SALT, self.offset * (H // 16) * (W // 16),
                                                 self.device)[0]
            if self.mae:
                call("cmu_genesis_mae", p(self.src), p(self.recs), p(mask.contiguous()), p(x), p(y), B, H, W, ops._stream())
                self.last_mask = mask
            else:
                call("cmu_genesis_gather_shuffle", p(self.src), p(self.recs), p(self.blocks), p(self.perms), p(x), p(y), p(self.minmax),
                     B, H, W, ops._stream())
                call("cmu_genesis_bezier", p(self.recs), p(self.minmax), B, H, W, p(self.ws), p(self.err), ops._stream())
                call("cmu_genesis_intensity_paint", p(self.recs), p(self.ws), p(noise), self.seed, self.offset, p(x), B, H, W,
                     ops._stream())
                self.last_noise = noise
            self.last_offset = self.offset
            self.offset += 1
        return x, y

    def records(self):
        """The last batch's records (+ block table and permutations) as numpy arrays (synchronises; tests and diagnostics)."""
        out = {"recs": self.recs.cpu().numpy().view(REC_DTYPE).copy()}
        if not self.mae:
            out["blocks"] = self.blocks.cpu().numpy().reshape(self.B, NBLOCKS, 4)
            out["perms"] = self.perms.cpu().numpy().reshape(self.B, NBLOCKS, self.slot)
        return out

    def check(self, err=None):
        """Raise if the Bezier rank merge ever computed a position outside its table (bit 1 of the error word; any number of monotone
        runs is sorted, so bit 0 is no longer raised).  ``err``: the error word already read back by the caller (else it is read here,
        which synchronises)."""
        e = int(self.err.item()) if err is None else int(err)
        if e:
            raise RuntimeError(f"cmu_genesis_bezier: error word {e:#x} (the Bezier merge ranked a sample outside its table)")


# ------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------
def mse_fwd_bwd(logits, y, loss, dlogits, loss_scale=1.0, amp=None, ws=None):
    """nn.MSELoss()(logits[:, 0], y) into ``loss`` (1,) f32; ``dlogits`` (nullable) its gradient (cmu_mse_fwd_bwd)."""
    B, K, H, W = logits.shape
    assert y.shape == (B, H, W) and y.dtype == torch.float32 and y.is_contiguous() and logits.is_contiguous()
    if ws is None:
        ws = ops.workspace("cmu_mse_ws_bytes", logits.device)
    call("cmu_mse_fwd_bwd", ops._p(logits), K, ops._p(y), ops._p(loss), ops._p(dlogits), float(loss_scale),
         ops._p(None if amp is None else amp.state), B, H, W, ops._p(ws), ops._stream())
    return loss


class GenesisPretrainer(ArenaTrainer):
    """Genesis_Chest_CT.py:86-145: ``UNet(out_classes=1)``, ``nn.MSELoss()(pred.squeeze(1), gt)``, ``SGD(lr 1e-2, momentum 0.9,
    weight_decay 0, nesterov False)``; ``set_epoch`` applies StepLR's closed form.  fp32 is the reference's arithmetic; an f16 model
    gets the dynamic loss scaler by default (``default_amp``).  ``step(x, y)`` returns the loss tensor on the device (reused by the
    next step: copy it to keep it)."""

    def __init__(self, model, lr=1e-2, momentum=0.9, weight_decay=0.0, nesterov=False, patience=50, process_group=None, amp=None):
        assert next(model.parameters()).is_cuda, "move the model to the GPU first"
        model.train()
        opt = FusedSGD(FlatParams(model), lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(model, opt, process_group)
        self.base_lr, self.patience = lr, patience
        amp = default_amp(model, amp)
        self.amp = ops.AmpScaler(self.device) if amp is True else (amp or None)
        self.engine = model._engine(self.device)
        self.sd = dict(model.named_parameters())
        self.sd.update(dict(model.named_buffers()))
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.vloss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._ws = ops.workspace("cmu_mse_ws_bytes", self.device)
        self._dlogits = None

    def set_epoch(self, epoch):
        self.opt.lr = step_lr(epoch, self.base_lr, self.patience)

    def forward_backward(self, x, y):
        eng = self.engine
        eng.prepack(self.sd)
        logits, ctx = eng.unet_forward(self.sd, x, True)
        if self._dlogits is None or self._dlogits.shape != logits.shape:
            self._dlogits = torch.empty_like(logits)
        mse_fwd_bwd(logits, y, self.loss, self._dlogits, 1.0, self.amp, self._ws)
        eng.grad_target, eng.grad_prefix = self.flat.grad_views, ""
        try:
            eng.unet_backward(self.sd, ctx, self._dlogits)
        finally:
            eng.grad_target = None
        return self.loss

    def step(self, x, y):
        loss = self.forward_backward(x, y)
        scale = 1.0
        if dp_exchanges(self.group):
            self._exchange_whole_arena()
            scale = 1.0 / self.world()
        self._checked_step(self.amp, grad_scale=scale)
        return loss

    @torch.no_grad()
    def evaluate(self, x, y):
        """Validation loss of one batch in eval mode (running BatchNorm statistics), on the device."""
        self.engine.prepack(self.sd)
        logits, _ = self.engine.unet_forward(self.sd, x, False)
        return mse_fwd_bwd(logits, y, self.vloss, None, ws=self._ws)

    def optimizer_state_dict(self):
        return self.opt.state_dict()


# ------------------------------------------------------------------------------------------------
# driver
# ------------------------------------------------------------------------------------------------
def load_genesis_images(data_dir, ratio=0.1, size=256, device=None):
    """Genesis_Chest_CT.py:25-59: sorted file list, train_test_split(test_size=0.2, random_state=42), then train_test_split(train,
    test_size=ratio/0.8, random_state=42) for the pretraining share; every .npy image (float32, PIL mode 'F') bicubic-resized to size x
    size on the device.  -> (x_train, x_valid) float32 numpy arrays."""
    from .dataset import train_test_split_indices
    names = sorted(os.listdir(data_dir))
    tr, te = train_test_split_indices(len(names), 0.2, 42)
    tr2, _ = train_test_split_indices(len(tr), ratio / 0.8, 42)
    pre = [names[i] for i in np.asarray(tr)[tr2]]
    test = [names[i] for i in te]
    dev = device or torch.device("cuda", torch.cuda.current_device())

    def load(lst):
        out = []
        for f in lst:
            s = np.load(os.path.join(data_dir, f))
            if s.dtype != np.float32 or s.ndim != 2:
                raise ValueError(f"{f}: expected a 2-D float32 image, got {s.shape} {s.dtype}")
            t = torch.from_numpy(np.ascontiguousarray(s))[None].to(dev)
            out.append(ops.resize_bicubic(t, size, size)[0].cpu().numpy())
        return np.array(out, dtype=np.float32).reshape(len(out), size, size)
    return load(pre), load(test)


def pretrain_genesis(config, images_train, images_valid, model=None, seed=0, reference_stream=None, base_ch=64, depth=5, dtype="f32",
                     losses_dir=".", device=None, log=print):
    """Genesis_Chest_CT.py:65-181.  Per epoch: StepLR's lr, N_train // B training steps, N_valid // B validation batches of CORRUPTED
    pairs in eval mode, early stopping after ``patience`` epochs without a lower validation loss.  The best epoch's checkpoint is
    ``{model_path}/{exp_name}.pt`` = {'epoch', 'state_dict': module.*, 'optimizer_state_dict'} (torch.optim.SGD's format);
    ``{losses_dir}/{exp_name}_train_valid_losses.pkl`` holds {'train_losses': {'fold_<epoch>': [...]}, 'valid_losses': {...}} with
    train losses rounded to 2 decimals as the reference logs them.  ``config.weights``: resume (model, momentum, epoch).
    -> dict(best_loss, epochs_run, checkpoint, losses_path, avg_train_losses, avg_valid_losses)."""
    from .model import UNet
    from .train import export_checkpoint
    conf = config
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if model is None:
        model = UNet(out_classes=1, base_ch=base_ch, depth=depth, dtype=dtype)
    model = model.to(dev)
    B = conf.batch_size
    py_np = reference_stream
    train_gen = GenesisPairGenerator(images_train, B, conf, seed=seed, offset=0, reference_stream=py_np, device=dev)
    valid_gen = GenesisPairGenerator(images_valid, B, conf, seed=seed, offset=1 << 40, reference_stream=py_np, device=dev)
    next(train_gen)                           # the reference draws one training batch before building the model
    if conf.weights is not None:
        ck = torch.load(conf.weights, map_location="cpu", weights_only=False)
        model.load_state_dict({k[len("module."):] if k.startswith("module.") else k: v for k, v in ck["state_dict"].items()})
    tr = GenesisPretrainer(model, lr=1e-2, momentum=0.9, weight_decay=0.0, nesterov=False, patience=conf.patience)
    initial_epoch = 0
    if conf.weights is not None:
        tr.opt.load_state_dict(ck["optimizer_state_dict"], amp=tr.amp)
        initial_epoch = int(ck["epoch"])
        log(f"Loading weights from {conf.weights}")
    ops.bump_param_generation()
    os.makedirs(conf.model_path, exist_ok=True)
    ck_path = os.path.join(conf.model_path, f"{conf.exp_name}.pt")
    n_tr, n_va = int(train_gen.N // B), int(valid_gen.N // B)
    best_loss, no_improve, epochs_run = 100000, 0, 0
    fold_train, fold_valid, avg_train, avg_valid = {}, {}, [], []
    tl = torch.zeros(max(n_tr, 1), dtype=torch.float32, device=dev)
    vl = torch.zeros(max(n_va, 1), dtype=torch.float32, device=dev)
    for epoch in range(initial_epoch, conf.nb_epoch):
        tr.set_epoch(epoch)
        model.train()
        for it in range(n_tr):
            x, y = next(train_gen)
            tl[it:it + 1].copy_(tr.step(x, y))
        model.eval()
        for it in range(n_va):
            x, y = next(valid_gen)
            vl[it:it + 1].copy_(tr.evaluate(x, y))
        # the epoch's one read-back: losses + both generators' error words
        host = torch.cat([tl[:n_tr], vl[:n_va], train_gen.err.float(), valid_gen.err.float()]).cpu().numpy()
        train_gen.check(host[n_tr + n_va])
        valid_gen.check(host[n_tr + n_va + 1])
        train_losses = [round(float(v), 2) for v in host[:n_tr]]
        valid_losses = [float(v) for v in host[n_tr:n_tr + n_va]]
        fold_train[f"fold_{epoch}"] = train_losses
        fold_valid[f"fold_{epoch}"] = valid_losses
        train_loss, valid_loss = np.average(train_losses), np.average(valid_losses)
        avg_train.append(train_loss)
        avg_valid.append(valid_loss)
        epochs_run += 1
        log("Epoch {}, validation loss is {:.4f}, training loss is {:.4f}".format(epoch + 1, valid_loss, train_loss))
        if valid_loss < best_loss:
            log("Validation loss decreases from {:.4f} to {:.4f}".format(best_loss, valid_loss))
            best_loss, no_improve = valid_loss, 0
            export_checkpoint(model.state_dict(), ck_path, "genesis", epoch=epoch + 1, optimizer_state=tr.opt.state_dict())
            log(f"Saving model {ck_path}")
        else:
            log("Validation loss does not decrease from {:.4f}, num_epoch_no_improvement {}".format(best_loss, no_improve))
            no_improve += 1
        if no_improve == conf.patience:
            log("Early Stopping")
            break
    losses_path = os.path.join(losses_dir, f"{conf.exp_name}_train_valid_losses.pkl")
    with open(losses_path, "wb") as f:
        pickle.dump({"train_losses": fold_train, "valid_losses": fold_valid}, f)
    return {"best_loss": best_loss, "epochs_run": epochs_run, "checkpoint": ck_path, "losses_path": losses_path,
            "avg_train_losses": avg_train, "avg_valid_losses": avg_valid, "trainer": tr}
