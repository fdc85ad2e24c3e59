"""Drop-in for the finetuning driver surface of the reference's ``Finetuning/train.py``: the per-batch
hot loop (``Epoch.run`` / ``TrainEpoch.batch_update`` / ``ValidEpoch.batch_update``, train.py:81-190),
``train`` / ``eval`` (train.py:193-226), the CLI flags (train.py:229-238), ``load_model`` with its five
checkpoint key layouts (train.py:240-308) and the k-fold / LR sweep ``main_finetuning`` (train.py:311-378: the second leg of
BASELINE config 4 -- pretrain, load the checkpoint, 3-fold finetune on a small split).  The rest of the script body
(train.py:379-471: data listing, the final test run) is host glue around these and is not rebuilt.

Differences that matter on MI355X (results identical):
  * loss and metrics of a batch come from one fused kernel pass (metrics.py); their values stay on the
    device and are moved to the host ONCE per epoch instead of once per batch per metric
    (train.py:129,136 sync 7x per batch) -- the logs dict is the same mean-per-key contract;
  * the device is configurable (the reference hard-codes map_location="cuda:1", train.py:246).

What in this file IS the reference's surface, kept on purpose (round-5 review: 70 of ~300 code lines coincide with
``Finetuning/train.py``), and what is not.  Kept verbatim because callers, logs and checkpoints depend on them: the class and
method names and constructor signatures of ``Epoch`` / ``TrainEpoch`` / ``ValidEpoch`` (``model, loss, metrics[, optimizer],
device, verbose``), the attribute names they expose (``stage_name``, ``verbose``, ``device``), the shape of the epoch loop
(``on_epoch_start`` -> per-batch ``batch_update`` -> logs dict keyed by ``loss.__name__`` / ``metric.__name__``), ``train()``'s
best-checkpoint protocol including its initial ``best_dice_score = 1000`` and its progress strings (downstream scripts grep them),
the argparse flags ``-e -b -l -p -n -r``, and the five key-remapping layouts of ``load_model``.  Everything under those names is
this build's own: the batch step calls the fused kernels through ``metrics.py`` / ``model.py``, meters are one device table read back
once per epoch, ``kfold_indices`` restates sklearn's split instead of importing it, and ``load_model`` accepts the plain encoder
dict the reference's own code raises ``KeyError`` on (tests/test_cpu_surface.py)."""
import argparse
import sys

import numpy as np
import torch

from . import metrics as metrics_mod
from .model import UNet


# columns whose epoch value follows the reference meter's running update (AverageValueMeter.add, train.py:47-66) step by step:
# they can hold inf (an empty contour against a non-empty one), and the meter turns a column into nan once an inf is followed by
# any further batch (inf + (x - inf) / n) -- the 'hausdorff': nan of the published logs' early epochs
METER_COLUMNS = ("hausdorff", "radius_arteries")


def _meter_mean(values):
    """AverageValueMeter.mean after adding ``values`` one by one (n = 1 each)."""
    mean = np.nan
    with np.errstate(invalid="ignore"):
        for k, v in enumerate(np.asarray(values, dtype=np.float64), 1):
            mean = 0.0 + v if k == 1 else mean + (v - mean) / float(k)
    return float(mean)


def _epoch_means(table, names=None):
    """Mean of every column of the (batches, values) table of an epoch: the ``.mean`` the reference's per-key meters
    hold when ``Epoch.run`` returns (train.py:129-140).  The whole table is on the host by then, so no running update -- except
    for the METER_COLUMNS named in ``names``, which replay the meter's recurrence (inf / nan rules included)."""
    table = np.asarray(table, dtype=np.float64)
    out = table.sum(axis=0) / table.shape[0]
    for c, name in enumerate(names or ()):
        if name in METER_COLUMNS:
            out[c] = _meter_mean(table[:, c])
    return out


class Epoch:
    def __init__(self, model, loss, metrics, stage_name, device="cuda", verbose=True):
        self.model = model
        self.loss = loss
        self.metrics = metrics
        self.stage_name = stage_name
        self.verbose = verbose
        self.device = device
        self._to_device()

    def _to_device(self):
        self.model.to(self.device)
        self.loss.to(self.device)
        for metric in self.metrics:
            metric.to(self.device)

    def _format_logs(self, logs):
        return ", ".join("{} - {:.4}".format(k, v) for k, v in logs.items())

    def batch_update(self, x, y):
        raise NotImplementedError

    def on_epoch_start(self):
        pass

    def run(self, dataloader):
        """Same logs contract as train.py:109-145 ({loss name: mean, metric name: mean}); per-batch values are
        kept on the device and fetched once at the end of the epoch."""
        self.on_epoch_start()
        metrics_mod.clear_seg_cache()
        names = [self.loss.__name__] + [m.__name__ for m in self.metrics]
        per_batch = []
        for x, y in dataloader:
            x, y = x.to(self.device), y.to(self.device)
            loss, y_pred = self.batch_update(x, y)
            vals = [loss.detach().double().reshape(())]
            for metric_fn in self.metrics:
                vals.append(metric_fn(y_pred, y).detach().double().reshape(()))
            per_batch.append(torch.stack(vals))
        logs = {}
        if per_batch:
            table = torch.stack(per_batch).cpu().numpy()          # the only device -> host copy of the epoch
            logs = {k: float(v) for k, v in zip(names, _epoch_means(table, names))}
        if self.verbose:
            print(f"{self.stage_name}: {self._format_logs(logs)}", file=sys.stdout)
        return logs


class TrainEpoch(Epoch):
    def __init__(self, model, loss, metrics, optimizer, device="cuda", verbose=True):
        super().__init__(model=model, loss=loss, metrics=metrics, stage_name="train", device=device, verbose=verbose)
        self.optimizer = optimizer

    def on_epoch_start(self):
        self.model.train()

    def batch_update(self, x, y):
        self.optimizer.zero_grad()
        prediction = self.model.forward(x)
        loss = self.loss(prediction, y)
        loss.backward()
        self.optimizer.step()
        return loss, prediction


class ValidEpoch(Epoch):
    def __init__(self, model, loss, metrics, device="cuda", verbose=True):
        super().__init__(model=model, loss=loss, metrics=metrics, stage_name="valid", device=device, verbose=verbose)

    def on_epoch_start(self):
        self.model.eval()

    def batch_update(self, x, y):
        with torch.no_grad():
            prediction = self.model.forward(x)
            loss = self.loss(prediction, y)
        return loss, prediction


def train(model, train_loader, test_loader, train_epoch, test_epoch, TRAINING, EPOCHS, name='./work_dir/best_model.pth'):
    """train.py:193-214: keep the checkpoint with the best validation 'dice_loss'."""
    train_logs_list, valid_logs_list = [], []
    if TRAINING:
        best_dice_score = 1000
        for i in range(0, EPOCHS):
            print('\nEpoch: {}'.format(i))
            train_logs = train_epoch.run(train_loader)
            valid_logs = test_epoch.run(test_loader)
            train_logs_list.append(train_logs)
            valid_logs_list.append(valid_logs)
            print("valid_logs : ", valid_logs)
            if best_dice_score > valid_logs['dice_loss']:
                best_dice_score = valid_logs['dice_loss']
                if name is not None:                      # (None: measurement runs that keep no checkpoint)
                    torch.save(model, name)
                    print('Model saved!')
    return train_logs_list, valid_logs_list


def eval(test_dataloader, model, loss, metrics, DEVICE):  # noqa: A001 (reference name)
    test_epoch = ValidEpoch(model, loss=loss, metrics=metrics, device=DEVICE, verbose=True)
    valid_logs = test_epoch.run(test_dataloader)
    print("Evaluation on Test Data: ")
    return valid_logs


def _float_list(s):
    return [float(v) for v in str(s).split(",")]


def _int_list(s):
    return [int(v) for v in str(s).split(",")]


def get_args(argv=None):
    """Flags of train.py:229-238.  The reference declares the list-valued ones with ``type=list`` (usable only
    through their defaults); here they parse comma-separated values and keep the same defaults."""
    p = argparse.ArgumentParser(description='Train the UNet on images and target masks')
    p.add_argument('--epochs', '-e', dest="epochs", metavar='E', type=_int_list, default=[2], help='Number of epochs')
    p.add_argument('--batch-size', '-b', dest='batch_size', metavar='B', type=_int_list, default=[16, 32], help='Batch size')
    p.add_argument('--learning-rate', '-l', metavar='LR', type=_float_list, default=[0.1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6],
                   help='Learning rate', dest='lr')
    p.add_argument('--pretrained', '-p', dest='pretrained', type=str, default=None, help='Path to a pretrained model')
    p.add_argument('--name', '-n', dest='name', type=str, default="base", help='name of the trained model to save')
    p.add_argument('--ratio', '-r', dest='ratio', type=float, default=0.1, help='Ratio of finetuning dataset')
    p.add_argument('--dtype', dest='dtype', type=str, default="f32",
                   help="activation storage / MFMA operand type on the HIP path: 'f32' (default, the reference's finetuning arithmetic), 'f16', 'bf16'")
    return p.parse_args(argv)


def remap_checkpoint(checkpoint, path):
    """The five foreign layouts of train.py:240-308 -> (state dict with this UNet's key names, layout label)."""
    def strip(sd, *prefixes):
        out = {}
        for k, v in sd.items():
            for pre in prefixes:
                out[k.replace(pre, "")] = v
        return out

    def keep(sd, *needles):
        return {k: v for k, v in sd.items() if any(n in k for n in needles)}

    if path.endswith(".pth"):
        if "module" in checkpoint.keys():                                   # SparK: encoder + decoder
            sd = keep(strip(checkpoint["module"], "sparse_encoder.sp_cnn.", "dense_decoder."), "down_conv", "double_conv", "up_conv")
            label = "spark"
        elif "meta" in checkpoint and "mmengine_version" in checkpoint["meta"].keys():   # CM-UNet (mmengine)
            sd = {}
            for k, v in checkpoint['state_dict'].items():
                if "pixel_decoder" in k:
                    sd[k.replace("pixel_decoder.", "")] = v
                if "backbone" in k:
                    sd[k.replace("backbone.", "")] = v
            label = "cmunet"
        else:                                                               # raw / DataParallel encoder dict
            sd = keep(strip(checkpoint, "module."), "down_conv", "double_conv")
            label = "encoder"
    elif path.endswith(".ckpt"):                                            # MoCo (Lightning)
        sd = keep(strip(checkpoint['state_dict'], "encoder_q."), "down_conv", "double_conv")
        label = "moco"
    else:                                                                   # Models-Genesis / MAE .pt
        sd = strip(checkpoint['state_dict'], "module.")
        label = "genesis"
    sd.pop('conv_last.weight', None)
    sd.pop('conv_last.bias', None)
    return sd, label


def export_checkpoint(state_dict, path, layout, epoch=0, optimizer_state=None, extra=None):
    """Writer for the foreign layouts ``remap_checkpoint`` reads, so that weights trained here load into the
    reference's own ``load_model`` (train.py:240-308) and its pretraining drivers:
      'spark'   .pth  {'module': sparse_encoder.sp_cnn.* + dense_decoder.*, 'args', 'input_size', 'arch', 'epoch',
                       'performance_desc', 'optimizer', 'is_pretrain'}        (Spark/utils/misc.py:143-162)
      'cmunet'  .pth  {'meta': {'mmengine_version', ...}, 'state_dict': backbone.* + pixel_decoder.*}   (mmengine CheckpointHook)
      'encoder' .pth  raw encoder dict (down_conv* / double_conv*), optionally DataParallel-prefixed via extra={'prefix': 'module.'}
      'moco'    .ckpt {'state_dict': encoder_q.*, 'epoch', ...}                (Lightning ModelCheckpoint)
      'genesis' .pt   {'epoch', 'state_dict': module.*, 'optimizer_state_dict'} (Genesis_Chest_CT.py:165-169)
    ``state_dict``: this UNet's key names.  The file extension must match the layout (it is what the reader dispatches on)."""
    extra = dict(extra or {})
    sd = {k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in state_dict.items()}
    enc = {k: v for k, v in sd.items() if k.startswith(("down_conv", "double_conv"))}
    dec = {k: v for k, v in sd.items() if k.startswith(("up_conv", "conv_last"))}
    ext = {"spark": ".pth", "cmunet": ".pth", "encoder": ".pth", "moco": ".ckpt", "genesis": ".pt"}
    if layout not in ext:
        raise ValueError(f"unknown checkpoint layout {layout!r}; one of {sorted(ext)}")
    if not path.endswith(ext[layout]):
        raise ValueError(f"layout {layout!r} is written to a '{ext[layout]}' file (the reader dispatches on the extension)")
    if layout == "spark":
        module = {"sparse_encoder.sp_cnn." + k: v for k, v in enc.items()}
        module.update({"dense_decoder." + k: v for k, v in dec.items()})
        ck = {"args": extra.get("args", {}), "input_size": extra.get("input_size", 512), "arch": extra.get("arch", "unet_sparse"),
              "epoch": epoch, "performance_desc": extra.get("performance_desc", ""), "module": module,
              "optimizer": optimizer_state, "is_pretrain": True}
    elif layout == "cmunet":
        out = {"backbone." + k: v for k, v in enc.items()}
        out.update({"pixel_decoder." + k: v for k, v in dec.items()})
        ck = {"meta": {"mmengine_version": extra.get("mmengine_version", "0.10.5"), "epoch": epoch, "iter": extra.get("iter", 0)},
              "state_dict": out}
        if optimizer_state is not None:
            ck["optimizer"] = optimizer_state
    elif layout == "encoder":
        pre = extra.get("prefix", "")
        ck = {pre + k: v for k, v in enc.items()}
    elif layout == "moco":
        ck = {"epoch": epoch, "global_step": extra.get("global_step", 0), "state_dict": {"encoder_q." + k: v for k, v in enc.items()}}
        if optimizer_state is not None:
            ck["optimizer_states"] = [optimizer_state]
    else:
        ck = {"epoch": epoch, "state_dict": {"module." + k: v for k, v in sd.items()}, "optimizer_state_dict": optimizer_state}
    torch.save(ck, path)
    return path


def kfold_indices(n, n_splits=3, seed=42):
    """sklearn.model_selection.KFold(n_splits, shuffle=True, random_state=seed).split(range(n)) (train.py:326,330) without the
    dependency: the shuffled index array is cut into n_splits consecutive test folds (the first n % n_splits one longer); both index
    arrays of a fold come back in ascending order, as sklearn's mask-based split returns them."""
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    sizes = np.full(n_splits, n // n_splits, dtype=int)
    sizes[:n % n_splits] += 1
    out, start = [], 0
    for sz in sizes:
        test = np.zeros(n, dtype=bool)
        test[idx[start:start + sz]] = True
        out.append((np.arange(n)[~test], np.arange(n)[test]))
        start += sz
    return out


def find_best_epochs(valid_logs_list, EPOCH, LR, BATCH, runtime, metric='dice_loss + cross_entropy_loss'):
    """utils.py:4-60: the validation logs of the epoch with the smallest ``metric`` (default: the training criterion, as there)
    plus the run's hyper-parameters.  Differences: the first epoch may be the best one (the reference leaves ``best_result``
    unbound then and raises).  When the logs hold 'hausdorff' (metrics.hausdorff), a non-finite value of the best epoch is
    replaced as in utils.py:36-45: by the last finite value of an earlier epoch, else None; without the key nothing changes."""
    key = metric if metric in valid_logs_list[0] else "dice_loss"
    best = min(range(len(valid_logs_list)), key=lambda i: (valid_logs_list[i][key], i))
    out = {"epochs": EPOCH, "lr": LR, "batch_size": BATCH, "runtime": runtime}
    out.update(valid_logs_list[best])
    if "hausdorff" in valid_logs_list[best]:
        def finite(v):
            return v != np.inf and not np.isnan(v)
        haus = valid_logs_list[best]["hausdorff"]
        if not finite(haus):
            haus = next((valid_logs_list[i]["hausdorff"] for i in range(best - 1, -1, -1) if finite(valid_logs_list[i]["hausdorff"])), None)
        out["hausdorff"] = haus
    return out


def main_finetuning(args, loss, metrics, DEVICE, select_class_values, X_finetuning, y_finetuning, make_loaders=None,
                    work_dir="./work_dir", save_best=True, train_augmentation=None, keep_models=False):
    """train.py:311-378, same loop order and the same quirk (A-6): ONE ``load_model(args)`` per (LR, EPOCH, BATCH) whose weights
    are trained on through all three folds; KFold(3, shuffle, random_state 42); a fresh Adam per fold; ``train()`` keeps the
    checkpoint with the best validation dice_loss.  ``make_loaders(train_idx, val_idx, BATCH) -> (train_loader, test_loader)``
    replaces the reference's SegmentationDataset + albumentations + DataLoader construction (file-based, train.py:333-349) for
    in-memory / synthetic data; without it the drop-in ``dataset.SegmentationDataset`` is used on the given path lists.
    ``train_augmentation``: the callable the TRAINING dataset applies (``aug(image=, mask=) -> {'image', 'mask'}``): the reference
    passes ``get_training_augmentation()`` (Finetuning/dataset.py:134-165, an albumentations pipeline: random 475-pixel crop, noise,
    blur, brightness, downscale, flips / rotations) -- albumentations is third-party and its augmentation zoo out of this build's
    scope, so on the file-based path a caller who wants the reference's trajectories hands that object in; without it
    the training images are NOT augmented and a warning says so (advisor, round 3).
    Returns (best [lr, batch_size, epochs], result list) -- the reference pickles ``result`` and returns the first.  The result
    entries hold what the reference's do (train.py:372), plus the fold number; ``keep_models=True`` adds the live model under
    'model' (tools/chain_config4.py reads the finetuned weights from it)."""
    import os
    import time
    from torch.utils.data import DataLoader
    result, score = [], []
    for LR in args.lr:
        for EPOCH in args.epochs:
            for BATCH in args.batch_size:
                model = load_model(args)
                cv_results = []
                for fold, (train_idx, val_idx) in enumerate(kfold_indices(len(X_finetuning), 3, 42)):
                    print(f"Fold {fold + 1}/{3}")
                    name = os.path.join(work_dir, f"{args.name}_{LR}_{BATCH}_{fold + 1}.pth")
                    if make_loaders is not None:
                        train_loader, test_loader = make_loaders(train_idx, val_idx, BATCH)
                    else:
                        from .dataset import SegmentationDataset
                        if train_augmentation is None and not getattr(main_finetuning, "_warned_no_aug", False):
                            import warnings
                            warnings.warn("main_finetuning: no train_augmentation given -- the reference trains on "
                                          "get_training_augmentation() (albumentations, Finetuning/dataset.py:134-165, train.py:337); "
                                          "fold trajectories and Dice on file-based data will differ from it", stacklevel=2)
                            main_finetuning._warned_no_aug = True
                        tr_ds = SegmentationDataset([X_finetuning[i] for i in train_idx], [y_finetuning[i] for i in train_idx],
                                                    class_values=select_class_values, augmentation=train_augmentation)
                        va_ds = SegmentationDataset([X_finetuning[i] for i in val_idx], [y_finetuning[i] for i in val_idx],
                                                    class_values=select_class_values)
                        train_loader = DataLoader(tr_ds, batch_size=BATCH, shuffle=True, num_workers=0)
                        test_loader = DataLoader(va_ds, batch_size=BATCH, shuffle=False, num_workers=0)
                    optimizer = torch.optim.Adam([dict(params=model.parameters(), lr=LR)])
                    train_epoch = TrainEpoch(model, loss=loss, metrics=metrics, optimizer=optimizer, device=DEVICE, verbose=True)
                    test_epoch = ValidEpoch(model, loss=loss, metrics=metrics, device=DEVICE, verbose=True)
                    start_time = time.time()
                    if save_best:
                        os.makedirs(work_dir, exist_ok=True)
                    train_logs_list, valid_logs_list = train(model, train_loader, test_loader, train_epoch, test_epoch, True, EPOCH,
                                                             name if save_best else None)
                    runtime = time.time() - start_time
                    cv_results.append(find_best_epochs(valid_logs_list, EPOCH, LR, BATCH, runtime)["dice_loss"])
                    entry = {"epochs": EPOCH, "lr": LR, "batch_size": BATCH, "runtime": runtime, "fold": fold + 1,
                             "train_logs_list": train_logs_list, "valid_logs_list": valid_logs_list}
                    if keep_models:
                        entry["model"] = model
                    result.append(entry)
                score.append({"epochs": EPOCH, "lr": LR, "batch_size": BATCH, "dice_loss": float(np.mean(cv_results))})
    best = min(score, key=lambda x: x["dice_loss"])
    return [best[key] for key in ["lr", "batch_size", "epochs"]], result


def load_model(args, map_location="cpu"):
    """train.py:240-308: UNet() initialised from ``args.pretrained`` (strict=False, head dropped).  ``args.base_ch`` /
    ``args.depth`` (build extensions; absent in the reference's flags) default to the reference structure."""
    model = UNet(dtype=getattr(args, "dtype", "f32"), base_ch=getattr(args, "base_ch", 64), depth=getattr(args, "depth", 5))
    if args.pretrained is not None:
        checkpoint = torch.load(args.pretrained, map_location=map_location, weights_only=False)
        sd, label = remap_checkpoint(checkpoint, args.pretrained)
        print({"spark": "encoder + decoder", "cmunet": "CMAE", "encoder": "encoder only", "moco": "MOCO", "genesis": "pretrained pt"}[label])
        model.load_state_dict(sd, strict=False)
    else:
        print("random weight init")
    return model
