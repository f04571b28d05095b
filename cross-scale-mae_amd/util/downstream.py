"""What the downstream drivers (main_linprobe.py; main_finetune.py with engine_finetune.py; main_knn.py; main_segprobe.py) are written from:
the flag groups of their command lines (`add_*_flags`), the head of `main` (`start_run`), the checkpoint reader (`read_pretrained`) with the
probe's loading policy on top (`load_pretrained`), the synthetic / fMoW-RGB / EuroSAT loaders, model construction, lr scaling printout and
output directory, the training epoch (`train_epoch` with its device-side loss drain, `PendingLosses`, and the LARS update of the probes) and
the epoch loop of `main` (`fit`).  A driver keeps what is its own: the flags and defaults that differ, its model and optimizer, its `evaluate`."""
import contextlib
import datetime
import json
import math
import os
import time
from pathlib import Path

import numpy as np
import torch

import models_vit
import util.lr_sched as lr_sched
import util.misc as misc
from util.checkpoint_keys import to_vit_keys


def nullable_string(val):
    return val if val else None


# ---- the flag table: a driver's get_args_parser is these groups, the defaults that differ, and the flags that are its own
def add_model_flags(p, input_size=224):
    p.add_argument("--model", default="vit_base_patch16", type=str, metavar="MODEL")
    p.add_argument("--input_size", default=input_size, type=int)
    p.add_argument("--patch_size", default=16, type=int)
    for name in ("--embed_dim", "--depth", "--num_heads"):   # additive flags of the MI355X build: override the factory's geometry
        p.add_argument(name, type=int, default=None)


def add_checkpoint_flags(p, what="probe from this pre-training checkpoint"):
    p.add_argument("--finetune", default="", help=what)
    p.add_argument("--transform_checkpoint_keys", action="store_true", default=False,
                   help="map the pre-training model's keys to ViT keys (applied by itself when the checkpoint holds encoder_pos_embed)")


def add_pooling_flags(p, global_pool=False):
    p.add_argument("--global_pool", action="store_true")
    p.set_defaults(global_pool=global_pool)
    p.add_argument("--cls_token", action="store_false", dest="global_pool", help="Use class token instead of global pool for classification")


def add_classification_data_flags(p):
    p.add_argument("--train_path", default="./train_64.csv", type=str, help="Train .csv path")
    p.add_argument("--test_path", default="/data2/HDD_16TB/fmow-rgb-preproc/val_224.csvv", type=str, help="Test .csv path")
    p.add_argument("--dataset_type", type=str, default="rgb", choices=["rgb", "sentinel", "euro_sat", "naip", "smart", "spacenetv1", "resisc45", "synthetic"])
    p.add_argument("--masked_bands", default=None, nargs="+", type=int, help="euro_sat: bands overwritten with their mean")
    p.add_argument("--dropped_bands", type=int, nargs="+", default=None, help="euro_sat: bands removed from the input")
    p.add_argument("--nb_classes", default=62, type=int, help="number of the classification types")
    p.add_argument("--input_channels", type=int, default=None, help="bands of the synthetic loader / model (3 when not given; euro_sat: 13 - len(dropped_bands))")


def add_run_flags(p):
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--output_dir_base", type=str, default="./out")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--num_workers", type=int, default=10, help="decoding worker processes of the file loaders")
    p.add_argument("--synthetic_len", type=int, default=64, help="iterations per epoch of the synthetic loader (a quarter of it for evaluation)")


def add_schedule_flags(p, batch_size=512, epochs=50, weight_decay=0.0, blr=0.1, min_lr=0.0, warmup_epochs=10):
    p.add_argument("--batch_size", default=batch_size, type=int, help="Batch size per GPU (effective batch size is batch_size * accum_iter * # gpus")
    p.add_argument("--epochs", default=epochs, type=int)
    p.add_argument("--accum_iter", type=int, default=1)
    p.add_argument("--weight_decay", type=float, default=weight_decay)
    p.add_argument("--lr", type=float, default=None, metavar="LR")
    p.add_argument("--blr", type=float, default=blr, metavar="LR", help="base learning rate: absolute_lr = base_lr * total_batch_size / 256")
    p.add_argument("--min_lr", type=float, default=min_lr, metavar="LR")
    p.add_argument("--warmup_epochs", type=int, default=warmup_epochs, metavar="N")
    p.add_argument("--resume", type=nullable_string, default=None)
    p.add_argument("--save_every", type=int, default=1)
    p.add_argument("--start_epoch", default=0, type=int, metavar="N")
    p.add_argument("--eval", action="store_true", help="Perform evaluation only")
    p.add_argument("--print_freq", type=int, default=20, help="iterations between two drains of the device-side loss / accuracy counters")


def start_run(args, script, what, why, validate=None):
    """The head of a driver's `main`: refuse a multi-process launch, `validate()` the driver's own flags, print the job, seed torch and numpy.
    -> the device"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError(f"multi-GPU {what} is not implemented: run {script} as one process ({why})")
    if validate is not None:
        validate()
    print(f"job dir: {os.path.dirname(os.path.dirname(os.path.realpath(__file__)))}")   # (the drivers' directory)
    print(f"{args}".replace(", ", ",\n"))
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    return device


def autocast(device):
    return torch.autocast("cuda", dtype=torch.bfloat16) if torch.device(device).type == "cuda" else contextlib.nullcontext()


class SyntheticLoader:
    """In-memory repeat loader: (samples [N, C, S, S] ~ N(0, 1), labels [N] int64) on `device`, the same batch every iteration."""

    def __init__(self, batch, channels, size, classes, length, device, seed):
        g = torch.Generator(device=device).manual_seed(seed)
        self.samples = torch.randn(batch, channels, size, size, device=device, generator=g)
        self.targets = torch.randint(0, classes, (batch,), device=device, generator=g)
        self.length = length

    def __len__(self):
        return self.length

    def __iter__(self):
        for _ in range(self.length):
            yield self.samples, self.targets


def resolve_input_channels(args):
    """Settle `args.input_channels` before loaders and model are built: euro_sat has 13 - len(dropped_bands) bands (a flag that says otherwise
    raises ValueError); every other type keeps the flag, 3 when it was not given."""
    if args.dataset_type == "euro_sat":
        from util.ms_input import eurosat_channels
        args.input_channels = eurosat_channels(args)
    elif getattr(args, "input_channels", None) is None:
        args.input_channels = 3
    return args.input_channels


def build_loaders(args, device):
    """-> (train loader or None under --eval, eval loader, number of eval images) for --dataset_type synthetic / rgb / euro_sat.  Any other type
    raises NotImplementedError; a missing CSV or tile list raises the FileNotFoundError of its read."""
    resolve_input_channels(args)
    if args.dataset_type == "euro_sat":
        # EuroSAT lists of `path label` lines (util/datasets.py:489-564): the workers read uint16 tiles, the transform runs on the device
        from util.ms_input import build_eurosat_loader
        loader_train = None if args.eval else build_eurosat_loader(args.train_path, True, args, device)
        loader_val = build_eurosat_loader(args.test_path, False, args, device)
        return loader_train, loader_val, len(loader_val.dataset)
    if args.dataset_type == "synthetic":
        loader_train = SyntheticLoader(args.batch_size, args.input_channels, args.input_size, args.nb_classes, args.synthetic_len, device, args.seed)
        loader_val = SyntheticLoader(args.batch_size, args.input_channels, args.input_size, args.nb_classes, max(1, args.synthetic_len // 4), device, args.seed)
        return loader_train, loader_val, len(loader_val) * args.batch_size
    if args.dataset_type != "rgb":
        raise NotImplementedError(f"--dataset_type {args.dataset_type}: this reader of the reference (util/datasets.py) depends on rasterio / fiona "
                                  "and is not wired here; use --dataset_type rgb / euro_sat / synthetic or drive train_one_epoch / evaluate with your own "
                                  "iterable of (samples, labels)")
    if args.input_channels != 3:
        raise ValueError(f"--dataset_type rgb decodes 3 bands: --input_channels {args.input_channels} does not fit")
    from util.gpu_input import build_fmow_rgb_loader
    loader_train = None if args.eval else build_fmow_rgb_loader(args.train_path, True, args, device)
    loader_val = build_fmow_rgb_loader(args.test_path, False, args, device)
    return loader_train, loader_val, len(loader_val.dataset)


class PendingLosses:
    """The (device loss, lr) pairs of the iterations since the last drain: nothing is read back until `drain`."""

    def __init__(self):
        self.pending = []

    def append(self, loss, lr):
        self.pending.append((loss, lr))

    def drain(self, metric_logger, counts=None):
        """One host read of the pending losses into the `loss` / `lr` meters; a non-finite loss raises.  `counts`: a model's `drain_counts`, folded
        into the `acc1` / `acc5` meters."""
        if not self.pending:
            return
        values = torch.stack([p[0].detach().float().reshape(()) for p in self.pending]).tolist()
        if counts is not None:
            top1, top5, seen = counts()
        for value, (_, lr) in zip(values, self.pending):
            if not math.isfinite(value):
                print(f"Loss is {value}, stopping training")
                raise ValueError(f"Loss is {value}, stopping training")
            metric_logger.update(loss=value)
            metric_logger.update(lr=lr)
        if counts is not None:
            metric_logger.meters["acc1"].update(100.0 * top1 / seen, n=seen)
            metric_logger.meters["acc5"].update(100.0 * top5 / seen, n=seen)
        self.pending.clear()


def lars_update(optimizer, accum_iter):
    """The probes' update step, `update(loss, it)`: backward, and at the end of each accumulation window a LARS step gated on the device by the
    window's summed losses (an update whose loss was not finite is skipped there).  Gradients are zeroed in place."""
    gate = None

    def update(loss, it):
        nonlocal gate
        gate = loss.detach().reshape(1) if it % accum_iter == 0 else gate + loss.detach().reshape(1)
        (loss / accum_iter).backward()
        if (it + 1) % accum_iter == 0:
            optimizer.step(gate=gate)
            optimizer.zero_grad(set_to_none=False)
    optimizer.zero_grad(set_to_none=False)
    return update


def train_epoch(model, data_loader, optimizer, device, epoch, args, update, transform=None, counts=None):
    """One training epoch of engine_finetune.py's shape: LR schedule per iteration, autocast forward of `model(samples, targets)` (the model
    computes its loss), `update(loss, it)` for backward and step, loss / lr meters.  Losses stay on the device and are read every
    `args.print_freq` iterations; a non-finite one raises at that drain.  `transform`: applied to (samples, targets) before the forward (mixup).
    `counts`: a model's `drain_counts`, cleared before the loop and folded into the acc1 / acc5 meters at each drain.  The lr logged is the
    largest group's (the probes have one group).  -> {meter: global average}"""
    model.train(True)
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    accum_iter, print_freq = args.accum_iter, getattr(args, "print_freq", 20)
    n_iters = len(data_loader)
    pending = PendingLosses()
    if counts is not None:
        counts()
    for it, (samples, targets) in enumerate(metric_logger.log_every(data_loader, print_freq, f"Epoch: [{epoch}]")):
        if it % accum_iter == 0:   # a per-iteration (not per-epoch) schedule
            lr_sched.adjust_learning_rate(optimizer, it / n_iters + epoch, args)
        samples, targets = samples.to(device, non_blocking=True), targets.to(device, non_blocking=True)
        if transform is not None:
            samples, targets = transform(samples, targets)
        with autocast(device):
            loss, _ = model(samples, targets)
        pending.append(loss, max(g["lr"] for g in optimizer.param_groups))
        update(loss, it)
        if it % print_freq == 0 or it == n_iters - 1:
            pending.drain(metric_logger, counts)   # exactly the iterations on which log_every prints the meters
    pending.drain(metric_logger, counts)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def build_model(args, drop_path_rate=0.0):
    """The reference's factory call, with --embed_dim / --depth / --num_heads overriding the factory's geometry."""
    geometry = {k: getattr(args, k) for k in ("embed_dim", "depth", "num_heads") if getattr(args, k) is not None}
    return models_vit.__dict__[args.model](patch_size=args.patch_size, img_size=args.input_size, in_chans=resolve_input_channels(args),
                                           num_classes=args.nb_classes, drop_path_rate=drop_path_rate, global_pool=args.global_pool, **geometry)


def read_pretrained(path, transform_keys=False):
    """-> the `model` state dict of a pre-training checkpoint, its keys mapped to ViT keys when asked or when it holds encoder_pos_embed"""
    checkpoint = torch.load(path, map_location="cpu", weights_only=False)
    print("Load pre-trained checkpoint from: %s" % path)
    sd = checkpoint["model"]
    return to_vit_keys(sd) if transform_keys or "encoder_pos_embed" in sd else sd


def load_pretrained(model, path, transform_keys=False):
    """The probes' policy (main_linprobe.py:441-512): load the trunk; only the head (and fc_norm under global pooling) may be missing.  A pos_embed of
    another grid size is left out: the model keeps its own sin-cos table."""
    sd = read_pretrained(path, transform_keys)
    own = model.state_dict()
    if "pos_embed" in sd and sd["pos_embed"].shape != own["pos_embed"].shape:
        print(f"pos_embed {tuple(sd['pos_embed'].shape)} of the checkpoint does not fit {tuple(own['pos_embed'].shape)}: keeping the model's sin-cos table")
        sd = {k: v for k, v in sd.items() if k != "pos_embed"}
    msg = model.load_state_dict(sd, strict=False)
    print(msg)
    expected = {"head.weight", "head.bias"} | ({"fc_norm.weight", "fc_norm.bias"} if model.global_pool else set())
    assert set(msg.missing_keys) == expected, sorted(set(msg.missing_keys) ^ expected)
    return msg


def scale_lr(args, model):
    """Print the effective batch size and the learning rates; `args.lr` is derived from `args.blr` when not given."""
    batch_size_eff = args.batch_size * args.accum_iter
    print("accumulate grad iterations: %d" % args.accum_iter)
    print("effective batch size: %d" % batch_size_eff)
    print("number of params (M): %.2f" % (sum(p.numel() for p in model.parameters() if p.requires_grad) / 1.0e6))
    if args.lr is None:
        args.lr = args.blr * batch_size_eff / 256
    print("base lr: %.2e" % (args.lr * 256 / batch_size_eff))
    print("actual lr: %.2e" % args.lr)


def make_output_dir(args, model_name):
    """`args.output_dir`, or out_<model_name> under `args.output_dir_base` when none is given, created."""
    if args.output_dir is None:
        args.output_dir = os.path.join(args.output_dir_base or ".", f"out_{model_name}")
    print(f"Output directory: {args.output_dir}")
    Path(args.output_dir).mkdir(parents=True, exist_ok=True)


def save_due(args, epoch, late):
    """The reference's checkpoint rule: every `save_every`-th epoch from epoch `late` on, every 5th before it, and the last one."""
    return (epoch % args.save_every == 0 and epoch >= late) or (epoch % 5 == 0 and epoch < late) or epoch + 1 == args.epochs


def fit(args, model, optimizer, loss_scaler, *, train, evaluate, save_at, best, log_name, report=None):
    """The epoch loop of a driver's `main`, epochs `args.start_epoch` .. `args.epochs`: `train(epoch)` -> train stats, a checkpoint when
    `save_at(epoch)`, `evaluate()` -> test stats, the line `report(test stats)` if given, the running maximum of test stat `best[0]` printed as
    `best[1]`, and one JSON line {train_*, epoch, test_*} appended to `<output_dir>/<log_name>`."""
    print(f"Start training for {args.epochs} epochs")
    start_time = time.time()
    key, label = best
    best_value = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        train_stats = train(epoch)
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}, "epoch": epoch}
        if save_at(epoch):
            misc.save_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer, loss_scaler=loss_scaler, epoch=epoch)
        test_stats = evaluate()
        if report is not None:
            print(report(test_stats))
        best_value = max(best_value, test_stats[key])
        print(f"{label}: {best_value:.2f}%")
        log_stats.update({f"test_{k}": v for k, v in test_stats.items()})
        with open(os.path.join(args.output_dir, log_name), mode="a", encoding="utf-8") as f:
            f.write(json.dumps(log_stats) + "\n")
    print(f"Training time {datetime.timedelta(seconds=int(time.time() - start_time))}")
