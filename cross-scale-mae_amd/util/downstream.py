"""What the two downstream drivers (main_linprobe.py; main_finetune.py with engine_finetune.py) share: the synthetic / fMoW-RGB loaders, the
autocast context, the device-side loss drain, and the pieces of `main` that are the same in both (model construction, lr scaling printout,
output directory)."""
import contextlib
import math
import os
from pathlib import Path

import torch

import models_vit


def nullable_string(val):
    return val if val else None


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


def build_model(args, drop_path_rate=0.0):
    """The reference's factory call, with --embed_dim / --depth / --num_heads overriding the factory's geometry."""
    geometry = {k: getattr(args, k) for k in ("embed_dim", "depth", "num_heads") if getattr(args, k) is not None}
    return models_vit.__dict__[args.model](patch_size=args.patch_size, img_size=args.input_size, in_chans=resolve_input_channels(args),
                                           num_classes=args.nb_classes, drop_path_rate=drop_path_rate, global_pool=args.global_pool, **geometry)


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
