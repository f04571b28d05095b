#!/usr/bin/env python3
"""Linear probing of a pre-trained encoder on the MI355X path — the reference's `main_linprobe.py` flags that make sense here (same
names, types and defaults), its model factory call, LR scaling, probe head (BatchNorm1d(affine=False) + Linear, everything else frozen,
:515-525), LARS, checkpoint layout and `log.jsonl`, and a `train_one_epoch` / `evaluate` pair after `engine_finetune.py`.

Differences:
  * `--dataset_type rgb` (the default) reads the fMoW-RGB CSVs `--train_path` / `--test_path`: the loader workers only decode, the
    training and the eval transform of `util/datasets.py` run on the device (`util/gpu_input.py`); `--dataset_type synthetic`
    (+ `--synthetic_len`, `--input_channels`) feeds fixed in-memory batches with fixed labels generated on the device; `--dataset_type euro_sat`
    reads lists of 13-band uint16 tiles (`path label` lines; `--masked_bands`, `--dropped_bands`; `util/ms_input.py`, the transform on the device)
    and sets the model's channels to 13 - len(dropped_bands); the other multi-band readers (Sentinel / NAIP / ...) need rasterio / fiona and are
    not wired (selecting them raises);
  * `--model` defaults to `vit_base_patch16` (the reference's default `mae_vit_base` names no factory of `models_vit`);
    `--embed_dim / --depth / --num_heads` override a factory's geometry for small runs;
  * the per-iteration loss and the top-1 / top-5 hit counts stay on the device and are drained every `--print_freq` iterations; a
    non-finite loss raises at that drain, and LARS skips on the device every update whose loss was not finite;
  * the probe head is always built (the reference builds it only with --finetune, so its --eval --resume of a probe checkpoint drops
    the head); a pos_embed of another grid size in --finetune is left out, the model keeps its own sin-cos table of the right size;
  * mixup, layer decay, drop-path, F1 / mIoU, W&B / TensorBoard and multi-GPU probing are out of scope (WORLD_SIZE > 1 raises).

    python main_linprobe.py --model vit_base_patch16 --finetune out/checkpoint-199.pth --transform_checkpoint_keys \\
        --dataset_type rgb --train_path train_62classes.csv --test_path val_62classes.csv --batch_size 128 --epochs 1
"""
import argparse
import datetime
import json
import os
import time

import numpy as np
import torch

import util.lr_sched as lr_sched
import util.misc as misc
from util.checkpoint_keys import to_vit_keys
from util.downstream import PendingLosses, autocast, build_loaders, build_model, make_output_dir, nullable_string, scale_lr
from util.lars import LARS


def get_args_parser():
    p = argparse.ArgumentParser("Cross-MAE Linear Probe", add_help=False)
    p.add_argument("--batch_size", default=512, type=int, help="Batch size per GPU (effective batch size is batch_size * accum_iter * # gpus")
    p.add_argument("--epochs", default=50, type=int)
    p.add_argument("--accum_iter", type=int, default=1)
    p.add_argument("--model", default="vit_base_patch16", type=str, metavar="MODEL")
    p.add_argument("--input_size", default=224, type=int)
    p.add_argument("--patch_size", default=16, type=int)
    p.add_argument("--weight_decay", type=float, default=0.0, help="weight decay (default: 0 for linear probe following MoCo v1)")
    p.add_argument("--lr", type=float, default=None, metavar="LR")
    p.add_argument("--blr", type=float, default=0.1, metavar="LR", help="base learning rate: absolute_lr = base_lr * total_batch_size / 256")
    p.add_argument("--min_lr", type=float, default=0.0, metavar="LR")
    p.add_argument("--warmup_epochs", type=int, default=10, metavar="N")
    p.add_argument("--finetune", default="", help="probe from this pre-training checkpoint")
    p.add_argument("--global_pool", action="store_true")
    p.set_defaults(global_pool=False)
    p.add_argument("--cls_token", action="store_false", dest="global_pool", help="Use class token instead of global pool for classification")
    p.add_argument("--transform_checkpoint_keys", action="store_true", default=False,
                   help="map the pre-training model's keys to ViT keys (applied by itself when the checkpoint holds encoder_pos_embed)")
    p.add_argument("--train_path", default="./train_64.csv", type=str, help="Train .csv path")
    p.add_argument("--test_path", default="/data2/HDD_16TB/fmow-rgb-preproc/val_224.csvv", type=str, help="Test .csv path")
    p.add_argument("--dataset_type", type=str, default="rgb", choices=["rgb", "sentinel", "euro_sat", "naip", "smart", "spacenetv1", "resisc45", "synthetic"])
    p.add_argument("--masked_bands", default=None, nargs="+", type=int, help="euro_sat: bands overwritten with their mean")
    p.add_argument("--dropped_bands", type=int, nargs="+", default=None, help="euro_sat: bands removed from the input")
    p.add_argument("--nb_classes", default=62, type=int, help="number of the classification types")
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--output_dir_base", type=str, default="./out")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", type=nullable_string, default=None)
    p.add_argument("--save_every", type=int, default=1)
    p.add_argument("--start_epoch", default=0, type=int, metavar="N")
    p.add_argument("--eval", action="store_true", help="Perform evaluation only")
    p.add_argument("--num_workers", type=int, default=10, help="decoding worker processes of the rgb loader")
    # ---- additive flags of the MI355X build
    p.add_argument("--synthetic_len", type=int, default=64, help="iterations per epoch of the synthetic loader (a quarter of it for evaluation)")
    p.add_argument("--input_channels", type=int, default=None, help="bands of the synthetic loader / model (3 when not given; euro_sat: 13 - len(dropped_bands))")
    p.add_argument("--print_freq", type=int, default=20, help="iterations between two drains of the device-side loss / accuracy counters")
    p.add_argument("--embed_dim", type=int, default=None)
    p.add_argument("--depth", type=int, default=None)
    p.add_argument("--num_heads", type=int, default=None)
    return p


def train_one_epoch(model, data_loader, optimizer, device, epoch, args=None, log_writer=None):
    """engine_finetune.py's epoch for the probe: LR schedule per iteration, loss / lr / acc1 / acc5 meters, gradient accumulation.  The
    model computes the cross-entropy itself (`model(samples, targets)`); loss and hit counts are read every `print_freq` iterations."""
    model.train(True)
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = f"Epoch: [{epoch}]"
    accum_iter, print_freq = args.accum_iter, getattr(args, "print_freq", 20)
    optimizer.zero_grad(set_to_none=False)
    n_iters = len(data_loader)
    pending = PendingLosses()
    gate = None
    model.drain_counts()

    for it, (samples, targets) in enumerate(metric_logger.log_every(data_loader, print_freq, header)):
        if it % accum_iter == 0:
            lr_sched.adjust_learning_rate(optimizer, it / n_iters + epoch, args)
        samples, targets = samples.to(device, non_blocking=True), targets.to(device, non_blocking=True)
        with autocast(device):
            loss, _ = model(samples, targets)
        pending.append(loss, optimizer.param_groups[0]["lr"])
        gate = loss.detach().reshape(1) if it % accum_iter == 0 else gate + loss.detach().reshape(1)   # the update's losses, summed
        (loss / accum_iter).backward()
        if (it + 1) % accum_iter == 0:
            optimizer.step(gate=gate)
            optimizer.zero_grad(set_to_none=False)
        if it % print_freq == 0 or it == n_iters - 1:
            pending.drain(metric_logger, model.drain_counts)   # exactly the iterations on which log_every prints the meters
    pending.drain(metric_logger, model.drain_counts)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


@torch.no_grad()
def evaluate(data_loader, model, device, args=None):
    """-> {"loss", "acc1", "acc5"} over the loader, in eval mode (running statistics normalise); one host read at the end."""
    model.eval()
    model.drain_counts()
    losses = []
    for samples, targets in data_loader:
        samples, targets = samples.to(device, non_blocking=True), targets.to(device, non_blocking=True)
        with autocast(device):
            loss, _ = model(samples, targets)
        losses.append(loss * samples.shape[0])
    top1, top5, seen = model.drain_counts()
    stats = {"loss": float(torch.stack(losses).sum()) / seen, "acc1": 100.0 * top1 / seen, "acc5": 100.0 * top5 / seen}
    print("* Acc@1 {acc1:.3f} Acc@5 {acc5:.3f} loss {loss:.3f}".format(**stats))
    return stats


def load_pretrained(model, path, transform_keys=False):
    """main_linprobe.py:441-512: load the trunk from a pre-training checkpoint; only the head (and fc_norm under global pooling) may be missing."""
    checkpoint = torch.load(path, map_location="cpu", weights_only=False)
    print("Load pre-trained checkpoint from: %s" % path)
    sd = checkpoint["model"]
    if transform_keys or "encoder_pos_embed" in sd:
        sd = to_vit_keys(sd)
    own = model.state_dict()
    if "pos_embed" in sd and sd["pos_embed"].shape != own["pos_embed"].shape:
        print(f"pos_embed {tuple(sd['pos_embed'].shape)} of the checkpoint does not fit {tuple(own['pos_embed'].shape)}: keeping the model's sin-cos table")
        sd = {k: v for k, v in sd.items() if k != "pos_embed"}
    msg = model.load_state_dict(sd, strict=False)
    print(msg)
    expected = {"head.weight", "head.bias"} | ({"fc_norm.weight", "fc_norm.bias"} if model.global_pool else set())
    assert set(msg.missing_keys) == expected, sorted(set(msg.missing_keys) ^ expected)
    return msg


def main(args):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("multi-GPU linear probing is not implemented: run main_linprobe.py as one process (the head is tiny; the "
                                  "frozen trunk could be sharded over ranks, which this script does not do)")
    print(f"job dir: {os.path.dirname(os.path.realpath(__file__))}")
    print(f"{args}".replace(", ", ",\n"))
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    loader_train, loader_val, n_val = build_loaders(args, device)

    model = build_model(args)
    if args.finetune and not args.eval:
        load_pretrained(model, args.finetune, args.transform_checkpoint_keys)
    model.probe_mode()
    model.to(device)
    print(f"Model = {model}")

    scale_lr(args, model)
    optimizer = LARS(model.head.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    print(optimizer)
    misc.load_model(args=args, model_without_ddp=model, optimizer=optimizer, loss_scaler=None)

    model_name = "_".join([args.model, f"i{args.input_size}-p{args.patch_size}", f"e{args.epochs}-we{args.warmup_epochs}",
                           f"b{args.batch_size}-a{args.accum_iter}", f"lr{args.lr}", "_global_pool" if args.global_pool else "_cls_only", "linprobe"])
    make_output_dir(args, model_name)

    if args.eval:
        stats = evaluate(loader_val, model, device, args)
        print(f"Evaluation on {n_val} test images:\n\tacc1: {stats['acc1']:.2f}%\n\tacc5: {stats['acc5']:.2f}%")
        return stats

    print(f"Start training for {args.epochs} epochs")
    start_time = time.time()
    max_accuracy = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        train_stats = train_one_epoch(model, loader_train, optimizer, device, epoch, args=args)
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}, "epoch": epoch}
        if (epoch % args.save_every == 0 and epoch >= args.epochs / 2) or (epoch % 5 == 0 and epoch < args.epochs / 2) or epoch + 1 == args.epochs:
            misc.save_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer, loss_scaler=None, epoch=epoch)
        test_stats = evaluate(loader_val, model, device, args)
        max_accuracy = max(max_accuracy, test_stats["acc1"])
        print(f"Max accuracy: {max_accuracy:.2f}%")
        log_stats.update({f"test_{k}": v for k, v in test_stats.items()})
        with open(os.path.join(args.output_dir, "log.jsonl"), mode="a", encoding="utf-8") as f:
            f.write(json.dumps(log_stats) + "\n")
    print(f"Training time {datetime.timedelta(seconds=int(time.time() - start_time))}")


if __name__ == "__main__":
    main(get_args_parser().parse_args())
