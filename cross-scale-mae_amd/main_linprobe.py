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

import torch

import util.misc as misc
from util.downstream import (add_checkpoint_flags, add_classification_data_flags, add_model_flags, add_pooling_flags, add_run_flags, add_schedule_flags,
                             autocast, build_loaders, build_model, fit, lars_update, load_pretrained, make_output_dir, save_due, scale_lr, start_run,
                             train_epoch)
from util.lars import LARS


def get_args_parser():
    p = argparse.ArgumentParser("Cross-MAE Linear Probe", add_help=False)
    add_schedule_flags(p)   # (weight decay 0 for the linear probe, following MoCo v1)
    add_model_flags(p)
    add_checkpoint_flags(p)
    add_pooling_flags(p)
    add_classification_data_flags(p)
    add_run_flags(p)
    return p


def train_one_epoch(model, data_loader, optimizer, device, epoch, args=None, log_writer=None):
    """engine_finetune.py's epoch for the probe: LR schedule per iteration, loss / lr / acc1 / acc5 meters, gradient accumulation.  The
    model computes the cross-entropy itself (`model(samples, targets)`); loss and hit counts are read every `print_freq` iterations."""
    return train_epoch(model, data_loader, optimizer, device, epoch, args, lars_update(optimizer, args.accum_iter), counts=model.drain_counts)


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


def main(args):
    device = start_run(args, "main_linprobe.py", "linear probing",
                       "the head is tiny; the frozen trunk could be sharded over ranks, which this script does not do")
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

    fit(args, model, optimizer, None, log_name="log.jsonl", best=("acc1", "Max accuracy"),
        train=lambda epoch: train_one_epoch(model, loader_train, optimizer, device, epoch, args=args),
        evaluate=lambda: evaluate(loader_val, model, device, args), save_at=lambda epoch: save_due(args, epoch, args.epochs / 2))


if __name__ == "__main__":
    main(get_args_parser().parse_args())
