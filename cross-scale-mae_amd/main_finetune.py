#!/usr/bin/env python3
"""End-to-end fine-tuning of a pre-trained encoder on the MI355X path — the reference's `main_finetune.py` flag table (same names, types
and defaults), its model factory call, position-embedding interpolation, head initialisation, layer-wise learning-rate decay, criterion
choice, checkpoint layout and `log.jsonl`, with `engine_finetune.train_one_epoch` / `evaluate`.

Differences:
  * `--drop_path` defaults to 0.0 (the reference: 0.1) and a value above 0 raises: drop-path is not implemented in the MI355X blocks;
  * `--dataset_type rgb` (the default) reads the fMoW-RGB CSVs `--train_path` / `--test_path`: the loader workers only decode, the
    training and the eval transform of `util/datasets.py` run on the device (`util/gpu_input.py`); `--dataset_type synthetic`
    (+ `--synthetic_len`, `--input_channels`) feeds fixed in-memory batches generated on the device; `--dataset_type euro_sat` reads
    lists of 13-band uint16 tiles (`path label` lines; `--masked_bands`, `--dropped_bands`; `util/ms_input.py`, the transform on the device) and sets
    the model's channels to 13 - len(dropped_bands); the other multi-band readers (Sentinel / NAIP / ...) need rasterio / fiona and are not wired
    (selecting them raises); the augmentation flags (`--aa`, `--color_jitter`,
    `--reprob`, ...) are parsed and unused, as the reference's fMoW-RGB dataset ignores them too;
  * `--model` defaults to `vit_base_patch16` (the reference's default `mae_vit_base` names no factory of `models_vit`);
    `--embed_dim / --depth / --num_heads` override a factory's geometry for small runs;
  * the model computes the criterion (soft-target cross-entropy under mixup, label-smoothed cross-entropy with `--smoothing`, otherwise plain
    cross-entropy) in HIP kernels; the optimizer is `csmae_hip.optim.FusedAdamW` over the layer-decay groups; mixup / cutmix is batch mode only;
  * losses are drained every `--print_freq` iterations; W&B / TensorBoard, `--use_psa` and multi-GPU fine-tuning are out of scope
    (WORLD_SIZE > 1 raises).

    python main_finetune.py --model vit_base_patch16 --finetune out/checkpoint-199.pth --transform_checkpoint_keys \\
        --dataset_type rgb --train_path train_62classes.csv --test_path val_62classes.csv --batch_size 128 --epochs 1
"""
import argparse
import datetime
import json
import os
import time

import numpy as np
import torch

import util.lr_decay as lrd
import util.misc as misc
from engine_finetune import evaluate, train_one_epoch
from util.checkpoint_keys import to_vit_keys
from util.downstream import build_loaders, build_model, make_output_dir, nullable_string, scale_lr
from util.misc import NativeScalerWithGradNormCount as NativeScaler
from util.mixup import Mixup
from util.pos_embed import interpolate_pos_embed


def get_args_parser():
    p = argparse.ArgumentParser("Cross-MAE fine-tuning", add_help=False)
    p.add_argument("--batch_size", default=512, type=int, help="Batch size per GPU (effective batch size is batch_size * accum_iter * # gpus")
    p.add_argument("--epochs", default=100, type=int)
    p.add_argument("--accum_iter", type=int, default=1)
    # model
    p.add_argument("--model_type", type=nullable_string, default=None, choices=["vanilla", None])
    p.add_argument("--model", default="vit_base_patch16", type=str, metavar="MODEL")
    p.add_argument("--input_size", default=128, type=int)
    p.add_argument("--patch_size", default=16, type=int)
    p.add_argument("--drop_path", type=float, default=0.0, metavar="PCT", help="Drop path rate: not implemented here, a value above 0 raises (reference default 0.1)")
    # optimizer
    p.add_argument("--clip_grad", type=float, default=None, metavar="NORM")
    p.add_argument("--weight_decay", type=float, default=0.05)
    p.add_argument("--lr", type=float, default=None, metavar="LR")
    p.add_argument("--blr", type=float, default=1e-3, metavar="LR", help="base learning rate: absolute_lr = base_lr * total_batch_size / 256")
    p.add_argument("--layer_decay", type=float, default=0.75, help="layer-wise lr decay from ELECTRA/BEiT")
    p.add_argument("--min_lr", type=float, default=1e-6, metavar="LR")
    p.add_argument("--warmup_epochs", type=int, default=5, metavar="N")
    # augmentation (parsed for compatibility: neither loader reads them)
    p.add_argument("--color_jitter", type=float, default=None, metavar="PCT")
    p.add_argument("--aa", type=str, default="rand-m9-mstd0.5-inc1", metavar="NAME")
    p.add_argument("--smoothing", type=float, default=0.1, help="Label smoothing (default: 0.1)")
    p.add_argument("--reprob", type=float, default=0.25, metavar="PCT")
    p.add_argument("--remode", type=str, default="pixel")
    p.add_argument("--recount", type=int, default=1)
    p.add_argument("--resplit", action="store_true", default=False)
    # mixup
    p.add_argument("--mixup", type=float, default=0.8, help="mixup alpha, mixup enabled if > 0.")
    p.add_argument("--cutmix", type=float, default=1.0, help="cutmix alpha, cutmix enabled if > 0.")
    p.add_argument("--cutmix_minmax", type=float, nargs="+", default=None)
    p.add_argument("--mixup_prob", type=float, default=1.0)
    p.add_argument("--mixup_switch_prob", type=float, default=0.5)
    p.add_argument("--mixup_mode", type=str, default="batch", help='only "batch" is implemented')
    # fine-tuning
    p.add_argument("--finetune", default="", help="finetune from checkpoint")
    p.add_argument("--use_psa", action="store_true")
    p.add_argument("--global_pool", action="store_true")
    p.set_defaults(global_pool=True)
    p.add_argument("--cls_token", action="store_false", dest="global_pool", help="Use class token instead of global pool for classification")
    # dataset
    p.add_argument("--train_path", default="./train_64.csv", type=str)
    p.add_argument("--test_path", default="/data2/HDD_16TB/fmow-rgb-preproc/val_224.csvv", type=str)
    p.add_argument("--dataset_type", type=str, default="rgb", choices=["rgb", "sentinel", "euro_sat", "naip", "smart", "spacenetv1", "resisc45", "synthetic"])
    p.add_argument("--masked_bands", default=None, nargs="+", type=int)
    p.add_argument("--dropped_bands", type=int, nargs="+", default=None)
    p.add_argument("--nb_classes", default=62, type=int, help="number of the classification types")
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--output_dir_base", type=str, default="./out")
    p.add_argument("--val_img_path", type=str, default="./images/")
    p.add_argument("--log_dir", default="./output_dir")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", type=nullable_string, default=None)
    p.add_argument("--save_every", type=int, default=1)
    p.add_argument("--wandb_entity", type=str, default="utk-iccv23")
    p.add_argument("--wandb_project", type=nullable_string, default=None)
    p.add_argument("--wandb_id", type=nullable_string, default=None)
    p.add_argument("--start_epoch", default=0, type=int, metavar="N")
    p.add_argument("--eval", action="store_true", help="Perform evaluation only")
    p.add_argument("--dist_eval", action="store_true", default=False)
    p.add_argument("--num_workers", type=int, default=10)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--local_rank", default=os.getenv("LOCAL_RANK", 0), type=int)
    p.add_argument("--dist_on_itp", action="store_true")
    p.add_argument("--dist_url", default="env://")
    p.add_argument("--transform_checkpoint_keys", action="store_true", default=False,
                   help="map the pre-training model's keys to ViT keys (applied by itself when the checkpoint holds encoder_pos_embed)")
    # ---- additive flags of the MI355X build
    p.add_argument("--synthetic_len", type=int, default=64, help="iterations per epoch of the synthetic loader (a quarter of it for evaluation)")
    p.add_argument("--input_channels", type=int, default=None, help="bands of the synthetic loader / model (3 when not given; euro_sat: 13 - len(dropped_bands))")
    p.add_argument("--print_freq", type=int, default=20, help="iterations between two drains of the device-side losses")
    p.add_argument("--embed_dim", type=int, default=None)
    p.add_argument("--depth", type=int, default=None)
    p.add_argument("--num_heads", type=int, default=None)
    return p


def load_pretrained(model, path, transform_keys=False):
    """main_finetune.py:546-618: load the trunk from a pre-training checkpoint (position table interpolated to the model's grid), then
    trunc_normal_(head.weight, std=2e-5)."""
    checkpoint = torch.load(path, map_location="cpu", weights_only=False)
    print("Load pre-trained checkpoint from: %s" % path)
    sd = checkpoint["model"]
    if transform_keys or "encoder_pos_embed" in sd:
        sd = to_vit_keys(sd)
    own = model.state_dict()
    for k in ("head.weight", "head.bias"):   # (a classifier of another width is not loaded)
        if k in sd and sd[k].shape != own[k].shape:
            print(f"Removing key {k} from pretrained checkpoint")
            del sd[k]
    interpolate_pos_embed(model, sd)
    msg = model.load_state_dict(sd, strict=False)
    print(msg)
    torch.nn.init.trunc_normal_(model.head.weight, std=2e-5)
    return msg


def main(args):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("multi-GPU fine-tuning is not implemented: run main_finetune.py as one process (the stand-alone encoder's "
                                  "backward has no data-parallel gradient hooks yet)")
    print(f"job dir: {os.path.dirname(os.path.realpath(__file__))}")
    print(f"{args}".replace(", ", ",\n"))
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    if args.drop_path > 0:
        raise NotImplementedError(f"--drop_path {args.drop_path}: drop-path is not implemented in the MI355X blocks (the reference's default is 0.1; here 0.0)")
    loader_train, loader_val, n_val = build_loaders(args, device)

    mixup_fn = None
    if args.mixup > 0 or args.cutmix > 0.0 or args.cutmix_minmax is not None:
        print("Mixup is activated!")
        mixup_fn = Mixup(mixup_alpha=args.mixup, cutmix_alpha=args.cutmix, cutmix_minmax=args.cutmix_minmax, prob=args.mixup_prob,
                         switch_prob=args.mixup_switch_prob, mode=args.mixup_mode, label_smoothing=args.smoothing, num_classes=args.nb_classes)
    else:
        print("Not using mixup")

    model = build_model(args, args.drop_path)
    if args.finetune and not args.eval:
        load_pretrained(model, args.finetune, args.transform_checkpoint_keys)
    model.finetune_mode()
    model.to(device)
    print(f"Model = {model}")

    scale_lr(args, model)

    # layer-wise lr decay (lrd) groups, stepped by one fused kernel launch each
    from csmae_hip.optim import FusedAdamW
    param_groups = lrd.param_groups_lrd(model, args.weight_decay, no_weight_decay_list=model.no_weight_decay(), layer_decay=args.layer_decay)
    optimizer = FusedAdamW(param_groups, lr=args.lr)
    loss_scaler = NativeScaler()

    # the criterion is computed by the model: soft-target cross-entropy on dense targets, label-smoothed or plain cross-entropy on labels
    if mixup_fn is not None:
        criterion, model.smoothing = "SoftTargetCrossEntropy()", 0.0     # (smoothing is handled with the mixup label transform)
    elif args.smoothing > 0.0:
        criterion, model.smoothing = f"LabelSmoothingCrossEntropy(smoothing={args.smoothing})", args.smoothing
    else:
        criterion, model.smoothing = "CrossEntropyLoss()", 0.0
    print("criterion = %s" % criterion)

    misc.load_model(args=args, model_without_ddp=model, optimizer=optimizer, loss_scaler=loss_scaler)

    model_name = "_".join([args.model, f"i{args.input_size}-p{args.patch_size}", f"e{args.epochs}-we{args.warmup_epochs}", f"b{args.batch_size}-a{args.accum_iter}",
                           f"-lr{args.lr}", f"-mixup{args.mixup}", f"-cutmix{args.cutmix}", f"-smoothing{args.smoothing}",
                           "_cls_only" if not args.global_pool else "_global_pool", "finetune"])
    make_output_dir(args, model_name)

    if args.eval:
        stats = evaluate(loader_val, model, device, args)
        acc5 = f"\n\tacc5: {stats['acc5']:.2f}%, " if "acc5" in stats else ""
        print(f"Evaluation on {n_val} test images:\n\tacc1: {stats['acc1']:.2f}%{acc5}\n\tmacro_f1: {stats['macro_f1']:.2f}%, \n\tmicro_f1: {stats['micro_f1']:.2f}%")
        return stats

    print(f"Start training for {args.epochs} epochs")
    start_time = time.time()
    max_accuracy = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        train_stats = train_one_epoch(model, criterion, loader_train, optimizer, device, epoch, loss_scaler, args.clip_grad, mixup_fn, log_writer=None, args=args)
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}, "epoch": epoch}
        if args.output_dir and ((epoch % args.save_every == 0 and epoch >= 3 * args.epochs / 2) or (epoch % 5 == 0 and epoch < 3 * args.epochs / 2)
                                or epoch + 1 == args.epochs):
            misc.save_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer, loss_scaler=loss_scaler, epoch=epoch)
        test_stats = evaluate(loader_val, model, device, args)
        print(f"Accuracy of the network on the {n_val} test images: {test_stats['acc1']:.1f}%")
        max_accuracy = max(max_accuracy, test_stats["acc1"])
        print(f"Max accuracy: {max_accuracy:.2f}%")
        log_stats.update({f"test_{k}": v for k, v in test_stats.items()})
        with open(os.path.join(args.output_dir, "log.jsonl"), mode="a", encoding="utf-8") as f:
            f.write(json.dumps(log_stats) + "\n")
    print(f"Training time {datetime.timedelta(seconds=int(time.time() - start_time))}")


if __name__ == "__main__":
    main(get_args_parser().parse_args())
