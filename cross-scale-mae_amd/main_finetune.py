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
import os

import torch

import util.lr_decay as lrd
import util.misc as misc
from engine_finetune import evaluate, train_one_epoch
from util.downstream import (add_checkpoint_flags, add_classification_data_flags, add_model_flags, add_pooling_flags, add_run_flags, add_schedule_flags,
                             build_loaders, build_model, fit, make_output_dir, nullable_string, read_pretrained, save_due, scale_lr, start_run)
from util.misc import NativeScalerWithGradNormCount as NativeScaler
from util.mixup import Mixup
from util.pos_embed import interpolate_pos_embed


def get_args_parser():
    p = argparse.ArgumentParser("Cross-MAE fine-tuning", add_help=False)
    add_schedule_flags(p, epochs=100, weight_decay=0.05, blr=1e-3, min_lr=1e-6, warmup_epochs=5)
    add_model_flags(p, input_size=128)
    add_checkpoint_flags(p, "finetune from checkpoint")
    add_pooling_flags(p, global_pool=True)
    add_classification_data_flags(p)
    add_run_flags(p)
    p.add_argument("--model_type", type=nullable_string, default=None, choices=["vanilla", None])
    p.add_argument("--drop_path", type=float, default=0.0, metavar="PCT", help="Drop path rate: not implemented here, a value above 0 raises (reference default 0.1)")
    p.add_argument("--clip_grad", type=float, default=None, metavar="NORM")
    p.add_argument("--layer_decay", type=float, default=0.75, help="layer-wise lr decay from ELECTRA/BEiT")
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
    # logging / distributed flags of the reference (parsed for compatibility)
    p.add_argument("--use_psa", action="store_true")
    p.add_argument("--val_img_path", type=str, default="./images/")
    p.add_argument("--log_dir", default="./output_dir")
    p.add_argument("--wandb_entity", type=str, default="utk-iccv23")
    p.add_argument("--wandb_project", type=nullable_string, default=None)
    p.add_argument("--wandb_id", type=nullable_string, default=None)
    p.add_argument("--dist_eval", action="store_true", default=False)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--local_rank", default=os.getenv("LOCAL_RANK", 0), type=int)
    p.add_argument("--dist_on_itp", action="store_true")
    p.add_argument("--dist_url", default="env://")
    return p


def load_pretrained(model, path, transform_keys=False):
    """The fine-tuning policy (main_finetune.py:546-618): load the trunk from a pre-training checkpoint (position table interpolated to the model's
    grid), then trunc_normal_(head.weight, std=2e-5)."""
    sd = read_pretrained(path, transform_keys)
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
    device = start_run(args, "main_finetune.py", "fine-tuning", "the stand-alone encoder's backward has no data-parallel gradient hooks yet")
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

    fit(args, model, optimizer, loss_scaler, log_name="log.jsonl", best=("acc1", "Max accuracy"),
        train=lambda epoch: train_one_epoch(model, criterion, loader_train, optimizer, device, epoch, loss_scaler, args.clip_grad, mixup_fn, log_writer=None, args=args),
        evaluate=lambda: evaluate(loader_val, model, device, args),
        save_at=lambda epoch: args.output_dir and save_due(args, epoch, 3 * args.epochs / 2),
        report=lambda stats: f"Accuracy of the network on the {n_val} test images: {stats['acc1']:.1f}%")


if __name__ == "__main__":
    main(get_args_parser().parse_args())
