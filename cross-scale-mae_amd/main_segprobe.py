#!/usr/bin/env python3
"""Linear segmentation probe of a pre-trained encoder on the MI355X path: the dense counterpart of `main_linprobe.py`, with its flag style,
model factory call, checkpoint loading, LR scaling, LARS and per-iteration schedule.  The frozen trunk yields one feature per patch
(`VisionTransformer.forward_patch_tokens`); BatchNorm1d(affine=False) + Linear over the patch rows gives patch logits, which the loss kernel
upsamples bilinearly to the label resolution and scores against uint8 masks (`models_seg.LinearSegProbe`, csrc/segment.hip).  After every
epoch the evaluation sweep accumulates one confusion matrix on the device; `mIoU`, `pixel_acc` and the per-class IoU are printed and appended
to `<output_dir>/log.txt` as one JSON line.

Data:
  * `--dataset_type synthetic` (+ `--synthetic_len`) needs no files: fixed in-memory batches whose label is a function of the patch's colour;
  * `--dataset_type folder --train_path DIR --test_path DIR`: DIR holds `images/*.png|jpg` and `masks/*.png` with equal stems; a mask is an 8-bit
    image of class indices, 255 = ignored, of its image's size (read with PIL).  Images go through the eval transform on the device
    (`util.gpu_input.GpuAugment(train=False)`: resize + centre crop, nothing random, also while training); the masks are centre-cropped and
    nearest-resized on the host to the same geometry.  Values in [nb_classes, 255) are the dataset's to avoid: they are not detected.
Multi-GPU probing is out of scope (WORLD_SIZE > 1 raises).

    python main_segprobe.py --model vit_base_patch16 --finetune out/checkpoint-199.pth --transform_checkpoint_keys \\
        --dataset_type folder --train_path data/train --test_path data/val --nb_classes 6 --batch_size 64 --epochs 20
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
from util.downstream import PendingLosses, autocast, build_model, make_output_dir, nullable_string, scale_lr
from util.lars import LARS
from util.metrics import miou_from_confusion, pixel_accuracy_from_confusion

IGNORE = 255


def get_args_parser():
    p = argparse.ArgumentParser("Cross-MAE Linear Segmentation Probe", add_help=False)
    p.add_argument("--batch_size", default=64, type=int, help="Batch size per GPU (effective batch size is batch_size * accum_iter * # gpus")
    p.add_argument("--epochs", default=50, type=int)
    p.add_argument("--accum_iter", type=int, default=1)
    p.add_argument("--model", default="vit_base_patch16", type=str, metavar="MODEL")
    p.add_argument("--input_size", default=224, type=int)
    p.add_argument("--patch_size", default=16, type=int)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--lr", type=float, default=None, metavar="LR")
    p.add_argument("--blr", type=float, default=0.1, metavar="LR", help="base learning rate: absolute_lr = base_lr * total_batch_size / 256")
    p.add_argument("--min_lr", type=float, default=0.0, metavar="LR")
    p.add_argument("--warmup_epochs", type=int, default=0, metavar="N")
    p.add_argument("--finetune", default="", help="probe from this pre-training checkpoint")
    p.add_argument("--transform_checkpoint_keys", action="store_true", default=False,
                   help="map the pre-training model's keys to ViT keys (applied by itself when the checkpoint holds encoder_pos_embed)")
    p.add_argument("--train_path", default="./seg/train", type=str, help="folder: directory with images/ and masks/")
    p.add_argument("--test_path", default="./seg/val", type=str, help="folder: directory with images/ and masks/")
    p.add_argument("--dataset_type", type=str, default="folder", choices=["folder", "synthetic"])
    p.add_argument("--nb_classes", default=6, type=int, help="number of segmentation classes (2 .. 64)")
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--output_dir_base", type=str, default="./out")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", type=nullable_string, default=None)
    p.add_argument("--save_every", type=int, default=1)
    p.add_argument("--start_epoch", default=0, type=int, metavar="N")
    p.add_argument("--eval", action="store_true", help="Perform evaluation only")
    p.add_argument("--num_workers", type=int, default=10, help="decoding worker processes of the folder loader")
    # ---- additive flags of the MI355X build
    p.add_argument("--synthetic_len", type=int, default=64, help="iterations per epoch of the synthetic loader (a quarter of it for evaluation)")
    p.add_argument("--print_freq", type=int, default=20, help="iterations between two drains of the device-side losses")
    p.add_argument("--embed_dim", type=int, default=None)
    p.add_argument("--depth", type=int, default=None)
    p.add_argument("--num_heads", type=int, default=None)
    return p


# ---- data
class SyntheticSegLoader:
    """In-memory repeat loader: (samples [N, 3, S, S] fp32, labels [N, S, S] uint8) on `device`, the same batch every iteration.  Every patch draws a
    class, its pixels take the class's colour plus noise, and about 3 % of the pixels are marked ignored."""

    def __init__(self, batch, size, patch, classes, length, device, seed):
        g = torch.Generator(device=device).manual_seed(seed)
        G = size // patch
        cells = torch.randint(0, classes, (batch, G, G), device=device, generator=g)
        full = cells.repeat_interleave(patch, 1).repeat_interleave(patch, 2)
        colours = torch.randn(classes, 3, device=device, generator=g)
        self.samples = (colours[full].permute(0, 3, 1, 2) + 0.5 * torch.randn(batch, 3, size, size, device=device, generator=g)).contiguous()
        drop = torch.rand(batch, size, size, device=device, generator=g) < 0.03
        self.targets = torch.where(drop, torch.full_like(full, IGNORE), full).to(torch.uint8).contiguous()
        self.length = length

    def __len__(self):
        return self.length

    def __iter__(self):
        for _ in range(self.length):
            yield self.samples, self.targets


class SegFolderDataset(torch.utils.data.Dataset):
    """`root/images/<stem>.png|jpg|jpeg` paired with `root/masks/<stem>.png`.  Returns (uint8 HWC image, uint8 HW mask) as decoded; no transform
    runs here.  A missing directory or an image without its mask raises FileNotFoundError when the dataset is built."""

    def __init__(self, root):
        img_dir, mask_dir = os.path.join(root, "images"), os.path.join(root, "masks")
        for d in (img_dir, mask_dir):
            if not os.path.isdir(d):
                raise FileNotFoundError(f"{d}: a segmentation folder holds images/ and masks/")
        names = sorted(f for f in os.listdir(img_dir) if os.path.splitext(f)[1].lower() in (".png", ".jpg", ".jpeg"))
        if not names:
            raise FileNotFoundError(f"{img_dir}: no .png / .jpg images")
        self.pairs = []
        for f in names:
            mask = os.path.join(mask_dir, os.path.splitext(f)[0] + ".png")
            if not os.path.isfile(mask):
                raise FileNotFoundError(f"{mask}: no mask for image {f}")
            self.pairs.append((os.path.join(img_dir, f), mask))

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        from PIL import Image
        ip, mp = self.pairs[i]
        with Image.open(ip) as im:
            img = np.asarray(im.convert("RGB"), dtype=np.uint8)
        with Image.open(mp) as im:
            if im.mode not in ("L", "P"):
                raise ValueError(f"{mp}: a mask is an 8-bit image of class indices (mode L or P), got mode {im.mode}")
            mask = np.asarray(im, dtype=np.uint8)
        if mask.shape != img.shape[:2]:
            raise ValueError(f"{mp}: mask of {mask.shape} for an image of {img.shape[:2]}")
        return torch.from_numpy(img.copy()), torch.from_numpy(mask.copy())


def label_eval_transform(mask, S):
    """The eval transform's geometry (util.gpu_input.eval_transform_params: resize of the shorter side, centre crop to S x S) applied to a label
    map [H, W] by nearest neighbour: output pixel (oy, ox) takes the label under the centre of pixel (oy + top, ox + left) of the resized grid."""
    from util.gpu_input import eval_transform_params
    H, W = int(mask.shape[0]), int(mask.shape[1])
    _, _, Hr, Wr, top, left, _, _ = eval_transform_params(H, W, S)
    ys = np.minimum(((np.arange(S) + top + 0.5) * H / Hr).astype(np.int64), H - 1)
    xs = np.minimum(((np.arange(S) + left + 0.5) * W / Wr).astype(np.int64), W - 1)
    return torch.as_tensor(mask)[torch.from_numpy(ys)][:, torch.from_numpy(xs)].contiguous()


def _collate_pairs(samples):
    return [s[0] for s in samples], [s[1] for s in samples]


class SegFolderLoader:
    """Batches of a SegFolderDataset as (fp32 [N, 3, S, S] on the device, uint8 [N, S, S] on the device)."""

    def __init__(self, root, is_train, args, device):
        from util.gpu_input import GpuAugment
        self.dataset = SegFolderDataset(root)
        sampler = torch.utils.data.RandomSampler(self.dataset) if is_train else torch.utils.data.SequentialSampler(self.dataset)
        self.raw = torch.utils.data.DataLoader(self.dataset, sampler=sampler, batch_size=args.batch_size, num_workers=args.num_workers, drop_last=is_train,
                                               collate_fn=_collate_pairs)
        self.augment, self.S, self.device = GpuAugment(args.input_size, device=device, train=False), args.input_size, device

    def __len__(self):
        return len(self.raw)

    def __iter__(self):
        for images, masks in self.raw:
            labels = torch.stack([label_eval_transform(m, self.S) for m in masks])
            yield self.augment(images), labels.to(self.device, non_blocking=True)


def build_seg_loaders(args, device):
    """-> (train loader or None under --eval, eval loader)"""
    if args.dataset_type == "synthetic":
        mk = lambda n: SyntheticSegLoader(args.batch_size, args.input_size, args.patch_size, args.nb_classes, n, device, args.seed)
        return (None if args.eval else mk(args.synthetic_len)), mk(max(1, args.synthetic_len // 4))
    return (None if args.eval else SegFolderLoader(args.train_path, True, args, device)), SegFolderLoader(args.test_path, False, args, device)


# ---- epochs
def train_one_epoch(model, data_loader, optimizer, device, epoch, args=None):
    """main_linprobe.py's epoch for the segmentation probe: LR schedule per iteration, gradient accumulation, losses drained every `print_freq`
    iterations; LARS skips on the device every update whose loss was not finite."""
    model.train(True)
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    accum_iter, print_freq = args.accum_iter, getattr(args, "print_freq", 20)
    optimizer.zero_grad(set_to_none=False)
    n_iters = len(data_loader)
    pending = PendingLosses()
    gate = None
    for it, (samples, labels) in enumerate(metric_logger.log_every(data_loader, print_freq, f"Epoch: [{epoch}]")):
        if it % accum_iter == 0:
            lr_sched.adjust_learning_rate(optimizer, it / n_iters + epoch, args)
        with autocast(device):
            loss, _ = model(samples, labels)
        pending.append(loss, optimizer.param_groups[0]["lr"])
        gate = loss.detach().reshape(1) if it % accum_iter == 0 else gate + loss.detach().reshape(1)
        (loss / accum_iter).backward()
        if (it + 1) % accum_iter == 0:
            optimizer.step(gate=gate)
            optimizer.zero_grad(set_to_none=False)
        if it % print_freq == 0 or it == n_iters - 1:
            pending.drain(metric_logger)
    pending.drain(metric_logger)
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


@torch.no_grad()
def evaluate(data_loader, model, device, args=None):
    """-> {"loss", "mIoU", "pixel_acc", "iou"} over the loader in eval mode: one confusion matrix accumulated on the device, one host read at the end."""
    model.eval()
    K = model.num_classes
    conf = torch.zeros(K, K, device=device, dtype=torch.int64)
    sums, counts = [], []
    for samples, labels in data_loader:
        with autocast(device):
            loss, count = model.evaluate_batch(samples, labels, conf)
        sums.append(loss.double() * count[0])
        counts.append(count[0])
    total = int(torch.stack(counts).sum())
    miou, per_class = miou_from_confusion(conf)
    stats = {"loss": float(torch.stack(sums).sum()) / max(total, 1), "mIoU": 100.0 * miou, "pixel_acc": 100.0 * pixel_accuracy_from_confusion(conf),
             "iou": [None if np.isnan(v) else round(100.0 * float(v), 3) for v in per_class]}
    print("* mIoU {mIoU:.3f} pixel_acc {pixel_acc:.3f} loss {loss:.3f}".format(**stats))
    print("  per-class IoU: " + " ".join("-" if v is None else f"{v:.1f}" for v in stats["iou"]))
    return stats


def main(args):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("multi-GPU segmentation probing is not implemented: run main_segprobe.py as one process (the head is tiny; the "
                                  "frozen trunk could be sharded over ranks, which this script does not do)")
    from main_linprobe import load_pretrained
    from models_seg import LinearSegProbe
    print(f"job dir: {os.path.dirname(os.path.realpath(__file__))}")
    print(f"{args}".replace(", ", ",\n"))
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    if args.input_size % args.patch_size:
        raise ValueError(f"--input_size {args.input_size} is no multiple of --patch_size {args.patch_size}")
    loader_train, loader_val = build_seg_loaders(args, device)

    args.global_pool, args.input_channels = False, 3   # dense features take the model's `norm`; both loaders yield RGB
    vit = build_model(args)
    if args.finetune and not args.eval:
        load_pretrained(vit, args.finetune, args.transform_checkpoint_keys)
    model = LinearSegProbe(vit.to(device), args.nb_classes, ignore_index=IGNORE)
    print(f"Model = {model}")

    scale_lr(args, model)
    optimizer = LARS(model.head_parameters(), lr=args.lr, weight_decay=args.weight_decay)
    print(optimizer)
    misc.load_model(args=args, model_without_ddp=model, optimizer=optimizer, loss_scaler=None)

    model_name = "_".join([args.model, f"i{args.input_size}-p{args.patch_size}", f"e{args.epochs}-we{args.warmup_epochs}",
                           f"b{args.batch_size}-a{args.accum_iter}", f"lr{args.lr}", f"k{args.nb_classes}", "segprobe"])
    make_output_dir(args, model_name)

    if args.eval:
        return evaluate(loader_val, model, device, args)

    print(f"Start training for {args.epochs} epochs")
    start_time = time.time()
    best = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        train_stats = train_one_epoch(model, loader_train, optimizer, device, epoch, args=args)
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}, "epoch": epoch}
        if (epoch % args.save_every == 0 and epoch >= args.epochs / 2) or (epoch % 5 == 0 and epoch < args.epochs / 2) or epoch + 1 == args.epochs:
            misc.save_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer, loss_scaler=None, epoch=epoch)
        test_stats = evaluate(loader_val, model, device, args)
        best = max(best, test_stats["mIoU"])
        print(f"Max mIoU: {best:.2f}%")
        log_stats.update({f"test_{k}": v for k, v in test_stats.items()})
        with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
            f.write(json.dumps(log_stats) + "\n")
    print(f"Training time {datetime.timedelta(seconds=int(time.time() - start_time))}")


if __name__ == "__main__":
    main(get_args_parser().parse_args())
