#!/usr/bin/env python3
"""Linear segmentation probe of a pre-trained encoder on the MI355X path: the dense counterpart of `main_linprobe.py`, with its flag style,
model factory call, checkpoint loading, LR scaling, LARS and per-iteration schedule.  The frozen trunk yields one feature per patch
(`VisionTransformer.forward_patch_tokens`); BatchNorm1d(affine=False) + Linear over the patch rows gives patch logits, which the loss kernel
upsamples bilinearly to the label resolution and scores against uint8 masks (`models_seg.LinearSegProbe`, csrc/segment.hip).  After every
epoch the evaluation sweep accumulates one confusion matrix on the device; `mIoU`, `pixel_acc` and the per-class IoU are printed and appended
to `<output_dir>/log.txt` as one JSON line.

Looking at the predictions (all off by default; any of them makes the evaluation sweep call `csmae_segpanel` once per batch, on the patch logits it has
just scored — util/seg_viz.py, csrc/seg_panel.hip; the printed lines and the returned numbers do not change, a later evaluation overwrites an earlier one):
  * `--panel_dir DIR` writes an overlay sheet `DIR/<name>.png` per image (`--panel_every N`: every N-th): the `--panes` side by side (default
    image gt_over pred_over; also gt, pred, errors), overlays blended with `--panel_alpha`;
  * `--pred_dir DIR` writes the argmax map `DIR/<name>.png` per image, a palette PNG whose pixel values are the class indices;
  * `--per_image` writes `<output_dir>/per_image.csv`: index, name, valid, pixel_acc, mIoU, iou_0 .. iou_{K-1} per image (an absent class: nan).
  `<name>` is the image file's stem for `folder` and `img_<i:06d>` for `synthetic`.

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
import os

import numpy as np
import torch

import util.misc as misc
from util.downstream import (add_checkpoint_flags, add_model_flags, add_run_flags, add_schedule_flags, autocast, build_model, fit, lars_update,
                             load_pretrained, make_output_dir, save_due, scale_lr, start_run, train_epoch)
from util.lars import LARS
from util.metrics import miou_from_confusion, pixel_accuracy_from_confusion

IGNORE = 255
PANE_CHOICES = ("image", "gt", "pred", "gt_over", "pred_over", "errors")   # util.seg_viz.PANE_CODES
DEFAULT_PANES = ("image", "gt_over", "pred_over")


def get_args_parser():
    p = argparse.ArgumentParser("Cross-MAE Linear Segmentation Probe", add_help=False)
    add_schedule_flags(p, batch_size=64, warmup_epochs=0)
    add_model_flags(p)
    add_checkpoint_flags(p)
    add_run_flags(p)
    p.add_argument("--train_path", default="./seg/train", type=str, help="folder: directory with images/ and masks/")
    p.add_argument("--test_path", default="./seg/val", type=str, help="folder: directory with images/ and masks/")
    p.add_argument("--dataset_type", type=str, default="folder", choices=["folder", "synthetic"])
    p.add_argument("--nb_classes", default=6, type=int, help="number of segmentation classes (2 .. 64)")
    # the outputs of the evaluation sweep: absent from the namespace unless given (argparse.SUPPRESS), so a run without them parses, prints and does what it did
    off = argparse.SUPPRESS
    p.add_argument("--panel_dir", type=str, default=off, help="write an overlay sheet per evaluated image (one PNG, the --panes side by side) here")
    p.add_argument("--panel_every", type=int, default=off, help="a sheet for every N-th image (default: every image)")
    p.add_argument("--panes", type=str, nargs="+", default=off, choices=PANE_CHOICES,
                   help="panes of a sheet: the image, the labels / the prediction as flat colours, each over the image, the wrong pixels in red "
                        "(default: image gt_over pred_over)")
    p.add_argument("--panel_alpha", type=float, default=off, help="weight of the colour in the overlay panes, 0 .. 1 (default 0.5)")
    p.add_argument("--pred_dir", type=str, default=off, help="write the predicted class map of every evaluated image (a palette PNG of class indices) here")
    p.add_argument("--per_image", action="store_true", default=off,
                   help="write <output_dir>/per_image.csv: valid pixels, pixel accuracy, mIoU and per-class IoU of every image")
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

    def image_name(self, i):
        return f"img_{i:06d}"


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

    def image_name(self, i):
        """The stem of the i-th image the loader yields (the eval loader is sequential: dataset order)."""
        return os.path.splitext(os.path.basename(self.dataset.pairs[i][0]))[0]

    def display_stats(self):
        """(mean, std) that turn a normalised sample back into [0, 1] values: the transform's own"""
        return self.augment.mean, 1.0 / self.augment.inv_std

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
    return train_epoch(model, data_loader, optimizer, device, epoch, args, lars_update(optimizer, args.accum_iter))


def wants_outputs(args):
    """True when a flag asks the evaluation sweep for more than its numbers (--panel_dir, --pred_dir, --per_image)."""
    return args is not None and bool(getattr(args, "panel_dir", None) or getattr(args, "pred_dir", None) or getattr(args, "per_image", False))


class SegOutputs:
    """The files of one evaluation sweep.  `batch` enqueues one csmae_segpanel on the patch logits the batch was scored with and reads back only
    what is written: the picked images' sheets, the class maps when --pred_dir is set; the counts stay on the device until `finish`."""

    def __init__(self, args, data_loader, K, device):
        from util.seg_viz import IGNORE_RGB, default_palette, device_palette, pane_codes
        self.panel_dir, self.pred_dir, self.per_image = getattr(args, "panel_dir", None), getattr(args, "pred_dir", None), bool(getattr(args, "per_image", False))
        self.every = max(int(getattr(args, "panel_every", None) or 1), 1)
        self.alpha = float(getattr(args, "panel_alpha", 0.5))
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError(f"--panel_alpha {self.alpha}: a weight in [0, 1]")
        # without sheets the kernel still writes one: the cheapest, a single flat pane
        self.codes, self.gap = (pane_codes(getattr(args, "panes", DEFAULT_PANES)), 2) if self.panel_dir else ([2], 0)
        self.K, self.device, self.loader, self.ignore_rgb = K, device, data_loader, IGNORE_RGB
        self.palette_host = default_palette(K)
        self.palette = device_palette(self.palette_host, K, device)
        self.mean, self.std = data_loader.display_stats() if hasattr(data_loader, "display_stats") else (None, None)
        if self.per_image and not getattr(args, "output_dir", None):
            raise ValueError("--per_image writes <output_dir>/per_image.csv: no output_dir is set")
        self.csv = os.path.join(args.output_dir, "per_image.csv") if self.per_image else None
        for d in (self.panel_dir, self.pred_dir, args.output_dir if self.csv else None):
            if d:
                os.makedirs(d, exist_ok=True)
        self.index, self.names, self.stats = 0, [], []

    def batch(self, model, samples, labels, pl):
        from util.seg_viz import segmentation_panels, write_mask_png
        from util.viz import write_sheet
        n, S = samples.shape[0], samples.shape[-1]
        pred = torch.empty(n, S, S, device=samples.device, dtype=torch.uint8) if self.pred_dir else None
        stats = torch.empty(n, self.K, 3, device=samples.device, dtype=torch.int32) if self.per_image else None
        sheets = segmentation_panels(model, samples, labels, panes=self.codes, alpha=self.alpha, palette=self.palette, mean=self.mean, std=self.std,
                                     patch_logits=pl, gap=self.gap, ignore_rgb=self.ignore_rgb, pred=pred, stats=stats)
        names = [self.loader.image_name(self.index + j) if hasattr(self.loader, "image_name") else f"img_{self.index + j:06d}" for j in range(n)]
        if self.panel_dir:
            picked = [j for j in range(n) if (self.index + j) % self.every == 0]
            if picked:
                host = sheets[picked].cpu().numpy()
                for t, j in enumerate(picked):
                    write_sheet(os.path.join(self.panel_dir, names[j] + ".png"), host[t])
        if pred is not None:
            host = pred.cpu().numpy()
            for j in range(n):
                write_mask_png(os.path.join(self.pred_dir, names[j] + ".png"), host[j], self.palette_host)
        if stats is not None:
            self.stats.append(stats)
        self.names += names
        self.index += n

    def finish(self):
        if self.csv is None:
            return
        import csv

        from util.metrics import per_image_scores
        sc = per_image_scores(torch.cat(self.stats)) if self.stats else None
        with open(self.csv, mode="w", encoding="utf-8", newline="") as f:
            w = csv.writer(f)
            w.writerow(["index", "name", "valid", "pixel_acc", "mIoU"] + [f"iou_{k}" for k in range(self.K)])
            for i, name in enumerate(self.names):
                w.writerow([i, name, int(sc["valid"][i]), repr(float(sc["pixel_acc"][i])), repr(float(sc["mIoU"][i]))] + [repr(float(v)) for v in sc["iou"][i]])


@torch.no_grad()
def evaluate(data_loader, model, device, args=None):
    """-> {"loss", "mIoU", "pixel_acc", "iou"} over the loader in eval mode: one confusion matrix accumulated on the device, one host read at the end.
    With --panel_dir, --pred_dir or --per_image (SegOutputs) every batch's logits also go through csmae_segpanel; the numbers are the same."""
    model.eval()
    K = model.num_classes
    conf = torch.zeros(K, K, device=device, dtype=torch.int64)
    outputs = SegOutputs(args, data_loader, K, device) if wants_outputs(args) else None
    sums, counts = [], []
    for samples, labels in data_loader:
        with autocast(device):
            if outputs is None:
                loss, count = model.evaluate_batch(samples, labels, conf)
            else:
                loss, count, pl = model.evaluate_batch(samples, labels, conf, want_logits=True)
                outputs.batch(model, samples, labels, pl)
        sums.append(loss.double() * count[0])
        counts.append(count[0])
    if outputs is not None:
        outputs.finish()
    total = int(torch.stack(counts).sum())
    miou, per_class = miou_from_confusion(conf)
    stats = {"loss": float(torch.stack(sums).sum()) / max(total, 1), "mIoU": 100.0 * miou, "pixel_acc": 100.0 * pixel_accuracy_from_confusion(conf),
             "iou": [None if np.isnan(v) else round(100.0 * float(v), 3) for v in per_class]}
    print("* mIoU {mIoU:.3f} pixel_acc {pixel_acc:.3f} loss {loss:.3f}".format(**stats))
    print("  per-class IoU: " + " ".join("-" if v is None else f"{v:.1f}" for v in stats["iou"]))
    return stats


def main(args):
    device = start_run(args, "main_segprobe.py", "segmentation probing",
                       "the head is tiny; the frozen trunk could be sharded over ranks, which this script does not do")
    from models_seg import LinearSegProbe
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

    fit(args, model, optimizer, None, log_name="log.txt", best=("mIoU", "Max mIoU"),
        train=lambda epoch: train_one_epoch(model, loader_train, optimizer, device, epoch, args=args),
        evaluate=lambda: evaluate(loader_val, model, device, args), save_at=lambda epoch: save_due(args, epoch, args.epochs / 2))


if __name__ == "__main__":
    main(get_args_parser().parse_args())
