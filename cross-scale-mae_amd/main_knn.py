#!/usr/bin/env python3
"""k-NN evaluation of a frozen pre-trained encoder on the MI355X path, across scales — the protocol the Cross-Scale MAE paper reports first:
no training, the validation images are classified by the weighted vote of their k nearest training images in feature space (DINO's
`knn_classifier`: cosine similarity, weights exp(sim / T)), and the evaluation is repeated with the validation images degraded to coarser
ground-sample distances.  It stands beside `main_linprobe.py` and takes its flags for model, checkpoint and data; model and loaders come from
`util.downstream`, the search and the vote from `csmae_hip.knn` (GEMM + `csmae_knn_select` + `csmae_knn_vote`).

  * Bank: `forward_features` of every training image under the EVAL transform at full scale (the train CSV read through the eval loader), under
    the same autocast as the probe.  `--bank_max N` keeps a seeded random subset of the training set.
  * Queries at scale s ("relative GSD" 1 / s): the validation images go through the eval transform at size round(s * input_size) — the
    `csmae_eval_u8` kernel with a smaller size; it is antialiased, so detail really is discarded — and are enlarged back to input_size by
    on-device bicubic interpolation (`torch.nn.functional.interpolate(mode="bicubic", align_corners=False)`: plumbing, not a hot path).  Scale
    1.0 skips the enlargement.  THIS DEFINITION IS THE PROJECT'S OWN: the reference repository has no code for its k-NN protocol or for the
    scale degradation, so numbers are comparable between checkpoints evaluated here, not with the paper's table.
  * `--dataset_type synthetic` has no images to transform: its device tensors are reduced with the antialiased bicubic `interpolate` instead of the
    eval kernel (a smoke path for the driver, not a measurement).
  * Output per scale: one line on stdout and one JSON line in `<output_dir>/log.txt` with the keys scale, knn_k, knn_t, bank_size, n_queries,
    top1, top5 (per cent), extract_img_per_s (feature extraction of the queries), search_s (search + vote).
  * `--dataset_type euro_sat` reads lists of 13-band uint16 tiles (`util/ms_input.py`; `--masked_bands`, `--dropped_bands`): bank and queries go
    through `csmae_eval_u16` exactly as the rgb ones go through `csmae_eval_u8`, the reduced query size per scale included.
  * Multi-process launches (WORLD_SIZE > 1) raise; the other multi-band readers raise as in `util.downstream`.

    python main_knn.py --model vit_base_patch16 --finetune out/checkpoint-199.pth --transform_checkpoint_keys --dataset_type rgb \\
        --train_path train_62classes.csv --test_path val_62classes.csv --batch_size 256 --knn_scales 1.0 0.5 0.25 0.125
"""
import argparse
import copy
import json
import os
import time

import torch

from util.downstream import (add_checkpoint_flags, add_classification_data_flags, add_model_flags, add_pooling_flags, add_run_flags, autocast, build_loaders,
                             build_model, load_pretrained, make_output_dir, resolve_input_channels, start_run)

LOG_KEYS = ("scale", "knn_k", "knn_t", "bank_size", "n_queries", "top1", "top5", "extract_img_per_s", "search_s")


def get_args_parser():
    p = argparse.ArgumentParser("Cross-MAE k-NN evaluation", add_help=False)
    add_model_flags(p)
    add_checkpoint_flags(p, "evaluate this pre-training checkpoint")
    add_pooling_flags(p)
    add_classification_data_flags(p)   # (--train_path is the bank, --test_path the queries)
    add_run_flags(p)
    p.add_argument("--batch_size", default=512, type=int, help="images per feature-extraction batch")
    # ---- the k-NN protocol
    p.add_argument("--knn_k", type=int, default=20, help="neighbours that vote (1 .. 64)")
    p.add_argument("--knn_t", type=float, default=0.07, help="temperature of the vote weights exp(sim / T)")
    p.add_argument("--knn_scales", type=float, nargs="+", default=[1.0, 0.5, 0.25, 0.125], help="relative scales of the query images")
    p.add_argument("--bank_max", type=int, default=None, help="use a seeded random subset of this many training images as the bank")
    p.add_argument("--knn_dtype", type=str, default="bf16", choices=["bf16", "fp32"], help="dtype of the normalised features the similarity GEMM reads")
    return p


def scaled_size(scale, input_size):
    """The side the query images are reduced to at `scale`."""
    if not 0.0 < scale <= 1.0:
        raise ValueError(f"--knn_scales {scale}: a scale lies in (0, 1]")
    return max(1, int(round(scale * input_size)))


def bank_subset(n_train, bank_max, seed):
    """Sorted indices of the training images that form the bank: all of them, or a seeded random subset of `bank_max`."""
    if bank_max is None or bank_max >= n_train:
        return None
    if bank_max < 1:
        raise ValueError(f"--bank_max {bank_max}: the bank needs at least one image")
    perm = torch.randperm(n_train, generator=torch.Generator().manual_seed(seed))
    return torch.sort(perm[:bank_max]).values


def eval_loader(args, device, path, size, bank_max=None):
    """-> (loader, its number of images): `path` under the eval transform at `size`, through util.downstream.build_loaders (which gives the eval
    loader of `test_path`).  `bank_max`: keep a seeded random subset of the images (rgb, euro_sat)."""
    a = copy.copy(args)
    a.eval, a.test_path, a.input_size = True, path, size
    _, loader, n = build_loaders(a, device)
    subset = bank_subset(n, bank_max, args.seed)
    if subset is not None:
        from util.gpu_input import PrefetchLoader, collate_uint8
        from util.ms_input import collate_uint16
        ds = torch.utils.data.Subset(loader.dataset, subset.tolist())
        raw = torch.utils.data.DataLoader(ds, sampler=torch.utils.data.SequentialSampler(ds), batch_size=args.batch_size, num_workers=args.num_workers,
                                          pin_memory=False, drop_last=False, collate_fn=collate_uint16 if args.dataset_type == "euro_sat" else collate_uint8)
        loader = PrefetchLoader(raw, loader.augment)
    return loader, n


@torch.no_grad()
def extract(model, loader, device, size_in=None, keep=None):
    """-> (features [n, D] fp32, labels [n] int64 on the device, images per second).  `size_in`: the batches arrive (rgb) or are reduced here
    (device tensors of the synthetic loader) at this side and are enlarged to the model's input size by bicubic interpolation.  `keep`: sorted
    indices into the loader's image sequence to keep."""
    import torch.nn.functional as F
    S = model.img_size
    feats, labels, seen = [], [], 0
    torch.cuda.synchronize(device)
    t0 = time.time()
    for samples, targets in loader:
        samples, targets = samples.to(device, non_blocking=True), targets.to(device, non_blocking=True)
        n = samples.shape[0]
        if keep is not None:
            sel = keep[(keep >= seen) & (keep < seen + n)] - seen
            seen += n
            if sel.numel() == 0:
                continue
            samples, targets = samples[sel.to(device)], targets[sel.to(device)]
        if size_in is not None and size_in != S:
            if samples.shape[-1] != size_in:
                samples = F.interpolate(samples.float(), size=(size_in, size_in), mode="bicubic", align_corners=False, antialias=True)
            samples = F.interpolate(samples.float(), size=(S, S), mode="bicubic", align_corners=False)
        with autocast(device):
            feats.append(model.forward_features(samples))
        labels.append(targets.to(torch.int64))
    torch.cuda.synchronize(device)
    feats, labels = torch.cat(feats), torch.cat(labels)
    return feats, labels, feats.shape[0] / max(time.time() - t0, 1e-9)


def main(args):
    sizes = []

    def validate():
        if not 1 <= args.knn_k <= 64:
            raise ValueError(f"--knn_k {args.knn_k}: the select kernel keeps 1 .. 64 neighbours")
        sizes.extend(scaled_size(s, args.input_size) for s in args.knn_scales)
    device = start_run(args, "main_knn.py", "k-NN evaluation",
                       "the bank and the search live on one device; sharding the bank over ranks is not done by this script", validate)
    args.eval = False
    resolve_input_channels(args)
    synthetic = args.dataset_type == "synthetic"
    keep = None
    if synthetic:
        loader_bank, loader_val, n_val = build_loaders(args, device)
        n_train = len(loader_bank) * args.batch_size
        keep = bank_subset(n_train, args.bank_max, args.seed)
    elif args.dataset_type in ("rgb", "euro_sat"):
        loader_bank, n_train = eval_loader(args, device, args.train_path, args.input_size, args.bank_max)
    else:
        build_loaders(args, device)   # raises: the multi-band readers are not wired
        raise NotImplementedError(f"--dataset_type {args.dataset_type}")

    from csmae_hip.knn import KnnIndex
    model = build_model(args)
    if args.finetune:
        load_pretrained(model, args.finetune, args.transform_checkpoint_keys)
    model.to(device).eval()
    make_output_dir(args, "_".join([args.model, f"i{args.input_size}-p{args.patch_size}", f"k{args.knn_k}-t{args.knn_t}",
                                    "_global_pool" if args.global_pool else "_cls_only", "knn"]))

    feats, labels, rate = extract(model, loader_bank, device, keep=keep)
    print(f"bank: {feats.shape[0]} of {n_train} training images, D = {feats.shape[1]}, {rate:.1f} img/s")
    index = KnnIndex(feats, labels, args.nb_classes, dtype=torch.bfloat16 if args.knn_dtype == "bf16" else torch.float32)
    del feats

    results = []
    for scale, size in zip(args.knn_scales, sizes):
        if synthetic:
            loader_q = loader_val
        else:
            loader_q, n_val = eval_loader(args, device, args.test_path, size)
        q, qlabels, rate = extract(model, loader_q, device, size_in=size)
        index.counts.zero_()
        torch.cuda.synchronize(device)
        t0 = time.time()
        index.classify(q, k=args.knn_k, T=args.knn_t, labels=qlabels)
        top1, top5 = index.counts.tolist()   # (the host read ends the timed window)
        search_s = time.time() - t0
        n = q.shape[0]
        stats = dict(scale=scale, knn_k=args.knn_k, knn_t=args.knn_t, bank_size=index.N, n_queries=n, top1=100.0 * top1 / n, top5=100.0 * top5 / n,
                     extract_img_per_s=rate, search_s=search_s)
        print("* scale {scale:g}  k {knn_k}  T {knn_t:g}  bank {bank_size}  Acc@1 {top1:.3f}  Acc@5 {top5:.3f}  "
              "extract {extract_img_per_s:.1f} img/s  search {search_s:.3f} s".format(**stats))
        with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
            f.write(json.dumps(stats) + "\n")
        results.append(stats)
    return results


if __name__ == "__main__":
    main(get_args_parser().parse_args())
