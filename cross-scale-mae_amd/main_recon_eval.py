#!/usr/bin/env python3
"""Batched reconstruction evaluation of pre-training checkpoints on the MI355X path: "how well does checkpoint A reconstruct compared with B,
clean and at noise 0.25".  Every image of a folder goes through every checkpoint `--num_runs_each` times with seeded masks (and, with
`--random_crop`, seeded crops); each run is scored per image with mse | mae | l1 | l2 | ssim by `util.viz.run_eval` — one forward and one
`csmae_recon_eval` per batch, no host sync inside the sweep.

  * `--chkpt_dirs A B ...` under `--chkpt_basedir` are loaded through `util.viz.prepare_model` (the latest `checkpoint-<epoch>.pth` of each).
  * `--data_dir`: every `**/*.jpg` below it.  `--dataset_type synthetic --synthetic_len N` scores N seeded smooth images instead and needs no files
    (a smoke path for the driver, not a measurement).
  * `--noise TYPE PARAM` (gaussian | poisson | s&p) is added to the normalised input on the device, seeded per (image, run): this seeding is this
    build's own, the reference draws its evaluation noise unseeded.
  * Output: `<output_dir>/log.txt` gets one JSON line per model — model, n_images, num_runs_each, noise, random_crop and `<metric>_mean` /
    `<metric>_std` over the images; `<output_dir>/per_image.csv` one row per (model, image) with the metrics as columns.
  * `--panel_dir DIR` also writes reconstruction contact sheets, `DIR/img_<i>.png` for every image (`--panel_every N`: every N-th): one row per
    checkpoint, each row the `--panels` (default x xm y: original | masked input | reconstruction) of run 0, from the forward that is scored
    (`csmae_recon_panel`); `log.txt` then gets one more line naming the directory and the count of sheets.
  * Multi-process launches (WORLD_SIZE > 1) raise.

    python main_recon_eval.py --chkpt_basedir ../Model_Saving --chkpt_dirs run_a run_b --data_dir /data/fmow-rgb/val --noise gaussian 0.25
"""
import argparse
import csv
import json
import os
from pathlib import Path

import numpy as np
import torch

METRIC_CHOICES = ("mse", "mae", "l1", "l2", "ssim", "ssd", "sad")
PANEL_CHOICES = ("x", "xm", "y", "ym", "xm_ym")   # util.viz.PANEL_CODES


def get_args_parser():
    p = argparse.ArgumentParser("Cross-MAE reconstruction evaluation", add_help=False)
    p.add_argument("--chkpt_basedir", default="../Model_Saving", type=str, help="folder that holds the checkpoint folders")
    p.add_argument("--chkpt_dirs", type=str, nargs="+", required=True, help="checkpoint folders under --chkpt_basedir, one per model to compare")
    p.add_argument("--data_dir", default=None, type=str, help="folder whose **/*.jpg are evaluated")
    p.add_argument("--dataset_type", type=str, default="folder", choices=["folder", "synthetic"])
    p.add_argument("--synthetic_len", type=int, default=64, help="images of the synthetic set")
    p.add_argument("--metrics", type=str, nargs="+", default=None, choices=METRIC_CHOICES, help="default: mse mae l1 l2 ssim")
    p.add_argument("--num_runs_each", type=int, default=5, help="seeded masks (and crops) per image")
    p.add_argument("--noise", nargs=2, default=None, metavar=("TYPE", "PARAM"), help="gaussian | poisson | s&p and its parameter")
    p.add_argument("--random_crop", action="store_true", default=False)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--max_samples", type=int, default=None, help="evaluate at most this many images")
    p.add_argument("--num_workers", type=int, default=4, help="decoding worker processes")
    p.add_argument("--output_dir", type=str, default="./out_recon_eval")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--panel_dir", type=str, default=None, help="write reconstruction contact sheets (one PNG per image, one row per checkpoint) here")
    p.add_argument("--panel_every", type=int, default=None, help="a sheet for every N-th image (default: every image)")
    p.add_argument("--panels", type=str, nargs="+", default=["x", "xm", "y"], choices=PANEL_CHOICES,
                   help="panels of a row: original, masked input, reconstruction, reconstruction on the masked patches, pasted")
    return p


def parse_noise(noise):
    """--noise TYPE PARAM -> ("type", float) or None."""
    if noise is None:
        return None
    kind, param = noise
    if kind not in ("gaussian", "poisson", "s&p"):
        raise ValueError(f"--noise {kind}: gaussian, poisson or s&p")
    return kind, float(param)


def summarize(mtrs, model_name):
    """{metric_mean, metric_std} of one model over the images (population standard deviation, as numpy's default)."""
    out = {}
    for metric, per_model in mtrs.items():
        v = np.asarray(per_model[model_name], dtype=np.float64)
        out[f"{metric}_mean"] = float(v.mean()) if v.size else float("nan")
        out[f"{metric}_std"] = float(v.std()) if v.size else float("nan")
    return out


def main(args):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("multi-GPU reconstruction evaluation is not implemented: run main_recon_eval.py as one process")
    use_noise = parse_noise(args.noise)
    if args.dataset_type == "folder" and not args.data_dir:
        raise ValueError("--data_dir is needed unless --dataset_type synthetic")
    from util import viz
    device = torch.device(args.device)
    models = {}
    for d in args.chkpt_dirs:
        model = viz.prepare_model(d, chkpt_basedir=args.chkpt_basedir)
        if model is None:
            raise ValueError(f"{d}: this build refuses the checkpoint's architecture options")
        models[d] = model.to(device)
        models[d].device = str(device)
    images = None
    if args.dataset_type == "synthetic":
        channels = next(iter(models.values())).input_channels

        def images(size):
            return viz.SyntheticEvalImages(args.synthetic_len, size, args.num_runs_each, channels=channels)
    panel_dir = getattr(args, "panel_dir", None)
    panel_kw = {} if panel_dir is None else dict(panel_dir=panel_dir, panel_every=getattr(args, "panel_every", None), panels=tuple(getattr(args, "panels", ("x", "xm", "y"))))
    mtrs = viz.run_eval(models, args.data_dir, comp_metrics=args.metrics, use_noise=use_noise, num_runs_each=args.num_runs_each, batch_size=args.batch_size,
                        random_crop=args.random_crop, max_samples=args.max_samples, num_workers=args.num_workers, images=images, **panel_kw)
    Path(args.output_dir).mkdir(parents=True, exist_ok=True)
    names = list(mtrs)
    results = []
    with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
        for model_name in models:
            n = len(mtrs[names[0]][model_name])
            stats = dict(model=model_name, n_images=n, num_runs_each=args.num_runs_each, noise=list(use_noise) if use_noise else None,
                         random_crop=bool(args.random_crop), **summarize(mtrs, model_name))
            print("* " + "  ".join(f"{k} {v:.6g}" if isinstance(v, float) else f"{k} {v}" for k, v in stats.items()))
            f.write(json.dumps(stats) + "\n")
            results.append(stats)
        if panel_dir is not None:
            every = max(int(panel_kw["panel_every"] or 1), 1)
            n_images = len(mtrs[names[0]][next(iter(models))])
            sheets = len(range(0, n_images, every)) * len({m.input_size for m in models.values()})
            f.write(json.dumps(dict(panel_dir=panel_dir, panel_every=every, panels=list(panel_kw["panels"]), sheets=sheets)) + "\n")
    with open(os.path.join(args.output_dir, "per_image.csv"), mode="w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["model", "image"] + names)
        for model_name in models:
            for i in range(len(mtrs[names[0]][model_name])):
                w.writerow([model_name, i] + [repr(mtrs[m][model_name][i]) for m in names])
    return results


if __name__ == "__main__":
    main(get_args_parser().parse_args())
