"""Reconstruction helpers around the pre-training path (reference util/viz.py:27-206): checkpoint -> model, image file -> normalised
array, one masked forward of a single image -> (original, masked input, reconstruction, reconstruction of the masked patches,
reconstruction pasted into the visible patches).

The model forward is the HIP path (`model(x, mask_ratio=, mask_seed=)`); everything else here is host-side array handling.

The picture of the reference's `plot_reconstruction` (util/viz.py:231-316) — Original | Input (Masked) | Reconstruction, one row per model — is
built without matplotlib, as a contact sheet whose bytes `csmae_recon_panel` writes on the device, for a whole batch, from the operands of the
forward: `reconstruction_panels` here, the row stacking and the PNG writer (`stack_sheets`, `write_sheet`) too.  The function itself,
`plot_reconstruction` with the reference's arguments, its path rule and its captions, is `util.recon_plot.plot_reconstruction`: this module keeps
no `plot_reconstruction` and no `plot_image` (tests/test_host_cpu.py holds it to that).  `plot_image` and `plot_metrics_comp`
(util/viz.py:208-229,501-624) are matplotlib UI — SURVEY §2 row 19, out of scope — and are still not rebuilt.

`run_eval` (reference util/viz.py:319-498) is rebuilt as the batched GPU sweep its TODO asks for: every image of a
folder, `num_runs_each` seeded masks (and crops) each, through several models -> `mtrs[metric][model_name]` = one score per image.  A batch
costs one forward and one `csmae_recon_eval` (util.metrics.batch_metrics); nothing is read back before the sweep ends.  What differs from
the reference, on purpose:
  * images run in batches: the mask of image i, run r is still the one `run_one_image(img, model, mask_seed=seed_str_to_int(f"{i}-{r}"))`
    draws (the batch's masking noise is built row by row from that seed), but a GEMM may round differently at another batch size;
  * the evaluation noise (`use_noise`) is drawn ON THE DEVICE from a generator seeded with the same per-(image, run) seed — the reference
    draws it unseeded on the host, so its noisy scores are not repeatable; this seeding is this build's own;
  * the multi-scale variants draw ONE crop box per batch (it only enters the training loss, never the prediction that is scored);
  * the compared original is the fp32 input the model saw, un-normalised (the reference keeps a float64 copy);
  * the reference's plot arguments are accepted and ignored; sheets are asked for with `panel_dir` / `panel_every` / `panels` instead, and come from
    the forward that is scored (same seeds, same noise)."""
import os
import re
from typing import Optional

import numpy as np
import torch

import models_mae
from util import metrics
from util.gpu_input import resized_crop_box
from util.misc import glob_helper, seed_str_to_int

# per-channel statistics the reference hard-codes for its plots (util/viz.py:23-24)
image_mean = np.array([0.40558367, 0.43378946, 0.43175863])
image_std = np.array([0.19208308, 0.19136319, 0.19783947])


def title_to_fname(title: str) -> str:
    """File-name form of a plot title (reference util/misc.py:428-436)."""
    s = re.sub(r"\s+", "_", re.sub(r"[^\w\s]", "_", title.replace("-", "")))
    while "__" in s:
        s = s.replace("__", "_")
    return s.strip("_")


def prepare_model(chkpt_dir, chkpt_basedir="../Model_Saving", chkpt_name=None, map_location="cpu"):
    """`<chkpt_basedir>/<chkpt_dir>/checkpoint-<epoch>.pth` (latest epoch when `chkpt_name` is None) -> the model its `args` describe,
    weights loaded (strict=False), moved to `model.device` when that is set (util/viz.py:27-89)."""
    folder = os.path.join(chkpt_basedir, chkpt_dir)
    if chkpt_name is None:
        names = [f for f in os.listdir(folder) if f.endswith(".pth")]
        if not names:
            raise IndexError(f"no checkpoint-*.pth under {folder}")
        chkpt_name = max(names, key=lambda f: int(f.split("-")[1].split(".")[0]))
    chkpt_name = str(chkpt_name)
    if not chkpt_name.endswith(".pth"):
        chkpt_name += ".pth"
    if not chkpt_name.startswith("checkpoint-"):
        chkpt_name = "checkpoint-" + chkpt_name
    path = os.path.join(folder, chkpt_name)
    print("Loading checkpoint: ", path)
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    args = dict(vars(ckpt["args"]))
    try:
        model = getattr(models_mae, args["model"])(**args)
    except AssertionError as e:  # an architecture option this build (like the reference) refuses
        print("Error: ", e)
        return None
    print(model.load_state_dict(ckpt["model"], strict=False))
    if model.device is not None:
        model = model.to(model.device)
    return model


def prepare_image(image_uri, img_size, random_crop=False, crop_seed=None, resample=None, **kwargs):
    """Image file -> [img_size, img_size, C] float64, scaled to [0, 1] and normalised with the plot statistics (util/viz.py:92-120).
    `random_crop`: torchvision's RandomResizedCrop(scale 0.25-1, bicubic) of the PIL image first, seeded by `crop_seed`."""
    from PIL import Image
    img = Image.open(image_uri)
    if random_crop:
        if crop_seed is not None:
            torch.manual_seed(crop_seed)
        i, j, h, w = resized_crop_box(img.height, img.width, scale=(0.25, 1.0))
        img = img.resize((img_size, img_size), Image.BICUBIC, box=(j, i, j + w, i + h))
    img = img.resize((img_size, img_size), resample=resample)
    return (np.array(img) / 255.0 - image_mean) / image_std


@torch.no_grad()
def run_one_image(img, model, mask_seed: Optional[int] = None, **kwargs):
    """One [H, W, C] normalised image through `model(x, mask_ratio=model.mask_ratio, mask_seed=)` -> five [1, H, W, C] CPU tensors in
    un-normalised image space: x, x with the masked patches blanked, y (reconstruction), y on the masked patches only, and x on the
    visible patches + y on the masked ones (util/viz.py:141-206)."""
    p, c = model.patch_size, model.input_channels
    x = torch.as_tensor(img).unsqueeze(0).permute(0, 3, 1, 2)
    mask_ratio = getattr(model, "mask_ratio", 0.75)
    xf = x.float()
    xf = xf.to(model.device if model.device is not None else next(model.parameters()).device)
    _, y, mask = model(xf, mask_ratio=mask_ratio, mask_seed=mask_seed)
    y = model.unpatchify(y, p=p, c=c).permute(0, 2, 3, 1).detach().cpu()
    mask = mask.detach().unsqueeze(-1).repeat(1, 1, model.patch_embed.patch_size[0] ** 2 * 3)   # 3 channels, as the reference (:186-188)
    mask = model.unpatchify(mask, p=p, c=c).permute(0, 2, 3, 1).cpu()                              # 1 = removed, 0 = kept
    x = x.permute(0, 2, 3, 1)
    std, mean = torch.as_tensor(image_std), torch.as_tensor(image_mean)
    x = x * std + mean
    y = y * std + mean
    xm = x * (1 - mask)
    ym = y * mask
    return x, xm, y, ym, xm + ym


def add_noise(image, noise_type="gaussian", noise_param=0.1, generator=None):
    """image + noise on the image's device (reference util/viz.py:123-137): gaussian = N(0, noise_param^2), poisson = Poisson(noise_param)
    counts, s&p = Bernoulli(noise_param) ones.  `generator` (a torch.Generator of the image's device) makes the draw repeatable."""
    if not isinstance(image, torch.Tensor):
        image = torch.as_tensor(image)
    if noise_type == "gaussian":
        noise = torch.randn(image.shape, generator=generator, device=image.device, dtype=image.dtype) * noise_param
    elif noise_type == "poisson":
        noise = torch.poisson(torch.ones_like(image) * noise_param, generator=generator)
    elif noise_type == "s&p":
        noise = torch.bernoulli(torch.ones_like(image) * noise_param, generator=generator)
    else:
        raise ValueError(f"Invalid noise type {noise_type!r}: gaussian, poisson or s&p")
    return image + noise


def eval_seed(img_i, run_i):
    """Crop seed and mask seed of run `run_i` of image `img_i` (reference util/viz.py:379,389)."""
    return seed_str_to_int(f"{img_i}-{run_i}")


class EvalImages(torch.utils.data.Dataset):
    """The sweep of run_eval as a dataset: item k = run k % num_runs_each of image k // num_runs_each -> (normalised fp32 [C, S, S], its seed)."""

    def __init__(self, paths, img_size, num_runs_each, random_crop=False, resample=None):
        self.paths, self.img_size, self.runs, self.random_crop, self.resample = list(paths), img_size, num_runs_each, random_crop, resample

    def __len__(self):
        return len(self.paths) * self.runs

    def __getitem__(self, k):
        i, r = divmod(k, self.runs)
        seed = eval_seed(i, r)
        img = prepare_image(self.paths[i], self.img_size, random_crop=self.random_crop, crop_seed=seed, resample=self.resample)
        return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).float(), seed


class SyntheticEvalImages(torch.utils.data.Dataset):
    """`n` seeded smooth images instead of files (the driver's --dataset_type synthetic): a coarse random grid per channel, enlarged bicubically,
    clamped to [0, 1] and normalised like prepare_image's output.  Every run of an image sees the same picture (there is nothing to crop)."""

    def __init__(self, n, img_size, num_runs_each, channels=3):
        self.n, self.img_size, self.runs, self.channels = n, img_size, num_runs_each, channels

    def __len__(self):
        return self.n * self.runs

    def __getitem__(self, k):
        i, r = divmod(k, self.runs)
        g = torch.Generator().manual_seed(1000 + i)
        coarse = torch.rand(1, self.channels, 6, 6, generator=g)
        img = torch.nn.functional.interpolate(coarse, size=(self.img_size, self.img_size), mode="bicubic", align_corners=False)[0].clamp(0.0, 1.0)
        c = np.arange(self.channels) % len(image_mean)
        mean, std = torch.as_tensor(image_mean[c], dtype=torch.float32), torch.as_tensor(image_std[c], dtype=torch.float32)
        return (img - mean[:, None, None]) / std[:, None, None], eval_seed(i, r)


def mask_draws(model, seeds, device):
    """The masking noise of a batch whose row j is image-run seed `seeds[j]`: exactly what `torch.manual_seed(seed_j); torch.rand(1, L)` gives on
    the device, so row j's mask is the one `model(x_j, mask_ratio, mask_seed=seed_j)` draws.  -> (noise, box) as `model._run` takes them: the
    multi-scale variants get the noise of both views (the same rows: they re-seed before each view) and one crop box, drawn under the first seed."""
    L = model.num_patches
    rows = []
    for s in seeds:
        torch.manual_seed(int(s))
        rows.append(torch.rand(1, L, device=device))
    noise = torch.cat(rows, dim=0)
    if not hasattr(model, "ms_range"):
        return noise, None
    from models_mae.MAE_ViT_MsLd import sample_crop_box
    torch.manual_seed(int(seeds[0]))
    box = torch.tensor(tuple(int(v) for v in sample_crop_box(model.input_size, model.ms_range)), dtype=torch.int32)
    return torch.cat([noise, noise], dim=0), box


def eval_noise(imgs, seeds, use_noise):
    """`add_noise(imgs[j], *use_noise)` under a device generator seeded with seeds[j], row by row (a row does not depend on its batch)."""
    if use_noise is None:
        return imgs
    gen = torch.Generator(device=imgs.device)
    return torch.stack([add_noise(imgs[j], use_noise[0], use_noise[1], generator=gen.manual_seed(int(s))) for j, s in enumerate(seeds)])


@torch.no_grad()
def eval_batch(model, imgs, seeds, names, mean=None, std=None):
    """The inner step of run_eval: one masked forward of the batch `imgs` (on the device; row j masked under seeds[j]) and one recon_eval of the
    returned prediction -> {name: fp32 [n] on the device}.  Nothing is read back."""
    noise, box = mask_draws(model, seeds, imgs.device)
    pred = model._run(imgs, getattr(model, "mask_ratio", 0.75), noise, box)[1]
    return metrics.batch_metrics(imgs, pred, model.patch_size, names, mean, std)


# ---- contact sheets (csrc/recon_panel.hip): the arrays of run_one_image, in its order, as panel names -> kernel codes, and the reference's titles
PANEL_CODES = {"x": 0, "xm": 1, "y": 2, "ym": 3, "xm_ym": 4}
PANEL_TITLES = {"x": "Original", "xm": "Input (Masked)", "y": "Reconstruction", "ym": "Reconstruction (Masked)", "xm_ym": "Reconstruction + Visible"}


def sheet_width(S, n_panels, gap):
    return n_panels * S + (n_panels - 1) * gap


def panel_codes(panels):
    """Panel names (or codes) -> the list of codes the kernel takes."""
    names = [panels] if isinstance(panels, (str, int)) else list(panels)
    try:
        return [PANEL_CODES[n] if isinstance(n, str) else int(n) for n in names]
    except KeyError as e:
        raise ValueError(f"unknown panel {e.args[0]!r}: {', '.join(PANEL_CODES)}") from None


def _model_device(model):
    return torch.device(model.device) if getattr(model, "device", None) is not None else next(model.parameters()).device


@torch.no_grad()
def masked_forward(model, imgs, seeds):
    """The forward of eval_batch: row j of `imgs` masked under seeds[j] -> (pred [n, L, p*p*C], mask [n, L]) on the device."""
    noise, box = mask_draws(model, seeds, imgs.device)
    out = model._run(imgs, getattr(model, "mask_ratio", 0.75), noise, box)
    return out[1], out[2]


@torch.no_grad()
def reconstruction_panels(model, imgs, seeds, panels=("x", "xm", "y"), gap=2, bands=None, mean=None, std=None, pred=None, mask=None):
    """Contact-sheet rows of a batch -> uint8 [n, S, W, 3] on the device, W = K S + (K - 1) gap: for every image its K = len(panels) panels side by
    side, `gap` white pixels between them, each value as the byte the reference's plot_image shows (int(clip(255 v, 0, 255))).  One masked forward
    of `imgs` (on the device, normalised; row j masked under seeds[j]) exactly as eval_batch makes it, then one `csmae_recon_panel`; with `pred` and
    `mask` given (the forward already made, e.g. the one that was scored) no forward runs and `seeds` is not used.  bands: the channels shown as red,
    green, blue (None: 0, 1, 2; one channel: 0, 0, 0) — what makes 4-band input viewable.  mean / std default to the plot statistics."""
    from csmae_hip import ops
    if pred is None or mask is None:
        pred, mask = masked_forward(model, imgs, seeds)
    C = imgs.shape[1]
    c = np.arange(C) % len(image_mean)
    mean, std = image_mean[c] if mean is None else mean, image_std[c] if std is None else std
    imgs = imgs.float().contiguous()
    return ops.recon_panel(imgs, pred, mask.float().contiguous(), metrics._channel_stats(mean, C, imgs.device), metrics._channel_stats(std, C, imgs.device),
                           model.patch_size, panels=panel_codes(panels), gap=gap, bands=bands)


def stack_sheets(rows, gap=2):
    """uint8 [H_i, W_i, 3] arrays top to bottom, `gap` white rows between neighbours, narrower ones padded with white on the right."""
    W = max(r.shape[1] for r in rows)
    parts = []
    for i, r in enumerate(rows):
        if i and gap:
            parts.append(np.full((gap, W, 3), 255, dtype=np.uint8))
        parts.append(r if r.shape[1] == W else np.concatenate([r, np.full((r.shape[0], W - r.shape[1], 3), 255, dtype=np.uint8)], axis=1))
    return np.ascontiguousarray(np.concatenate(parts, axis=0))


def write_sheet(path, sheet, meta=None):
    """`sheet` (uint8 [H, W, 3]) as a PNG at `path`; `meta` as JSON beside it (the same name, .json)."""
    from PIL import Image
    Image.fromarray(sheet, mode="RGB").save(path, format="PNG")
    if meta is not None:
        import json
        with open(os.path.splitext(path)[0] + ".json", "w", encoding="utf-8") as f:
            json.dump(meta, f)


def run_eval(models, basedir, comp_metrics=None, use_noise=None, num_runs_each=5, batch_size=64, random_crop=False, max_samples=None,
             random_walk=False, walk_seed=None, resample=None, num_workers=4, images=None, panel_dir=None, panel_every=None, panels=("x", "xm", "y"),
             **kwargs):
    """Scores of every `<basedir>/**/*.jpg` under each model of the dict `models`: `mtrs[metric][model_name]` = a list with one float per image, the
    mean over `num_runs_each` runs (run r of image i: crop seed and mask seed seed_str_to_int(f"{i}-{r}")).  `comp_metrics`: a name or a list of
    names of util.metrics.batch_metrics; None = all of METRICS_DICT but ms_ssim, as in the reference.  `use_noise`: e.g. ("gaussian", 0.25).
    `images`: a callable img_size -> dataset of (image, seed) items in EvalImages' order, instead of the files (main_recon_eval.py's synthetic
    images).  The reference's plot arguments (do_plot_metrics_comp, do_plot_image_comp, plot_every, title, ...) are accepted and ignored.
    `panel_dir`: write a contact sheet `<panel_dir>/img_<i:06d>.png` for every image i with i % panel_every == 0 (None: every image) — one row of
    `panels` per model, from run 0 of that image and from the very forward that is scored; models of different input_size go to separate sheets
    `img_<i:06d>_s<size>.png`.  Only the written images' bytes are read back.  None: nothing is written, and nothing else changes."""
    if not isinstance(models, dict):
        models = {"model": models}
    if comp_metrics is not None:
        names = [comp_metrics] if isinstance(comp_metrics, str) else list(comp_metrics)
    else:
        names = [m for m in metrics.METRICS_DICT if m != "ms_ssim"]   # (needs images larger than 160 px; per-image ms_ssim is not built)
    if kwargs:
        print(f"run_eval: no figures in this build, ignoring {sorted(kwargs)}")
    paths = None if images is not None else list(glob_helper(f"{basedir}/**/*.jpg", max_samples=max_samples, random_walk=random_walk, walk_seed=walk_seed))
    scores = {name: {model_name: [] for model_name in models} for name in names}
    n_items = 0
    sizes = sorted({m.input_size for m in models.values()})
    if panel_dir is not None:
        os.makedirs(panel_dir, exist_ok=True)
        every, runs = max(int(panel_every or 1), 1), max(num_runs_each, 1)
    for size in sizes:
        group = {k: m for k, m in models.items() if m.input_size == size}
        ds = images(size) if images is not None else EvalImages(paths, size, num_runs_each, random_crop=random_crop, resample=resample)
        n_items = len(ds)
        loader = torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=num_workers, pin_memory=True, drop_last=False)
        stats = {}
        k0 = 0                       # the dataset index of the batch's first item: item k is run k % runs of image k // runs
        for imgs, seeds in loader:   # (the workers decode the next batches while the GPU runs this one)
            seeds = seeds.tolist()
            clean = {}
            picked = [] if panel_dir is None else [j for j in range(len(seeds)) if (k0 + j) % runs == 0 and ((k0 + j) // runs) % every == 0]
            sheets = []
            for model_name, model in group.items():
                dev = torch.device(model.device) if model.device is not None else next(model.parameters()).device
                if dev not in clean:
                    clean[dev] = eval_noise(imgs.to(dev, non_blocking=True), seeds, use_noise)
                    if dev not in stats:
                        C = imgs.shape[1]
                        c = np.arange(C) % len(image_mean)
                        stats[dev] = (torch.as_tensor(image_mean[c], dtype=torch.float32).to(dev), torch.as_tensor(image_std[c], dtype=torch.float32).to(dev))
                if picked:           # score and draw from one forward: eval_batch's two steps, with the prediction and the mask kept for the sheets
                    pred, mask = masked_forward(model, clean[dev], seeds)
                    got = metrics.batch_metrics(clean[dev], pred, model.patch_size, names, *stats[dev])
                    sheets.append(reconstruction_panels(model, clean[dev][picked], None, panels=panels, mean=stats[dev][0], std=stats[dev][1],
                                                        pred=pred[picked], mask=mask[picked]))
                else:
                    got = eval_batch(model, clean[dev], seeds, names, *stats[dev])
                for name in names:
                    scores[name][model_name].append(got[name])
            for t, j in enumerate(picked):
                i = (k0 + j) // runs
                fname = f"img_{i:06d}.png" if len(sizes) == 1 else f"img_{i:06d}_s{size}.png"
                write_sheet(os.path.join(panel_dir, fname), stack_sheets([s[t].cpu().numpy() for s in sheets]))
            k0 += len(seeds)
    n_images = n_items // max(num_runs_each, 1)
    mtrs = {name: {} for name in names}
    for name in names:
        for model_name in models:
            per_run = torch.cat(scores[name][model_name]).double().cpu() if scores[name][model_name] else torch.zeros(0, dtype=torch.float64)
            mtrs[name][model_name] = (per_run.view(n_images, num_runs_each).sum(1) / num_runs_each).tolist()
    print(f"# Finished evaluating on: {basedir} - {n_images} images for {len(models)} models ({num_runs_each} runs each)")
    return mtrs
