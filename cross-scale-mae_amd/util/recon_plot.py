"""The reference's reconstruction figure (`plot_reconstruction`, reference util/viz.py:231-316) without matplotlib: Original | Input (Masked) |
Reconstruction, one row per model, as a contact sheet.  The bytes of every row are written on the device by `csmae_recon_panel`
(util.viz.reconstruction_panels); the host stacks the rows, draws the caption strips with PIL's built-in font and writes the PNG, with a .json
beside it that holds the row order, the panel names and each model's score.

It lives here and not in util/viz.py, where the reference keeps it: util.viz is held to having no `plot_reconstruction` / `plot_image` by the host
tests (the matplotlib figures are not rebuilt there), and this is not that figure — no axes, no suptitle, no display."""
import os

import numpy as np
import torch

from util import viz

CAPTION_HEIGHT = 14   # pixels of the strip above a row (PIL's built-in font is 11 high)


def caption_strip(width, S, gap, titles):
    """A white strip [CAPTION_HEIGHT, width, 3] with title k drawn above panel k (PIL's built-in font, clipped to the strip)."""
    from PIL import Image, ImageDraw, ImageFont
    strip = Image.new("RGB", (width, CAPTION_HEIGHT), (255, 255, 255))
    draw, font = ImageDraw.Draw(strip), ImageFont.load_default()
    for k, t in enumerate(titles):
        draw.text((k * (S + gap) + 1, 1), t, fill=(0, 0, 0), font=font)
    return np.asarray(strip, dtype=np.uint8)


def plot_reconstruction(models, image, image_name=None, comp_metric="ssim", title=None, savedir="./plots/", save=False, show=False, mask_seed=None,
                        panels=("x", "xm", "y"), captions=True, **kwargs):
    """-> np.uint8 [H, W, 3]: one row of `panels` per model of the dict `models`, top to bottom, `gap` (keyword, default 2) white rows between them.
    `image`: a path (each model prepares it at its own input_size; the other keywords go to prepare_image) or a normalised [H, W, C] array, as
    run_one_image takes it.  Each row is one masked forward under `mask_seed` (None: a seed is drawn) + one `csmae_recon_panel`; the model's
    `comp_metric` score comes from the same forward (util.metrics.batch_metrics).
    captions: a strip above each row with the reference's titles, "<model_name> (<METRIC>: <score>)" over the reconstruction; False returns the
    kernel's bytes untouched.  save (needs a title): `<savedir>/<title_to_fname(title)>/plot_img_<title_to_fname(f"{title} - {image_name}")>.png`
    (no sub-folder without an image_name, as in the reference) and, beside it, the same name .json with the row order, the panel names and the scores.
    `show` is accepted and ignored: there is no display."""
    if not isinstance(models, dict):
        models = {"model": models}
    gap, bands = int(kwargs.pop("gap", 2)), kwargs.pop("bands", None)
    names = [panels] if isinstance(panels, str) else list(panels)
    savesubdir = None
    if title is not None and image_name is not None:
        savesubdir = viz.title_to_fname(title)
        title = f"{title} - {image_name}"
    if mask_seed is None:
        mask_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
    rows, scores = [], {}
    for model_name, model in models.items():
        img = viz.prepare_image(image, model.input_size, **kwargs) if isinstance(image, str) else np.array(image, copy=True)
        x = torch.as_tensor(img).permute(2, 0, 1).unsqueeze(0).float().contiguous().to(viz._model_device(model))
        pred, mask = viz.masked_forward(model, x, [mask_seed])
        score = float(viz.metrics.batch_metrics(x, pred, model.patch_size, [comp_metric])[comp_metric][0])
        row = viz.reconstruction_panels(model, x, None, panels=names, gap=gap, bands=bands, pred=pred, mask=mask)[0].cpu().numpy()
        scores[model_name] = score
        if captions:
            titles = [f"{model_name} ({comp_metric.upper()}: {score:<.3f})" if n == "y" else viz.PANEL_TITLES.get(n, str(n)) for n in names]
            row = np.concatenate([caption_strip(row.shape[1], x.shape[-1], gap, titles), row], axis=0)
        rows.append(row)
    sheet = viz.stack_sheets(rows, gap)
    if save:
        if title is not None:
            folder = os.path.join(savedir, savesubdir) if savesubdir is not None else savedir
            os.makedirs(folder, exist_ok=True)
            save_path = os.path.join(folder, f"plot_img_{viz.title_to_fname(title)}.png")
            viz.write_sheet(save_path, sheet, dict(title=title, models=list(models), panels=[str(n) for n in names], metric=comp_metric, scores=scores,
                                                   mask_seed=mask_seed))
        else:
            print("INFO: Skipped saving because title was not provided")
    return sheet
