"""What a user looks at after a segmentation-probe run (main_segprobe.py --panel_dir / --pred_dir / --per_image): overlay sheets whose bytes
`csmae_segpanel` writes on the device from the patch logits that were scored, the argmax map as a palette PNG, and the colour map both use.  The
dense counterpart of the reconstruction sheets of util/viz.py, whose PNG writer (`write_sheet`) is reused; the per-image scores are
`util.metrics.per_image_scores`."""
import numpy as np
import torch

# pane names -> kernel codes (include/csmae.h, csmae_segpanel)
PANE_CODES = {"image": 0, "gt": 1, "pred": 2, "gt_over": 3, "pred_over": 4, "errors": 5}
PANE_TITLES = {"image": "Image", "gt": "Ground truth", "pred": "Prediction", "gt_over": "Ground truth over image", "pred_over": "Prediction over image",
               "errors": "Errors"}
NEEDS_LABELS = ("gt", "gt_over", "errors")
DEFAULT_PANES = ("image", "gt_over", "pred_over")
IGNORE_RGB = (224, 224, 192)   # PASCAL VOC's colour of the void label


def default_palette(K):
    """The PASCAL-VOC colour map, uint8 [K, 3]: bit j of the class index, j = 0, 1, 2 within each group of three bits, goes to red, green, blue, the
    lowest group to the highest bit of the byte (class 1 = (128, 0, 0), 2 = (0, 128, 0), 3 = (128, 128, 0), ...).  The rows are distinct for K <= 256."""
    pal = np.zeros((int(K), 3), dtype=np.uint8)
    for k in range(int(K)):
        c = k
        for j in range(8):
            for ch in range(3):
                pal[k, ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
    return pal


def pane_codes(names):
    """Pane names (or codes) -> the list of codes the kernel takes."""
    names = [names] if isinstance(names, (str, int)) else list(names)
    try:
        return [PANE_CODES[n] if isinstance(n, str) else int(n) for n in names]
    except KeyError as e:
        raise ValueError(f"unknown pane {e.args[0]!r}: {', '.join(PANE_CODES)}") from None


def device_palette(palette, K, device):
    """`palette` (None: default_palette(K); an array or a tensor [K, 3]) as the contiguous uint8 device tensor the kernel reads."""
    pal = torch.as_tensor(default_palette(K) if palette is None else palette)
    if pal.shape != (K, 3):
        raise ValueError(f"a palette of {tuple(pal.shape)} for {K} classes: it holds one (r, g, b) row per class")
    return pal.to(device=device, dtype=torch.uint8).contiguous()


@torch.no_grad()
def segmentation_panels(probe, samples, labels=None, panes=DEFAULT_PANES, alpha=0.5, palette=None, mean=None, std=None, patch_logits=None, gap=2, bands=None,
                        ignore_rgb=IGNORE_RGB, pred=None, stats=None):
    """Overlay sheets of a batch -> uint8 [n, S, W, 3] on the device, W = P S + (P - 1) gap: for every image its P = len(panes) panes side by side,
    `gap` white pixels between them.  One forward of `probe` (a models_seg.LinearSegProbe) on `samples` (on the device, normalised), then one
    `csmae_segpanel`; with `patch_logits` given (the forward already made, e.g. the one that was scored) no forward runs.  labels: uint8
    [n, S, S] or None — the panes gt, gt_over and errors need them.  mean / std default to the plot statistics of util.viz; pred / stats: optional
    outputs, as ops.seg_panel takes them."""
    from csmae_hip import ops
    from util import metrics
    from util.viz import image_mean, image_std
    if patch_logits is None:
        patch_logits, _ = probe._logits(samples)
    C, K = samples.shape[1], patch_logits.shape[-1]
    c = np.arange(C) % len(image_mean)
    mean, std = image_mean[c] if mean is None else mean, image_std[c] if std is None else std
    samples = samples.float().contiguous()
    dev = samples.device
    return ops.seg_panel(samples, patch_logits.float().contiguous(), None if labels is None else labels.contiguous(), metrics._channel_stats(mean, C, dev),
                         metrics._channel_stats(std, C, dev), device_palette(palette, K, dev), panes=pane_codes(panes), alpha=alpha, gap=gap, bands=bands,
                         ignore_rgb=ignore_rgb, pred=pred, stats=stats)


def write_mask_png(path, pred, palette):
    """`pred` (uint8 [S, S] class indices; a tensor or an array) as a mode-P PNG at `path`: the pixel values ARE the class indices, `palette`
    ([K, 3] uint8) is the file's colour table, so a viewer shows colours and a tool reads classes."""
    from PIL import Image
    a = np.ascontiguousarray(pred.detach().cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred), dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError(f"a mask is [H, W], got {a.shape}")
    pal = np.asarray(palette.detach().cpu().numpy() if torch.is_tensor(palette) else palette, dtype=np.uint8).reshape(-1, 3)
    im = Image.fromarray(a, mode="P")
    im.putpalette(pal.reshape(-1).tolist())
    im.save(path, format="PNG")
