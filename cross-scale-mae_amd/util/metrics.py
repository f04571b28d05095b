"""Image-comparison metrics of the evaluation tools (reference util/metrics.py): `calc_metric(x, y, name)` with
name in mse | mae | l1 | l2 | ssim | ms_ssim (aliases ssd -> l2, sad -> l1), returning a python float.

The four element-wise metrics are one-line reductions on whatever device the tensors live on, as in the reference (it calls
them on CPU copies of single images).  `ssim` / `ms_ssim` are the gaussian-window structural similarity of pytorch-msssim 0.2.1
with `data_range=1, size_average=True` (util/metrics.py:5-10,41-46): they run on the MI355X through the same HIP kernels as the
ssim loss family (`csmae_ssim_fwd` with flags 1|2: operands as they are, signed score) — there is no CPU implementation here.

`batch_metrics(img, pred, p, names)` is the batched route of util/viz.py run_eval: ONE score PER IMAGE of a batch, straight from the normalised
input and the model's patch rows (`csmae_recon_eval`: no planes in memory, no host sync), as fp32 tensors on the device."""
import torch


def _as_nchw(t, num_channels):
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.shape[-1] == num_channels and t.shape[1] != num_channels:  # channel-last -> [N, C, H, W] (util/metrics.py:6-9)
        t = t.permute(0, 3, 1, 2)
    return t


def _ssim_score(x, y, levels, num_channels=3):
    from csmae_hip import ops
    x, y = _as_nchw(torch.as_tensor(x), num_channels), _as_nchw(torch.as_tensor(y), num_channels)
    if x.shape != y.shape or x.shape[2] != x.shape[3]:
        raise ValueError(f"ssim metrics need two batches of square images of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    dev = x.device if x.is_cuda else (y.device if y.is_cuda else torch.device("cuda"))
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("ssim / ms_ssim run on the MI355X only (no CPU fallback)")
    x, y = x.to(dev, torch.float32).contiguous(), y.to(dev, torch.float32).contiguous()
    N, C, S, _ = x.shape
    p = next(q for q in (16, 8, 4, 2, 1) if S % q == 0)      # any patch size that tiles the image: the planes are what is compared
    L, P = (S // p) ** 2, p * p * C
    rows = torch.zeros(N, L + 1, P, device=dev)
    rows[:, 1:] = x.reshape(N, C, S // p, p, S // p, p).permute(0, 2, 4, 3, 5, 1).reshape(N, L, P)   # patch rows of x ("nchpwq->nhwpqc")
    ws = torch.empty(ops.ssim_workspace_floats(N, C, S, p, levels), device=dev)
    terms = torch.empty(2, device=dev)
    ops.ssim_fwd(levels, False, y, None, rows.view(N * (L + 1), P), None, ws, terms, N, N, C, S, p, flags=3)
    return 1.0 - float(terms[0])


def calc_ssim(x, y, num_channels=3):
    return _ssim_score(x, y, 1, num_channels)


def calc_ms_ssim(x, y, num_channels=3):
    return _ssim_score(x, y, 5, num_channels)


METRICS_DICT = {
    "mse": {"full_name": "Mean Squared Error", "is_lower_better": True, "lambda": lambda x, y: torch.mean((x - y) ** 2).item()},
    "mae": {"full_name": "Mean Absolute Error", "is_lower_better": True, "lambda": lambda x, y: torch.mean(torch.abs(x - y)).item()},
    "l1": {"full_name": "L1 Norm", "is_lower_better": True, "lambda": lambda x, y: torch.sum(torch.abs(x - y)).item()},
    "l2": {"full_name": "L2 Norm", "is_lower_better": True, "lambda": lambda x, y: torch.sum((x - y) ** 2).item()},
    "ssim": {"full_name": "Structural Similarity Index", "is_lower_better": False, "lambda": calc_ssim},
    # needs images larger than 160 px (four 2x down-samplings of an 11-tap window)
    "ms_ssim": {"full_name": "Multi-Scale Structural Similarity Index", "is_lower_better": False, "lambda": calc_ms_ssim},
}


def calc_metric(x, y, metric_name):
    name = metric_name.lower()
    name = {"ssd": "l2", "sad": "l1"}.get(name, name)
    return METRICS_DICT[name]["lambda"](x, y)


BATCH_METRICS = ("mse", "mae", "l1", "l2", "ssim")


def _channel_stats(v, C, dev):
    """Per-channel statistics as the fp32 [C] device tensor the kernel reads (a tensor that already is one is used as it is: no copy, no sync)."""
    if torch.is_tensor(v) and v.device == dev and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == C:
        return v
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
    if t.numel() != C:
        raise ValueError(f"{t.numel()} channel statistics for images of {C} channels")
    return t.to(dev).contiguous()


def batch_metrics(img, pred, p, names, mean=None, std=None):
    """Per-image scores of a batched forward: img [N, C, S, S] normalised input, pred [N, L, p*p*C] the model's patch rows (fp32 or bf16; any
    view with a dense last dimension), both on the GPU.  With X = img * std + mean and Y = unpatchify(pred) * std + mean (mean / std default to
    util.viz.image_mean / image_std), -> {name: fp32 [N] on the device} for the names mse | mae | l1 | l2 | ssim (aliases ssd -> l2, sad -> l1, keyed as
    asked); each value is what `calc_metric(X[n], Y[n], name)` scores for that one image.  One `csmae_recon_eval` launch pair, no host sync.
    ms_ssim is not computed per image: `calc_metric` is the single-batch route for it."""
    from csmae_hip import ops
    names = [names] if isinstance(names, str) else list(names)
    canon = [{"ssd": "l2", "sad": "l1"}.get(n.lower(), n.lower()) for n in names]
    for n, c in zip(names, canon):
        if c == "ms_ssim":
            raise ValueError("batch_metrics does not compute ms_ssim per image: calc_metric(x, y, 'ms_ssim') is the single-batch route")
        if c not in BATCH_METRICS:
            raise ValueError(f"unknown metric {n!r}: batch_metrics knows {', '.join(BATCH_METRICS)} and the aliases ssd, sad")
    if not (torch.is_tensor(img) and torch.is_tensor(pred) and img.is_cuda and pred.is_cuda) or not torch.cuda.is_available():
        raise RuntimeError("ssim / ms_ssim run on the MI355X only (no CPU fallback)")
    if img.dim() != 4 or img.shape[2] != img.shape[3]:
        raise ValueError(f"batch_metrics needs a batch of square images [N, C, S, S], got {tuple(img.shape)}")
    if mean is None or std is None:
        from util.viz import image_mean, image_std
        mean, std = image_mean if mean is None else mean, image_std if std is None else std
    N, C, S, _ = img.shape
    img = img.float().contiguous()
    rows = ops.recon_eval(img, pred, _channel_stats(mean, C, img.device), _channel_stats(std, C, img.device), p)
    count = float(C * S * S)
    col = {"l2": rows[:, 0], "l1": rows[:, 1], "ssim": rows[:, 2]}
    out = {}
    for n, c in zip(names, canon):
        out[n] = rows[:, 0] / count if c == "mse" else rows[:, 1] / count if c == "mae" else col[c].clone()
    return out


def confusion_matrix(y_true, y_pred, num_classes=None):
    """[K, K] int64 counts, rows = true class, columns = predicted class (numpy, on the host)."""
    import numpy as np
    y_true, y_pred = np.asarray(y_true).astype(np.int64).reshape(-1), np.asarray(y_pred).astype(np.int64).reshape(-1)
    if num_classes is None:
        num_classes = int(max(y_true.max(initial=-1), y_pred.max(initial=-1))) + 1
    cm = np.zeros((num_classes, num_classes), dtype=np.int64)
    np.add.at(cm, (y_true, y_pred), 1)
    return cm


def f1_scores(y_true, y_pred, num_classes=None):
    """-> (macro F1, micro F1, per-class F1) as sklearn.metrics.f1_score(average="macro" / "micro" / None) computes them: the classes are the
    labels that occur in y_true or y_pred, a class without predicted and without true samples in its denominator scores 0."""
    import numpy as np
    cm = confusion_matrix(y_true, y_pred, num_classes)
    tp = np.diag(cm).astype(np.float64)
    pred, true = cm.sum(0).astype(np.float64), cm.sum(1).astype(np.float64)
    present = (pred + true) > 0
    denom = pred + true          # 2 tp + fp + fn
    per_class = np.where(denom > 0, 2.0 * tp / np.maximum(denom, 1.0), 0.0)[present]
    macro = float(per_class.mean()) if per_class.size else 0.0
    micro = float(2.0 * tp.sum() / max(denom.sum(), 1.0))
    return macro, micro, per_class


def miou_from_confusion(conf):
    """-> (mIoU, per-class IoU [K] float64) of a confusion matrix [K, K] (rows = true class, columns = predicted class; a tensor or an array):
    IoU_k = tp_k / (tp_k + fp_k + fn_k).  A class absent from both truth and prediction (an all-zero row and column) has no IoU: its entry is NaN
    and it is left out of the mean (sklearn's jaccard_score would count it as 0).  With no class present the mean is 0."""
    import numpy as np
    cm = np.asarray(conf.detach().cpu() if torch.is_tensor(conf) else conf).astype(np.float64)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"a confusion matrix is square, got {cm.shape}")
    tp = np.diag(cm)
    union = cm.sum(0) + cm.sum(1) - tp
    present = union > 0
    per_class = np.where(present, tp / np.maximum(union, 1.0), np.nan)
    return (float(per_class[present].mean()) if present.any() else 0.0), per_class


def pixel_accuracy_from_confusion(conf):
    """The share of the counted pixels on the diagonal of a confusion matrix [K, K]; 0 for an empty matrix."""
    import numpy as np
    cm = np.asarray(conf.detach().cpu() if torch.is_tensor(conf) else conf).astype(np.float64)
    total = cm.sum()
    return float(np.trace(cm) / total) if total > 0 else 0.0


def per_image_scores(stats):
    """Per-image scores from the counts `csmae_segpanel` gathers: stats [N, K, 3] (a tensor or an array) of (intersection, label area, prediction
    area) per image and class, counted over the image's valid pixels.  -> dict of numpy arrays: valid [N] int64 (the valid pixels = the sum of the
    label areas), pixel_acc [N] (the intersections / valid; NaN for an image without a valid pixel), iou [N, K] = intersection / (label area +
    prediction area - intersection), NaN for a class the image neither holds nor predicts, and mIoU [N] over the classes with
    label area + prediction area > 0 (NaN where there is none) — miou_from_confusion's rule, image by image."""
    import numpy as np
    s = np.asarray(stats.detach().cpu() if torch.is_tensor(stats) else stats).astype(np.float64)
    if s.ndim != 3 or s.shape[2] != 3:
        raise ValueError(f"stats are [N, K, 3] (intersection, label area, prediction area), got {s.shape}")
    inter, area_l, area_p = s[..., 0], s[..., 1], s[..., 2]
    valid = area_l.sum(1)
    present = (area_l + area_p) > 0
    iou = np.where(present, inter / np.maximum(area_l + area_p - inter, 1.0), np.nan)
    n_present = present.sum(1)
    miou = np.where(n_present > 0, np.where(present, iou, 0.0).sum(1) / np.maximum(n_present, 1), np.nan)
    acc = np.where(valid > 0, inter.sum(1) / np.maximum(valid, 1.0), np.nan)
    return dict(valid=valid.astype(np.int64), pixel_acc=acc, mIoU=miou, iou=iou)
