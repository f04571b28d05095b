"""Batch-mode mixup / cutmix (timm 0.4.12 `timm.data.mixup.Mixup`, as main_finetune.py uses it) on the MI355X: the draws are made on the host
with `np.random` in timm's order, the images are mixed and the dense targets built by HIP kernels (csmae_mixup_cutmix, csmae_mixup_target).

Draw order per batch: `rand() < prob`; when both alphas are positive `rand() < switch_prob` (cutmix if true); `beta(alpha, alpha)` of the
chosen kind; for cutmix `randint(0, H)` then `randint(0, W)` for the box centre.  Box: ratio = sqrt(1 - lam), cut = int(size * ratio),
lo = clip(c - cut // 2, 0, size), hi = clip(c + cut // 2, 0, size); lam is then corrected to 1 - area / (H W).

Only `mode="batch"`: `pair`, `elem` and `cutmix_minmax` raise NotImplementedError.  Unlike timm's, `__call__` leaves its input alone and
returns a new tensor (sample n reads sample N - 1 - n: the kernel cannot work in place)."""
import numpy as np
import torch


def rand_bbox(img_shape, lam):
    """-> (yl, yh, xl, xh) of the cutmix box for `lam` (two np.random.randint draws: row, then column of the centre)."""
    H, W = int(img_shape[-2]), int(img_shape[-1])
    ratio = np.sqrt(1.0 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    cy = np.random.randint(0, H)
    cx = np.random.randint(0, W)
    clip = lambda v, size: int(min(max(v, 0), size))
    return clip(cy - cut_h // 2, H), clip(cy + cut_h // 2, H), clip(cx - cut_w // 2, W), clip(cx + cut_w // 2, W)


class Mixup:
    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch", correct_lam=True,
                 label_smoothing=0.1, num_classes=1000):
        if cutmix_minmax is not None:
            raise NotImplementedError("Mixup(cutmix_minmax=...) is not implemented on the MI355X path: use cutmix_alpha")
        if mode != "batch":
            raise NotImplementedError(f"Mixup(mode={mode!r}) is not implemented on the MI355X path: only mode='batch' (one lam / box per batch)")
        self.mixup_alpha, self.cutmix_alpha, self.mix_prob, self.switch_prob = mixup_alpha, cutmix_alpha, prob, switch_prob
        self.label_smoothing, self.num_classes, self.mode, self.correct_lam = label_smoothing, num_classes, mode, correct_lam
        self.mixup_enabled = True   # (timm's switch: set to False to stop mixing, the targets are still smoothed)

    def params_per_batch(self, img_shape):
        """-> (lam, box or None): the host draws of one batch."""
        lam, box = 1.0, None
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = bool(np.random.rand() < self.switch_prob)
            elif self.mixup_alpha > 0.0:
                use_cutmix = False
            elif self.cutmix_alpha > 0.0:
                use_cutmix = True
            else:
                raise ValueError("One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true.")
            alpha = self.cutmix_alpha if use_cutmix else self.mixup_alpha
            lam = float(np.random.beta(alpha, alpha))
            if use_cutmix:
                box = rand_bbox(img_shape, lam)
                if self.correct_lam:
                    lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(img_shape[-2] * img_shape[-1])
        return lam, box

    def mix(self, x, target, lam, box=None):
        """The device half for given draws: -> (mixed images, dense targets [N, num_classes])."""
        from csmae_hip import ops
        if len(x) % 2 != 0:
            raise ValueError("Batch size should be even when using this")
        x = x.contiguous().float()
        soft = torch.empty(x.shape[0], self.num_classes, device=x.device, dtype=torch.float32)
        ops.mixup_target(target.contiguous(), soft, lam=lam, smoothing=self.label_smoothing)
        if lam == 1.0 and box is None:   # (timm: nothing to mix)
            return x, soft
        out = torch.empty_like(x)
        ops.mixup_cutmix(x, out, lam=lam, box=box)
        return out, soft

    def __call__(self, x, target):
        if len(x) % 2 != 0:
            raise ValueError("Batch size should be even when using this")
        lam, box = self.params_per_batch(x.shape)
        return self.mix(x, target, lam, box)
