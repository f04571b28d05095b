"""Shared helpers of the linear-probing and fine-tuning tests (test_linprobe_gpu.py, test_finetune_gpu.py, test_mixup_cpu.py): the bars, the
NaN-guarded output buffers and the elementwise comparison, the micro ViT with its oracle features and its pre-training checkpoint, torch
restatements of the fine-tune criteria and of the whole fine-tune loss (differentiable, on the CPU), and timm 0.4.12's batch-mode Mixup
restated for the CPU test.  Restatements that a kernel is compared against alone run in float64."""
import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
MICRO = dict(dim_model=128, encoder_num_layers=2, encoder_num_heads=2, decoder_embed_dim=64, decoder_num_layers=2, decoder_num_heads=2)
VIT_MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2)
LOSS_RTOL = 1e-4
VAL = (2e-5, 1e-6)    # rtol, atol of an fp32 kernel's values
GRAD = (1e-4, 1e-7)   # ... of its gradients


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def assert_close(actual, expected, rtol, atol, what=""):
    a, e = actual.detach().double().cpu(), expected.detach().double().cpu()
    assert a.shape == e.shape, (what, a.shape, e.shape)
    err = (a - e).abs()
    tol = atol + rtol * e.abs()
    print(f"{what}: max|err| {float(err.max()):.3e} (ref absmax {float(e.abs().max()):.3e}), worst err/tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), f"{what}: max|err|={float(err.max()):.3e}, bad={int((err > tol).sum())}/{err.numel()}"


def guarded(rows, cols, dtype=torch.float32):
    """[rows, cols] view inside a NaN-filled buffer with one guard row on each side."""
    big = torch.full((rows + 2, cols), float("nan"), device="cuda", dtype=dtype)
    return big, big[1:rows + 1]


def guards_intact(big):
    return bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all())


def _ce_case(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, K, generator=g) * 3
    logits[0] = torch.linspace(-80, 80, K)[torch.randperm(K, generator=g)]   # an unstable softmax overflows on this row (exp(80) ~ 5e34, squared sums beyond fp32)
    labels = torch.randint(0, K, (N,), generator=g)
    labels[0] = int(logits[0].argmin())
    return logits, labels


def micro_sd():
    d = np.load(os.path.join(G, "model_micro.npz"), allow_pickle=False)
    return {k[3:]: torch.from_numpy(np.asarray(d[k])) for k in d.files if k.startswith("sd_")}


def write_pretrain_checkpoint(out):
    """A micro MAE_ViT_MsLdCeCd checkpoint written by misc.save_model into the directory `out` -> its path."""
    import models_mae
    import util.misc as misc
    m = models_mae.MAE_ViT_MsLdCeCd(**MICRO, input_size=64, patch_size="16", predictor_hidden_size=128)
    sd = micro_sd()
    m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()}, strict=True)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    misc.save_model(args=argparse.Namespace(output_dir=str(out)), epoch=0, model=m, model_without_ddp=m, optimizer=opt, loss_scaler=None)
    return str(out / "checkpoint-0.pth")


def oracle_tokens(sd, imgs, heads=2, p=16):
    """The residual stream behind the last block [N, L + 1, D] from the oracle's pieces, on timm-named weights (`pos_embed` from sd when present)."""
    import csmae_oracle as O
    x = F.conv2d(imgs, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    D = x.shape[-1]
    pos = sd["pos_embed"] if "pos_embed" in sd else torch.from_numpy(O.sincos_2d(D, int(x.shape[1] ** 0.5))).float().unsqueeze(0)
    x = torch.cat([sd["cls_token"].expand(x.shape[0], -1, -1), x], dim=1) + pos
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        x = O.vit_block(x, sd, f"blocks.{i}.", heads)
        i += 1
    return x


def oracle_features(sd, imgs, global_pool, norm_w, norm_b, heads=2, p=16):
    """The reference's forward_features (models_vit.py:39-60)."""
    x = oracle_tokens(sd, imgs, heads, p)
    return F.layer_norm(x[:, 1:].mean(1) if global_pool else x[:, 0], (x.shape[-1],), norm_w, norm_b, 1e-6)


def smooth_one_hot(y, K, on, off, dtype=torch.float64):
    t = torch.full((y.shape[0], K), off, dtype=dtype)
    ok = (y >= 0) & (y < K)   # a label outside [0, K) indexes nothing
    t[ok.nonzero().reshape(-1), y[ok]] = on
    return t


def mixup_target_ref(y, K, lam=1.0, smoothing=0.0, dtype=torch.float64):
    """timm.data.mixup.mixup_target."""
    off = smoothing / K
    on = 1.0 - smoothing + off
    return lam * smooth_one_hot(y, K, on, off, dtype) + (1.0 - lam) * smooth_one_hot(y.flip(0), K, on, off, dtype)


def soft_ce_ref(logits, target):
    """timm.loss.SoftTargetCrossEntropy."""
    return torch.sum(-target * F.log_softmax(logits, dim=-1), dim=-1).mean()


def mix_images_ref(x, lam=1.0, box=None):
    """timm Mixup._mix_batch on a copy: mixup with the flipped batch, or the box (yl, yh, xl, xh) copied from it."""
    if box is None:
        l32 = torch.tensor(lam, dtype=torch.float32)
        return x * l32 + x.flip(0) * (1 - l32)
    yl, yh, xl, xh = box
    out = x.clone()
    out[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
    return out


def finetune_loss_ref(sd, imgs, target, global_pool, heads=2, p=16):
    """The whole fine-tune loss on the CPU, differentiable w.r.t. every tensor of `sd` (timm names: pos_embed, cls_token, patch_embed.*, blocks.*,
    fc_norm.* or norm.*, head.*): oracle features -> F.linear -> soft-target cross-entropy against dense targets [N, K]."""
    n = "fc_norm" if global_pool else "norm"
    feats = oracle_features(sd, imgs, global_pool, sd[n + ".weight"], sd[n + ".bias"], heads, p)
    logits = F.linear(feats, sd["head.weight"], sd["head.bias"])
    return soft_ce_ref(logits, target), logits


# ---- timm 0.4.12 Mixup, batch mode, restated (timm/data/mixup.py: rand_bbox, cutmix_bbox_and_lam, Mixup._params_per_batch)
def timm_rand_bbox(img_shape, lam):
    ratio = np.sqrt(1 - lam)
    img_h, img_w = img_shape[-2:]
    cut_h, cut_w = int(img_h * ratio), int(img_w * ratio)
    cy = np.random.randint(0, img_h)
    cx = np.random.randint(0, img_w)
    yl = np.clip(cy - cut_h // 2, 0, img_h)
    yh = np.clip(cy + cut_h // 2, 0, img_h)
    xl = np.clip(cx - cut_w // 2, 0, img_w)
    xh = np.clip(cx + cut_w // 2, 0, img_w)
    return yl, yh, xl, xh


def timm_params_per_batch(img_shape, mixup_alpha, cutmix_alpha, prob, switch_prob):
    """-> (lam, box or None): the draws of one batch."""
    lam, box = 1.0, None
    if np.random.rand() < prob:
        if mixup_alpha > 0.0 and cutmix_alpha > 0.0:
            use_cutmix = np.random.rand() < switch_prob
            lam_mix = np.random.beta(cutmix_alpha, cutmix_alpha) if use_cutmix else np.random.beta(mixup_alpha, mixup_alpha)
        elif mixup_alpha > 0.0:
            use_cutmix, lam_mix = False, np.random.beta(mixup_alpha, mixup_alpha)
        else:
            use_cutmix, lam_mix = True, np.random.beta(cutmix_alpha, cutmix_alpha)
        lam = float(lam_mix)
        if use_cutmix:
            yl, yh, xl, xh = timm_rand_bbox(img_shape, lam)
            lam = 1.0 - (yh - yl) * (xh - xl) / float(img_shape[-2] * img_shape[-1])
            box = (int(yl), int(yh), int(xl), int(xh))
    return lam, box
