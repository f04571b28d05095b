"""Helpers of the reconstruction-evaluation tests (test_recon_eval_gpu.py) and of their CPU self-check (test_recon_eval_cpu.py): numpy float64
restatements of what csrc/recon_eval.hip computes, seeded inputs, the error bounds, guarded buffers and an fp32 emulation with seeded defects.

Definitions (include/csmae.h): X = img * std + mean, Y = unpatchify(pred) * std + mean; pixel (c, y, x) of the prediction is element
((y % p) p + x % p) C + c of patch row (y / p) (S / p) + x / p.  Per image: sse = sum (X - Y)^2, sae = sum |X - Y| over all C S S elements,
ssim = pytorch-msssim 0.2.1's ssim(data_range 1, signed): 11-tap gaussian (sigma 1.5, the package builds it in fp32), valid windows, the H axis
first; the mean of the map per plane, the mean of the planes.

Bounds of the two sums, from counted fp32 operations (u = 2^-24), per image, computed from the float64 intermediates:
  - un-normalisation x~ = img * std + mean: one product and one sum (or one fused multiply-add, which rounds once):
        e_x = u (|img std| + |X|), likewise e_y (a bf16 prediction converts to fp32 exactly; the float64 reference takes the bf16-rounded values);
  - the subtraction d~ = x~ - y~:  e_d = e_x + e_y + u |d|;
  - the terms: |d~| carries e_d;  d~^2 carries 2 |d| e_d + e_d^2 + u d^2;
  - the summation, depth k along the longest chain of additions: a thread of the tile kernel adds at most cdiv(42 * 42, 256) = 7 owned elements in a
    row, the wave folds 64 lanes in 6 steps, the block adds its 4 waves in a row (block_sum) — 17 — then one lane of the fold adds at most
    cdiv(C * tiles, 64) tile partials in a row and the wave folds in 6 more steps:
        k = 17 + cdiv(C * tiles, 64) + 6,   |error of the sum| <= sum e_t + k u / (1 - k u) * sum (|t| + e_t).
ssim: 1e-4 absolute per image, the bar tests/test_model_gpu.py holds util.metrics.calc_ssim to against the oracle.

Worst observed |ssim - float64| on an MI355X over the shapes of test_recon_eval_gpu.py: see WORST_SSIM_OBSERVED (both kernels share the FIR code and
land within a few fp32 roundings of each other; the error grows with the number of windows averaged)."""
import functools

import numpy as np
import torch

from gemm_bounds import U32
from norm_ref import Guarded, cdiv  # noqa: F401  (Guarded is re-exported for the GPU tests)

WIN, TILE, STAGE = 11, 32, 42
SSIM_ATOL = 1e-4
# recorded on an MI355X by test_recon_eval_gpu.py::test_kernel_vs_float64 (it prints both figures): the new kernel over all shapes and layouts (worst at
# (1, 3, 544, 16) bf16; 3.43e-6 there in fp32) / calc_ssim, image by image, on the fp32 inputs (worst at the same shape).  The sums stayed below 0.04 of
# their bounds.
WORST_SSIM_OBSERVED = {"recon_eval": 3.452e-06, "calc_ssim": 3.490e-06}
IMAGE_MEAN = np.array([0.40558367, 0.43378946, 0.43175863])   # util/viz.py
IMAGE_STD = np.array([0.19208308, 0.19136319, 0.19783947])

# (N, C, S, p): Ho = 1; exactly one tile; ragged 2 x 2; exact 2 x 2 with one channel; four channels; the project's geometry (4 x 4 tiles);
# 49 tiles (under one wave of partials); 289 tiles x 3 planes (the fold loops)
SHAPES = ((2, 3, 11, 11), (3, 3, 42, 7), (3, 3, 48, 16), (2, 1, 74, 2), (5, 4, 96, 8), (2, 3, 128, 16), (1, 3, 224, 16), (1, 3, 544, 16))


def gaussian_window():
    """The package's window: built in fp32 (`_fspecial_gauss_1d(11, 1.5)`), then used in the operands' precision."""
    c = torch.arange(WIN, dtype=torch.float32) - WIN // 2
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).double().numpy()


def tiles_x(S):
    return cdiv(S - (WIN - 1), TILE)


def channel_stats(C):
    c = np.arange(C) % 3
    return torch.tensor(IMAGE_MEAN[c], dtype=torch.float32), torch.tensor(IMAGE_STD[c], dtype=torch.float32)


def patchify(planes, p):
    """[N, C, S, S] -> patch rows [N, L, p p C] ("nchpwq->nhwpqc")."""
    N, C, S, _ = planes.shape
    G = S // p
    return planes.reshape(N, C, G, p, G, p).transpose(0, 2, 4, 3, 5, 1).reshape(N, G * G, p * p * C)


def unpatchify(rows, C, S, p):
    """Patch rows [N, L, p p C] -> [N, C, S, S], from the definition above."""
    N = rows.shape[0]
    G = S // p
    return rows.reshape(N, G, G, p, p, C).transpose(0, 5, 1, 3, 2, 4).reshape(N, C, S, S)


@functools.lru_cache(maxsize=None)
def inputs(N, C, S, p, seed=0):
    """Seeded operands (shared: do not write to them): img [N, C, S, S] and pred [N, L, P] fp32 CPU tensors in normalised space, mean / std [C].
    X and Y are a smooth field plus noise, mostly inside [0, 1]; every image and plane has its own frequencies and phase and every pixel its own
    noise, so no two patches agree."""
    rng = np.random.default_rng(7000 + 13 * N + 101 * C + 1009 * S + 17 * p + seed)
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    X, Y = np.empty((N, C, S, S)), np.empty((N, C, S, S))
    for n in range(N):
        for c in range(C):
            fy, fx, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 2 * np.pi)
            X[n, c] = 0.5 + 0.3 * np.sin(2 * np.pi * (fy * yy + fx * xx) / S + ph) + 0.05 * rng.standard_normal((S, S))
            Y[n, c] = X[n, c] + 0.08 * np.sin(2 * np.pi * (fx * yy - fy * xx) / S + 2 * ph) + 0.05 * rng.standard_normal((S, S))
    mean, std = channel_stats(C)
    m, s = mean.double().numpy()[None, :, None, None], std.double().numpy()[None, :, None, None]
    img = torch.from_numpy((X - m) / s).float()
    pred = torch.from_numpy(patchify((Y - m) / s, p)).float().contiguous()
    return dict(img=img, pred=pred, mean=mean, std=std)


def _blur(a, w):
    """Valid 11-tap filter along H, then along W, of [..., H, W]."""
    Ho = a.shape[-2] - WIN + 1
    h = sum(w[k] * a[..., k:k + Ho, :] for k in range(WIN))
    Wo = a.shape[-1] - WIN + 1
    return sum(w[k] * h[..., :, k:k + Wo] for k in range(WIN))


def ssim_planes(X, Y, w=None):
    """Signed ssim of every plane of [N, C, S, S] float64 operands, data_range 1 -> [N, C]."""
    w = gaussian_window() if w is None else w
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = _blur(X, w), _blur(Y, w)
    s1, s2, s12 = _blur(X * X, w) - mu1 * mu1, _blur(Y * Y, w) - mu2 * mu2, _blur(X * Y, w) - mu1 * mu2
    cs = (2 * s12 + c2) / (s1 + s2 + c2)
    sm = (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * cs
    return sm.reshape(sm.shape[0], sm.shape[1], -1).mean(-1)


def operands64(img, pred, mean, std, p):
    """(X, Y, img * std, pred-planes * std) in float64 from the (already rounded) kernel operands."""
    N, C, S, _ = img.shape
    m, s = mean.double().numpy()[None, :, None, None], std.double().numpy()[None, :, None, None]
    a = img.double().numpy() * s
    b = unpatchify(pred.double().numpy(), C, S, p) * s
    return a + m, b + m, a, b


def sum_depth(C, S):
    return 17 + cdiv(C * tiles_x(S) ** 2, 64) + 6


def reference(img, pred, mean, std, p):
    """float64 scores per image and the bounds of the two sums: dict(sse, sae, ssim, b_sse, b_sae), numpy [N]."""
    N, C, S, _ = img.shape
    X, Y, a, b = operands64(img, pred, mean, std, p)
    d = X - Y
    e_x, e_y = U32 * (np.abs(a) + np.abs(X)), U32 * (np.abs(b) + np.abs(Y))
    e_d = e_x + e_y + U32 * np.abs(d)
    e_sq = 2 * np.abs(d) * e_d + e_d ** 2 + U32 * d * d
    k = sum_depth(C, S)
    grow = k * U32 / (1 - k * U32)
    flat = lambda t: t.reshape(N, -1).sum(1)   # noqa: E731
    return dict(sse=flat(d * d), sae=flat(np.abs(d)), ssim=ssim_planes(X, Y).mean(1),
                b_sse=flat(e_sq) + grow * flat(d * d + e_sq), b_sae=flat(e_d) + grow * flat(np.abs(d) + e_d))


def violations(got, ref):
    """Names of the checks an [N, 4] result misses against `reference`'s dict (empty: all hold)."""
    g = np.asarray(got, dtype=np.float64)
    bad = []
    if not (np.abs(g[:, 0] - ref["sse"]) <= ref["b_sse"]).all():
        bad.append("sse")
    if not (np.abs(g[:, 1] - ref["sae"]) <= ref["b_sae"]).all():
        bad.append("sae")
    if not (np.abs(g[:, 2] - ref["ssim"]) <= SSIM_ATOL).all():
        bad.append("ssim")
    if not (g[:, 3] == 0).all():
        bad.append("pad")
    return bad


# ------------------------------------------------------------------------------------------------ fp32 emulation (CPU self-check)
DEFECTS = ("drop_last_rows", "drop_last_cols", "overlap_twice", "swap_elem_order", "cls_as_patch0", "unsigned_ssim")


def emulate(img, pred, mean, std, p, defect=None):
    """The kernel's arithmetic in fp32 torch -> [N, 4]: tile partials over the owned pixels, folded plane by plane and tile by tile.
    Defects: the sums skip the last 10 rows / columns (the map's extent instead of the image's); every tile sums its whole staged window (the 10-pixel
    overlaps count twice); the patch element is read channel-major (c p p + pixel); patch row l is read from row l of a buffer that has a cls row
    (zeros here) in front; the planes' ssim is clamped at zero before the mean."""
    N, C, S, _ = img.shape
    G = S // p
    rows = pred.float()
    if defect == "cls_as_patch0":
        rows = torch.cat([torch.zeros_like(rows[:, :1]), rows[:, :-1]], dim=1)
    if defect == "swap_elem_order":
        planes = rows.reshape(N, G, G, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(N, C, S, S)
    else:
        planes = rows.reshape(N, G, G, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(N, C, S, S)
    m, s = mean.float()[None, :, None, None], std.float()[None, :, None, None]
    X, Y = img.float() * s + m, planes * s + m
    d = X - Y
    sq, ab = d * d, d.abs()
    T = tiles_x(S)
    sse, sae = torch.zeros(N), torch.zeros(N)
    for c in range(C):
        for ty in range(T):
            for tx in range(T):
                y0, x0 = ty * TILE, tx * TILE
                y1 = S if ty == T - 1 else y0 + TILE
                x1 = S if tx == T - 1 else x0 + TILE
                if defect == "overlap_twice":
                    y1, x1 = min(y0 + STAGE, S), min(x0 + STAGE, S)
                if defect == "drop_last_rows":
                    y1 = min(y1, S - (WIN - 1))
                if defect == "drop_last_cols":
                    x1 = min(x1, S - (WIN - 1))
                sse = sse + sq[:, c, y0:y1, x0:x1].reshape(N, -1).sum(1)
                sae = sae + ab[:, c, y0:y1, x0:x1].reshape(N, -1).sum(1)
    w = torch.from_numpy(gaussian_window()).float()
    F = torch.nn.functional

    def blur(t):
        t = F.conv2d(t, w.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
        return F.conv2d(t, w.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)
    c1, c2 = 1.0e-4, 9.0e-4
    mu1, mu2 = blur(X), blur(Y)
    s1, s2, s12 = blur(X * X) - mu1 * mu1, blur(Y * Y) - mu2 * mu2, blur(X * Y) - mu1 * mu2
    sm = (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * ((2 * s12 + c2) / (s1 + s2 + c2))
    per_plane = sm.flatten(2).mean(-1)
    if defect == "unsigned_ssim":
        per_plane = per_plane.clamp_min(0.0)
    return torch.stack([sse, sae, per_plane.mean(1), torch.zeros(N)], dim=1)
