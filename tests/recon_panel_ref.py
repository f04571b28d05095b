"""Helpers of the contact-sheet tests (test_recon_panel_gpu.py) and of their CPU self-check (test_recon_panel_cpu.py): a numpy float64 restatement of
what csrc/recon_panel.hip writes, the per-byte error bound, seeded masks, the table of cases and an fp32 emulation with seeded defects.

Definitions (include/csmae.h): X = img * std + mean, Y = unpatchify(pred) * std + mean (recon_eval_ref's element order), m = the mask value of the
pixel's patch (1 = removed).  Panel codes 0 X, 1 X (1 - m), 2 Y, 3 Y m, 4 X (1 - m) + Y m; a sheet row is the K panels side by side, `gap` white
pixels between neighbours, W = K S + (K - 1) gap; the three bytes of a pixel are the channels bands[0], bands[1], bands[2]; a value v becomes
byte = floor(min(max(255 v, 0), 255)).

Bound of the kernel's fp32 value of 255 v, per byte, counted the way recon_eval_ref counts (u = 2^-24):
  - un-normalisation x~ = img * std + mean, one product and one sum (or one fused multiply-add): e_x = u (|img std| + |X|), likewise e_y (a bf16
    prediction converts exactly; the reference takes the bf16-rounded values);
  - the products with a 0 / 1 mask and the sum X (1 - m) + Y m (one term is 0) are exact: the panel's error is e_x, e_y, or whichever term is there;
  - the scale 255 v~ rounds once: u |255 v~| <= u (|255 v| + 255 e);
        delta = 255 e + u (|255 v| + 255 e).
A byte is DECIDED when 255 v is farther than delta from every integer of [0, 255] (values clamped from beyond that range are decided), otherwise
BORDERLINE: the kernel may land on either side of the integer.  Stated as what it means — every value within delta of 255 v gives the same byte,
floor(clip(255 v - delta)) == floor(clip(255 v + delta)) — so that the two cases the wording leaves open are decided as well: a blanked pixel is
exactly 0 with delta 0 (the kernel's value is exact there), and just below 0 both ends clamp to 0.  Never more borderline bytes than the wording gives.
Decided bytes must match exactly, borderline ones within 1, gap bytes are 255.
The share of borderline bytes of a case is capped at BORDERLINE_CAP — a condition on the inputs (asserted on the CPU for every case), not a tolerance."""
import functools

import numpy as np
import torch

import recon_eval_ref as R
from gemm_bounds import U32

BORDERLINE_CAP = 0.005
NAMES = ("x", "xm", "y", "ym", "xm_ym")

P1, P3, P5, P2 = (0,), (0, 1, 2), (4, 3, 2, 1, 0), (2, 2)
# (N, C, S, p): one patch per image; 60-byte panel rows, sheets whose row stride is no multiple of 4; grey; four bands shown as (3, 1, 0); odd patch
# size, more images than any per-workgroup count, sheets that start at every alignment; the project's geometry
SHAPES = ((2, 3, 16, 16), (3, 3, 20, 4), (2, 1, 24, 8), (2, 4, 32, 8), (5, 3, 42, 7), (1, 3, 224, 16))
BANDS = {1: (0, 0, 0), 3: (0, 1, 2), 4: (3, 1, 0)}
# (shape, panels, gap, bf16, strided): every panel list, gap, dtype and layout on at least two shapes
CASES = (
    (SHAPES[0], P3, 3, False, False), (SHAPES[0], P5, 0, True, True),
    (SHAPES[1], P1, 0, False, True), (SHAPES[1], P3, 3, True, False), (SHAPES[1], P2, 3, False, False),
    (SHAPES[2], P5, 3, False, False), (SHAPES[2], P2, 0, True, True), (SHAPES[2], P1, 3, False, False),
    (SHAPES[3], P3, 0, False, True), (SHAPES[3], P5, 3, True, False),
    (SHAPES[4], P3, 3, False, True), (SHAPES[4], P2, 3, True, False), (SHAPES[4], P1, 0, False, False),
    (SHAPES[5], P3, 3, True, True), (SHAPES[5], P5, 0, False, False),
)


def case_id(case):
    shape, panels, gap, bf16, strided = case
    return "x".join(map(str, shape)) + "-p" + "".join(map(str, panels)) + f"-g{gap}-" + ("bf16" if bf16 else "fp32") + ("-strided" if strided else "-dense")


def sheet_width(S, K, gap):
    return K * S + (K - 1) * gap


@functools.lru_cache(maxsize=None)
def masks(N, L, seed=0):
    """fp32 [N, L] of 0 / 1 (shared: do not write to it), about 75 % ones per row, seeded; with three images or more the last two are all kept (0) and
    all removed (1); with two, image 1 is all removed when L is odd, all kept otherwise."""
    g = torch.Generator().manual_seed(4100 + 7 * N + 31 * L + seed)
    m = (torch.rand(N, L, generator=g) < 0.75).float()
    if N >= 3:
        m[N - 2] = 0.0
        m[N - 1] = 1.0
    elif N == 2:
        m[1] = float(L % 2)
    return m


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """The operands of a case (shared: do not write to them): recon_eval_ref.inputs, the prediction rounded to bf16 when the case says so, the mask."""
    shape, panels, gap, bf16, strided = case
    N, C, S, p = shape
    o = dict(R.inputs(*shape))
    if bf16:
        o["pred"] = o["pred"].bfloat16()
    o["mask"] = masks(N, (S // p) ** 2)
    o["bands"] = BANDS[C]
    return o


def pixel_mask(mask, S, p):
    """[N, L] -> [N, 1, S, S]: the value of each pixel's patch."""
    N, G = mask.shape[0], S // p
    return np.repeat(np.repeat(np.asarray(mask, dtype=np.float64).reshape(N, G, G), p, axis=1), p, axis=2)[:, None]


def reference(img, pred, mask, mean, std, p, panels, gap, bands):
    """dict(v255, byte, delta, gap, borderline): float64 255 v per output byte [N, S, W, 3], the expected byte (uint8), the bound of the kernel's fp32
    255 v, which bytes are gap bytes and which are borderline."""
    N, C, S, _ = img.shape
    X, Y, a, b = R.operands64(img, pred.float(), mean, std, p)
    e_x, e_y = U32 * (np.abs(a) + np.abs(X)), U32 * (np.abs(b) + np.abs(Y))
    m = pixel_mask(mask.numpy(), S, p)
    K, W = len(panels), sheet_width(S, len(panels), gap)
    v = np.full((N, S, W, 3), 1.0)
    e = np.zeros((N, S, W, 3))
    is_gap = np.ones((N, S, W, 3), dtype=bool)
    sel = list(bands)
    for k, code in enumerate(panels):
        V, E = {0: (X, e_x), 1: (X * (1 - m), e_x * (1 - m)), 2: (Y, e_y), 3: (Y * m, e_y * m), 4: (X * (1 - m) + Y * m, e_x * (1 - m) + e_y * m)}[code]
        x0 = k * (S + gap)
        v[:, :, x0:x0 + S] = V[:, sel].transpose(0, 2, 3, 1)
        e[:, :, x0:x0 + S] = E[:, sel].transpose(0, 2, 3, 1)
        is_gap[:, :, x0:x0 + S] = False
    v255 = 255.0 * v
    delta = 255.0 * e + U32 * (np.abs(v255) + 255.0 * e)
    tobyte = lambda t: np.floor(np.clip(t, 0.0, 255.0))   # noqa: E731
    borderline = (tobyte(v255 - delta) != tobyte(v255 + delta)) & ~is_gap
    return dict(v255=v255, byte=np.floor(np.clip(v255, 0.0, 255.0)).astype(np.uint8), delta=delta, gap=is_gap, borderline=borderline)


def borderline_share(ref):
    return float(ref["borderline"].mean())


def differing_borderline_share(got, ref):
    """Share of ALL bytes that are borderline and differ from the float64 byte."""
    g = np.asarray(got)
    return float(((g != ref["byte"]) & ref["borderline"]).mean())


def violations(got, ref):
    """Names of the checks a [N, S, W, 3] uint8 result misses against `reference`'s dict (empty: all hold)."""
    g = np.asarray(got)
    bad = []
    if g.shape != ref["byte"].shape or g.dtype != np.uint8:
        return ["shape"]
    if not (g[ref["gap"]] == 255).all():
        bad.append("gap")
    decided = ~ref["borderline"] & ~ref["gap"]
    if not (g[decided] == ref["byte"][decided]).all():
        bad.append("decided")
    if not (np.abs(g[ref["borderline"]].astype(np.int64) - ref["byte"][ref["borderline"]].astype(np.int64)) <= 1).all():
        bad.append("borderline")
    return bad


# ------------------------------------------------------------------------------------------------ fp32 emulation (CPU self-check)
DEFECTS = ("round_nearest", "mask_inverted", "bgr", "bands_ignored", "gap_short", "channel_major", "cls_as_patch0", "no_clamp")


def emulate(img, pred, mask, mean, std, p, panels, gap, bands, defect=None):
    """The kernel's arithmetic in fp32 torch -> uint8 [N, S, W, 3] (numpy).  Defects: the byte is rounded to nearest instead of truncated; the mask is
    read as 1 - m; the three bytes of a pixel leave in the order blue, green, red; `bands` is ignored (0, 1, 2, or 0, 0, 0 for one channel); panel k
    starts at k (S + gap - 1) (a gap one pixel short: the panels shift, white is left behind the last); the patch element is read channel-major
    (c p p + pixel); patch row l is read from row l of a buffer with a cls row (zeros here) in front; the int conversion is not clamped and wraps."""
    N, C, S, _ = img.shape
    G = S // p
    rows = pred.float()
    if defect == "cls_as_patch0":
        rows = torch.cat([torch.zeros_like(rows[:, :1]), rows[:, :-1]], dim=1)
    if defect == "channel_major":
        planes = rows.reshape(N, G, G, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(N, C, S, S)
    else:
        planes = rows.reshape(N, G, G, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(N, C, S, S)
    mn, sd = mean.float()[None, :, None, None], std.float()[None, :, None, None]
    X, Y = img.float() * sd + mn, planes * sd + mn
    m = torch.from_numpy(pixel_mask(mask.numpy(), S, p)).float()
    if defect == "mask_inverted":
        m = 1.0 - m
    sel = list(bands)
    if defect == "bands_ignored":
        sel = [0, 0, 0] if C == 1 else [0, 1, 2]
    if defect == "bgr":
        sel = sel[::-1]
    K, W = len(panels), sheet_width(S, len(panels), gap)
    step = S + gap - (1 if defect == "gap_short" and gap > 0 else 0)
    out = np.full((N, S, W, 3), 255, dtype=np.uint8)
    for k, code in enumerate(panels):
        V = {0: X, 1: X * (1 - m), 2: Y, 3: Y * m, 4: X * (1 - m) + Y * m}[code]
        t = V[:, sel].permute(0, 2, 3, 1) * torch.tensor(255.0)
        if defect == "no_clamp":
            b = (t.to(torch.int32) & 255).to(torch.uint8)
        elif defect == "round_nearest":
            b = t.clamp(0.0, 255.0).round().to(torch.uint8)
        else:
            b = t.clamp(0.0, 255.0).to(torch.int32).to(torch.uint8)
        out[:, :, k * step:k * step + S] = b.numpy()
    return out
