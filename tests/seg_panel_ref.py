"""Helpers of the overlay-sheet tests (test_seg_panel_gpu.py) and of their CPU self-check (test_seg_panel_cpu.py): a float64 restatement of what
csrc/seg_panel.hip writes, the rule a result is held to, the table of cases with their seeded inputs and an fp32 emulation with seeded defects.
Nothing here imports the product.

Definitions (include/csmae.h, csmae_segpanel).  b = the displayed image's byte, recon_panel's rule floor(min(max(255 (img std + mean), 0), 255)) of the
channels bands[0], bands[1], bands[2]; arg = the argmax class of the bilinearly upsampled patch logits (align_corners=False, the lowest index wins
ties: seg_ref.upsample in float64); valid = label < K (255 and stray labels in [K, 255) are ignored); blend(b, c) = (b (256 - a8) + c a8 + 128) >> 8.
Pane codes: 0 b; 1 palette[label] | ignore_rgb; 2 palette[arg]; 3 blend(b, palette[label] | ignore_rgb); 4 blend(b, palette[arg]);
5 valid ? (arg != label ? blend(b, red) : b) : blend(b, ignore_rgb).  A sheet row is the panes side by side, `gap` white pixels between neighbours.
stats[n, k] = (#(label = k and arg = k), #(label = k), #(arg = k and label < K)) over image n.

What fp32 may change, and nothing else:
  * the byte b: recon_panel_ref's bound delta of the kernel's fp32 255 v decides it or leaves the pair floor(clip(255 v -+ delta)).  Everything behind b
    is integer arithmetic, so an output byte is decided exactly, or is one of the two candidates pushed through the integer blend — the same
    candidate in every pane of the pixel's channel;
  * arg where the float64 top-two logits are closer than seg_ref.TIE_GAP: either of the two top classes (at an exact tie the two LOWEST indices among
    the maxima) is accepted, the same one in every pane of the pixel and in pred.
The shares of such bytes and pixels are capped per case (recon_panel_ref.BORDERLINE_CAP, seg_ref.TIE_CAP): conditions on the inputs, not tolerances."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import recon_eval_ref as E
import recon_panel_ref as P
import seg_ref as R

PANES = ("image", "gt", "pred", "gt_over", "pred_over", "errors")
NEEDS_LABELS = (1, 3, 5)
IGNORE_RGB = (224, 224, 192)
RED = (255, 0, 0)
LABEL_PATTERNS = R.PATTERNS + (None,)          # None: labels=None
CHANNELS = (3, 1, 4)                           # bands (0, 1, 2), (0, 0, 0), (3, 1, 0): recon_panel_ref.BANDS
ALPHAS = (0.0, 0.5, 1.0)
GAPS = (0, 2)
PANE_SETS = ((5,), (0, 1, 2, 3, 4, 5), (0, 3, 4), (3, 1, 5, 2))          # with labels: a single pane, all six, the default, the rest reordered
PANE_SETS_UNLABELLED = ((2,), (4, 2, 0, 0, 2, 4), (0, 2, 4))             # without: only the panes that show no label


def _combos():
    """seg_ref.CASES x the label patterns x the channel counts; alpha, gap and the pane set cycle underneath, so that each of the 15 combinations of a
    case sees every alpha, both gaps and every pane set its labels allow."""
    out = []
    for case in R.CASES:
        for pattern in LABEL_PATTERNS:
            for C in CHANNELS:
                i = len(out)
                sets = PANE_SETS if pattern is not None else PANE_SETS_UNLABELLED
                out.append((case, pattern, C, ALPHAS[i % 3], GAPS[(i // 3) % 2], sets[(i // 2) % len(sets)]))
    return tuple(out)


COMBOS = _combos()


def combo_id(combo):
    case, pattern, C, alpha, gap, panes = combo
    return "N%d-G%d-p%d-K%d" % case + f"-{pattern or 'nolabels'}-C{C}-a{alpha:g}-g{gap}-p" + "".join(map(str, panes))


def a8_of(alpha):
    return int(round(256.0 * alpha))


def voc_palette(K):
    """The PASCAL-VOC colour map, restated: bit 0 / 1 / 2 of each 3-bit group of the index -> red / green / blue, first group to the top bit."""
    pal = np.zeros((K, 3), dtype=np.uint8)
    for k in range(K):
        c, r, g, b = k, 0, 0, 0
        for j in range(8):
            r |= (c & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal[k] = (r, g, b)
    return pal


def combo_inputs(combo):
    """The operands of a combination (shared: do not write to them): img / mean / std of recon_eval_ref.inputs, pl / labels of seg_ref.case_inputs."""
    (N, G, p, K), pattern, C, alpha, gap, panes = combo
    o = E.inputs(N, C, G * p, p)
    pl, labels = R.case_inputs(N, G, p, K, pattern or "random")
    return dict(img=o["img"], mean=o["mean"], std=o["std"], bands=P.BANDS[C], pl=pl, labels=None if pattern is None else labels, palette=voc_palette(K), p=p,
                panes=panes, gap=gap, a8=a8_of(alpha), ignore_rgb=IGNORE_RGB)


def with_stray_labels(labels, K):
    """Labels with values in [K, 255) planted (the pattern of test_segprobe_gpu's stray-label test)."""
    out = labels.clone()
    out[0, ::3, ::2] = 254
    out[-1, 1::4, :] = K
    return out


def with_exact_ties(pl):
    """Logits whose image 0 is all zeros: every pixel there is a K-way exact tie, so arg is 0 and the accepted pair is (0, 1)."""
    out = pl.clone()
    out[0] = 0.0
    return out


# ------------------------------------------------------------------------------------------------ the float64 side
def image_bytes(img, mean, std, p, bands):
    """-> (lo, hi) int64 [N, S, S, 3]: the displayed byte's two candidates under recon_panel_ref's bound (equal where the byte is decided)."""
    N, C, S, _ = img.shape
    L = (S // p) ** 2
    ref = P.reference(img, torch.zeros(N, L, p * p * C), torch.zeros(N, L), mean, std, p, (0,), 0, bands)
    tobyte = lambda t: np.floor(np.clip(t, 0.0, 255.0)).astype(np.int64)   # noqa: E731
    return tobyte(ref["v255"] - ref["delta"]), tobyte(ref["v255"] + ref["delta"])


def top_two(pl, p):
    """-> arg, arg2 int64 [N, S, S] (the lowest index among the maxima; the lowest index among the maxima of the rest) and tie (float64 gap < TIE_GAP)"""
    z = R.upsample(pl.double(), p).numpy()
    arg = z.argmax(-1)                     # (numpy: the first occurrence)
    top = np.take_along_axis(z, arg[..., None], -1)[..., 0]
    rest = z.copy()
    np.put_along_axis(rest, arg[..., None], -np.inf, -1)
    arg2 = rest.argmax(-1)
    second = np.take_along_axis(rest, arg2[..., None], -1)[..., 0]
    return arg, arg2, (top - second) < R.TIE_GAP


def compose(b, arg, labels, K, palette, panes, gap, a8, ignore_rgb, defect=None):
    """The integer rule: bytes b [N, S, S, 3], classes arg [N, S, S], labels [N, S, S] or None -> uint8 [N, S, W, 3].  `defect`: see DEFECTS."""
    N, S = arg.shape[:2]
    b = np.asarray(b, dtype=np.int64)
    lab = np.full((N, S, S), 255, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    if defect == "ignore_as_class":
        lab = np.where(lab == 255, K - 1, lab)
    if defect == "stray_as_class":
        lab = np.where((lab >= K) & (lab < 255), lab % K, lab)
    valid = (lab < K)[..., None]
    pal, ign, red = np.asarray(palette, dtype=np.int64), np.asarray(ignore_rgb, dtype=np.int64), np.asarray(RED, dtype=np.int64)
    col_l = np.where(valid, pal[np.clip(lab, 0, K - 1)], ign)
    col_p = pal[arg]
    half = 0 if defect == "blend_truncates" else 128
    blend = lambda x, c: (x * (256 - a8) + c * a8 + half) >> 8   # noqa: E731
    wrong = (arg != lab)[..., None]
    marked = np.where(wrong, blend(b, red), b)
    errors = marked if defect == "errors_on_ignored" else np.where(valid, marked, blend(b, ign))
    pane = {0: b, 1: col_l, 2: col_p, 3: blend(b, col_l), 4: blend(b, col_p), 5: errors}
    W = P.sheet_width(S, len(panes), gap)
    step = S + gap - (1 if defect == "gap_short" and gap > 0 else 0)
    out = np.full((N, S, W, 3), 255, dtype=np.uint8)
    for k, code in enumerate(panes):
        v = np.broadcast_to(pane[code], (N, S, S, 3)).astype(np.uint8)
        out[:, :, k * step:k * step + S] = v[..., ::-1] if defect == "bgr" else v
    return out


def count_stats(arg, labels, K, defect=None):
    """int64 [N, K, 3]: (intersection, label area, prediction area) per image and class over the pixels whose label is < K."""
    N = arg.shape[0]
    lab = np.asarray(labels, dtype=np.int64).reshape(N, -1)
    a = np.asarray(arg, dtype=np.int64).reshape(N, -1)
    if defect == "stats_count_ignored":      # an ignored pixel counts as a right one
        lab = np.where(lab == 255, a, lab)
    out = np.zeros((N, K, 3), dtype=np.int64)
    for n in range(N):
        v = lab[n] < K
        out[n, :, 0] = np.bincount(a[n][v & (a[n] == lab[n])], minlength=K)
        out[n, :, 1] = np.bincount(lab[n][v], minlength=K)
        out[n, :, 2] = np.bincount(a[n] if defect == "pred_area_all_pixels" else a[n][v], minlength=K)
    return out


def reference(img, pl, labels, mean, std, palette, p, panes, gap, bands, a8, ignore_rgb=IGNORE_RGB):
    """dict: byte / byte_hi uint8 [N, S, W, 3] (the decided value, or the borderline pair where they differ), alt / alt_hi (the same with the second top
    class: what a tie pixel may show instead), borderline and gap masks per byte, arg / arg2 / tie per pixel, stats (from arg), and the arguments
    `violations` needs."""
    K = pl.shape[-1]
    lo, hi = image_bytes(img, mean, std, p, bands)
    arg, arg2, tie = top_two(pl, p)
    lab = None if labels is None else labels.numpy()
    sheets = [compose(bb, aa, lab, K, palette, panes, gap, a8, ignore_rgb) for aa in (arg, arg2) for bb in (lo, hi)]
    S = arg.shape[1]
    is_gap = np.ones(sheets[0].shape, dtype=bool)
    for k in range(len(panes)):
        is_gap[:, :, k * (S + gap):k * (S + gap) + S] = False
    return dict(byte=sheets[0], byte_hi=sheets[1], alt=sheets[2], alt_hi=sheets[3], borderline=(sheets[0] != sheets[1]) & ~is_gap, gap=is_gap, arg=arg, arg2=arg2,
                tie=tie, stats=None if lab is None else count_stats(arg, lab, K), labels=lab, K=K, S=S, n_panes=len(panes), gap_px=gap)


def tie_share(ref):
    return float(ref["tie"].mean())


def borderline_share(ref):
    return float(ref["borderline"].mean())


def violations(got, ref):
    """Names of the checks a result misses against `reference`'s dict (empty: all hold).  got: dict(out=uint8 [N, S, W, 3][, pred=uint8 [N, S, S]][,
    stats=int [N, K, 3]]), or the sheet alone.  stats are held, exactly, to the counts of the result's own pred (of the float64 arg without one)."""
    if not isinstance(got, dict):
        got = dict(out=got)
    g = np.asarray(got["out"])
    if g.shape != ref["byte"].shape or g.dtype != np.uint8:
        return ["shape"]
    bad = []
    if not (g[ref["gap"]] == 255).all():
        bad.append("gap")
    S, step, tie = ref["S"], ref["S"] + ref["gap_px"], ref["tie"]
    shape = tie.shape + (3,)
    lo_a, hi_a, lo_b, hi_b = (np.ones(shape, dtype=bool) for _ in range(4))
    decided_ok, pair_ok = np.ones(shape, dtype=bool), np.ones(shape, dtype=bool)
    for k in range(ref["n_panes"]):
        sl = (slice(None), slice(None), slice(k * step, k * step + S))
        gk, a0, a1 = g[sl], ref["byte"][sl], ref["byte_hi"][sl]
        lo_a &= gk == a0
        hi_a &= gk == a1
        lo_b &= gk == ref["alt"][sl]
        hi_b &= gk == ref["alt_hi"][sl]
        decided_ok &= (a0 != a1) | (gk == a0)
        pair_ok &= (a0 == a1) | (gk == a0) | (gk == a1)
    ok_a, ok_b = (lo_a | hi_a).all(-1), (lo_b | hi_b).all(-1)     # (one candidate of b per channel, one class per pixel, in every pane)
    pred = None
    if got.get("pred") is not None:
        pred = np.asarray(got["pred"]).astype(np.int64)
        if pred.shape != tie.shape:
            return bad + ["pred_shape"]
        if not (pred[~tie] == ref["arg"][~tie]).all():
            bad.append("pred")
        if not ((pred == ref["arg"]) | (pred == ref["arg2"]))[tie].all():
            bad.append("pred_tie")
        ok_a &= pred == ref["arg"]
        ok_b &= pred == ref["arg2"]
    if not decided_ok[~tie].all():
        bad.append("decided")
    if not pair_ok[~tie].all():
        bad.append("borderline")
    if not ok_a[~tie].all() and "decided" not in bad and "borderline" not in bad and "pred" not in bad:
        bad.append("inconsistent")
    if not (ok_a | ok_b)[tie].all():
        bad.append("tie")
    if got.get("stats") is not None:
        if ref["labels"] is None:
            bad.append("stats_without_labels")
        else:
            want = count_stats(pred if pred is not None else ref["arg"], ref["labels"], ref["K"])
            s = np.asarray(got["stats"]).astype(np.int64)
            if s.shape != want.shape or not (s == want).all():
                bad.append("stats")
    return bad


# ------------------------------------------------------------------------------------------------ fp32 emulation (CPU self-check)
DEFECTS = ("align_corners", "tie_highest", "blend_truncates", "bgr", "ignore_as_class", "stray_as_class", "errors_on_ignored", "gap_short", "stats_count_ignored",
           "pred_area_all_pixels")


def emulate(img, pl, labels, mean, std, palette, p, panes, gap, bands, a8, ignore_rgb=IGNORE_RGB, defect=None):
    """The kernel's arithmetic in fp32 torch + the integer rule -> dict(out, pred, stats (None without labels)).  Defects: the logits are upsampled
    with align_corners=True; the highest index wins a tie; the blend drops its + 128; a pixel's bytes leave as blue, green, red; label 255 is shown
    and counted as class K - 1; a stray label in [K, 255) as class label % K; the errors pane marks ignored pixels red; pane k starts at
    k (S + gap - 1); an ignored pixel is counted as a right one; the prediction area counts every pixel."""
    N, C, S, _ = img.shape
    K = pl.shape[-1]
    mn, sd = mean.float()[None, :, None, None], std.float()[None, :, None, None]
    X = (img.float() * sd + mn)[:, list(bands)].permute(0, 2, 3, 1) * torch.tensor(255.0)
    b = X.clamp(0.0, 255.0).to(torch.int32).numpy().astype(np.int64)
    z = F.interpolate(pl.float().permute(0, 3, 1, 2), size=(S, S), mode="bilinear", align_corners=defect == "align_corners").permute(0, 2, 3, 1).numpy()
    arg = (K - 1 - z[..., ::-1].argmax(-1)) if defect == "tie_highest" else z.argmax(-1)
    lab = None if labels is None else labels.numpy()
    out = compose(b, arg, lab, K, palette, panes, gap, a8, ignore_rgb, defect)
    slab = lab
    if lab is not None and defect == "ignore_as_class":
        slab = np.where(lab == 255, K - 1, lab)
    if lab is not None and defect == "stray_as_class":
        slab = np.where((lab >= K) & (lab < 255), lab % K, lab)
    return dict(out=out, pred=arg.astype(np.uint8), stats=None if lab is None else count_stats(arg, slab, K, defect))


@functools.lru_cache(maxsize=None)
def combo_reference(combo):
    o = combo_inputs(combo)
    return reference(o["img"], o["pl"], o["labels"], o["mean"], o["std"], o["palette"], o["p"], o["panes"], o["gap"], o["bands"], o["a8"], o["ignore_rgb"])
