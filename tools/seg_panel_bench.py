#!/usr/bin/env python3
"""Cost of the overlay sheets of the segmentation probe (`csmae_segpanel`), on one GPU, at N 64, ViT-B/16 at 224 x 224 (G 14, p 16), K 16, with the
three default panes (image | ground truth over image | prediction over image), gap 2, alpha 0.5:

  kernel   `ops.seg_panel`: the sheets, the argmax map and the per-image counts of the whole batch in one launch, from the patch logits;
  torch    the sheets composed with torch ops: `F.interpolate` of the logits to [N, K, S, S] (the tensor the kernel never writes), argmax, two palette
           gathers, the image's bytes, two integer blends and a cat of the panes and the white gaps into [N, S, W, 3] (no counts);
  copy     a plain device-to-device copy of out's 3 N S W bytes: what merely moving the result costs.

Device events around single calls, the three alternating, medians over `--rounds` rounds with the spread (min .. max) beside them, each warmed up
first.  The kernel's bytes are compared with the torch composition's before anything is timed (they may differ where fp32 rounds the image's byte or a
near-tie the other way).  A measurement needs the GPU: there is no fallback.  No threshold anywhere: the file records what the machine gave.

    python tools/seg_panel_bench.py --out profiles/seg_panel_bench.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-scale-mae_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(v):
    return f"{statistics.median(v):9.4f}  ({min(v):.4f} .. {max(v):.4f})"


def torch_sheets(img, pl, labels, mean, std, palette, ignore_rgb, a8, panes, gap):
    """The kernel's sheets from torch ops -> uint8 [N, S, W, 3]."""
    N, C, S, _ = img.shape
    K = pl.shape[-1]
    arg = F.interpolate(pl.permute(0, 3, 1, 2), size=(S, S), mode="bilinear", align_corners=False).argmax(1)
    b = torch.clip((img.permute(0, 2, 3, 1) * std.view(1, 1, 1, C) + mean.view(1, 1, 1, C)) * 255, 0, 255).to(torch.int32)
    pal = torch.cat([palette.to(torch.int32), torch.tensor([ignore_rgb], dtype=torch.int32, device=img.device)])
    col_l = pal[torch.where(labels < K, labels.long(), torch.full_like(labels, K, dtype=torch.long))]
    col_p = pal[arg]
    blend = lambda x, c: (x * (256 - a8) + c * a8 + 128) >> 8   # noqa: E731
    white = torch.full((N, S, gap, 3), 255, dtype=torch.uint8, device=img.device)
    parts = []
    for k, code in enumerate(panes):
        if code == 5:
            valid, wrong = (labels < K).unsqueeze(-1), (arg != labels.long()).unsqueeze(-1)
            v = torch.where(valid, torch.where(wrong, blend(b, pal.new_tensor([255, 0, 0])), b), blend(b, pal[K]))
        else:
            v = {0: b, 1: col_l, 2: col_p}[code] if code < 3 else blend(b, col_l if code == 3 else col_p)
        if k and gap:
            parts.append(white)
        parts.append(v.to(torch.uint8))
    return torch.cat(parts, dim=2)


def bench(N, S, p, K, panes, gap, alpha, rounds, say):
    from csmae_hip import ops
    from util.seg_viz import IGNORE_RGB, default_palette
    g = torch.Generator(device="cuda").manual_seed(S + 7 * K + len(panes))
    G, C = S // p, 3
    mean, std = torch.full((C,), 0.42, device="cuda"), torch.full((C,), 0.19, device="cuda")
    img = (torch.rand(N, C, S, S, generator=g, device="cuda") - mean.view(1, C, 1, 1)) / std.view(1, C, 1, 1)
    pl = torch.randn(N, G, G, K, generator=g, device="cuda")
    labels = torch.randint(0, K, (N, S, S), generator=g, device="cuda").to(torch.uint8)
    labels[torch.rand(N, S, S, generator=g, device="cuda") < 0.03] = 255
    palette = torch.from_numpy(default_palette(K)).cuda()
    a8 = int(round(256 * alpha))
    P = len(panes)
    W = P * S + (P - 1) * gap
    out = torch.empty(N, S, W, 3, dtype=torch.uint8, device="cuda")
    pred = torch.empty(N, S, S, dtype=torch.uint8, device="cuda")
    stats = torch.empty(N, K, 3, dtype=torch.int32, device="cuda")
    src = torch.empty(out.numel(), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def kernel():
        ops.seg_panel(img, pl, labels, mean, std, palette, panes=panes, alpha=alpha, gap=gap, ignore_rgb=IGNORE_RGB, out=out, pred=pred, stats=stats)

    def sheets_only():
        ops.seg_panel(img, pl, labels, mean, std, palette, panes=panes, alpha=alpha, gap=gap, ignore_rgb=IGNORE_RGB, out=out)

    def composed():
        return torch_sheets(img, pl, labels, mean, std, palette, IGNORE_RGB, a8, panes, gap)

    def copy():
        dst.copy_(src)

    kernel()
    want = composed()
    off = float((out != want).float().mean())
    assert off < 1e-3, f"the kernel and the torch composition disagree on {off:.2e} of the bytes"
    for fn in (kernel, sheets_only, composed, copy):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t_k, t_s, t_t, t_c = [], [], [], []
    for _ in range(rounds):
        t_k.append(event_ms(kernel))
        t_s.append(event_ms(sheets_only))
        t_t.append(event_ms(composed))
        t_c.append(event_ms(copy))
    med = statistics.median
    written = out.numel()
    read = 4 * N * C * S * S + N * S * S + 4 * pl.numel()
    say(f"N {N}  S {S}  p {p}  K {K}  panes {tuple(panes)}  gap {gap}  alpha {alpha}  sheet {S} x {W}  bytes written {written / 1e6:.2f} MB (+ pred {pred.numel() / 1e6:.2f} MB), "
        f"read once {read / 1e6:.2f} MB  (kernel vs torch: {off:.1e} of the bytes differ)")
    say(f"    csmae_segpanel, out + pred + stats (one launch + one clear)  ms : {spread(t_k)}   {written / med(t_k) / 1e6:8.1f} GB/s of the bytes written")
    say(f"    csmae_segpanel, out alone (one launch)                       ms : {spread(t_s)}")
    say(f"    torch composition of the sheets (no counts)                  ms : {spread(t_t)}   ({med(t_t) / med(t_k):.2f} x the kernel)")
    say(f"    device-to-device copy of out's bytes                         ms : {spread(t_c)}   (the kernel takes {med(t_k) / med(t_c):.2f} x the copy)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--classes", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_panel_bench needs the GPU: nothing is measured without one")
    if args.rounds < 20:
        raise SystemExit("--rounds: at least 20 interleaved rounds")
    import csmae_hip
    csmae_hip.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"seg_panel_bench  device {torch.cuda.get_device_name(0)}  csrc {csmae_hip.source_hash()[:12]}")
    say(f"device events around single calls, kernel / torch / copy alternating, median (min .. max) over {args.rounds} rounds after 5 warm-up calls each")
    bench(args.batch, args.size, 16, args.classes, (0, 3, 4), 2, 0.5, args.rounds, say)
    bench(args.batch, args.size, 16, args.classes, (0, 1, 2, 3, 4, 5), 2, 0.5, args.rounds, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
