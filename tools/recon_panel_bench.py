#!/usr/bin/env python3
"""Cost of the reconstruction contact sheets of a batch (`csmae_recon_panel`), on one GPU, at N 64, S 224, p 16:

  kernel   `ops.recon_panel`: the sheets of the whole batch in one launch, straight from the image, the patch rows and the mask;
  torch    the same bytes composed with torch ops: un-patchify the prediction (a reshape and a permute), un-normalise both operands, expand the
           mask to pixels, form each panel, clip(255 v, 0, 255), .to(uint8), and cat the panels and the white gaps into [N, S, W, 3];
  copy     a plain device-to-device copy of as many bytes as the kernel moves (half read, half written): the ceiling of a memory-bound kernel.

for 3 channels with 3 panels, for the 4-band input (bands 3, 1, 0) and for all 5 panels; the prediction in bf16 as the models return it under
autocast, and in fp32.  Bytes moved are counted from the shapes: every shown channel of the image (4 bytes) and of the prediction, each once, plus
the 3 W S bytes written — what the kernel needs, not what the cache lets it re-read.  Device events around single calls, the three alternating,
medians over `--rounds` rounds with the spread (min .. max) beside them, every shape warmed up first.  The kernel's bytes are compared with the
torch composition's before anything is timed.  A measurement needs the GPU: there is no fallback.  No threshold anywhere: the file records what
the machine gave.

    python tools/recon_panel_bench.py --out profiles/recon_panel_bench.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-scale-mae_amd"))

import torch  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(v):
    return f"{statistics.median(v):9.4f}  ({min(v):.4f} .. {max(v):.4f})"


def torch_sheets(img, pred, mask, mean, std, p, panels, gap, bands):
    """The kernel's result from torch ops -> uint8 [N, S, W, 3]."""
    N, C, S, _ = img.shape
    G = S // p
    sel = list(bands)
    m, s = mean[sel].view(1, 1, 1, 3), std[sel].view(1, 1, 1, 3)
    X = img[:, sel].permute(0, 2, 3, 1) * s + m
    Y = pred.float().reshape(N, G, G, p, p, C).permute(0, 1, 3, 2, 4, 5).reshape(N, S, S, C)[..., sel] * s + m
    mk = mask.view(N, G, 1, G, 1, 1).expand(N, G, p, G, p, 1).reshape(N, S, S, 1)
    white = torch.full((N, S, gap, 3), 255, dtype=torch.uint8, device=img.device)
    parts = []
    for k, code in enumerate(panels):
        v = X if code == 0 else X * (1 - mk) if code == 1 else Y if code == 2 else Y * mk if code == 3 else X * (1 - mk) + Y * mk
        if k and gap:
            parts.append(white)
        parts.append(torch.clip(v * 255, 0, 255).to(torch.uint8))
    return torch.cat(parts, dim=2)


def bench(N, C, S, p, panels, gap, bands, dtype, rounds, say):
    from csmae_hip import ops
    g = torch.Generator(device="cuda").manual_seed(S + 7 * C + len(panels))
    L, P = (S // p) ** 2, p * p * C
    mean, std = torch.full((C,), 0.42, device="cuda"), torch.full((C,), 0.19, device="cuda")
    img = (torch.rand(N, C, S, S, generator=g, device="cuda") - mean.view(1, C, 1, 1)) / std.view(1, C, 1, 1)
    pred = ((torch.rand(N, L, P, generator=g, device="cuda") * 1.1 - 0.05 - 0.42) / 0.19).to(dtype)
    mask = (torch.rand(N, L, generator=g, device="cuda") < 0.75).float()
    K = len(panels)
    W = K * S + (K - 1) * gap
    out = torch.empty(N, S, W, 3, dtype=torch.uint8, device="cuda")
    shown = len(set(bands))
    moved = N * (shown * S * S * (4 + pred.element_size()) + 4 * L + 3 * W * S)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def kernel():
        ops.recon_panel(img, pred, mask, mean, std, p, panels=panels, gap=gap, bands=bands, out=out)

    def composed():
        return torch_sheets(img, pred, mask, mean, std, p, panels, gap, bands)

    def copy():
        dst.copy_(src)

    kernel()
    want = composed()
    diff = (out.int() - want.int()).abs()
    off = float((diff > 0).float().mean())
    assert int(diff.max()) <= 1 and off < 1e-3, f"the kernel and the torch composition disagree: max |difference| {int(diff.max())}, share of bytes {off:.2e}"
    for fn in (kernel, composed, copy):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t_k, t_t, t_c = [], [], []
    for _ in range(rounds):
        t_k.append(event_ms(kernel))
        t_t.append(event_ms(composed))
        t_c.append(event_ms(copy))
    gbs = lambda t: moved / statistics.median(t) / 1e6   # noqa: E731
    say(f"N {N}  C {C}  S {S}  p {p}  panels {tuple(panels)}  gap {gap}  bands {tuple(bands)}  pred {str(dtype).split('.')[-1]}  sheet {S} x {W}  "
        f"bytes moved {moved / 1e6:.2f} MB  (kernel vs torch: {off:.1e} of the bytes differ, by 1)")
    say(f"    csmae_recon_panel (one launch)                 ms : {spread(t_k)}   {gbs(t_k):8.1f} GB/s of the bytes moved")
    say(f"    torch composition of the same bytes            ms : {spread(t_t)}   {gbs(t_t):8.1f} GB/s   ({statistics.median(t_t) / statistics.median(t_k):.2f} x the kernel)")
    say(f"    device-to-device copy of the same bytes        ms : {spread(t_c)}   {gbs(t_c):8.1f} GB/s   (kernel at {statistics.median(t_c) / statistics.median(t_k):.2f} of it)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recon_panel_bench needs the GPU: nothing is measured without one")
    if args.rounds < 20:
        raise SystemExit("--rounds: at least 20 interleaved rounds")
    import csmae_hip
    csmae_hip.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"recon_panel_bench  device {torch.cuda.get_device_name(0)}  csrc {csmae_hip.source_hash()[:12]}")
    say(f"device events around single calls, kernel / torch / copy alternating, median (min .. max) over {args.rounds} rounds after 5 warm-up calls each")
    N, S = args.batch, args.size
    for dtype in (torch.bfloat16, torch.float32):
        bench(N, 3, S, 16, (0, 1, 2), 2, (0, 1, 2), dtype, args.rounds, say)
        bench(N, 4, S, 16, (0, 1, 2), 2, (3, 1, 0), dtype, args.rounds, say)
        bench(N, 3, S, 16, (0, 1, 2, 3, 4), 2, (0, 1, 2), dtype, args.rounds, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
