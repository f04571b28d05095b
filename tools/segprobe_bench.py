#!/usr/bin/env python3
"""Time of the segmentation criterion, forward + backward, on the MI355X: `csmae_hip.ops.seg_ce` (csrc/segment.hip: bilinear upsampling inside the
loss kernel, gather backward) beside the torch composition it stands for (F.interpolate(bilinear, align_corners=False) + F.cross_entropy(
ignore_index=255) + autograd), on the same card, same inputs, at a probe batch of ViT-B/16: N = 64, G = 14, p = 16, K = 16.

Device events around `--iters` back-to-back calls after a warm-up; the two sides alternate over `--rounds` rounds and every round is printed, so
the spread is visible.  Bytes: the least traffic the criterion needs (labels + logits read, gradient written), not what either side moves.
No threshold: the torch composition is the yardstick.

    python tools/segprobe_bench.py [--out profiles/segprobe_bench.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-scale-mae_amd"))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segprobe_bench.txt"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segprobe_bench needs an MI355X: there is nothing to measure on a CPU")
    import csmae_hip
    from csmae_hip import ops
    N, G, p, K = 64, 14, 16, 16
    S = G * p
    g = torch.Generator(device="cuda").manual_seed(0)
    pl = torch.randn(N, G, G, K, device="cuda", generator=g)
    labels = torch.randint(0, K, (N, S, S), device="cuda", generator=g).to(torch.uint8)
    labels[torch.rand(N, S, S, device="cuda", generator=g) < 0.1] = 255
    loss, count, dpl = torch.empty(1, device="cuda"), torch.empty(1, device="cuda", dtype=torch.int64), torch.empty_like(pl)
    scratch = torch.empty(ops.SEG_CE_SCRATCH_FLOATS, device="cuda")
    lab64 = labels.long()
    plt = pl.clone().requires_grad_(True)

    def hip():
        ops.seg_ce(pl, labels, loss, count, dpl=dpl, scratch=scratch)

    def hip_fwd():
        ops.seg_ce(pl, labels, loss, count, scratch=scratch)

    def composition():
        plt.grad = None
        up = F.interpolate(plt.permute(0, 3, 1, 2), size=(S, S), mode="bilinear", align_corners=False)
        F.cross_entropy(up, lab64, ignore_index=255).backward()

    hip()
    composition()
    torch.cuda.synchronize()
    err = float((dpl - plt.grad).abs().max())
    for fn in (hip, hip_fwd, composition):
        for _ in range(a.warmup):
            fn()
    rows = []
    for r in range(a.rounds):
        rows.append((timed(hip, a.iters), timed(hip_fwd, a.iters), timed(composition, a.iters)))
    need = N * S * S + 2 * 4 * pl.numel()
    best = [min(c) for c in zip(*rows)]
    lines = [f"segprobe_bench: seg_ce forward + backward beside the torch composition, N={N} G={G} p={p} K={K} (S={S}), fp32, 10 % ignored",
             f"library source hash {csmae_hip.source_hash()[:16]}, device {torch.cuda.get_device_name(0)}, {a.iters} calls per timing after {a.warmup} warm-up calls",
             f"max |dpl - autograd gradient of the composition| = {err:.3e}",
             "round   seg_ce fwd+bwd [us]   seg_ce fwd [us]   torch composition fwd+bwd [us]"]
    lines += [f"{i:5d}   {h:19.1f}   {f:15.1f}   {c:30.1f}" for i, (h, f, c) in enumerate(rows)]
    lines += [f"best    {best[0]:19.1f}   {best[1]:15.1f}   {best[2]:30.1f}",
              f"composition / seg_ce (best of rounds): {best[2] / best[0]:.2f}x",
              f"least traffic of the criterion (labels + logits read, gradient written): {need / 1e6:.2f} MB -> {need / best[0] / 1e6:.3f} TB/s at the seg_ce time "
              "(whole-call rate over device events, launch gaps included; not a kernel's share of peak)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
