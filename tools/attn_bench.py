#!/usr/bin/env python3
"""Attention fwd/bwd micro-benchmark on the step's shapes (decoder: B=256,T=197,H=16,hd=32; encoder: B=256,T=50,H=12,hd=64; --huge14: the ViT-H/14 preset's).
--shape NAME,B,T,H,hd (repeatable) times other shapes; --hires the attention shapes of large inputs at 64 images per GPU (two views: B = 128) — ViT-B/16
decoder at 384^2 / 512^2, ViT-B/16 encoder at 512^2, ViT-H/14 encoder at mask 0.5 — and, for orientation, the decoder shapes both kernel families can run
(T = 197 and 257, head_dim 32) on the resident kernels and, through csmae_attn_stream_mode(2), on the streaming ones.  Each line names the route that ran.
With a library of an older revision (CSMAE_LIB_PATH) the mode switch does not exist: the shapes run that library's routing and the mode-2 lines are left out."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-scale-mae_amd"))
import csmae_hip  # noqa: E402
from csmae_hip import ops  # noqa: E402

SHAPES = [("dec", 256, 197, 16, 32), ("enc", 256, 50, 12, 64)]
if "--huge14" in sys.argv:   # ViT-H/14 at 256 per GPU (BASELINE.json configs[4]): encoder 65 tokens x 16 heads of 80, decoder 257 x 16 x 32
    sys.argv.remove("--huge14")
    SHAPES = [("h14 enc", 512, 65, 16, 80), ("h14 dec", 512, 257, 16, 32)]
HIRES = [("B/16 dec 384", 128, 577, 16, 32, 1), ("B/16 dec 512", 128, 1025, 16, 32, 1), ("B/16 enc 512", 128, 257, 12, 64, 1), ("H/14 enc m.5", 128, 129, 16, 80, 1),
         ("dec 224 resident", 128, 197, 16, 32, 1), ("dec 224 stream", 128, 197, 16, 32, 2), ("dec 256 resident", 128, 257, 16, 32, 1), ("dec 256 stream", 128, 257, 16, 32, 2)]
extra = "--hires" in sys.argv or "--shape" in sys.argv
if extra:
    SHAPES = []
    if "--hires" in sys.argv:
        sys.argv.remove("--hires")
        SHAPES += HIRES
    while "--shape" in sys.argv:
        i = sys.argv.index("--shape")
        f = sys.argv[i + 1].split(",")
        SHAPES.append((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), 1))
        del sys.argv[i:i + 2]
    has_mode = hasattr(csmae_hip.load(), "csmae_attn_stream_mode")
    ROUTES = {csmae_hip.ATTN_ROUTE_RESIDENT: "resident", csmae_hip.ATTN_ROUTE_STREAM: "stream", csmae_hip.ATTN_ROUTE_ANY: "any-length"}
for name, B, T, H, hd, *mode in SHAPES:
    route = ""
    if extra:
        if not has_mode and mode[0] != 1:
            continue
        if has_mode:
            ops.attn_stream_mode(mode[0])
            route = f" [{ROUTES[ops.attn_route(ops.BF16, T, hd)]}]"
        else:
            route = " [any-length]" if not ops.attn_resident(ops.BF16, T, hd) else " [resident]"
    D = H * hd
    qkv = torch.randn(B * T, 3 * D, device="cuda").to(torch.bfloat16)
    dout = torch.randn(B * T, D, device="cuda").to(torch.bfloat16)
    out = torch.empty(B * T, D, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, T, device="cuda")
    dqkv = torch.empty_like(qkv)
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    for fn, label, fl in ((lambda: ops.attn_fwd(qkv, out, lse, B, T, H, hd), "fwd", 4.0), (lambda: ops.attn_bwd(qkv, out, dout, lse, dqkv, B, T, H, hd), "bwd", 10.0)):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        print(f"attn {name} {label}{route}: {ms * 1e3:8.1f} us  {fl * B * H * T * T * hd / ms / 1e9:7.1f} TF/s (algorithmic)")
    if extra and has_mode:
        ops.attn_stream_mode(1)
