#!/usr/bin/env python3
"""Throughput of a linear-probe step (frozen trunk + pool + BatchNorm + classifier + cross-entropy + head backward + LARS) against its
yardstick, the trunk alone (Engine.encode_stream at mask ratio 0) on the same batch.  Prints images/s of both and the share of the step
spent behind the last block, from HIP events around whole steps.

    python tools/linprobe_bench.py [--model vit_base_patch16] [--batch 128] [--classes 62] [--dtype bf16|fp32] [--steps 20] [--warmup 5]
                                   [--trace-steps N]   # only run N probe steps after the warm-up (for a kernel trace of its own)
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-scale-mae_amd"))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vit_base_patch16")
    ap.add_argument("--input_size", type=int, default=224)
    ap.add_argument("--patch_size", type=int, default=16)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=62)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args()
    import csmae_hip
    import models_vit
    from util.lars import LARS
    csmae_hip.load()
    torch.manual_seed(0)
    m = models_vit.__dict__[a.model](img_size=a.input_size, patch_size=a.patch_size, num_classes=a.classes, global_pool=True).probe_mode().cuda().train()
    m.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    x = torch.randn(a.batch, 3, a.input_size, a.input_size, device="cuda")
    y = torch.randint(0, a.classes, (a.batch,), device="cuda")
    opt = LARS(m.head.parameters(), lr=0.1)

    def step():
        loss, _ = m(x, y)
        loss.backward()
        opt.step(gate=loss.detach().reshape(1))
        opt.zero_grad(set_to_none=False)

    if a.trace_steps:
        for _ in range(a.warmup + a.trace_steps):
            step()
        torch.cuda.synchronize()
        return
    ms_step = timed(step, a.steps, a.warmup)
    eng = m._engine(x)
    ramp = m._bufs["ramp"]
    ms_trunk = timed(lambda: eng.encode_stream(x, 0.0, ramp), a.steps, a.warmup)
    print(f"{a.model} {a.input_size}^2/{a.patch_size} batch {a.batch} {a.dtype} K={a.classes} lib {csmae_hip.source_hash()[:12]}")
    print(f"probe step   {ms_step:8.3f} ms  {a.batch / ms_step * 1e3:10.1f} images/s")
    print(f"trunk alone  {ms_trunk:8.3f} ms  {a.batch / ms_trunk * 1e3:10.1f} images/s")
    print(f"behind the last block (pool + head + loss + LARS, host gaps included): {ms_step - ms_trunk:7.3f} ms = {100 * (ms_step - ms_trunk) / ms_step:5.2f} % of the step")


if __name__ == "__main__":
    main()
