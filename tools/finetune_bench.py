#!/usr/bin/env python3
"""Throughput of a fine-tune step (trunk forward, pool + classifier + soft-target cross-entropy, the head's backward, the trunk's backward
with the position-embedding gradient, FusedAdamW over the layer-decay groups; mixup of images and targets included) against the trunk
forward alone (Engine.encode_stream at mask ratio 0) on the same batch.  Prints images/s of both, from HIP events around whole steps.

    python tools/finetune_bench.py [--model vit_base_patch16] [--batch 128] [--classes 62] [--dtype bf16|fp32] [--steps 20] [--warmup 5]
                                   [--no-mixup] [--trace-steps N]   # only run N steps after the warm-up (for a kernel trace of its own)
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
    ap.add_argument("--no-mixup", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import csmae_hip
    import models_vit
    import util.lr_decay as lrd
    from csmae_hip.optim import FusedAdamW
    from util.mixup import Mixup
    csmae_hip.load()
    torch.manual_seed(0)
    np.random.seed(0)
    m = models_vit.__dict__[a.model](img_size=a.input_size, patch_size=a.patch_size, num_classes=a.classes, global_pool=True).finetune_mode().cuda().train()
    m.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    m.smoothing = 0.1
    x = torch.randn(a.batch, 3, a.input_size, a.input_size, device="cuda")
    y = torch.randint(0, a.classes, (a.batch,), device="cuda")
    mix = None if a.no_mixup else Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=a.classes)
    state = {}

    def step():
        xs, ys = (x, y) if mix is None else mix(x, y)
        loss, _ = m(xs, ys)
        loss.backward()
        if "opt" not in state:   # (the parameters are homed in the flat buffer by the first forward)
            state["opt"] = FusedAdamW(lrd.param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75), lr=1e-4)
            for g in state["opt"].param_groups:
                g["lr"] = 1e-4 * g["lr_scale"]
        state["opt"].step()
        state["opt"].zero_grad()

    if a.trace_steps:
        for _ in range(a.warmup + a.trace_steps):
            step()
        torch.cuda.synchronize()
        return
    ms_step = timed(step, a.steps, a.warmup)
    eng = m._engine(x)
    ramp = m._bufs["ramp"]
    ms_trunk = timed(lambda: eng.encode_stream(x, 0.0, ramp), a.steps, a.warmup)
    print(f"{a.model} {a.input_size}^2/{a.patch_size} batch {a.batch} {a.dtype} K={a.classes} mixup={'off' if mix is None else 'on'} lib {csmae_hip.source_hash()[:12]}")
    print(f"fine-tune step       {ms_step:8.3f} ms  {a.batch / ms_step * 1e3:10.1f} images/s")
    print(f"trunk forward alone  {ms_trunk:8.3f} ms  {a.batch / ms_trunk * 1e3:10.1f} images/s")
    print(f"step / trunk forward: {ms_step / ms_trunk:5.2f} x")


if __name__ == "__main__":
    main()
