#!/usr/bin/env python3
"""Throughput of the multispectral input kernels (`augment_u16`, `eval_u16`; csrc/multispectral.hip) on resident EuroSAT-sized batches: 64 x 64 x 13
uint16 tiles to S = 64 / 96 / 224, all 13 bands kept.  Per size and kernel: images/s (kernel alone, source resident), and the bytes the transform
has to move (the tiles read once, the fp32 output written once) over the time a plain `copy_` takes for the same number of bytes read + written.
`--rounds` alternating windows of `--iters` launches each, timed with device events after a warm-up; medians with min / max.  One JSON line per size.
    python tools/ms_input_bench.py [--n 512] [--iters 50] [--rounds 7] > profiles/ms_input_bench.txt"""
import argparse, json, os, statistics, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-scale-mae_amd"))
from csmae_hip import ops, source_hash
from util.gpu_input import eval_transform_params
from util.ms_input import band_plan

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512); ap.add_argument("--tile", type=int, default=64); ap.add_argument("--sizes", type=int, nargs="+", default=[64, 96, 224])
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ms_input_bench needs the GPU: there is nothing to time without one")


def clock_note():
    """The engine clock as rocm-smi reports it while the benchmark holds the device (read only); falls back to the property torch knows."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
        sclk = [ln.strip() for ln in out.splitlines() if "sclk" in ln]
        if sclk:
            return sclk[0]
    except Exception:
        pass
    return f"max engine clock {torch.cuda.get_device_properties(0).clock_rate / 1e3:.0f} MHz (current clock not read)"


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


T, C = a.tile, 13
g = torch.Generator().manual_seed(0)
src = torch.randint(0, 65536, (a.n, T, T, C), generator=g, dtype=torch.int32).to(torch.uint16).cuda()
band, mean, inv_std = band_plan(None, None)
band = torch.tensor(band, dtype=torch.int32)
mean, inv_std = torch.tensor(mean, dtype=torch.float32).cuda(), torch.tensor(inv_std, dtype=torch.float32).cuda()
print(json.dumps({"device": torch.cuda.get_device_name(0), "clock": clock_note(), "csrc": source_hash()[:12], "n": a.n, "tile": [T, T, C], "iters": a.iters,
                  "rounds": a.rounds, "timing": "device events around `iters` launches, 3 warm-up launches per kernel, windows of the three alternate"}))
for S in a.sizes:
    dst = torch.empty(a.n, C, S, S, device="cuda")
    metas = {"augment_u16": torch.tensor([(T, T, 0, 0, T, T, 0, 0)] * a.n, dtype=torch.int32).cuda(),
             "eval_u16": torch.tensor([eval_transform_params(T, T, S)] * a.n, dtype=torch.int32).cuda()}
    moved = src.numel() * 2 + dst.numel() * 4                    # bytes the transform has to read + write
    half = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"); other = torch.empty_like(half)   # a copy that reads + writes `moved` bytes
    fns = {"augment_u16": lambda: ops.augment_u16(src, metas["augment_u16"], band, mean, inv_std, dst),
           "eval_u16": lambda: ops.eval_u16(src, metas["eval_u16"], band, mean, inv_std, dst),
           "copy": lambda: other.copy_(half)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, a.iters))
    out = {"S": S, "bytes_moved_mb": round(moved / 2 ** 20, 1), "copy_us": round(statistics.median(times["copy"]) * 1e6, 1),
           "copy_gbps": round(moved / statistics.median(times["copy"]) / 1e9, 1)}
    for k in ("augment_u16", "eval_u16"):
        med = statistics.median(times[k])
        out[f"{k}_images_per_s"] = round(a.n / med, 1)
        out[f"{k}_images_per_s_min_max"] = [round(a.n / max(times[k]), 1), round(a.n / min(times[k]), 1)]
        out[f"{k}_us"] = round(med * 1e6, 1)
        out[f"{k}_gbps_algorithmic"] = round(moved / med / 1e9, 1)
        out[f"{k}_over_copy_time"] = round(med / statistics.median(times["copy"]), 2)
    print(json.dumps(out))
