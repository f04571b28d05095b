#!/usr/bin/env python3
"""Cost of the batched reconstruction evaluation per evaluated image, on synthetic images with a ViT-B model (p 16, N 256, S 128 and 224):

  (a) loop    the loop a user had to write before: `run_one_image` + `calc_metric` for mse, mae, l1, l2, ssim, one image at a time
              (a batch-1 forward, a csmae_ssim_fwd pipeline with its host read, four reductions on CPU copies);
  (b) batch   `util.viz.eval_batch`, the inner step of `run_eval`: one forward of the whole batch and one `csmae_recon_eval`;
  kernels     `csmae_recon_eval` alone beside `csmae_ssim_fwd` (flags 3: operands as they are, signed) on the same batch.  The second is the
              kernel pipeline that existed before; it returns only the mean over the batch and needs the prediction as patch rows of X.

Host-clock times around a device synchronise for (a) and (b); device events around single calls for the kernels, the two alternating, medians
over `--rounds` rounds with the spread (min .. max) beside them.  Every shape is warmed up first.  A measurement needs the GPU: there is no
fallback.

    python tools/recon_eval_bench.py --out profiles/recon_eval_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-scale-mae_amd"))

import torch  # noqa: E402

NAMES = ["mse", "mae", "l1", "l2", "ssim"]
VIT_B = dict(dim_model=768, encoder_num_layers=12, encoder_num_heads=12, decoder_embed_dim=512, decoder_num_layers=8, decoder_num_heads=16)


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(v):
    return f"{statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})"


def bench_size(S, N, loop_images, rounds, dtype, say):
    import models_mae
    from csmae_hip import ops
    from util import metrics, viz
    torch.manual_seed(0)
    model = models_mae.MAE_ViT_Baseline(**VIT_B, input_size=S, patch_size="16", mask_ratio=0.75).cuda().eval()
    model.compute_dtype = dtype
    ds = viz.SyntheticEvalImages(N, S, 1)
    items = [ds[k] for k in range(N)]
    imgs = torch.stack([x for x, _ in items]).cuda()
    seeds = [s for _, s in items]
    mean = torch.as_tensor(viz.image_mean, dtype=torch.float32).cuda()
    std = torch.as_tensor(viz.image_std, dtype=torch.float32).cuda()
    hwc = [x.permute(1, 2, 0).double().numpy() for x, _ in items[:loop_images]]

    def loop():
        out = []
        for img, seed in zip(hwc, seeds):
            x, _, y, _, _ = viz.run_one_image(img, model, mask_seed=seed)
            out.append([metrics.calc_metric(x, y, n) for n in NAMES])
        return out

    def batch():
        got = viz.eval_batch(model, imgs, seeds, NAMES, mean, std)
        return {k: v.cpu() for k, v in got.items()}      # (the read at the end of a sweep, charged to every batch here)

    loop(), batch()                                        # warm-up of every shape of the timed windows
    t_loop = [sync_time(loop) / loop_images * 1e3 for _ in range(rounds)]
    t_batch = [sync_time(batch) / N * 1e3 for _ in range(rounds)]
    say(f"S {S}  N {N}  ViT-B p16  {str(dtype).replace('torch.', '')}   per evaluated image, ms: median (min .. max) over {rounds} rounds")
    say(f"  (a) loop  run_one_image + calc_metric x5, {loop_images} images : {spread(t_loop)}")
    say(f"  (b) batch eval_batch, one forward + one recon_eval          : {spread(t_batch)}")
    say(f"      ratio of the medians (a) / (b)                           : {statistics.median(t_loop) / statistics.median(t_batch):9.1f}")

    # the kernels alone, on the same batch: the prediction of one forward
    with torch.no_grad():
        noise, box = viz.mask_draws(model, seeds, imgs.device)
        pred = model._run(imgs, 0.75, noise, box)[1].float().contiguous()
    C, p = 3, 16
    L, P = (S // p) ** 2, p * p * C
    out = torch.empty(N, 4, device="cuda")
    part = torch.empty(ops.recon_eval_workspace_floats(N, C, S), device="cuda")
    # csmae_ssim_fwd compares planes as they are: it needs X = img * std + mean as an image and Y as patch rows with a cls row (what calc_ssim builds)
    X = (imgs * std[None, :, None, None] + mean[None, :, None, None]).contiguous()
    rows = torch.zeros(N, L + 1, P, device="cuda")
    rows[:, 1:] = (pred.view(N, L, p * p, C) * std + mean).reshape(N, L, P)
    ws = torch.empty(ops.ssim_workspace_floats(N, C, S, p, 1), device="cuda")
    terms = torch.empty(2, device="cuda")

    def fused():
        ops.recon_eval(imgs, pred, mean, std, p, out=out, ws=part)

    def parent():
        ops.ssim_fwd(1, False, X, None, rows.view(N * (L + 1), P), None, ws, terms, N, N, C, S, p, flags=3)

    for _ in range(5):
        fused(), parent()
    t_f, t_p = [], []
    for _ in range(max(rounds * 10, 50)):                  # alternating, one call per event pair
        t_f.append(event_ms(fused))
        t_p.append(event_ms(parent))
    gap = abs(float(out[:, 2].double().mean()) - (1.0 - float(terms[0])))
    byt = N * C * S * S * 8.0
    say(f"  kernels on the batch, ms per call: median (min .. max) over {len(t_f)} alternating calls")
    say(f"      csmae_recon_eval (per-image sse, sae, ssim; 2 launches)  : {spread(t_f)}   {byt / statistics.median(t_f) / 1e6:7.1f} GB/s of operand bytes")
    say(f"      csmae_ssim_fwd flags 3 (batch-mean ssim only; 10 launches): {spread(t_p)}")
    say(f"      ratio of the medians ssim_fwd / recon_eval                : {statistics.median(t_p) / statistics.median(t_f):9.2f}    |mean ssim gap| {gap:.2e}")
    del model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 224])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--loop_images", type=int, default=32, help="images the one-by-one loop is timed on")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recon_eval_bench needs the GPU: nothing is measured without one")
    import csmae_hip
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"recon_eval_bench  device {torch.cuda.get_device_name(0)}  csrc {csmae_hip.source_hash()[:12]}")
    for S in a.sizes:
        bench_size(S, a.batch, a.loop_images, a.rounds, torch.bfloat16 if a.dtype == "bf16" else torch.float32, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
