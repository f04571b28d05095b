#!/usr/bin/env python3
"""Search time of the k-NN evaluation at fMoW size on the GPU: bank 363 k, queries 53 k, D = 768 and 1024, k = 20, bf16 features (csmae_hip.knn.KnnIndex).

For each D: the whole search (normalise the queries, then per chunk pair one GEMM + one csmae_knn_select) timed end to end with device events,
median of --reps runs after a warm-up run; one more run under ops.KernelTimer, whose events around every launch split the time into GEMM and
select (the events themselves cost a few microseconds per launch: the split is a share, the end-to-end figure is the time).  As a yardstick
torch.topk(k) is timed on the same device tile the select kernel reads — here only; the product never calls it.  Features are random normal
vectors (the select's cost depends on how often a list changes, which for random data falls off as k / rows-seen, as for real features after
the first tiles); the first tile of a search, where every list fills, is timed on its own.

    python tools/knn_bench.py --out profiles/knn_bench.txt
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-scale-mae_amd"))

import torch  # noqa: E402


def timed(fn, reps):
    """Median and spread (ms, device events) of `reps` calls of fn()."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return "; ".join(ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln)[:400] or "not available"
    except Exception as e:   # noqa: BLE001
        return f"not available ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bank", type=int, default=363_000)
    ap.add_argument("--queries", type=int, default=53_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--q_chunk", type=int, default=4096)
    ap.add_argument("--b_chunk", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs the GPU: nothing is measured without one")
    import csmae_hip
    from csmae_hip import ops
    from csmae_hip.knn import KnnIndex
    csmae_hip.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/knn_bench.py  device {torch.cuda.get_device_name(0)}  torch {torch.__version__}  csrc {csmae_hip.source_hash()[:12]}")
    say(f"# clocks while idle before the run: {clocks()}")
    say(f"# bank {a.bank}  queries {a.queries}  k {a.k}  bf16 features, fp32 similarity tile {a.q_chunk} x {a.b_chunk} "
        f"({a.q_chunk * a.b_chunk * 4 / 2 ** 20:.0f} MiB)  timing: device events, median [min, max] of {a.reps} after one warm-up run")
    g = torch.Generator(device="cuda").manual_seed(0)
    for D in a.dims:
        bank = torch.randn(a.bank, D, device="cuda", generator=g)
        labels = torch.randint(0, 62, (a.bank,), device="cuda", generator=g)
        queries = torch.randn(a.queries, D, device="cuda", generator=g)
        index = KnnIndex(bank, labels, 62, dtype=torch.bfloat16)
        del bank
        run = lambda: index.search(queries, a.k, q_chunk=a.q_chunk, b_chunk=a.b_chunk)   # noqa: E731
        run()
        torch.cuda.synchronize()
        med, lo, hi = timed(run, a.reps)
        flops = 2.0 * a.queries * a.bank * D
        say(f"D {D}: search end to end {med:9.2f} ms [{lo:.2f}, {hi:.2f}]   ({flops / med / 1e9:.0f} TFLOP/s of similarity products over the whole search)")
        with ops.KernelTimer() as kt:
            run()
        s = kt.summary()
        gemm = sum(v["ms"] for kname, v in s.items() if kname.startswith("gemm"))
        sel = s["knn_select"]["ms"]
        launches = s["knn_select"]["launches"]
        say(f"D {D}: per-launch events  GEMM {gemm:9.2f} ms ({flops / gemm / 1e9:.0f} TFLOP/s)   select {sel:9.2f} ms "
            f"({s['knn_select']['work'] / sel / 1e9:.2f} TB/s of tile bytes)   {launches} launch pairs   select share of GEMM + select "
            f"{100 * sel / (gemm + sel):.1f} %   select / GEMM {sel / gemm:.2f}")
        # the yardstick on one device tile: a tile of a running search (lists already hold the best of the tiles before it) and the first tile
        nq, nb = min(a.q_chunk, a.queries), min(a.b_chunk, index.N)
        qn = index._scratch["qn"][: a.queries * D].view(a.queries, D)
        tile = torch.empty(nq, nb, device="cuda", dtype=torch.float32)
        ops.gemm(qn[:nq], index.bank[:nb], tile)
        val, idx = index.search(queries[:nq], a.k, q_chunk=a.q_chunk, b_chunk=a.b_chunk)
        val, idx = val.clone(), idx.clone()
        fresh_v = torch.full_like(val, float("-inf"))
        fresh_i = torch.full_like(idx, -1)
        steady = timed(lambda: ops.knn_select(tile, val, idx, base=0), 20)            # (re-offering tile 0 to full lists: nothing enters)
        def first():
            fresh_v.fill_(float("-inf")); fresh_i.fill_(-1)
            ops.knn_select(tile, fresh_v, fresh_i, base=0)
        first_t = timed(first, 20)
        topk = timed(lambda: torch.topk(tile, a.k, dim=1), 20)
        gemm_t = timed(lambda: ops.gemm(qn[:nq], index.bank[:nb], tile), 20)
        say(f"D {D}: one tile {nq} x {nb}:  GEMM {gemm_t[0]:.3f} ms   knn_select into full lists {steady[0]:.3f} ms ({nq * nb * 4 / steady[0] / 1e9:.2f} TB/s)   "
            f"knn_select first tile (incl. two fills) {first_t[0]:.3f} ms   torch.topk {topk[0]:.3f} ms")
        del index, queries, tile
        torch.cuda.empty_cache()
    say(f"# clocks after the run: {clocks()}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
