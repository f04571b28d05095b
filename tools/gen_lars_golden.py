#!/usr/bin/env python3
"""tests/golden/lars.npz: the reference's util/lars.py run in float64 on the CPU over the cases of tests/lars_cases.py (three steps each).

    python tools/gen_lars_golden.py --reference <checkout of the reference> [--out tests/golden/lars.npz]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lars_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lars.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_lars", os.path.join(args.reference, "util", "lars.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    stat = lambda t: np.array([t.double().norm().item(), t.double().sum().item()])
    for name, (shapes, wd, _, _) in C.CASES.items():
        params, grads = C.inputs(name)
        ps = [torch.nn.Parameter(p.double()) for p in params]
        opt = mod.LARS(ps, lr=C.LR, weight_decay=wd, momentum=C.MOMENTUM, trust_coefficient=C.TRUST)
        for i, p in enumerate(params):
            out[f"{name}_in_p{i}"] = stat(p)
        for step in range(C.STEPS):
            for i, (p, g) in enumerate(zip(ps, grads[step])):
                p.grad = g.double()
                out[f"{name}_in_g{step}_{i}"] = stat(g)
            opt.step()
            for i, p in enumerate(ps):
                idx = C.sample_index(p.numel())
                mu = opt.state[p]["mu"]
                out[f"{name}_s{step}_p{i}"] = p.detach().reshape(-1)[idx].numpy()
                out[f"{name}_s{step}_mu{i}"] = mu.reshape(-1)[idx].numpy()
                out[f"{name}_s{step}_pstat{i}"] = stat(p.detach())
                out[f"{name}_s{step}_mustat{i}"] = stat(mu)
    np.savez(args.out, **out)
    print(f"{args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
