"""Inputs of the LARS golden vectors (tests/golden/lars.npz): shared by tools/gen_lars_golden.py, which runs the reference's util/lars.py on
them in float64, and tests/test_linprobe_gpu.py, which runs the HIP kernel on them in float32.  The full tensors do not fit a committed
file (1000 x 1024 floats per tensor and step), so the golden file holds, per case and step, the float64 result at `sample_index(n)` plus
its 2-norm and sum — and the norm and sum of the inputs, so that a torch build whose CPU generator drew other numbers fails loudly."""
import torch

LR, MOMENTUM, TRUST, STEPS = 0.3, 0.9, 0.001, 3

# name -> (shapes, weight decay, zero the first tensor's gradient, zero the first tensor itself)
CASES = {
    "k62_wd0": ([(62, 768), (62,)], 0.0, False, False),
    "k62_wd01": ([(62, 768), (62,)], 0.1, False, False),
    "k1000_wd0": ([(1000, 1024), (1000,)], 0.0, False, False),
    "k1000_wd01": ([(1000, 1024), (1000,)], 0.1, False, False),
    "zero_grad_wd0": ([(7, 33), (7,)], 0.0, True, False),      # |dp| = 0 -> q = 1
    "zero_param_wd01": ([(7, 33), (7,)], 0.1, False, True),    # |p| = 0 -> q = 1
}


def inputs(name):
    """-> (params, grads[step]) as float32 CPU tensors: the head's scale (weights ~ 2e-5 is the probe's init; here 0.02 so that weight decay matters)."""
    shapes, wd, zero_g, zero_p = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    params = [torch.randn(*s, generator=g) * 0.02 for s in shapes]
    grads = [[torch.randn(*s, generator=g) * 0.1 for s in shapes] for _ in range(STEPS)]
    if zero_p:
        params[0].zero_()
    if zero_g:
        for step in grads:
            step[0].zero_()
    return params, grads


def sample_index(n):
    """Every 521st element (a prime: walks every column and every 4-element group phase) plus the last 16."""
    idx = torch.cat([torch.arange(0, n, 521 if n > 4096 else 1), torch.arange(max(n - 16, 0), n)])
    return torch.unique(idx)
