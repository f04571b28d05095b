"""LARS for linear probing (reference util/lars.py, MoCo v3's rule): no rate scaling or weight decay for parameters with ndim <= 1.
Same constructor, param-group keys and state layout (`state[p]["mu"]`) as the reference; `step()` is one csmae_lars_step call per
param group — a partial-norm launch and an apply launch over a pointer table, the learning rate a kernel argument, nothing read back."""
import torch


class LARS(torch.optim.Optimizer):
    def __init__(self, params, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001):
        defaults = dict(lr=lr, weight_decay=weight_decay, momentum=momentum, trust_coefficient=trust_coefficient)
        super().__init__(params, defaults)
        self._plans = {}

    @torch.no_grad()
    def step(self, closure=None, gate=None):
        """gate: optional device scalar (the step's loss); a non-finite value turns the launches into no-ops (csmae_adamw's convention)."""
        from csmae_hip import ops
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, g in enumerate(self.param_groups):
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            mus = []
            for p in ps:
                if not p.is_cuda:
                    raise RuntimeError("util.lars.LARS steps GPU tensors: the MI355X path has no CPU fallback")
                if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                    raise RuntimeError("util.lars.LARS needs contiguous fp32 parameters and gradients")
                st = self.state[p]
                if "mu" not in st:
                    st["mu"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                mus.append(st["mu"])
            key = tuple((p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), p.numel()) for p, m in zip(ps, mus))
            plan = self._plans.get(gi)
            if plan is None or plan[0] != key:   # (a gradient re-allocated by zero_grad(set_to_none=True), a loaded state: new addresses)
                plan = self._plans[gi] = (key, ops.lars_table(ps, [p.grad for p in ps], mus),
                                          torch.empty(len(ps) * ops.LARS_NORM_FLOATS, device=ps[0].device, dtype=torch.float32))
            ops.lars_step(plan[1], plan[2], g["lr"], g["weight_decay"], g["momentum"], g["trust_coefficient"], gate=gate)
        return loss
