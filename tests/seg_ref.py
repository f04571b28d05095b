"""fp64 restatement of the segmentation-probe kernels (csrc/segment.hip) with per-element error bounds, the test cases and their seeded inputs,
and guarded buffers for every dtype the kernels touch.  Nothing here imports the product.

Reference: torch.nn.functional.interpolate(mode="bilinear", align_corners=False) in fp64, cross_entropy(ignore_index=255, reduction="sum") / count,
autograd for the gradient, numpy.bincount for the confusion matrix, LayerNorm in fp64.

Bounds.  u = 2^-24 is the fp32 rounding unit.  Every bound below is first-order rounding analysis of the formula the header states, evaluated on
the fp64 reference's own intermediate values — never on a kernel's output.  The constants:

  upsampled logit  z = hy0 (hx0 a + hx1 b) + hy1 (hx0 c + hx1 d).  For p a power of two (every case here) the fractions are multiples of
      1 / (2 p) <= 1 / 32 and both weights of an axis are exact.  Each of the four terms then passes through at most 4 roundings (inner product, inner
      sum, outer product, outer sum; fused multiply-adds only remove some): |dz| <= CZ u sum w |v|, CZ = 5 (4 + room for second order).  sum w |v| is
      the upsampling of |pl|, since the weights are non-negative.
  pixel log-sum-exp  lse = log(sum_k exp(z_k - m)) + m, m = max_k z_k.  The argument z_k - m rounds once (u |z_k - m|), expf and logf are within
      2 ulp (the ROCm device library documents 1), the K-term sum of positive numbers adds (K - 1) u relative, the final sum rounds once; errors of the
      z_k propagate with the softmax weights (d lse / d z_k = P_k).  |d lse| <= sum_k P_k dz_k + u (max_k |z_k - m| + K + 2) + 2 u log K + u |lse|.
  pixel loss  l = lse - z_label: |dl| <= d lse + dz_label + u |l|.
  loss  = (sum of l over valid pixels) / count: a summation chain of `depth` additions contributes depth u sum |l|; depth is the longest chain of the
      kernel's documented order (a thread's strided pixels, 6 shuffle steps, 4 waves, then the same for the fold of the per-workgroup partials);
      the conversion of count and the division add 4 u |loss|.
  gradient  dpl = g / count * sum_pixels w (P_k - onehot), P_k = exp(z_k - lse).  w = wy wx is exact (multiples of 1 / 1024).  Per term:
      P_k carries the relative error u (|z_k - lse| + 2) + dz_k + d lse, the subtraction and the product round once each:
      |dt| <= w (P_k (u (|z_k - lse| + 2) + dz_k + d lse) + 2 u |P_k - onehot|).  The sum over the footprint is a chain of at most
      ceil(4 p^2 / slots) + slots additions, slots = 256 / (K rounded up to a power of two); the scaling adds 5 u |dpl|.
  LayerNorm  y = (x - mean) rstd gamma + beta with mean and the centred squares each summed over a chain of ceil(D / 64) + 8 additions and rsqrtf
      within 2 ulp: propagated term by term in ln_ref below."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
IGNORE = 255
CZ = 5.0
CASES = ((1, 1, 4, 2), (2, 2, 4, 5), (3, 3, 8, 21), (2, 4, 16, 64), (1, 14, 16, 16))   # (N, G, p, K)
PATTERNS = ("random", "ignore30", "image_ignored", "all_ignored")
TIE_GAP = 1e-4        # pixels whose fp64 top-two logits are closer than this are left out of the exact comparisons
TIE_CAP = 1e-3        # ... and may be at most this share of a case's pixels
SEG_CE_BLOCKS = 1024  # csrc/segment.hip: the forward's grid cap


# ------------------------------------------------------------------------------------------------ guarded buffers
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8, torch.int64: torch.int64}
_SENTINEL = {torch.float32: 0x7FC0BEEF, torch.bfloat16: 0x7FC5, torch.uint8: 0xA5, torch.int64: 0x7EADBEEF7EADBEEF}


class Guarded:
    """A contiguous tensor of `shape` inside a larger flat allocation with 256 bytes of sentinel elements on both sides (NaN patterns for the float
    types); the view starts 256-byte aligned and is prefilled with the sentinel unless `fill` is given."""

    def __init__(self, shape, dtype, device="cuda", fill=None):
        es = torch.empty(0, dtype=dtype).element_size()
        self.g = 256 // es
        self.n = int(np.prod(shape))
        self.sentinel = _SENTINEL[dtype]
        self.ibase = torch.full((2 * self.g + self.n + (-self.n) % self.g,), self.sentinel, dtype=_INT[dtype], device=device)
        self.t = self.ibase.view(dtype)[self.g:self.g + self.n].view(*shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0
        if fill is not None:
            self.t.copy_(fill.to(device=device, dtype=dtype))

    def outside_intact(self):
        return bool((self.ibase[:self.g] == self.sentinel).all()) and bool((self.ibase[self.g + self.n:] == self.sentinel).all())

    def unwritten(self):
        return int((self.ibase[self.g:self.g + self.n] == self.sentinel).sum())


def violations(got, want, bound):
    """-> (number of elements of `got` farther than `bound` from `want`, a message about the worst, the worst error / bound ratio)"""
    got, want, bound = got.detach().cpu().double().reshape(-1), want.double().reshape(-1), bound.double().reshape(-1)
    err = (got - want).abs()
    bad = ~(err <= bound)   # (a NaN counts as a violation)
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    i = int(torch.argmax((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")))) if err.numel() else 0
    return int(bad.sum()), f"element {i}: got {float(got[i]):.9g}, want {float(want[i]):.9g}, bound {float(bound[i]):.3g}", ratio


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def case_inputs(N, G, p, K, pattern, seed=0):
    """-> pl [N, G, G, K] fp32 ~ N(0, 1), labels [N, S, S] uint8"""
    S = G * p
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + 31 * G + 131 * p + 977 * K)
    pl = torch.randn(N, G, G, K, generator=g, dtype=torch.float32)
    labels = torch.randint(0, K, (N, S, S), generator=g).to(torch.uint8)
    if pattern == "ignore30":
        labels[torch.rand(N, S, S, generator=g) < 0.3] = IGNORE
    elif pattern == "image_ignored":
        labels[0] = IGNORE
    elif pattern == "all_ignored":
        labels[:] = IGNORE
    else:
        assert pattern == "random"
    return pl, labels


# ------------------------------------------------------------------------------------------------ bilinear upsampling
def upsample(pl, p):
    """[N, G, G, K] -> [N, S, S, K] in the dtype of pl (fp64 for the reference)"""
    G = pl.shape[1]
    up = F.interpolate(pl.permute(0, 3, 1, 2), size=(G * p, G * p), mode="bilinear", align_corners=False)
    return up.permute(0, 2, 3, 1)


def adjoint(X, G, p):
    """sum over pixels of w(pixel, cell) X[pixel]: [N, S, S, K] -> [N, G, G, K] (the transpose of `upsample`, by autograd)"""
    z = torch.zeros(X.shape[0], G, G, X.shape[3], dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(upsample(z, p), z, grad_outputs=X.double())[0]


def axis_weights(G, p):
    """[S, G] fp64: row i holds the weights output position i gives to the G cells of its axis (from the stated rule, not from torch)"""
    S = G * p
    W = torch.zeros(S, G, dtype=torch.float64)
    for i in range(S):
        src = max((i + 0.5) / p - 0.5, 0.0)
        i0 = min(int(math.floor(src)), G - 1)
        i1 = min(i0 + 1, G - 1)
        f = src - i0
        W[i, i0] += 1.0 - f
        W[i, i1] += f
    return W


# ------------------------------------------------------------------------------------------------ cross-entropy
def fwd_depth(npix):
    blocks = min(-(-npix // 256), SEG_CE_BLOCKS)
    return -(-npix // (blocks * 256)) + 6 + 4 + -(-blocks // 256) + 6 + 4


def bwd_depth(p, K):
    kp = 2
    while kp < K:
        kp *= 2
    slots = 256 // kp
    return -(-(4 * p * p) // slots) + slots


@functools.lru_cache(maxsize=None)
def _ce_ref_cached(N, G, p, K, pattern, seed, gscale):
    pl, labels = case_inputs(N, G, p, K, pattern, seed)
    return ce_ref(pl, labels, p, gscale)


def ce_case_ref(N, G, p, K, pattern, seed=0, gscale=1.0):
    return _ce_ref_cached(N, G, p, K, pattern, seed, gscale)


def ce_ref(pl, labels, p, gscale=1.0):
    """fp64 reference of csmae_seg_ce / _bwd for fp32 logits pl [N, G, G, K] and uint8 labels [N, S, S], with the bounds of the module docstring.
    -> dict: loss, b_loss, count, dpl, b_dpl, conf [K, K] int64 (near-tie pixels left out), arg [N, S, S] int64, tie [N, S, S] bool."""
    assert p in (4, 8, 16), "the bounds assume exact interpolation weights: p a power of two"
    N, G, _, K = pl.shape
    S = G * p
    u = U32
    x = pl.double().requires_grad_(True)
    z = upsample(x, p)                                  # [N, S, S, K]
    lab = labels.long()
    valid = lab != IGNORE
    count = int(valid.sum())
    total = F.cross_entropy(z.reshape(-1, K), lab.reshape(-1), ignore_index=IGNORE, reduction="sum")   # (ce_loss below, with z kept for the bounds)
    if count:
        loss = total / count
        dpl = torch.autograd.grad(loss, x)[0] * gscale
    else:
        loss, dpl = torch.zeros((), dtype=torch.float64), torch.zeros_like(x)
    z = z.detach()
    # ---- bounds
    absz = upsample(pl.double().abs(), p)
    ez = CZ * u * absz                                  # [N, S, S, K]
    m = z.max(-1, keepdim=True).values
    lse = torch.logsumexp(z, -1, keepdim=True)
    P = torch.exp(z - lse)
    e_lse = (P * ez).sum(-1, keepdim=True) + u * ((z - m).abs().max(-1, keepdim=True).values + K + 2) + 2 * u * math.log(K) + u * lse.abs()
    onehot = torch.zeros_like(z)
    onehot.scatter_(-1, lab.clamp(max=K - 1).unsqueeze(-1), 1.0)
    onehot = onehot * valid.unsqueeze(-1)
    l = (lse.squeeze(-1) - (z * onehot).sum(-1)) * valid
    e_l = (e_lse.squeeze(-1) + (ez * onehot).sum(-1) + u * l.abs()) * valid
    if count:
        b_loss = (e_l.sum() + fwd_depth(N * S * S) * u * l.abs().sum()) / count + 4 * u * loss.detach().abs()
        vmask = valid.unsqueeze(-1).double()
        e_t = vmask * (P * (u * ((z - lse).abs() + 2) + ez + e_lse) + 2 * u * (P - onehot).abs())
        b_dpl = abs(gscale) * (adjoint(e_t, G, p) + bwd_depth(p, K) * u * adjoint(vmask * (P - onehot).abs(), G, p)) / count + 5 * u * dpl.abs()
    else:
        b_loss, b_dpl = torch.zeros((), dtype=torch.float64), torch.zeros_like(dpl)
    # ---- exact outputs
    top2 = z.topk(2, dim=-1).values
    tie = (top2[..., 0] - top2[..., 1]) < TIE_GAP
    arg = z.argmax(-1)
    keep = (valid & ~tie).reshape(-1).numpy()
    idx = (lab.reshape(-1).numpy()[keep] * K + arg.reshape(-1).numpy()[keep]).astype(np.int64)
    conf = torch.from_numpy(np.bincount(idx, minlength=K * K).reshape(K, K).astype(np.int64))
    return dict(loss=loss.detach(), b_loss=b_loss, count=count, dpl=dpl.detach(), b_dpl=b_dpl, conf=conf, arg=arg, tie=tie)


def ce_loss(pl64, labels, p):
    """The loss alone, differentiable: fp64 patch logits [N, G, G, K] -> sum over valid pixels / count (0 without a valid pixel)"""
    K = pl64.shape[3]
    lab = labels.long()
    count = int((lab != IGNORE).sum())
    total = F.cross_entropy(upsample(pl64, p).reshape(-1, K), lab.reshape(-1), ignore_index=IGNORE, reduction="sum")
    return total / count if count else total * 0.0


def conf_labels(labels, tie):
    """The labels a kernel is given for the confusion-matrix check: near-tie pixels are marked ignored, so both sides leave them out."""
    out = labels.clone()
    out[tie] = IGNORE
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm of the patch tokens
def ln_inputs(N, T, D, dtype, seed=0):
    g = torch.Generator().manual_seed(5000 + 100 * seed + N + 17 * T + 257 * D)
    x = (torch.randn(N, T, D, generator=g) * 1.5 + 0.3 * torch.randn(N, T, 1, generator=g)).to(dtype)   # (rounded to the kernel's input type first)
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    return x, gamma, beta


def ln_ref(x, gamma, beta, eps=1e-6):
    """fp64 LayerNorm of the patch rows x[:, 1:] of x [N, T, D] (values as the kernel reads them) -> y [N (T-1), D], bound [N (T-1), D]"""
    u = U32
    N, T, D = x.shape
    v = x[:, 1:].double().reshape(N * (T - 1), D)
    g, b = gamma.double(), beta.double()
    depth = -(-D // 64) + 8
    mean = v.mean(1, keepdim=True)
    e_mean = (depth + 1) * u * v.abs().mean(1, keepdim=True)
    c = v - mean
    e_c = e_mean + u * c.abs()
    var = (c * c).mean(1, keepdim=True)
    e_var = ((2 * c.abs() * e_c + u * c * c).sum(1, keepdim=True) + depth * u * (c * c).sum(1, keepdim=True)) / D + u * var
    r = 1.0 / torch.sqrt(var + eps)
    e_r = r * (0.5 * (e_var / (var + eps) + u) + 2 * u)
    y = c * r * g + b
    bound = g.abs() * (c.abs() * e_r + r * e_c) + 3 * u * (c * r * g).abs() + u * y.abs()
    return y, bound
