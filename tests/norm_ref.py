"""Helpers of the norm kernel tests (test_norm_gpu.py) and of their CPU self-check (test_norm_bounds_cpu.py): fp64 references of what
csrc/norm.hip computes, seeded inputs that make a mix-up of rows, columns or channels visible, per-element error bounds, contiguous
guarded buffers, and fp32 emulations of the kernels' arithmetic (honest, in two summation orders, and with seeded defects).

Bounds are derived from the operation with counted fp32 operations (u = 2^-24 each), never from a global maximum:
  - a sum whose longest chain of additions is k deep:  |err| <= k u sum |terms|.  k is counted from the kernel: a LayerNorm lane adds its
    4 NV values in a row and the wave folds 64 lanes in 6 steps (k = 4 NV + 6); a BatchNorm thread adds its share of the channel, the wave
    folds in 6 steps, the 16 waves are added in a row (k = share + 22);
  - mean~ = mean + e_mu, e_mu = (k u + DIV) mean|x|;  var~ + eps = (var + eps) (1 + theta), theta = (k + 4) u + DIV + e_mu^2 rstd^2
    (x - mean~ : u, its square: 3 u in all, the sum: k u, the division, the addition of eps; a shifted mean adds its square to the variance);
  - rstd~ = rstd (1 + e_rs), e_rs = theta / (2 (1 - theta)) + RSQRT (the derivative of x^-1/2, and the hardware's rsqrtf);
  - y = xhat gamma + beta:  |gamma| (rstd e_mu + |xhat| (e_rs + 3 u)) + u (|xhat gamma| + |beta|), then ONE output rounding
    u_out (|y| + e) + e  (u_out = 2^-8 for bf16, 2^-24 for fp32);
  - the packed bf16 backward forms xhat as x rs + (-mu rs): 2 u |mu| rstd more than (x - mu) rs;
  - dgamma / dbeta and the fold: the terms' own error plus depth x u x sum |terms|, depth counted along the longest chain of additions
    (rows per wave, 3 LDS adds, then one atomic per block or the fold kernel's cdiv(n, 64) + 2 + 16 + 1);
  - BatchNorm's one-pass shifted variance q / cnt - ms^2 (q = sum (v - shift)^2, ms = mean - shift) loses
    (k + 3) u (var + ms^2) + 2 |ms| e_ms + ...: what the algorithm can lose when the shift is far from the mean.
"""
import functools

import torch

from gemm_bounds import SENTINEL, U16, U32, violations  # noqa: F401  (violations is re-exported for the two test files)

# Hardware accuracy of the two operations whose rounding cannot be counted from the source: rsqrtf and the fp32 division, relative to the
# exact result.  ROCm ships no accuracy table on the test machines, so both were measured on an MI355X against fp64 (rsqrtf through
# csmae_bnrelu_fwd's eval mode, which writes rsqrtf(running_var + eps) unchanged, over 2^16 arguments in [1e-4, 1e3], a range that holds every variance
# of these tests; the division through LayerNorm means of 4096 integer-valued rows, whose sums are exact, at every tested width); twice the
# worst case is allowed.
RSQRT_REL = 2 * 1.51 * U32  # measured worst case: 1.507 x 2^-24 (mean 0.39 x 2^-24)
DIV_REL = 2 * 0.99 * U32    # measured worst case: 0.992 x 2^-24 (a correctly rounded quotient; 0 where the width is a power of two)

LN_EPS, BN_EPS, BN_MOMENTUM = 1e-6, 1e-5, 0.1
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}

# ---- the geometry classes both test files walk
LN_WIDTHS = (4, 64, 252, 256, 260, 512, 516, 768, 772, 1024, 1028, 1280, 1284, 1536, 1792, 2044, 2048)
LN_ROWS = (1, 5, 37)
LN_WS_ROWS = (1, 2, 3, 10)                      # partial rows of the workspace at M = 37: a wave walks 10, 5, 4 rows, or 1
LN_LONG = ((4100, 64), (4100, 260))             # backward, grid capped at 1024 blocks
LN_LONG_EMIT = ((8197, 64), (8197, 260))        # forward with an fp8 copy, grid capped at 2048 blocks
FOLD_ROWS = (1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 1024)
FOLD_D = (4, 36, 512)
BN_GEOMS = tuple([(2048, n) for n in (1, 3, 4, 5, 15, 16, 17, 37)] + [(64, n) for n in (6, 127, 128, 129, 513)] +
                 [(8, 5), (8192, 5), (24, 5), (100, 5)])    # (Hp, N)
BN_L = (1, 5)
BN_SPECIAL = (2048, 5, 5)                       # (Hp, N, L) of the outlier / far-mean channels


def f32(v):
    """A Python number as the fp32 value a kernel argument of type float holds."""
    return float(torch.tensor(v, dtype=torch.float32))


def cdiv(a, b):
    return -(-a // b)


def finish(R, e, dtype):
    """The output rounding on top of an error e of the value rounded."""
    u = U16 if dtype == torch.bfloat16 else U32
    return u * (R.abs() + e) + e


# ------------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """A contiguous [rows, cols] view inside a larger flat allocation: at least two rows' worth of sentinel elements before and behind it
    (a multiple of 16 bytes), the view itself prefilled with the sentinel unless `fill` is given.  The view starts 16-byte aligned, or,
    with off8, 8 bytes behind a 16-byte boundary."""

    def __init__(self, rows, cols, dtype, device="cuda", fill=None, off8=False):
        es = torch.empty(0, dtype=dtype).element_size()
        q = 16 // es
        g = cdiv(max(2 * cols, q), q) * q
        self.rows, self.cols, self.dtype, self.g = rows, cols, dtype, g
        self.start = g + (8 // es if off8 else 0)
        self.n = rows * cols
        self.sentinel = SENTINEL[dtype]
        self.ibase = torch.full((self.start + self.n + g + q,), self.sentinel, dtype=_INT[dtype], device=device)
        assert self.ibase.data_ptr() % 16 == 0
        self.base = self.ibase.view(dtype)
        self.t = self.base[self.start:self.start + self.n].view(rows, cols)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (8 if off8 else 0)
        if fill is not None:
            self.t.copy_(fill.to(device=device, dtype=dtype) if torch.is_tensor(fill) else torch.full((rows, cols), fill, dtype=dtype))

    @property
    def vec(self):
        assert self.rows == 1
        return self.t[0]

    def bits(self):
        return self.ibase[self.start:self.start + self.n].view(self.rows, self.cols)

    def outside_intact(self):
        """True when every element outside the view still holds the sentinel, bit for bit."""
        return bool((self.ibase[:self.start] == self.sentinel).all()) and bool((self.ibase[self.start + self.n:] == self.sentinel).all())

    def unwritten(self):
        """Elements of the view that still hold the sentinel."""
        return int((self.bits() == self.sentinel).sum())

    def untouched(self):
        return self.outside_intact() and self.unwritten() == self.n


# ------------------------------------------------------------------------------------------------ LayerNorm
def nv_instance(D):
    """Column groups of the kernel instance that takes width D (ln_fwd_launch / ln_bwd_launch)."""
    nv = cdiv(D, 256)
    return nv if nv <= 5 else 8


def ln_depth(D):
    return 4 * nv_instance(D) + 6


def ln_packed(D):
    """Widths the all-bf16 deferred backward runs in ln_bwd_bf16_kernel."""
    return 2 <= cdiv(D, 256) <= 5


def ln_bwd_blocks(M, D, part_elems=None):
    blocks = min(cdiv(M, 4), 1024)
    if part_elems is not None and part_elems // (2 * D) < blocks:
        blocks = part_elems // (2 * D)
    return blocks


@functools.lru_cache(maxsize=None)
def ln_inputs(M, D):
    """fp32 CPU operands (shared: do not write to them).  Row r has mean 0.37 (r % 31) - 2 and a scale in [0.5, 3] of its own; gamma and beta
    rise over the columns, with noise; dy and dres are independent draws."""
    g = torch.Generator().manual_seed(5000 + 7 * M + 13 * D)
    r = torch.arange(M, dtype=torch.float32)
    mean = 0.37 * (r % 31) - 2.0
    scale = 0.5 + 2.5 * ((r * 0.6180339887) % 1.0)
    x = mean[:, None] + scale[:, None] * torch.randn(M, D, generator=g)
    c = torch.arange(D, dtype=torch.float32) / D
    gamma = 0.5 + c + 0.05 * torch.randn(D, generator=g)
    beta = -0.3 + 0.6 * c + 0.05 * torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g) * (0.5 + ((r * 0.37) % 1.0))[:, None]
    dres = torch.randn(M, D, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, dres=dres)


def ln_fwd_ref(x, gamma, beta, eps=LN_EPS):
    """fp64 LayerNorm of the (already rounded) x: y, mean, rstd, the error e_y of y before its output rounding, bounds of mean and rstd."""
    X, g, b = x.double(), gamma.double(), beta.double()
    k, eps = ln_depth(X.shape[1]), f32(eps)
    mu = X.mean(1, keepdim=True)
    var = ((X - mu) ** 2).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xhat = (X - mu) * rstd
    y = xhat * g + b
    e_mu = (k * U32 + DIV_REL) * X.abs().mean(1, keepdim=True)
    theta = (k + 4) * U32 + DIV_REL + e_mu ** 2 * rstd ** 2
    e_rs = 0.5 * theta / (1 - theta) + RSQRT_REL
    e_y = g.abs() * (rstd * e_mu + xhat.abs() * (e_rs + 3 * U32)) + U32 * ((xhat * g).abs() + b.abs())
    return dict(y=y, mean=mu[:, 0], rstd=rstd[:, 0], e_y=e_y, b_mean=e_mu[:, 0], b_rstd=(rstd * e_rs)[:, 0])


def ln_bwd_ref(dy, x, mean, rstd, gamma, dres=None, packed=False):
    """fp64 LayerNorm backward of the rounded operands with the GIVEN fp32 row statistics:
    dx = rstd (g - mean(g) - xhat mean(g xhat)) + dres_in, dgamma = sum dy xhat, dbeta = sum dy.  Returns the error e_dx of dx before its
    output rounding(s), and what param_bound needs for dgamma / dbeta."""
    DY, X, g = dy.double(), x.double(), gamma.double()
    k = ln_depth(X.shape[1])
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (X - mu) * rs
    G = DY * g
    s1 = G.mean(1, keepdim=True)
    s2 = (G * xh).mean(1, keepdim=True)
    inner = G - s1 - xh * s2
    dx = rs * inner + (dres.double() if dres is not None else 0.0)
    e_xh = 2 * U32 * xh.abs() + (2 * U32 * mu.abs() * rs if packed else 0.0)
    e_s1 = ((k + 1) * U32 + DIV_REL) * G.abs().mean(1, keepdim=True)
    e_s2 = (G.abs() * e_xh).mean(1, keepdim=True) + ((k + 2) * U32 + DIV_REL) * (G * xh).abs().mean(1, keepdim=True)
    e_in = U32 * G.abs() + e_s1 + e_xh * s2.abs() + xh.abs() * e_s2 + U32 * (xh * s2).abs() + 2 * U32 * (G.abs() + s1.abs() + (xh * s2).abs())
    e_dx = rs * e_in + U32 * (rs * inner).abs() + U32 * dx.abs()
    tg = DY * xh
    return dict(dx=dx, e_dx=e_dx, dgamma=tg.sum(0), dbeta=DY.sum(0), abs_g=tg.abs().sum(0), abs_b=DY.abs().sum(0),
                e_g=(DY.abs() * e_xh).sum(0) + U32 * tg.abs().sum(0), e_b=torch.zeros_like(g))


def ln_param_depth(M, blocks, atomics):
    """Longest chain of additions behind one dgamma / dbeta element: a wave's rows, the LDS fold of four waves, then one atomic per block
    or the fold kernel."""
    return cdiv(M, 4 * blocks) + 3 + (blocks if atomics else fold_depth(blocks))


def fold_depth(n):
    """ln_param_reduce_kernel: four accumulators of cdiv(n, 64) rows each, two additions between them, 16 lanes in a row, the final +=."""
    return cdiv(n, 64) + 2 + 16 + 1


def param_bound(depth, abs_terms, e_terms, prev=None):
    p = prev.double().abs() if prev is not None else 0.0
    return e_terms + depth * U32 * (abs_terms + p)


def fold_ref(parts, prev):
    """Column sums of partial rows [n, 2 D] on top of prev [2 D] in fp64, and their bound."""
    P = parts.double()
    return prev.double() + P.sum(0), param_bound(fold_depth(P.shape[0]), P.abs().sum(0), 0.0, prev)


# ------------------------------------------------------------------------------------------------ BatchNorm(token axis) + ReLU
def bn_fast(dtype, Hp):
    return dtype == torch.bfloat16 and Hp % 8 == 0 and Hp // 8 <= 1024 and 1024 % (Hp // 8) == 0


def bn_rl_n(Hp):
    return 1024 // (Hp // 8)


def bn_depth(N, Hp, fast):
    share = 8 * cdiv(N, bn_rl_n(Hp)) if fast else 4 * cdiv(N * (Hp // 4), 1024)
    return share + 6 + 16 + 1


def _chan(t, N, L, Hp):
    """[N * L, Hp] -> [L, N * Hp]: the values of each channel (token position)."""
    return t.reshape(N, L, Hp).permute(1, 0, 2).reshape(L, N * Hp)


def _unchan(t, N, L, Hp):
    return t.reshape(L, N, Hp).permute(1, 0, 2).reshape(N * L, Hp)


def bn_fwd_ref(u, gamma, beta, N, L, Hp, run_mean=None, run_var=None, training=True, fast=False, eps=BN_EPS, momentum=BN_MOMENTUM):
    """fp64 BatchNorm over (n, h) per token position + ReLU of the rounded u [N * L, Hp].  Training: batch statistics (biased variance
    for the normalisation, the unbiased cnt / (cnt - 1) one into running_var).  Eval: the given running statistics."""
    V = _chan(u.double(), N, L, Hp)
    cnt, k, eps, mom = N * Hp, bn_depth(N, Hp, fast), f32(eps), f32(momentum)
    gm, bt = gamma.double()[:, None], beta.double()[:, None]
    out = {}
    if training:
        mu = V.mean(1, keepdim=True)
        var = ((V - mu) ** 2).mean(1, keepdim=True)
        if fast:     # one pass over d = v - shift:  ms = sum d / cnt,  var = sum d^2 / cnt - ms^2,  mean = shift + ms
            shift = V[:, :1]
            ms = mu - shift
            e_ms = ((k + 1) * U32 + DIV_REL) * (V - shift).abs().mean(1, keepdim=True)
            m2 = var + ms ** 2
            e_var = ((k + 3) * U32 + DIV_REL) * m2 + 2 * ms.abs() * e_ms + e_ms ** 2 + U32 * ms ** 2 + U32 * (m2 + ms ** 2)
            e_mu = e_ms + U32 * mu.abs()
            theta = e_var / (var + eps) + U32
        else:
            e_mu = (k * U32 + DIV_REL) * V.abs().mean(1, keepdim=True)
            e_var = ((k + 3) * U32 + DIV_REL) * var + e_mu ** 2
            theta = e_var / (var + eps) + U32
        if run_mean is not None:
            f = cnt / (cnt - 1.0)
            rm, rv = run_mean.double()[:, None], run_var.double()[:, None]
            out["run_mean"] = ((1 - mom) * rm + mom * mu)[:, 0]
            out["run_var"] = ((1 - mom) * rv + mom * var * f)[:, 0]
            out["e_run_mean"] = (mom * e_mu + 3 * U32 * (((1 - mom) * rm).abs() + (mom * mu).abs()))[:, 0]
            out["e_run_var"] = (mom * f * e_var + U32 * (3 * ((1 - mom) * rv).abs() + 5 * (mom * var * f).abs()))[:, 0]
    else:
        mu, var = run_mean.double()[:, None], run_var.double()[:, None]
        e_mu, theta = torch.zeros_like(mu), torch.full_like(mu, U32)
    rstd = (var + eps).rsqrt()
    e_rs = 0.5 * theta / (1 - theta) + RSQRT_REL
    xhat = (V - mu) * rstd
    pre = xhat * gm + bt
    e_pre = gm.abs() * (rstd * e_mu + xhat.abs() * (e_rs + 3 * U32)) + U32 * ((xhat * gm).abs() + bt.abs())
    out.update(r=_unchan(pre.clamp_min(0.0), N, L, Hp), pre=_unchan(pre, N, L, Hp), e_r=_unchan(e_pre, N, L, Hp), mean=mu[:, 0], rstd=rstd[:, 0],
               b_mean=e_mu[:, 0], b_rstd=(rstd * e_rs)[:, 0])
    return out


def bn_bwd_ref(u, dr, gamma, beta, mean, rstd, N, L, Hp, fast=False):
    """fp64 backward of BatchNorm + ReLU with the GIVEN fp32 channel statistics.  The ReLU mask is taken from the fp64 pre-activation;
    `margin` is the smallest distance of a pre-activation from zero in units of its own fp32 evaluation error (must be > 1)."""
    V, G = _chan(u.double(), N, L, Hp), _chan(dr.double(), N, L, Hp)
    cnt, k = N * Hp, bn_depth(N, Hp, fast)
    gm, bt = gamma.double()[:, None], beta.double()[:, None]
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (V - mu) * rs
    pre = xh * gm + bt
    margin = float((pre.abs() / (4 * U32 * ((xh * gm).abs() + bt.abs()) + 1e-300)).min())
    gg = torch.where(pre > 0, G, torch.zeros_like(G))
    m1 = gg.mean(1, keepdim=True)
    m2 = (gg * xh).mean(1, keepdim=True)
    inner = gg - m1 - xh * m2
    du = gm * rs * inner
    e_xh = 2 * U32 * xh.abs()
    e_m1 = (k * U32 + DIV_REL) * gg.abs().mean(1, keepdim=True)
    e_m2 = (gg.abs() * e_xh).mean(1, keepdim=True) + ((k + 1) * U32 + DIV_REL) * (gg * xh).abs().mean(1, keepdim=True)
    e_in = e_m1 + e_xh * m2.abs() + xh.abs() * e_m2 + U32 * (xh * m2).abs() + 2 * U32 * (gg.abs() + m1.abs() + (xh * m2).abs())
    e_du = (gm * rs).abs() * e_in + 2 * U32 * du.abs()
    tg = gg * xh
    return dict(du=_unchan(du, N, L, Hp), e_du=_unchan(e_du, N, L, Hp), margin=margin, dgamma=tg.sum(1), dbeta=gg.sum(1),
                abs_g=tg.abs().sum(1), abs_b=gg.abs().sum(1), e_g=(gg.abs() * e_xh).sum(1) + U32 * tg.abs().sum(1), depth=k + 1)


@functools.lru_cache(maxsize=None)
def bn_inputs(N, L, Hp, dtype, special=False):
    """Seeded CPU operands, u and dr already in `dtype` (shared: do not write to them).  Channel l has mean 0.9 l - 1.3 and a scale of its
    own.  special: channel 1's first value (the fast kernel's shift) is a 20-sigma outlier, channel 2's mean lies 50 sigma from zero.
    No fp64 pre-activation lies within the forward bound of zero (reseeded until that holds, for the fast and the generic kernel's bound)."""
    for attempt in range(64):
        g = torch.Generator().manual_seed(9000 + 7 * N + 13 * L + 31 * Hp + 1000003 * attempt + (17 if special else 0) + (3 if dtype == torch.bfloat16 else 0))
        l = torch.arange(L, dtype=torch.float32)
        mean = 0.9 * l - 1.3
        scale = 0.5 + 2.5 * ((l * 0.6180339887 + 0.3) % 1.0)
        if special:
            mean[2] = 50.0 * scale[2]
        v = mean[:, None] + scale[:, None] * torch.randn(L, N * Hp, generator=g)
        v[:, 0] = mean + 0.1 * scale        # the fast kernel's shift near the mean: its variance bound at its tightest (special: far away)
        if special:
            v[1, 0] = mean[1] + 20.0 * scale[1]
        u = _unchan(v, N, L, Hp).to(dtype)
        gamma = 0.7 + 0.2 * l + 0.05 * torch.randn(L, generator=g)
        beta = -0.4 + 0.25 * l + 0.05 * torch.randn(L, generator=g)
        dr = (torch.randn(N * L, Hp, generator=g) * 0.8).to(dtype)
        run_mean = 0.3 * torch.randn(L, generator=g) + 0.1
        run_var = 0.1 + torch.rand(L, generator=g) * 0.4
        o = dict(u=u, dr=dr, gamma=gamma, beta=beta, run_mean=run_mean, run_var=run_var)
        if bn_mask_margin(o, N, L, Hp, dtype) > 1.0:
            return o
    raise AssertionError("no unambiguous ReLU mask in 64 draws")


def bn_mask_margin(o, N, L, Hp, dtype):
    """min |pre| / forward bound over the kernels that can take the geometry (> 1: no pre-activation is within the bound of zero)."""
    worst = float("inf")
    for fast in {False, bn_fast(dtype, Hp)}:
        f = bn_fwd_ref(o["u"], o["gamma"], o["beta"], N, L, Hp, fast=fast)
        worst = min(worst, float((f["pre"].abs() / finish(f["pre"], f["e_r"], dtype)).min()))
    return worst


# ------------------------------------------------------------------------------------------------ fp32 emulations (CPU self-check)
def sum32(v, lanes, order):
    """fp32 sum over the last dimension the way a kernel does it: each of `lanes` lanes adds its share in a row, then a tree over the lanes.
    order 0: lane j takes elements j, j + lanes, ...; the tree adds halves.  order 1: lane j takes a contiguous share, walked backwards;
    the tree adds neighbours.  Both have the depth the bounds count."""
    assert v.dtype == torch.float32 and lanes & (lanes - 1) == 0
    n = v.shape[-1]
    per = max(cdiv(n, lanes), 1)
    v = torch.nn.functional.pad(v, (0, per * lanes - n))
    if order == 0:
        v = v.reshape(*v.shape[:-1], per, lanes)
        acc = v[..., 0, :].clone()
        for i in range(1, per):
            acc = acc + v[..., i, :]
        while acc.shape[-1] > 1:
            h = acc.shape[-1] // 2
            acc = acc[..., :h] + acc[..., h:]
    else:
        v = v.reshape(*v.shape[:-1], lanes, per)
        acc = v[..., per - 1].clone()
        for i in range(per - 2, -1, -1):
            acc = acc + v[..., i]
        while acc.shape[-1] > 1:
            acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def _rsqrt32(v):
    return v.double().rsqrt().float()


def _wave_first_row(M, grid):
    """Row whose statistics a defective wave would reuse: its first row (row - 4 grid for every later row)."""
    r = torch.arange(M)
    return torch.where(r >= 4 * grid, r % (4 * grid), r)


LN_FWD_DEFECTS = ("stats_skip_last_group", "divisor_nv256", "second_row_stats")
LN_BWD_DEFECTS = ("stats_skip_last_group", "divisor_nv256", "second_row_stats", "dres_skip_last_group")
FOLD_DEFECTS = ("drop_tail", "one_too_many")
BN_FWD_DEFECTS = ("cnt_n", "biased_running_var", "drop_tail_rows")
BN_BWD_DEFECTS = ("cnt_n", "mask_beta_sign", "drop_tail_rows")


def ln_defect_applies(defect, M, D, grid, dres=True):
    if defect == "stats_skip_last_group":
        return D % 256 != 0 and D > 256
    if defect == "divisor_nv256":
        return nv_instance(D) * 256 != D
    if defect == "second_row_stats":
        return M > 4 * grid
    if defect == "dres_skip_last_group":
        return dres and D % 256 != 0 and D > 256
    raise ValueError(defect)


def ln_fwd_emu(x, gamma, beta, out_dtype, order=0, defect=None, grid=None, eps=LN_EPS):
    """ln_fwd_kernel in fp32 torch: (y in out_dtype, y32, mean, rstd)."""
    X = x.float()
    M, D = X.shape
    S = X[:, :(D // 256) * 256] if defect == "stats_skip_last_group" else X
    div = torch.tensor(float(nv_instance(D) * 256 if defect == "divisor_nv256" else D))
    mu = sum32(S, 64, order) / div
    d = S - mu[:, None]
    rs = _rsqrt32(sum32(d * d, 64, order) / div + torch.tensor(eps))
    mu_n, rs_n = mu, rs
    if defect == "second_row_stats":
        src = _wave_first_row(M, grid)
        mu_n, rs_n = mu[src], rs[src]
    y = (X - mu_n[:, None]) * rs_n[:, None] * gamma + beta
    return y.to(out_dtype), y, mu, rs


def ln_bwd_emu(dy, x, mean, rstd, gamma, dres, out_dtype, order=0, defect=None, grid=None, packed=False):
    """ln_bwd_kernel / ln_bwd_bf16_kernel in fp32 torch: (dx in out_dtype, dgamma, dbeta) — the parameter gradients summed over all rows
    in one chain of `order`."""
    DY, X = dy.float(), x.float()
    M, D = X.shape
    mu, rs = mean.clone(), rstd.clone()
    if defect == "second_row_stats":
        src = _wave_first_row(M, grid)
        mu, rs = mu[src], rs[src]
    xh = X * rs[:, None] + (-mu * rs)[:, None] if packed else (X - mu[:, None]) * rs[:, None]
    G = DY * gamma
    full = (D // 256) * 256
    sl = slice(0, full) if defect == "stats_skip_last_group" else slice(0, D)
    div = torch.tensor(float(nv_instance(D) * 256 if defect == "divisor_nv256" else D))
    s1 = sum32(G[:, sl].contiguous(), 64, order) / div
    s2 = sum32((G * xh)[:, sl].contiguous(), 64, order) / div
    dx = (G - s1[:, None] - xh * s2[:, None]) * rs[:, None]
    if dres is not None:
        R = dres.float().clone()
        if defect == "dres_skip_last_group":
            R[:, full:] = 0.0
        dx = dx + R
    dg = sum32((DY * xh).t().contiguous(), 4, order)
    db = sum32(DY.t().contiguous(), 4, order)
    return dx.to(out_dtype), dg, db


def fold_emu(parts_ext, n, prev, order=0, defect=None):
    """ln_param_reduce_kernel on rows [0, n) of parts_ext [>= n + 1, 2 D]."""
    rows = parts_ext[:n]
    if defect == "drop_tail":
        rows = parts_ext[:(n // 64) * 64]
    elif defect == "one_too_many":
        rows = parts_ext[:n + 1]
    if rows.shape[0] == 0:
        return prev.clone()
    return prev + sum32(rows.t().contiguous(), 16, order)


def bn_defect_applies(defect, N, Hp, fast, bwd):
    if defect == "drop_tail_rows":
        return fast and N % ((2 if bwd else 4) * bn_rl_n(Hp)) != 0
    return True


def bn_fwd_emu(o, N, L, Hp, dtype, fast, order=0, defect=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    """bnrelu_fwd_kernel / bnrelu_fwd_fast_kernel (training) in fp32 torch: (r, mean, rstd, running_mean, running_var)."""
    V = _chan(o["u"].float(), N, L, Hp)
    S = V
    if defect == "drop_tail_rows":
        keep = (N // (4 * bn_rl_n(Hp))) * 4 * bn_rl_n(Hp)
        S = V[:, :keep * Hp]
    cnt = torch.tensor(float(N if defect == "cnt_n" else N * Hp))
    if fast:
        shift = V[:, :1]
        d = S - shift
        ms = sum32(d, 1024, order) / cnt
        var = (sum32(d * d, 1024, order) / cnt - ms * ms).clamp_min(0.0)
        mu = shift[:, 0] + ms
    else:
        mu = sum32(S, 1024, order) / cnt
        d = S - mu[:, None]
        var = sum32(d * d, 1024, order) / cnt
    rs = _rsqrt32(var + torch.tensor(eps))
    r = ((V - mu[:, None]) * rs[:, None] * o["gamma"][:, None] + o["beta"][:, None]).clamp_min(0.0)
    mom = torch.tensor(momentum)
    unb = torch.tensor(1.0) if defect == "biased_running_var" else cnt / (cnt - 1.0)
    rm = (1.0 - mom) * o["run_mean"] + mom * mu
    rv = (1.0 - mom) * o["run_var"] + mom * var * unb
    return _unchan(r, N, L, Hp).to(dtype), mu, rs, rm, rv


def bn_bwd_emu(o, mean, rstd, N, L, Hp, dtype, fast, order=0, defect=None):
    """bnrelu_bwd_kernel / bnrelu_bwd_fast_kernel in fp32 torch: (du, dgamma, dbeta) on zero-initialised parameter gradients."""
    V, G = _chan(o["u"].float(), N, L, Hp), _chan(o["dr"].float(), N, L, Hp)
    gm, bt = o["gamma"][:, None], o["beta"][:, None]
    xh = (V - mean[:, None]) * rstd[:, None]
    pre = xh * gm - bt if defect == "mask_beta_sign" else xh * gm + bt
    gg = torch.where(pre > 0, G, torch.zeros_like(G))
    cnt = torch.tensor(float(N if defect == "cnt_n" else N * Hp))
    keep = N * Hp
    if defect == "drop_tail_rows":
        keep = (N // (2 * bn_rl_n(Hp))) * 2 * bn_rl_n(Hp) * Hp
    s1 = sum32(gg[:, :keep].contiguous(), 1024, order)
    s2 = sum32((gg * xh)[:, :keep].contiguous(), 1024, order)
    m1, m2 = s1 / cnt, s2 / cnt
    du = gm * rstd[:, None] * (gg - m1[:, None] - xh * m2[:, None])
    return _unchan(du, N, L, Hp).to(dtype), s2, s1
