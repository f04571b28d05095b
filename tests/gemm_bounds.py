"""Helpers of the GEMM route tests (test_gemm_routes_gpu.py) and of their CPU self-check (test_gemm_bounds_cpu.py): guarded buffers, the
route x layout x shape x epilogue matrix, seeded operands, and the per-element error bound of every GEMM epilogue.

Bounds are derived from the operation, element by element, never from a global maximum:
  - accumulation: K exact products (bf16 x bf16 and fp8 x fp8 fit in fp32) summed in fp32 in any order and split:
        |err| <= (K + adds) * 2^-24 * (|A| |B|)_ij
  - each further fp32 operation (bias, residual, scale, atomic add): 2^-24 of the magnitudes involved;
  - the output rounding: 2^-8 |R| for bf16 (8 significant bits), 2^-24 |R| for fp32;
  - GELU / gelu' in the bf16 epilogues: the documented limits of the polynomial in csrc/common.h (gelu_both2_fast: max |Phi error| 2.3e-4,
    max |gelu error| 8e-4), the 8-bit gelu' code's half step 2.5e-3 (csrc/gemm_common.h, GP_Q8), and the derivative bounds |gelu'| <= 1.13,
    |gelu''| <= 2 phi(0) < 0.8 that carry the pre-activation's error through.
"""
import math

import torch

U32 = 2.0 ** -24          # fp32 unit roundoff
U16 = 2.0 ** -8           # bf16 unit roundoff (8 significant bits)
GELU_H_BF16 = 8e-4        # csrc/common.h gelu_both2_fast: max |gelu error| of the bf16 epilogues (at x = 3.5)
GELU_G_BF16 = 2.5e-4      # csrc/common.h gelu_both2_fast: max |Phi error| 2.3e-4 (gelu' = Phi + x phi; phi from exp2 to a few fp32 ulps)
GELU_F32_ULPS = 4 * U32   # fp32 epilogues: erff / __expf to a few ulps, relative to 1 + |x| (1 + erf(x) cancels for x << 0)
# fp8 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4): its 128-wide block dot product does not round like a chain of fp32 adds (the products are
# aligned and summed with fewer bits, as fp8 matrix units commonly do); on this suite's shapes the error reaches 2^-15.7 (|A| |B|)_ij, past the
# K 2^-24 term.  Allowed: 2^-14 (|A| |B|)_ij — still far inside the change a dropped K step or a wrong scale makes.
FP8_MFMA_REL = 2.0 ** -14
Q8_HALF_STEP = 2.5e-3     # csrc/gemm_common.h GP_Q8: q = round(200 g + 26), |error| <= half a code step
GELU1_MAX, GELU2_MAX = 1.13, 0.8   # max |gelu'|, max |gelu''|

# the fill outside every view: bit patterns a kernel does not produce by accident (NaN with a payload for the float types)
SENTINEL = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FC0A5A5, torch.uint8: 0xA5}
FP8_NAN = 0x7F            # NaN in e4m3fn and in e5m2: the fill around fp8 operands
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}


class Guarded:
    """A [rows, cols] view inside a larger allocation: >= 2 guard rows before and after it, a row pitch ld > cols, and everything outside the
    view (pad columns, guard rows) filled with a sentinel bit pattern.  The view starts 16-byte aligned (guard rows x ld x element size is a
    multiple of 16).  `fill` sets the view's own initial content (default: the sentinel too)."""

    def __init__(self, rows, cols, dtype, ld, device="cuda", sentinel=None, fill=None):
        assert ld > cols
        es = torch.empty(0, dtype=dtype).element_size()
        g = 2
        while (g * ld * es) % 16:
            g += 1
        self.rows, self.cols, self.ld, self.g, self.dtype = rows, cols, ld, g, dtype
        self.sentinel = SENTINEL[dtype] if sentinel is None else sentinel
        self.ibase = torch.full(((rows + 2 * g) * ld,), self.sentinel, dtype=_INT[dtype], device=device)
        self.base = self.ibase.view(dtype)
        self.t = self.base[g * ld:(g + rows) * ld].view(rows, ld)[:, :cols]
        assert self.t.data_ptr() % 16 == 0
        if fill is not None:
            self.t.copy_(fill.to(device=device, dtype=dtype) if torch.is_tensor(fill) else torch.full((rows, cols), fill, dtype=dtype))

    @property
    def vec(self):
        """The view of a one-row buffer as a contiguous vector."""
        assert self.rows == 1
        return self.t[0]

    def outside_intact(self):
        """True when every element outside the view still holds the sentinel, bit for bit."""
        c = self.ibase.clone()
        c[self.g * self.ld:(self.g + self.rows) * self.ld].view(self.rows, self.ld)[:, :self.cols] = self.sentinel
        return bool((c == self.sentinel).all())

    def untouched(self):
        """True when the whole allocation, the view included, still holds the sentinel (an output that must not be written)."""
        return bool((self.ibase == self.sentinel).all())


def ld_for(width, mult=8, pad=8):
    """A row pitch larger than the width: rounded up to `mult` elements, plus `pad`."""
    return -(-width // mult) * mult + pad


# ---- the route matrix.  Route codes: csmae_gemm_route / csmae_gemm_ks_route (include/csmae.h).  Layout names give the kernel's flags:
# the first letter A, the second B; N = K-contiguous ([M][K] / [N][K]), T = K-strided ([K][M] / [K][N]).
F32_ROUTE, KSLAB_ROUTE = 7, 8
ROUTES = {   # name -> (layouts, shapes (M, N, K), extra shapes of the TT layout, the route code expected)
    # fp32 kernel: 64 x 64 tiles, K step 16
    "f32": (("NN", "NT", "TN", "TT"), [(64, 64, 16), (65, 68, 40), (130, 4, 16), (200, 136, 100)], [(65, 68, 37), (70, 4, 1)], F32_ROUTE),
    # 128 x 128 tiles, K step 32, per-piece predicates (K % 8 == 0 unless both operands are K-strided)
    "cfg0": (("NN", "NT", "TN", "TT"), [(128, 128, 32), (129, 132, 40), (100, 4, 8), (300, 264, 136)], [(129, 132, 37), (100, 4, 1)], 0),
    # 256 x 256 tiles, K step 32
    "cfg2": (("NN", "NT", "TN", "TT"), [(256, 256, 32), (257, 260, 72), (64, 4, 8), (520, 516, 200)], [(257, 260, 37), (64, 4, 1)], 2),
    # 256 x 256 x 64 pipelined: whole 64-wide K steps unless both operands are K-strided (no TN instantiation)
    "cfg4": (("NN", "NT", "TT"), [(256, 256, 64), (257, 260, 128), (256, 4, 64), (520, 516, 192)], [(257, 260, 67), (256, 4, 1)], 4),
    # the same kernel with 192-row tiles: K-contiguous A, split-K 1
    "cfg5": (("NN", "NT"), [(192, 256, 64), (193, 260, 128), (192, 4, 64), (400, 516, 192)], [], 5),
    # 128 x 256 tiles, two workgroups per CU: K-contiguous A, K-strided B, M >= 128, N >= 256, K % 64 == 0, split-K 1
    "cfg6": (("NT",), [(128, 256, 64), (129, 260, 128), (300, 516, 192)], [], 6),
    # csmae_gemm_ks on the K-slab weight mirror (y = x W^T: both operands K-contiguous), same limits as cfg6
    "ks_k2": (("NN",), [(128, 256, 64), (129, 260, 128), (300, 516, 192)], [], KSLAB_ROUTE),
    # csmae_gemm_ks handing the product to csmae_gemm with the plain weight (K-slab use switched off): the heuristic's routes 0, 2 and 5
    "ks_fallback": (("NN",), [(64, 256, 128), (256, 260, 96), (300, 516, 192)], [], {(64, 256, 128): 0, (256, 260, 96): 2, (300, 516, 192): 5}),
}
EPIS_BF16 = ("none_f32_bias", "none_f32", "none_bf16_bias", "none_bf16", "gelu_bf16", "gelu_u8", "resid_f32", "resid_f32_inplace",
             "resid_bf16", "resid_bf16_inplace", "dgelu_bf16", "dgelu_u8", "atomic_s1", "atomic_s3")
EPIS_F32 = ("none_f32_bias", "none_f32", "gelu_f32", "resid_f32", "resid_f32_inplace", "dgelu_f32", "atomic_s1", "atomic_s3")


def route_epilogues(route):
    if route == "f32":
        return EPIS_F32
    if route in ("ks_k2", "ks_fallback"):      # csmae_gemm_ks takes NONE .. DGELU
        return tuple(e for e in EPIS_BF16 if not e.startswith("atomic"))
    if route == "cfg6":                        # accumulating products do not run on the k2 kernel (test_k2_route_leaves_atomic_products...)
        return tuple(e for e in EPIS_BF16 if not e.startswith("atomic"))
    if route == "cfg5":                        # split-K would leave the route
        return tuple(e for e in EPIS_BF16 if e != "atomic_s3")
    return EPIS_BF16


def route_cases():
    """[(route, layout, (M, N, K), output row pitch)]: every layout a route takes at an exact tile, M = tile + 1 with M % 8 != 0 and
    N % 8 == 4, N = 4 (where the route takes it), the minimum K, a partial last K step, several tiles in both dimensions; odd K and K = 1 for
    the both-K-strided layout.  Output pitch: N + 8 / N + 4 (rows of 8-element multiples: the buffer-addressed epilogue where N % 8 == 0, the
    pointer-addressed one where N % 8 == 4); N + 12 on the several-tiles shape (the generic epilogue with pitch % 8 == 4)."""
    out = []
    for route, (layouts, shapes, tt_extra, _) in ROUTES.items():
        for layout in layouts:
            for i, (M, N, K) in enumerate(shapes + (tt_extra if layout == "TT" else [])):
                pad = 12 if i == 3 else (8 if N % 8 == 0 else 4)
                out.append((route, layout, (M, N, K), N + pad))
    return out


def expected_route(route, mnk):
    code = ROUTES[route][3]
    return code[mnk] if isinstance(code, dict) else code


def case_id(route, layout, mnk, ldc):
    return f"{route}-{layout}-{mnk[0]}x{mnk[1]}x{mnk[2]}-ldc{ldc}"


def operands(route, layout, mnk, seed=0):
    """Seeded CPU operands in the values the kernel sees: A [M, K], B [K, N] (logical), bias [N] fp32, and what the epilogues read."""
    M, N, K = mnk
    g = torch.Generator().manual_seed(1000 + 7 * M + 13 * N + 31 * K + seed)
    dt = torch.float32 if route == "f32" else torch.bfloat16
    A = torch.randn(M, K, generator=g).to(dt)
    B = (torch.randn(K, N, generator=g) * K ** -0.5).to(dt)
    bias = torch.randn(N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    R = torch.randn(M, N, generator=g)
    gp = torch.rand(M, N, generator=g) * 1.25 - 0.125                       # gelu' values span [-0.125, 1.125]
    codes = torch.randint(0, 253, (M, N), generator=g, dtype=torch.uint8)   # 8-bit gelu' codes 0 .. 252
    return dict(A=A, B=B, bias=bias, C0=C0, R=R, gp=gp, codes=codes)


def products(A, B):
    """fp64 A B and |A| |B| on whatever device A / B live."""
    a, b = A.double(), B.double()
    return a @ b, a.abs() @ b.abs()


def gelu64(x):
    phi_cdf = 0.5 * (1.0 + torch.erf(x * (0.5 ** 0.5)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * phi_cdf, phi_cdf + x * pdf


def _finish(R, e, out_dtype):
    """The output rounding on top of an error e of the value rounded: |fl(x~) - R| <= u (|R| + e) + e."""
    u = U16 if out_dtype == torch.bfloat16 else U32
    return u * (R.abs() + e) + e


def reference(kind, acc, P, K, *, out_dtype, bias=None, resid=None, aux=None, c0=None, splitk=1, gelu_dtype=None, fp8=False):
    """fp64 reference and per-element bound of one GEMM epilogue.  acc = A B and P = |A| |B| in fp64; aux for DGELU as the values the kernel
    multiplies by (decoded codes for the 8-bit form).  GELU returns ((h, bound_h), (g, bound_g_before_storage)): the caller adds the
    storage of g (bf16 rounding or the code's half step)."""
    e_acc = ((K + 8 + splitk) * U32 + (FP8_MFMA_REL if fp8 else 0.0)) * P
    if kind == "none":
        b = bias.double() if bias is not None else torch.zeros_like(acc[0])
        R = acc + b
        return R, _finish(R, e_acc + U32 * (acc.abs() + b.abs()), out_dtype)
    if kind == "resid":
        b = bias.double() if bias is not None else torch.zeros_like(acc[0])
        r = resid.double()
        R = acc + b + r
        return R, _finish(R, e_acc + 2 * U32 * (acc.abs() + b.abs() + r.abs()), out_dtype)
    if kind == "gelu":
        b = bias.double() if bias is not None else torch.zeros_like(acc[0])
        x = acc + b
        xe = e_acc + U32 * (acc.abs() + b.abs())
        h, g = gelu64(x)
        if (gelu_dtype or out_dtype) == torch.bfloat16:
            eh, eg = GELU_H_BF16 + GELU1_MAX * xe, GELU_G_BF16 + GELU2_MAX * xe
        else:
            eh, eg = GELU_F32_ULPS * (1 + x.abs()) + GELU1_MAX * xe, GELU_F32_ULPS * (1 + x.abs()) + GELU2_MAX * xe
        return (h, _finish(h, eh, out_dtype)), (g, eg)
    if kind == "dgelu":
        a = aux.double()
        R = acc * a
        return R, _finish(R, a.abs() * (e_acc + U32 * acc.abs()) + 3 * U32 * R.abs(), out_dtype)
    if kind == "atomic":
        c = c0.double()
        R = c + acc
        return R, _finish(R, e_acc + (splitk + 1) * U32 * (c.abs() + P), torch.float32)
    raise ValueError(kind)


def violations(got, want, bound):
    """Elements outside the bound (a NaN anywhere counts) and a one-line description of the worst."""
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    n = int(bad.sum())
    if n == 0:
        return 0, ""
    excess = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err - bound)
    idx = int(excess.reshape(-1).argmax())
    r, c = divmod(idx, got.shape[1]) if got.dim() == 2 else (0, idx)
    return n, (f"{n}/{got.numel()} outside the bound; worst at ({r}, {c}): got {float(got.reshape(-1)[idx]):.6g} want {float(want.reshape(-1)[idx]):.6g} "
               f"bound {float(bound.reshape(-1)[idx]):.3g}")
