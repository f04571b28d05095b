"""CPU-only self-check of the per-element GEMM bounds (tests/gemm_bounds.py) that test_gemm_routes_gpu.py holds every kernel to: on every shape of
the route matrix the bound is tight enough to reject a product that lost its last K columns or a bias shifted by one column — the kind of
subtle slip (a dropped K tail, an off-by-one epilogue column) a loose, max-relative tolerance lets through."""
import pytest
import torch

import gemm_bounds as GB


def _shapes():
    seen = {}
    for route, layout, mnk, ldc in GB.route_cases():
        seen.setdefault((route, mnk), (route, layout, mnk))
    return list(seen.values())


@pytest.mark.parametrize("route,layout,mnk", _shapes(), ids=[f"{r}-{m[0]}x{m[1]}x{m[2]}" for r, _, m in _shapes()])
def test_bound_rejects_a_dropped_k_tail_and_a_shifted_bias(route, layout, mnk):
    M, N, K = mnk
    o = GB.operands(route, layout, mnk)
    A, B, bias = o["A"], o["B"], o["bias"]
    acc, P = GB.products(A, B)
    drop = max(0, K - 8)
    acc_drop, _ = GB.products(A[:, :drop], B[:drop])
    shifted = torch.roll(bias, 1)
    for odt in (torch.bfloat16, torch.float32):
        R, bound = GB.reference("none", acc, P, K, out_dtype=odt, bias=bias)
        assert bool(((acc_drop + bias.double() - R).abs() > bound).any()), f"the {odt} bound accepts a product without its last 8 K columns"
        assert bool(((acc + shifted.double() - R).abs() > bound).any()), f"the {odt} bound accepts a bias shifted by one column"
        assert bool(((R.to(odt).double() - R).abs() <= bound).all()), f"the {odt} bound rejects the correctly rounded result"
    # the GELU epilogue's looser bound too (its polynomial's error is part of it)
    (h, bh), _ = GB.reference("gelu", acc, P, K, out_dtype=torch.bfloat16, bias=bias)
    (hd, _), _ = GB.reference("gelu", acc_drop, P, K, out_dtype=torch.bfloat16, bias=bias)
    (hs, _), _ = GB.reference("gelu", acc, P, K, out_dtype=torch.bfloat16, bias=shifted)
    assert bool(((hd - h).abs() > bh).any()) and bool(((hs - h).abs() > bh).any()), "the GELU bound accepts a dropped K tail or a shifted bias"


def test_guarded_buffer_layout():
    """The helper's own contract: guard rows and pad columns hold the sentinel, the view is 16-byte aligned, outside_intact sees a stray write."""
    for dtype, ld in ((torch.bfloat16, 268), (torch.float32, 70), (torch.uint8, 268)):
        g = GB.Guarded(5, ld - 4, dtype, ld, device="cpu", fill=torch.ones(5, ld - 4, dtype=torch.float32).to(dtype))
        assert g.g >= 2 and (g.g * ld * g.t.element_size()) % 16 == 0 and g.t.data_ptr() % 16 == g.base.data_ptr() % 16
        assert g.outside_intact() and not g.untouched()
        g.base[g.g * ld + ld - 1] = 0          # the last pad column of the first row
        assert not g.outside_intact()


def test_every_route_code_is_covered():
    """The matrix reaches every code the route queries can return: the bf16 tile configurations 0, 2, 4, 5, 6, the fp32 kernel, the K-slab kernel."""
    codes = set()
    for route, layout, mnk, ldc in GB.route_cases():
        codes.add(GB.expected_route(route, mnk))
    assert codes == {0, 2, 4, 5, 6, GB.F32_ROUTE, GB.KSLAB_ROUTE}
