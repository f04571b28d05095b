"""CPU-only self-check of the norm bounds (tests/norm_ref.py) that test_norm_gpu.py holds csrc/norm.hip to.  For every geometry class of the
GPU file: the kernels' arithmetic emulated honestly in fp32, in two summation orders, meets the bound; each seeded defect (a column group
left out of the statistics, a wrong divisor, a neighbour's statistics, a dropped tail, ...) is rejected by it; no BatchNorm pre-activation
is within the forward bound of zero; the guarded buffer is laid out as promised."""
import pytest
import torch

import norm_ref as R

BF, F32 = torch.bfloat16, torch.float32


def _ok(got, want, bound):
    return R.violations(got if got.dim() else got[None], want if want.dim() else want[None], bound if bound.dim() else bound[None])[0] == 0


def _ln_fwd_ok(o, x, ref, out_dtype):
    y, y32, mu, rs = o
    return (_ok(y, ref["y"], R.finish(ref["y"], ref["e_y"], out_dtype)) and _ok(y32, ref["y"], R.finish(ref["y"], ref["e_y"], F32)) and
            _ok(mu, ref["mean"], ref["b_mean"]) and _ok(rs, ref["rstd"], ref["b_rstd"]))


# M x D classes of the GPU file: every width at its three row counts, the long launches, and M = 37 under every workspace-limited grid
def _ln_classes():
    out = [(M, D, None) for D in R.LN_WIDTHS for M in R.LN_ROWS]
    out += [(M, D, None) for M, D in R.LN_LONG]
    out += [(37, D, ws) for D in (64, 260) for ws in R.LN_WS_ROWS]
    return out


@pytest.mark.parametrize("D", R.LN_WIDTHS)
def test_layernorm_forward_bound(D):
    for M, grid in [(M, R.cdiv(M, 4)) for M in R.LN_ROWS] + ([(M, 2048) for M, d in R.LN_LONG_EMIT if d == D]):
        i = R.ln_inputs(M, D)
        for xdt, odt in ((F32, BF), (F32, F32), (BF, BF)):
            x = i["x"].to(xdt)
            ref = R.ln_fwd_ref(x, i["gamma"], i["beta"])
            for order in (0, 1):
                assert _ln_fwd_ok(R.ln_fwd_emu(x, i["gamma"], i["beta"], odt, order), x, ref, odt), (M, D, xdt, odt, order)
            for defect in R.LN_FWD_DEFECTS:
                if R.ln_defect_applies(defect, M, D, grid):
                    assert not _ln_fwd_ok(R.ln_fwd_emu(x, i["gamma"], i["beta"], odt, 0, defect, grid), x, ref, odt), (M, D, xdt, odt, defect)


def _ln_bwd_ok(o, ref, dtype, M, blocks):
    dx, dg, db = o
    depth = R.ln_param_depth(M, blocks, atomics=True)
    return (_ok(dx, ref["dx"], R.finish(ref["dx"], ref["e_dx"], dtype)) and _ok(dg, ref["dgamma"], R.param_bound(depth, ref["abs_g"], ref["e_g"])) and
            _ok(db, ref["dbeta"], R.param_bound(depth, ref["abs_b"], ref["e_b"])))


@pytest.mark.parametrize("M,D,ws", _ln_classes(), ids=[f"{M}x{D}" + (f"-ws{ws}" if ws else "") for M, D, ws in _ln_classes()])
def test_layernorm_backward_bound(M, D, ws):
    i = R.ln_inputs(M, D)
    blocks = R.ln_bwd_blocks(M, D, ws * 2 * D if ws else None)
    for dydt, xdt, packed in ((BF, BF, R.ln_packed(D)), (F32, F32, False), (BF, F32, False), (F32, BF, False)):
        x, dy = i["x"].to(xdt), i["dy"].to(dydt)
        f = R.ln_fwd_ref(x, i["gamma"], i["beta"])
        mean, rstd = f["mean"].float(), f["rstd"].float()
        for dres in (i["dres"].to(xdt), None):
            ref = R.ln_bwd_ref(dy, x, mean, rstd, i["gamma"], dres, packed)
            for order in (0, 1):
                assert _ln_bwd_ok(R.ln_bwd_emu(dy, x, mean, rstd, i["gamma"], dres, xdt, order, packed=packed), ref, xdt, M, blocks), (xdt, dydt, order)
            for defect in R.LN_BWD_DEFECTS:
                if R.ln_defect_applies(defect, M, D, blocks, dres is not None):
                    assert not _ln_bwd_ok(R.ln_bwd_emu(dy, x, mean, rstd, i["gamma"], dres, xdt, 0, defect, blocks, packed), ref, xdt, M, blocks), (xdt, dydt, defect)


@pytest.mark.parametrize("rows", R.FOLD_ROWS)
def test_fold_bound(rows):
    for D in R.FOLD_D:
        g = torch.Generator().manual_seed(rows * 131 + D)
        parts = torch.randn(rows + 1, 2 * D, generator=g) * (1.0 + torch.arange(2 * D) % 7)
        prev = torch.randn(2 * D, generator=g)
        want, bound = R.fold_ref(parts[:rows], prev)
        for order in (0, 1):
            assert _ok(R.fold_emu(parts, rows, prev, order), want, bound), (rows, D, order)
        for defect in R.FOLD_DEFECTS:
            if defect == "drop_tail" and rows % 64 == 0:
                continue
            assert not _ok(R.fold_emu(parts, rows, prev, 0, defect), want, bound), (rows, D, defect)


def _bn_cases():
    out = [(Hp, N, L, False) for Hp, N in R.BN_GEOMS for L in R.BN_L]
    return out + [R.BN_SPECIAL[:1] + R.BN_SPECIAL[1:] + (True,)]


@pytest.mark.parametrize("Hp,N,L,special", _bn_cases(), ids=[f"Hp{h}-N{n}-L{l}" + ("-special" if s else "") for h, n, l, s in _bn_cases()])
def test_batchnorm_bounds(Hp, N, L, special):
    for dtype in (BF, F32):
        o = R.bn_inputs(N, L, Hp, dtype, special)
        assert R.bn_mask_margin(o, N, L, Hp, dtype) > 1.0                    # (c): no pre-activation within the forward bound of zero
        for fast in sorted({False, R.bn_fast(dtype, Hp)}):                    # the generic kernel also takes the fast geometries (misaligned operands)
            f = R.bn_fwd_ref(o["u"], o["gamma"], o["beta"], N, L, Hp, o["run_mean"], o["run_var"], fast=fast)

            def fwd_ok(e):
                r, mu, rs, rm, rv = e
                return (_ok(r, f["r"], R.finish(f["r"], f["e_r"], dtype)) and _ok(mu, f["mean"], f["b_mean"]) and _ok(rs, f["rstd"], f["b_rstd"]) and
                        _ok(rm, f["run_mean"], f["e_run_mean"]) and _ok(rv, f["run_var"], f["e_run_var"]))

            for order in (0, 1):
                assert fwd_ok(R.bn_fwd_emu(o, N, L, Hp, dtype, fast, order)), (dtype, fast, order)
            for defect in R.BN_FWD_DEFECTS:
                if R.bn_defect_applies(defect, N, Hp, fast, False):
                    assert not fwd_ok(R.bn_fwd_emu(o, N, L, Hp, dtype, fast, 0, defect)), (dtype, fast, defect)
            mean, rstd = f["mean"].float(), f["rstd"].float()
            b = R.bn_bwd_ref(o["u"], o["dr"], o["gamma"], o["beta"], mean, rstd, N, L, Hp, fast)
            assert b["margin"] > 1.0

            def bwd_ok(e):
                du, dg, db = e
                return (_ok(du, b["du"], R.finish(b["du"], b["e_du"], dtype)) and _ok(dg, b["dgamma"], R.param_bound(b["depth"], b["abs_g"], b["e_g"])) and
                        _ok(db, b["dbeta"], R.param_bound(b["depth"], b["abs_b"], 0.0)))

            for order in (0, 1):
                assert bwd_ok(R.bn_bwd_emu(o, mean, rstd, N, L, Hp, dtype, fast, order)), (dtype, fast, order)
            for defect in R.BN_BWD_DEFECTS:
                if R.bn_defect_applies(defect, N, Hp, fast, True):
                    assert not bwd_ok(R.bn_bwd_emu(o, mean, rstd, N, L, Hp, dtype, fast, 0, defect)), (dtype, fast, defect)


def test_every_seeded_defect_meets_a_geometry():
    """Each defect of the lists applies to at least one geometry class walked above (so none is skipped everywhere)."""
    ln = [(M, D, R.ln_bwd_blocks(M, D, ws * 2 * D if ws else None)) for M, D, ws in _ln_classes()]
    for d in R.LN_FWD_DEFECTS:
        assert any(R.ln_defect_applies(d, M, D, R.cdiv(M, 4)) for M, D, _ in ln) or any(R.ln_defect_applies(d, M, D, 2048) for M, D in R.LN_LONG_EMIT), d
    for d in R.LN_BWD_DEFECTS:
        assert any(R.ln_defect_applies(d, M, D, b) for M, D, b in ln), d
    assert any(r % 64 for r in R.FOLD_ROWS)
    for d in R.BN_FWD_DEFECTS + R.BN_BWD_DEFECTS:
        for bwd in (False, True):
            assert any(R.bn_defect_applies(d, N, Hp, R.bn_fast(BF, Hp), bwd) for Hp, N in R.BN_GEOMS), d


def test_guarded_buffer_layout():
    for dtype, rows, cols in ((BF, 5, 260), (F32, 1, 7), (torch.uint8, 3, 36), (BF, 2, 3), (F32, 37, 4)):
        for off8 in (False, True):
            es = torch.empty(0, dtype=dtype).element_size()
            g = R.Guarded(rows, cols, dtype, device="cpu", off8=off8)
            assert g.g >= 2 * cols and (g.g * es) % 16 == 0
            assert g.t.shape == (rows, cols) and g.t.is_contiguous() and g.t.data_ptr() % 16 == (8 if off8 else 0)
            assert g.untouched() and g.unwritten() == rows * cols
            if dtype != torch.uint8:
                assert bool(torch.isnan(g.t.float()).all())                    # the float sentinels are NaNs
            g.t.copy_(torch.ones(rows, cols).to(dtype))
            assert g.outside_intact() and g.unwritten() == 0 and not g.untouched()
            for pos in (g.start - 1, g.start + g.n, 0, g.ibase.numel() - 1):    # one element before / behind the view, and the allocation's ends
                h = R.Guarded(rows, cols, dtype, device="cpu", fill=1.0, off8=off8)
                h.ibase[pos] = 0
                assert not h.outside_intact(), (dtype, pos)
