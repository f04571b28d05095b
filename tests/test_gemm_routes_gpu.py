"""Every kernel the GEMM dispatcher can pick, forced and confirmed through csmae_gemm_route / csmae_gemm_ks_route, at the edges of its tile and K
step, with every epilogue it takes — against fp64 on the exact operand values, element by element (tests/gemm_bounds.py states the bounds).
All tensors live inside guarded allocations (tests/gemm_bounds.py Guarded): NaN in pad columns and guard rows of the operands, so a read that
reaches a result shows up; a sentinel bit pattern around every output, checked bit for bit after the call, so a stray write shows up; outputs
start as NaN, so an element left unwritten shows up.  The other GEMM entry points (fp8, LayerNorm-fused, weight gradients) get the same
treatment below."""
import pytest
import torch

import gemm_bounds as GB
from gemm_bounds import U16, U32, Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from csmae_hip import ops as o
    import csmae_hip
    csmae_hip.load()
    return o


@pytest.fixture(autouse=True)
def restore_routes():
    """The forcing hooks are process-wide: every test leaves the heuristic and the k2 defaults (csrc/gemm.hip) behind, failed or not."""
    yield
    if torch.cuda.is_available():
        import csmae_hip
        lib = csmae_hip.load()
        lib.csmae_gemm_force_tile(-1)
        lib.csmae_gemm_k2_mode(1, 2)


def _force(route):
    import csmae_hip
    lib = csmae_hip.load()
    lib.csmae_gemm_force_tile(int(route[3:]) if route.startswith("cfg") else -1)
    lib.csmae_gemm_k2_mode(1, {"ks_k2": 3, "ks_fallback": 0}.get(route, 2))


def _check(what, got, want, bound):
    n, msg = GB.violations(got, want, bound)
    assert n == 0, f"{what}: {msg}"


# ------------------------------------------------------------------------------------------------ the route matrix
_operand_cache = {}


def _case_operands(route, layout, mnk):
    """Guarded device operands of one case (A, B as the layout stores them, the K-slab mirror for csmae_gemm_ks, bias) and fp64 A B, |A| |B|."""
    key = (route, layout, mnk)
    if key not in _operand_cache:
        _operand_cache.clear()
        M, N, K = mnk
        o = GB.operands(route, layout, mnk)
        dt = o["A"].dtype
        ta, tb = layout[0] == "T", layout[1] == "T"
        a_st = o["A"].t() if ta else o["A"]               # [K, M] or [M, K]
        b_st = o["B"] if tb else o["B"].t()               # [K, N] or [N, K]
        A = Guarded(a_st.shape[0], a_st.shape[1], dt, GB.ld_for(a_st.shape[1]), fill=a_st)
        B = Guarded(b_st.shape[0], b_st.shape[1], dt, GB.ld_for(b_st.shape[1]), fill=b_st)
        bias = Guarded(1, N, torch.float32, N + 4, fill=o["bias"][None])
        bk = None
        if route.startswith("ks"):
            w = o["B"].t().contiguous()                   # W [N, K]
            ks = w.view(N, K // 32, 32).permute(1, 0, 2).reshape(1, -1) if K % 32 == 0 else torch.zeros(1, N * K, dtype=dt)
            bk = Guarded(1, N * K, dt, N * K + 8, fill=ks)
        acc, P = GB.products(o["A"].cuda(), o["B"].cuda())
        _operand_cache[key] = (o, A, B, bias, bk, acc, P)
    return _operand_cache[key]


def _matrix():
    out = []
    for route, layout, mnk, ldc in GB.route_cases():
        for epi in GB.route_epilogues(route):
            out.append(pytest.param(route, layout, mnk, ldc, epi, id=f"{GB.case_id(route, layout, mnk, ldc)}-{epi}"))
    return out


def _launch(ops, route, layout, mnk, ldc, epi, o, A, B, bias, bk):
    """Force the route, confirm it with the route query, run one call.  Returns (out, aux or None, every guarded buffer, reference inputs)."""
    M, N, K = mnk
    kind, rest = epi.split("_", 1)
    ta, tb = layout[0] == "T", layout[1] == "T"
    odt = torch.float32 if ("f32" in rest or kind == "atomic") else torch.bfloat16
    splitk = int(rest[1:]) if kind == "atomic" else 1
    use_bias = rest.endswith("_bias") or kind in ("gelu", "resid")
    from csmae_hip import EPI_ATOMIC, EPI_DGELU, EPI_GELU, EPI_NONE, EPI_RESID
    code = dict(none=EPI_NONE, gelu=EPI_GELU, resid=EPI_RESID, dgelu=EPI_DGELU, atomic=EPI_ATOMIC)[kind]
    bufs, aux, resid, c0 = [A, B, bias], None, None, None
    if kind == "atomic":
        out = Guarded(M, N, odt, ldc, fill=o["C0"])
        c0 = o["C0"]
    elif kind == "resid" and rest.endswith("inplace"):
        out = Guarded(M, N, odt, ldc, fill=o["R"])
        resid = out
    else:
        out = Guarded(M, N, odt, ldc)
    if kind == "resid" and resid is None:
        resid = Guarded(M, N, odt, ldc, fill=o["R"])
        bufs.append(resid)
    if kind == "gelu":
        adt = torch.uint8 if rest == "u8" else odt
        aux = Guarded(M, N, adt, ldc, fill=255 if adt == torch.uint8 else None)   # (255: no code the kernel writes)
    elif kind == "dgelu":
        if rest == "u8":
            aux = Guarded(M, N, torch.uint8, ldc, fill=o["codes"])
        else:
            aux = Guarded(M, N, odt, ldc, fill=o["gp"])
    bufs.append(out)
    if aux is not None:
        bufs.append(aux)
    kw = dict(bias=bias.vec if use_bias else None, epilogue=code, aux=aux.t if aux is not None else None, resid=resid.t if resid is not None else None)
    _force(route)
    want_route = GB.expected_route(route, mnk)
    if route.startswith("ks"):
        got_route = ops.gemm_ks_route(A.t, bk.vec, B.t, out.t, epilogue=code, aux=kw["aux"])
    else:
        got_route = ops.gemm_route(A.t, B.t, out.t, trans_a=ta, trans_b=tb, epilogue=code, aux=kw["aux"], splitk=splitk)
    assert got_route == want_route, f"route {got_route}, expected {want_route}"
    if route.startswith("ks"):
        ops.gemm_ks(A.t, bk.vec, B.t, out.t, **kw)
    else:
        ops.gemm(A.t, B.t, out.t, trans_a=ta, trans_b=tb, splitk=splitk, **kw)
    return out, aux, bufs, dict(kind=kind, rest=rest, odt=odt, splitk=splitk, use_bias=use_bias, c0=c0)


@pytest.mark.parametrize("route,layout,mnk,ldc,epi", _matrix())
def test_gemm_route_matrix(ops, route, layout, mnk, ldc, epi):
    M, N, K = mnk
    o, A, B, bias, bk, acc, P = _case_operands(route, layout, mnk)
    out, aux, bufs, r = _launch(ops, route, layout, mnk, ldc, epi, o, A, B, bias, bk)
    torch.cuda.synchronize()
    for gb in bufs:
        assert gb.outside_intact(), f"a write outside a tensor's view ({gb.rows}x{gb.cols}, ld {gb.ld}, {gb.dtype})"
    kind, rest, odt = r["kind"], r["rest"], r["odt"]
    b = o["bias"].cuda() if r["use_bias"] else None
    if kind == "gelu":
        (h, bh), (g, bg) = GB.reference("gelu", acc, P, K, out_dtype=odt, bias=b)
        _check("gelu out", out.t, h, bh)
        if aux.dtype == torch.uint8:
            _check("gelu' code", (aux.t.double() - 26.0) / 200.0, g, bg + GB.Q8_HALF_STEP)
        else:
            u = U16 if aux.dtype == torch.bfloat16 else U32
            _check("gelu' aux", aux.t, g, u * (g.abs() + bg) + bg)
        return
    if kind == "none":
        R, bound = GB.reference("none", acc, P, K, out_dtype=odt, bias=b)
    elif kind == "resid":
        R, bound = GB.reference("resid", acc, P, K, out_dtype=odt, bias=b, resid=o["R"].to(odt).cuda())
    elif kind == "dgelu":
        a = ((o["codes"].double() - 26.0) / 200.0) if rest == "u8" else o["gp"].to(odt)
        R, bound = GB.reference("dgelu", acc, P, K, out_dtype=odt, aux=a.cuda())
    else:
        R, bound = GB.reference("atomic", acc, P, K, out_dtype=odt, c0=r["c0"].cuda(), splitk=r["splitk"])
    _check(epi, out.t, R, bound)
    # the two-workgroups-per-CU kernels promise the one-workgroup kernel's bits (same MFMA shape, same K order): csrc/gemm_k2.hip
    if route in ("cfg6", "ks_k2") and kind != "atomic":
        import csmae_hip
        lib = csmae_hip.load()
        lib.csmae_gemm_force_tile(4)
        lib.csmae_gemm_k2_mode(0, 0)
        out2, aux2, _, _ = _launch_plain(ops, route, layout, mnk, ldc, epi, o, A, B, bias)
        assert torch.equal(out.t.view(torch.int16 if odt == torch.bfloat16 else torch.int32), out2.t.view(torch.int16 if odt == torch.bfloat16 else torch.int32)), \
            "k2 result differs from the one-workgroup kernel's"


def _launch_plain(ops, route, layout, mnk, ldc, epi, o, A, B, bias):
    """The same call on the one-workgroup pipelined kernel (route 4) through csmae_gemm: B as the k2 call's plain weight / K-strided operand."""
    from csmae_hip import EPI_DGELU, EPI_GELU, EPI_NONE, EPI_RESID
    M, N, K = mnk
    kind, rest = epi.split("_", 1)
    odt = torch.float32 if "f32" in rest else torch.bfloat16
    code = dict(none=EPI_NONE, gelu=EPI_GELU, resid=EPI_RESID, dgelu=EPI_DGELU)[kind]
    out = Guarded(M, N, odt, ldc, fill=o["R"] if rest.endswith("inplace") else None)
    resid = out if rest.endswith("inplace") else (Guarded(M, N, odt, ldc, fill=o["R"]) if kind == "resid" else None)
    aux = None
    if kind == "dgelu":
        aux = Guarded(M, N, torch.uint8, ldc, fill=o["codes"]) if rest == "u8" else Guarded(M, N, odt, ldc, fill=o["gp"])
    tb = layout[1] == "T"
    use_bias = rest.endswith("_bias") or kind == "resid"
    assert ops.gemm_route(A.t, B.t, out.t, trans_b=tb, epilogue=code) == 4
    ops.gemm(A.t, B.t, out.t, trans_b=tb, bias=bias.vec if use_bias else None, epilogue=code, aux=aux.t if aux is not None else None,
             resid=resid.t if resid is not None else None)
    return out, aux, None, None


@pytest.mark.parametrize("forced", [6, -1])
def test_k2_route_leaves_atomic_products_to_the_pipelined_kernel(ops, forced):
    """An accumulating (ATOMIC) dX-layout product never runs on the two-workgroups-per-CU kernel: its epilogue has no accumulating store and
    overwrote C with the product (csmae_gemm with EPI_ATOMIC, K-strided B, split-K 1, M >= 128, N >= 256, K % 64 == 0 — also under the
    heuristic, at K <= 512).  Forced or not, the product goes to a pipelined one-workgroup kernel and accumulates."""
    import csmae_hip
    from csmae_hip import EPI_ATOMIC
    lib = csmae_hip.load()
    lib.csmae_gemm_force_tile(forced)
    M, N, K = 300, 516, 192
    o = GB.operands("cfg6", "NT", (M, N, K))
    A = Guarded(M, K, torch.bfloat16, GB.ld_for(K), fill=o["A"])
    B = Guarded(K, N, torch.bfloat16, GB.ld_for(N), fill=o["B"])
    out = Guarded(M, N, torch.float32, N + 4, fill=o["C0"])
    route = ops.gemm_route(A.t, B.t, out.t, trans_b=True, epilogue=EPI_ATOMIC)
    assert route == 4 if forced == 6 else route in (4, 5), route   # (the heuristic picks the 192-row tiles here)
    ops.gemm(A.t, B.t, out.t, trans_b=True, epilogue=EPI_ATOMIC)
    acc, P = GB.products(o["A"].cuda(), o["B"].cuda())
    R, bound = GB.reference("atomic", acc, P, K, out_dtype=torch.float32, c0=o["C0"].cuda())
    assert out.outside_intact()
    _check("atomic on the dX layout", out.t, R, bound)


# ------------------------------------------------------------------------------------------------ fp8 products
FP8_CASES = [("pipe", (256, 256, 128)), ("pipe", (257, 260, 256)), ("pipe", (300, 4, 128)), ("pipe", (520, 516, 384)),
             ("twostage", (257, 260, 144)), ("twostage", (64, 4, 16)), ("twostage", (520, 516, 400))]
FP8_EPIS = ("none_f32_bias", "none_bf16_bias", "resid_bf16", "gelu_bf16", "gelu_u8", "dgelu_bf16", "dgelu_u8", "emit_none", "emit_dgelu", "emit_skip")
_fp8_cache = {}


def _fp8_operands(mnk):
    if mnk not in _fp8_cache:
        _fp8_cache.clear()
        M, N, K = mnk
        g = torch.Generator().manual_seed(5000 + M + 3 * N + 7 * K)
        a8 = (torch.randn(M, K, generator=g) * 40).to(torch.float8_e4m3fn)
        b8 = (torch.randn(N, K, generator=g) * 40).to(torch.float8_e4m3fn)
        A = Guarded(M, K, torch.uint8, GB.ld_for(K, 16, 16), sentinel=GB.FP8_NAN, fill=a8.view(torch.uint8))
        B = Guarded(N, K, torch.uint8, GB.ld_for(K, 16, 16), sentinel=GB.FP8_NAN, fill=b8.view(torch.uint8))
        dqa, dqb = torch.tensor([0.0137], device="cuda"), torch.tensor([0.0021 * K ** -0.5], device="cuda")
        s = float(dqa) * float(dqb)
        acc, P = GB.products(a8.float().cuda(), b8.float().t().cuda())
        o = GB.operands("cfg4", "NN", mnk, seed=1)
        _fp8_cache[mnk] = (o, A, B, dqa, dqb, acc * s, P * s)
    return _fp8_cache[mnk]


@pytest.mark.parametrize("epi", FP8_EPIS)
@pytest.mark.parametrize("kernel,mnk", FP8_CASES, ids=[f"{k}-{m}x{n}x{kk}" for k, (m, n, kk) in FP8_CASES])
def test_gemm_fp8_guarded(ops, kernel, mnk, epi):
    """csmae_gemm_fp8 on its pipelined kernel (K % 128 == 0) and its two-stage kernel (K % 16 == 0, K % 128 != 0): dq_a dq_b A8 B8^T against fp64
    on the same fp8 values, every epilogue, the fused fp8 copy (q_out: delayed scaling, saturating) with and without the bf16 output."""
    from csmae_hip import EPI_DGELU, EPI_GELU, EPI_NONE, EPI_RESID
    M, N, K = mnk
    assert (K % 128 == 0) == (kernel == "pipe")
    o, A, B, dqa, dqb, acc, P = _fp8_operands(mnk)
    kind, rest = epi.split("_", 1)
    emit = kind == "emit"
    odt = torch.float32 if "f32" in rest else torch.bfloat16
    ldc = GB.ld_for(N) if emit else N + (12 if M > 512 else (8 if N % 8 == 0 else 4))
    bias = Guarded(1, N, torch.float32, N + 4, fill=o["bias"][None])
    out = Guarded(M, N, odt, ldc)
    bufs, aux, resid = [A, B, bias, out], None, None
    if kind == "resid":
        resid = Guarded(M, N, odt, ldc, fill=o["R"]); bufs.append(resid)
    base_kind = "dgelu" if rest == "dgelu" else ("none" if emit else kind)
    if base_kind == "gelu":
        aux = Guarded(M, N, torch.uint8 if rest == "u8" else odt, ldc, fill=255 if rest == "u8" else None)
    elif base_kind == "dgelu":
        aux = Guarded(M, N, torch.uint8, ldc, fill=o["codes"]) if rest == "u8" else Guarded(M, N, odt, ldc, fill=o["gp"])
    if aux is not None:
        bufs.append(aux)
    code = dict(none=EPI_NONE, gelu=EPI_GELU, resid=EPI_RESID, dgelu=EPI_DGELU)[base_kind]
    use_bias = base_kind != "dgelu"
    em = None
    if emit:
        R0 = acc + (o["bias"].double().cuda() if use_bias else 0.0)
        if base_kind == "dgelu":
            R0 = acc * o["gp"].to(odt).double().cuda()
        prev = torch.zeros(64, device="cuda"); prev[17] = 0.8 * float(R0.abs().max())   # (below today's maximum: the saturation path)
        q = Guarded(M, N, torch.uint8, GB.ld_for(N))
        nxt, dqo = torch.zeros(64, device="cuda"), torch.zeros(1, device="cuda")
        em = (q.t, 0, prev, nxt, dqo)
        bufs.append(q)
    ops.gemm_fp8(A.t, B.t, out.t, dqa, dqb, a_fmt=0, bias=bias.vec if use_bias else None, epilogue=code, aux=aux.t if aux is not None else None,
                 resid=resid.t if resid is not None else None, emit=em, skip_out=rest == "skip")
    torch.cuda.synchronize()
    for gb in bufs:
        assert gb.outside_intact(), f"a write outside a tensor's view ({gb.rows}x{gb.cols}, ld {gb.ld}, {gb.dtype})"
    b = o["bias"].cuda() if use_bias else None
    if base_kind == "gelu":
        (h, bh), (g, bg) = GB.reference("gelu", acc, P, K, out_dtype=odt, bias=b, fp8=True)
        _check("fp8 gelu out", out.t, h, bh)
        if rest == "u8":
            _check("fp8 gelu' code", (aux.t.double() - 26.0) / 200.0, g, bg + GB.Q8_HALF_STEP)
        else:
            _check("fp8 gelu' aux", aux.t, g, U16 * (g.abs() + bg) + bg)
        return
    if base_kind == "none":
        R, bound = GB.reference("none", acc, P, K, out_dtype=odt, bias=b, fp8=True)
    elif base_kind == "resid":
        R, bound = GB.reference("resid", acc, P, K, out_dtype=odt, bias=b, resid=o["R"].to(odt).cuda(), fp8=True)
    else:
        a = ((o["codes"].double() - 26.0) / 200.0) if rest == "u8" else o["gp"].to(odt)
        R, bound = GB.reference("dgelu", acc, P, K, out_dtype=odt, aux=a.cuda(), fp8=True)
    if rest == "skip":
        assert out.untouched(), "skip_out: the bf16 output was written"
    else:
        _check(f"fp8 {epi}", out.t, R, bound)
    if emit:
        am = float(prev.max())
        assert float(dqo) == float(torch.tensor(am, dtype=torch.float32) / 448.0), (float(dqo), am)
        i = int(R.abs().reshape(-1).argmax())
        assert abs(float(nxt.max()) - float(R.abs().reshape(-1)[i])) <= float(bound.reshape(-1)[i]), "amax_next is not this product's max |C|"
        want = R.clamp(-am, am)
        deq = q.t.view(torch.float8_e4m3fn).double() * float(dqo)
        qb = 2.0 ** -4 * (want.abs() + bound) + am / 448.0 * 2.0 ** -10 + bound   # e4m3: half a step (3 mantissa bits; subnormal step 2^-9)
        _check("fp8 copy", deq, want, qb)


# ------------------------------------------------------------------------------------------------ LayerNorm-fused products
LN_CASES = [(128, 512, 64), (129, 256, 128), (300, 384, 192)]


def _vec(x, pad=4):
    return Guarded(1, x.numel(), x.dtype, x.numel() + pad, fill=x.reshape(1, -1))


@pytest.mark.parametrize("mnk", LN_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in LN_CASES])
def test_gemm_ln_fwd_guarded(ops, mnk):
    """csmae_gemm_ln_fwd: X = A Wk^T + bias + resid, Y = LayerNorm(X), mean / rstd — X against fp64, the statistics and Y against fp64 of the
    kernel's own X; every output inside guards."""
    M, N, K = mnk
    assert ops.gemm_ln_supported(M, N, K)
    g = torch.Generator().manual_seed(6000 + M)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    bias, gam, bet = torch.randn(N, generator=g) * 0.1, torch.randn(N, generator=g) * 0.2 + 1.0, torch.randn(N, generator=g) * 0.1
    res = (torch.randn(M, N, generator=g) * 2 + 0.5).to(torch.bfloat16)
    A = Guarded(M, K, torch.bfloat16, GB.ld_for(K), fill=a)
    Wk = _vec(w.view(N, K // 32, 32).permute(1, 0, 2).contiguous(), 8)
    Bi, Ga, Be = _vec(bias), _vec(gam), _vec(bet)
    Rs = Guarded(M, N, torch.bfloat16, N + 8, fill=res)
    X, Y = Guarded(M, N, torch.bfloat16, N + 8), Guarded(M, N, torch.bfloat16, N + 8)
    Mu, Rstd = Guarded(1, M, torch.float32, M + 4), Guarded(1, M, torch.float32, M + 4)
    ops.gemm_ln_fwd(A.t, Wk.vec, Bi.vec, Rs.t, X.t, Ga.vec, Be.vec, Y.t, Mu.vec, Rstd.vec)
    torch.cuda.synchronize()
    for gb in (A, Wk, Bi, Ga, Be, Rs, X, Y, Mu, Rstd):
        assert gb.outside_intact(), f"a write outside a tensor's view ({gb.rows}x{gb.cols}, ld {gb.ld}, {gb.dtype})"
    acc, P = GB.products(a.cuda(), w.t().cuda())
    R, bound = GB.reference("resid", acc, P, K, out_dtype=torch.bfloat16, bias=bias.cuda(), resid=res.cuda())
    _check("gemm_ln_fwd x", X.t, R, bound)
    x = X.t.double()
    m64 = x.mean(1)
    var = ((x - m64[:, None]) ** 2).mean(1)
    r64 = (var + 1e-6).rsqrt()
    em = (N + 4) * U32 * x.abs().mean(1)                                    # fp32 row sum of N values, one division
    er = r64 * (0.5 * (N + 8) * U32 * (x * x).mean(1) / (var + 1e-6) + 4 * U32)   # variance to (N + 8) ulps of E[x^2], rsqrt to a few ulps
    _check("gemm_ln_fwd mean", Mu.vec[None], m64[None], em[None])
    _check("gemm_ln_fwd rstd", Rstd.vec[None], r64[None], er[None])
    xh = (x - m64[:, None]) * r64[:, None]
    ga, be = gam.double().cuda(), bet.double().cuda()
    y = xh * ga + be
    ey = ga.abs() * (r64[:, None] * em[:, None] + (x - m64[:, None]).abs() * er[:, None]) + 4 * U32 * ((xh * ga).abs() + be.abs())
    _check("gemm_ln_fwd y", Y.t, y, U16 * (y.abs() + ey) + ey)


@pytest.mark.parametrize("with_dres", [True, False], ids=["dres", "nodres"])
@pytest.mark.parametrize("mnk", LN_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in LN_CASES])
def test_gemm_ln_bwd_guarded(ops, mnk, with_dres):
    """csmae_gemm_ln_bwd: dx = LayerNorm'(dY W) + dres (the product rounded to bf16 first, as the two-kernel path it replaces) and the tiles'
    dgamma / dbeta partial rows, against fp64 with the product's rounding carried through; every output inside guards."""
    M, N, K = mnk
    g = torch.Generator().manual_seed(7000 + M)
    dy = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(K, N, generator=g) * K ** -0.5).to(torch.bfloat16)
    x = (torch.randn(M, N, generator=g) * 2 + 0.5).to(torch.bfloat16)
    gam = torch.randn(N, generator=g) * 0.2 + 1.0
    dres = torch.randn(M, N, generator=g).to(torch.bfloat16)
    xd = x.double()
    mean = xd.mean(1).float()
    rstd = ((xd - xd.mean(1, keepdim=True)) ** 2).mean(1).add(1e-6).rsqrt().float()
    DY = Guarded(M, K, torch.bfloat16, GB.ld_for(K), fill=dy)
    W = Guarded(K, N, torch.bfloat16, N + 8, fill=w)
    Xg = Guarded(M, N, torch.bfloat16, N + 8, fill=x)
    Mu, Rs, Ga = _vec(mean), _vec(rstd), _vec(gam)
    Dr = Guarded(M, N, torch.bfloat16, N + 8, fill=dres) if with_dres else None
    DX = Guarded(M, N, torch.bfloat16, N + 8)
    rows = -(-M // 128)
    Part = Guarded(1, rows * 2 * N, torch.float32, rows * 2 * N + 8)
    ops.gemm_ln_bwd(DY.t, W.t, Xg.t, Mu.vec, Rs.vec, Ga.vec, Dr.t if with_dres else None, DX.t, partial_ws=Part.vec)
    torch.cuda.synchronize()
    for gb in [DY, W, Xg, Mu, Rs, Ga, DX, Part] + ([Dr] if with_dres else []):
        assert gb.outside_intact(), f"a write outside a tensor's view ({gb.rows}x{gb.cols}, ld {gb.ld}, {gb.dtype})"
    t, P = GB.products(dy.cuda(), w.cuda())
    et = U16 * t.abs() + (1 + U16) * (K + 8) * U32 * P                     # the product, accumulated in fp32 and rounded to bf16
    xh = (xd.cuda() - mean.double().cuda()[:, None]) * rstd.double().cuda()[:, None]
    r = rstd.double().cuda()[:, None]
    ga = gam.double().cuda()
    gt = ga * t
    want = r * (gt - gt.mean(1, keepdim=True) - xh * (gt * xh).mean(1, keepdim=True)) + (dres.double().cuda() if with_dres else 0.0)
    eg = ga.abs() * et
    e = r * (eg + eg.mean(1, keepdim=True) + xh.abs() * (eg * xh.abs()).mean(1, keepdim=True))
    e = e + (N + 8) * U32 * r * (gt.abs() + gt.abs().mean(1, keepdim=True) + xh.abs() * (gt * xh).abs().mean(1, keepdim=True) + 1e-30)
    if with_dres:
        e = e + U32 * (want.abs() + dres.double().cuda().abs())
    _check("gemm_ln_bwd dx", DX.t, want, U16 * (want.abs() + e) + e)
    part = Part.vec.view(rows, 2, N)
    pad = rows * 128 - M
    tp = torch.cat([t, t.new_zeros(pad, N)]).view(rows, 128, N)
    xp = torch.cat([xh, xh.new_zeros(pad, N)]).view(rows, 128, N)
    ep = torch.cat([et, et.new_zeros(pad, N)]).view(rows, 128, N)
    dg, db = (tp * xp).sum(1), tp.sum(1)
    edg = (ep * xp.abs()).sum(1) + (128 + 8) * U32 * (tp * xp).abs().sum(1)
    edb = ep.sum(1) + (128 + 8) * U32 * tp.abs().sum(1)
    _check("gemm_ln_bwd dgamma partial rows", part[:, 0], dg, edg)
    _check("gemm_ln_bwd dbeta partial rows", part[:, 1], db, edb)


# ------------------------------------------------------------------------------------------------ weight gradients
class Slabs:
    """Several fp32 tensors in ONE allocation with 64 sentinel elements before, between and after them (dW / db of weight gradients)."""
    G = 64

    def __init__(self, tensors):
        sizes = [t.numel() for t in tensors]
        self.ibase = torch.full((sum(sizes) + self.G * (len(sizes) + 1),), GB.SENTINEL[torch.float32], dtype=torch.int32, device="cuda")
        base = self.ibase.view(torch.float32)
        self.views, self.spans, off = [], [], self.G
        for t, n in zip(tensors, sizes):
            v = base[off:off + n].view(t.shape)
            v.copy_(t)
            self.views.append(v)
            self.spans.append((off, n))
            off += n + self.G

    def outside_intact(self):
        c = self.ibase.clone()
        for off, n in self.spans:
            c[off:off + n] = GB.SENTINEL[torch.float32]
        return bool((c == GB.SENTINEL[torch.float32]).all())


def _dw_reference(dY, X, c0, db0, S):
    """dW = c0 + dY^T X, db = db0 + colsum(dY) in fp64 and their bounds: K products and S K-slices accumulated in fp32, one fold."""
    K = dY.shape[0]
    acc, P = GB.products(dY.t(), X)
    R, bound = GB.reference("atomic", acc, P, K, out_dtype=torch.float32, c0=c0, splitk=S)
    cs, csa = dY.double().sum(0), dY.double().abs().sum(0)
    Rb = db0.double() + cs
    bb = U32 * Rb.abs() + (K + 8 + S) * U32 * csa + (S + 1) * U32 * (db0.double().abs() + csa)
    return R, bound, Rb, bb


def _dw_inputs(K, M, N, dtype, seed, fp8=False):
    g = torch.Generator().manual_seed(seed)
    dy, x = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    c0, db0 = torch.randn(M, N, generator=g), torch.randn(M, generator=g)
    if fp8:
        dy8, x8 = (dy * 3).to(torch.float8_e5m2), (x * 30).to(torch.float8_e4m3fn)
        DY = Guarded(K, M, torch.uint8, GB.ld_for(M, 16, 16), sentinel=GB.FP8_NAN, fill=dy8.view(torch.uint8))
        XX = Guarded(K, N, torch.uint8, GB.ld_for(N, 16, 16), sentinel=GB.FP8_NAN, fill=x8.view(torch.uint8))
        return DY, XX, dy8.float().cuda(), x8.float().cuda(), c0.cuda(), db0.cuda()
    dy, x = dy.to(dtype), x.to(dtype)
    DY, XX = Guarded(K, M, dtype, GB.ld_for(M), fill=dy), Guarded(K, N, dtype, GB.ld_for(N), fill=x)
    return DY, XX, dy.cuda(), x.cuda(), c0.cuda(), db0.cuda()


DW_CASES = [("bf16", (256, 256, 300)), ("bf16", (100, 68, 1000)), ("bf16", (520, 264, 616)), ("f32", (64, 48, 1000))]


@pytest.mark.parametrize("dt,mnk", DW_CASES, ids=[f"{d}-{m}x{n}x{k}" for d, (m, n, k) in DW_CASES])
def test_gemm_dw_guarded(ops, dt, mnk):
    """csmae_gemm_dw: dW += dY^T X and db += colsum(dY) through split-K slabs, dW and db inside one guarded allocation, operands NaN-padded."""
    M, N, K = mnk
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    DY, XX, dy, x, c0, db0 = _dw_inputs(K, M, N, dtype, 8000 + M)
    sl = Slabs([c0, db0])
    ws = torch.empty(M * N * 40 + 4096, device="cuda")
    ops.gemm_dw(DY.t, XX.t, sl.views[0], ws, db=sl.views[1])
    torch.cuda.synchronize()
    assert sl.outside_intact() and DY.outside_intact() and XX.outside_intact()
    R, b, Rb, bb = _dw_reference(dy, x, c0, db0, 64)
    _check("gemm_dw dW", sl.views[0], R, b)
    _check("gemm_dw db", sl.views[1][None], Rb[None], bb[None])


DWG_CASES = [("fused-1slice", "bf16", 1000, [(256, 256), (520, 264)], 160), ("fused-slices", "bf16", 1000, [(256, 256), (520, 264)], 16),
             ("fallback-small", "bf16", 1000, [(256, 256), (100, 68)], 160), ("fallback-f32", "f32", 600, [(256, 256), (64, 48)], 160)]


@pytest.mark.parametrize("name,dt,K,prods,slots", DWG_CASES, ids=[c[0] for c in DWG_CASES])
def test_gemm_dw_group_guarded(ops, name, dt, K, prods, slots):
    """csmae_gemm_dw_group fused (one launch; one K slice or several) and its per-product fallback (a product under 256, or fp32): every dW / db
    of the group inside one guarded allocation."""
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    ins = [_dw_inputs(K, M, N, dtype, 9000 + 10 * i + M) for i, (M, N) in enumerate(prods)]
    sl = Slabs([t for (_, _, _, _, c0, db0) in ins for t in (c0, db0)])
    ws = torch.empty(16 << 20, device="cuda")
    ops.DwGroup([(DY.t, XX.t, sl.views[2 * i], sl.views[2 * i + 1]) for i, (DY, XX, *_) in enumerate(ins)], ws).launch(slots)
    torch.cuda.synchronize()
    assert sl.outside_intact() and all(DY.outside_intact() and XX.outside_intact() for DY, XX, *_ in ins)
    for i, (DY, XX, dy, x, c0, db0) in enumerate(ins):
        R, b, Rb, bb = _dw_reference(dy, x, c0, db0, 64)
        _check(f"dw_group dW {i}", sl.views[2 * i], R, b)
        _check(f"dw_group db {i}", sl.views[2 * i + 1][None], Rb[None], bb[None])


@pytest.mark.parametrize("K", [512, 131])
def test_gemm_dw_group_fp8_guarded(ops, K):
    """csmae_gemm_dw_group_fp8: dW += dq_y dq_x dY8^T X8, db += dq_y colsum(dY8), NaN-padded fp8 operands, dW / db inside one guarded allocation."""
    prods = [(256, 256), (520, 272)]
    ins = [_dw_inputs(K, M, N, None, 9500 + M, fp8=True) for M, N in prods]
    dq = [(torch.tensor([0.37 + 0.1 * i], device="cuda"), torch.tensor([0.021], device="cuda")) for i in range(len(prods))]
    sl = Slabs([t for (_, _, _, _, c0, db0) in ins for t in (c0, db0)])
    ws = torch.empty(64 << 20, device="cuda")
    ops.DwGroup8([(DY.t, dqy, XX.t, dqx, sl.views[2 * i], sl.views[2 * i + 1]) for i, ((DY, XX, *_), (dqy, dqx)) in enumerate(zip(ins, dq))], ws).launch(16)
    torch.cuda.synchronize()
    assert sl.outside_intact() and all(DY.outside_intact() and XX.outside_intact() for DY, XX, *_ in ins)
    for i, ((DY, XX, dy, x, c0, db0), (dqy, dqx)) in enumerate(zip(ins, dq)):
        sy, sx = float(dqy), float(dqx)
        acc, P = GB.products(dy.t(), x)
        R, b = GB.reference("atomic", acc * (sy * sx), P * (sy * sx), K, out_dtype=torch.float32, c0=c0, splitk=64, fp8=True)
        _check(f"dw_group_fp8 dW {i}", sl.views[2 * i], R, b)
        cs, csa = dy.double().sum(0) * sy, dy.double().abs().sum(0) * sy
        Rb = db0.double() + cs
        bb = U32 * Rb.abs() + ((K + 72) * U32 + GB.FP8_MFMA_REL) * csa + 65 * U32 * (db0.double().abs() + csa)
        _check(f"dw_group_fp8 db {i}", sl.views[2 * i + 1][None], Rb[None], bb[None])
