"""csrc/norm.hip against fp64 in guarded buffers: the three LayerNorm kernels at every width bucket and its edges, every dtype route and
parameter-gradient form, waves that walk several rows, the partial-row fold alone, fp8 emission at masked widths, and BatchNorm+ReLU in
its three geometries (training twice, eval, misaligned operands, accumulating parameter gradients, a far shift).  Every operand and output
lives in a contiguous buffer with sentinel guard rows (tests/norm_ref.py); after each launch the guards are intact, no output element is
left unwritten, and every element is within the bound derived for it.  Each case prints its worst error / bound ratio (-s shows them).
Not covered: the packed backward's fall-back for tensors of 4 GB and more (four such tensors and tens of seconds per case do not belong
in this suite).  Needs an MI355X."""
import functools

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from csmae_hip import ops as o
    import csmae_hip
    csmae_hip.load()
    return o


def G(rows, cols, dtype, fill=None, off8=False):
    return R.Guarded(rows, cols, dtype, "cuda", fill, off8)


def V(n, fill=None, dtype=F32):
    return R.Guarded(1, n, dtype, "cuda", fill)


def settle(ins, outs):
    """After a launch: every guard intact, every input unchanged, no output element unwritten or NaN."""
    torch.cuda.synchronize()
    for name, (b, want) in ins.items():
        assert b.outside_intact(), f"{name}: written outside the view"
        assert torch.equal(b.t.cpu(), want.to(b.dtype).reshape(b.t.shape)), f"{name}: an input was changed"
    for name, b in outs.items():
        assert b.outside_intact(), f"{name}: written outside the view"
        assert b.unwritten() == 0, f"{name}: {b.unwritten()} elements left unwritten"
        if b.dtype != U8:
            assert not bool(torch.isnan(b.t).any()), f"{name}: NaN (a guard or an unwritten element was read)"


def within(worst, name, got, want, bound):
    got, want, bound = [t.reshape(1, -1) if t.dim() < 2 else t for t in (got.detach().cpu(), want, bound)]
    n, msg = R.violations(got, want, bound)
    ratio = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())
    worst[name] = max(worst.get(name, 0.0), ratio)
    assert n == 0, f"{name}: {msg} (ratio {ratio:.3f})"


def report(what, worst):
    print(f"{what}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def prior(n, seed):
    """Existing content of a parameter-gradient buffer."""
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 2.0 + 0.5


# ------------------------------------------------------------------------------------------------ LayerNorm forward
@functools.lru_cache(maxsize=None)
def fwd_ref(M, D, xdt):
    i = R.ln_inputs(M, D)
    return R.ln_fwd_ref(i["x"].to(xdt), i["gamma"], i["beta"])


def run_ln_fwd(ops, M, D, xdt, odt, with32, worst, emit=None):
    i, ref = R.ln_inputs(M, D), fwd_ref(M, D, xdt)
    x, gamma, beta = G(M, D, xdt, i["x"]), V(D, i["gamma"]), V(D, i["beta"])
    y, mean, rstd = G(M, D, odt), V(M), V(M)
    y32 = G(M, D, F32) if with32 else None
    ops.layernorm_fwd(x.t, gamma.vec, beta.vec, y.t, mean.vec, rstd.vec, y32=y32.t if with32 else None, emit=emit)
    outs = dict(y=y, mean=mean, rstd=rstd)
    if with32:
        outs["y32"] = y32
    settle(dict(x=(x, i["x"].to(xdt)), gamma=(gamma, i["gamma"]), beta=(beta, i["beta"])), outs)
    within(worst, "y", y.t, ref["y"], R.finish(ref["y"], ref["e_y"], odt))
    if with32:
        within(worst, "y32", y32.t, ref["y"], R.finish(ref["y"], ref["e_y"], F32))
    within(worst, "mean", mean.vec, ref["mean"], ref["b_mean"])
    within(worst, "rstd", rstd.vec, ref["rstd"], ref["b_rstd"])
    return y.t, mean.vec, rstd.vec


FWD_ROUTES = ((F32, BF), (F32, F32), (BF, BF))


@pytest.mark.parametrize("D", R.LN_WIDTHS)
def test_layernorm_forward(ops, D):
    for xdt, odt in FWD_ROUTES:
        worst = {}
        for M in R.LN_ROWS:
            for with32 in (True, False):
                run_ln_fwd(ops, M, D, xdt, odt, with32, worst)
        report(f"ln fwd D={D} {xdt}->{odt}", worst)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
# (dy, x / dres / dx, low-precision copy): the six GO(...) entries of csmae_layernorm_bwd
BWD_ROUTES = ((BF, BF, BF), (F32, BF, BF), (BF, F32, BF), (F32, F32, BF), (F32, F32, F32), (BF, F32, F32))
FORMS = ("atomic", "fold", "deferred")


def lp_optional(dydt, xdt, lpdt):
    """Without dx_lp the binding names dy's dtype as the copy's: the route is reached only where that is the route's own."""
    return xdt == BF or lpdt == dydt


@functools.lru_cache(maxsize=None)
def bwd_ref(M, D, dydt, xdt, dres, packed):
    i, f = R.ln_inputs(M, D), fwd_ref(M, D, xdt)
    mean, rstd = f["mean"].float(), f["rstd"].float()
    return mean, rstd, R.ln_bwd_ref(i["dy"].to(dydt), i["x"].to(xdt), mean, rstd, i["gamma"], i["dres"].to(xdt) if dres else None, packed)


def run_ln_bwd(ops, M, D, route, lp, dres, form, worst, ws_rows=64, emit=None):
    dydt, xdt, lpdt = route
    packed = route == (BF, BF, BF) and form == "deferred" and not lp and R.ln_packed(D)
    i = R.ln_inputs(M, D)
    mean_c, rstd_c, ref = bwd_ref(M, D, dydt, xdt, dres, packed)
    dy, x, gamma = G(M, D, dydt, i["dy"]), G(M, D, xdt, i["x"]), V(D, i["gamma"])
    mean, rstd = V(M, mean_c), V(M, rstd_c)
    dr = G(M, D, xdt, i["dres"]) if dres else None
    dx = G(M, D, xdt)
    dxlp = G(M, D, lpdt) if lp else None
    prev_g, prev_b = prior(D, 1), prior(D, 2)
    dg, db = (None, None) if form == "deferred" else (V(D, prev_g), V(D, prev_b))
    part = None if form == "atomic" else V(ws_rows * 2 * D)
    blocks = R.ln_bwd_blocks(M, D, part.n if part else None)
    ops.layernorm_bwd(dy.t, x.t, mean.vec, rstd.vec, gamma.vec, dx.t, dg.vec if dg else None, db.vec if db else None, dres_in=dr.t if dres else None,
                      dx_lp=dxlp.t if lp else None, partial_ws=part.vec if part else None, emit=emit)
    flat = None
    if form == "deferred":        # the fold as the engine runs it: a later launch with the same M, D and slice size, into a flat gradient buffer
        off_g, off_b = D + 8, 3 * D + 16
        prev_flat = prior(4 * D + 24, 3)
        prev_g, prev_b = prev_flat[off_g:off_g + D], prev_flat[off_b:off_b + D]
        flat = V(4 * D + 24, prev_flat)
        goff = torch.tensor([[off_g, off_b]], dtype=torch.long, device="cuda")
        ops.ln_param_reduce(1, M, D, part.t, goff, flat.vec)
    ins = dict(dy=(dy, i["dy"].to(dydt)), x=(x, i["x"].to(xdt)), gamma=(gamma, i["gamma"]), mean=(mean, mean_c), rstd=(rstd, rstd_c))
    if dres:
        ins["dres"] = (dr, i["dres"].to(xdt))
    outs = dict(dx=dx)
    if lp:
        outs["dx_lp"] = dxlp
    if dg:
        outs.update(dgamma=dg, dbeta=db)
    if flat:
        outs["flat"] = flat
    settle(ins, outs)
    if part:   # the rows the launch writes hold numbers; everything behind them still holds the sentinel (and was not read: no NaN came out)
        assert part.outside_intact()
        pb = part.bits()[0]
        assert int((pb[:blocks * 2 * D] == part.sentinel).sum()) == 0 and not bool(torch.isnan(part.vec[:blocks * 2 * D]).any()), "partial rows unwritten"
        assert bool((pb[blocks * 2 * D:] == part.sentinel).all()), "written behind the launch's partial rows"
    within(worst, "dx", dx.t, ref["dx"], R.finish(ref["dx"], ref["e_dx"], xdt))
    if lp:
        within(worst, "dx_lp", dxlp.t, ref["dx"], R.finish(ref["dx"], ref["e_dx"], lpdt))
    depth = R.ln_param_depth(M, blocks, form == "atomic")
    got_g, got_b = (flat.vec[off_g:off_g + D], flat.vec[off_b:off_b + D]) if flat else (dg.vec, db.vec)
    within(worst, "dgamma", got_g, prev_g.double() + ref["dgamma"], R.param_bound(depth, ref["abs_g"], ref["e_g"], prev_g))
    within(worst, "dbeta", got_b, prev_b.double() + ref["dbeta"], R.param_bound(depth, ref["abs_b"], ref["e_b"], prev_b))
    if flat:
        keep = torch.ones(flat.n, dtype=torch.bool)
        keep[off_g:off_g + D] = False
        keep[off_b:off_b + D] = False
        assert torch.equal(flat.vec.cpu()[keep], prev_flat[keep]), "the fold wrote outside dgamma / dbeta"
    return dict(dx=dx.t.clone(), params=torch.cat([got_g, got_b]).clone(), packed=packed)


@pytest.mark.parametrize("D", R.LN_WIDTHS)
def test_layernorm_backward(ops, D):
    """Every route at every width, the options rotating so that each route meets each parameter-gradient form, dres_in present and absent,
    the copy present and absent; then the all-bf16 deferred form (the packed kernel for 256 < D <= 1280, the generic one outside)."""
    for ri, route in enumerate(BWD_ROUTES):
        worst = {}
        for mi, M in enumerate(R.LN_ROWS):
            run_ln_bwd(ops, M, D, route, True, True, FORMS[(ri + mi) % 3], worst)
            run_ln_bwd(ops, M, D, route, not lp_optional(*route), False, FORMS[(ri + mi + 1) % 3], worst)
        report(f"ln bwd D={D} dy {route[0]} x {route[1]} lp {route[2]}", worst)
    worst, packed = {}, set()
    for M in R.LN_ROWS:
        for dres in (True, False):
            packed.add(run_ln_bwd(ops, M, D, (BF, BF, BF), False, dres, "deferred", worst)["packed"])
    assert packed == {R.ln_packed(D)}
    report(f"ln bwd D={D} all-bf16 deferred ({'packed' if R.ln_packed(D) else 'generic'} kernel)", worst)


@pytest.mark.parametrize("D", [260, 512])
def test_layernorm_backward_full_product(ops, D):
    """A ragged and an exact width: route x copy x dres_in x parameter-gradient form in full."""
    for route in BWD_ROUTES:
        worst = {}
        for lp in (True, False):
            if not lp and not lp_optional(*route):
                continue
            for dres in (True, False):
                for form in FORMS:
                    run_ln_bwd(ops, 5, D, route, lp, dres, form, worst)
        report(f"ln bwd product D={D} dy {route[0]} x {route[1]} lp {route[2]}", worst)


def test_layernorm_refuses_unsupported_widths(ops):
    for D in (2052, 6):
        x, y, mean, rstd, gamma = G(3, D, F32, 1.0), G(3, D, F32), V(3), V(3), V(D, 1.0)
        with pytest.raises(RuntimeError):
            ops.layernorm_fwd(x.t, gamma.vec, gamma.vec, y.t, mean.vec, rstd.vec)
        dx, dg, db = G(3, D, F32), V(D), V(D)
        with pytest.raises(RuntimeError):
            ops.layernorm_bwd(x.t, x.t, gamma.vec[:3], gamma.vec[:3], gamma.vec, dx.t, dg.vec, db.vec)
        torch.cuda.synchronize()
        for b in (y, mean, rstd, dx, dg, db):
            assert b.untouched()                  # refused before any launch


# ------------------------------------------------------------------------------------------------ rows per wave
@pytest.mark.parametrize("D", [64, 260])
@pytest.mark.parametrize("ws_rows", R.LN_WS_ROWS)
def test_layernorm_backward_workspace_limited_grid(ops, D, ws_rows):
    """M = 37 under a workspace of 1, 2, 3 and 10 partial rows: each wave walks 10, 5, 4 rows or one; the deferred fold must agree with
    the launch on the row count."""
    worst = {}
    for route, form in (((BF, BF, BF), "deferred"), ((F32, F32, F32), "fold"), ((F32, F32, F32), "deferred")):
        a = run_ln_bwd(ops, 37, D, route, False, True, form, worst, ws_rows=ws_rows)
        b = run_ln_bwd(ops, 37, D, route, False, True, form, worst, ws_rows=ws_rows)
        assert torch.equal(a["dx"], b["dx"]) and torch.equal(a["params"], b["params"]), "two runs differ"
    a = run_ln_bwd(ops, 37, D, (BF, BF, BF), False, False, "deferred", worst, ws_rows=ws_rows)
    assert a["packed"] == (D == 260)
    report(f"ln bwd M=37 D={D} workspace of {ws_rows} rows", worst)


@pytest.mark.parametrize("M,D", R.LN_LONG)
def test_layernorm_backward_capped_grid(ops, M, D):
    """M = 4100: 1025 row quads on a grid capped at 1024 blocks; the workspace holds more rows than the launch writes."""
    worst = {}
    for route, form in (((BF, BF, BF), "deferred"), ((F32, F32, F32), "deferred"), ((F32, F32, F32), "atomic")):
        a = run_ln_bwd(ops, M, D, route, False, True, form, worst, ws_rows=1030)
        if form == "deferred":
            b = run_ln_bwd(ops, M, D, route, False, True, form, worst, ws_rows=1030)
            assert torch.equal(a["dx"], b["dx"]) and torch.equal(a["params"], b["params"]), "two runs differ"
    report(f"ln bwd M={M} D={D}", worst)


# ------------------------------------------------------------------------------------------------ fp8 emission
def emit_buffers(amax):
    prev = torch.zeros(64)
    prev[5] = amax
    return V(64, prev), V(64, 0.0), V(1, 0.0)


def check_emission(out, q, fmt, prev, nxt, dq, clamp):
    """The assertion form of test_layernorm_emits_fp8_copy: dq = amax / fmax, the dequantised copy within the format's step, amax recorded."""
    edt, fmax = (torch.float8_e4m3fn, 448.0) if fmt == 0 else (torch.float8_e5m2, 57344.0)
    for b in (q, prev, nxt, dq):
        assert b.outside_intact()
    am = float(prev.vec.max())
    assert abs(float(dq.vec) - am / fmax) <= 1e-6 * am / fmax
    assert abs(float(nxt.vec.max()) - float(out.float().abs().max())) <= 8e-3 * float(nxt.vec.max())
    deq = q.t.view(edt).float().cpu() * float(dq.vec)
    want = out.float().cpu()
    if clamp:
        want = want.clamp(-am, am)
    tol = (0.0625 if fmt == 0 else 0.125) * want.abs() + am * (2.0 ** -9 if fmt == 0 else 2.0 ** -16) + 8e-3 * want.abs()
    assert bool(((deq - want).abs() <= tol).all()), "fp8 copy outside the format's step"


def emitting_forward(ops, M, D, fmt):
    worst = {}
    y0, mean0, rstd0 = run_ln_fwd(ops, M, D, BF, BF, False, worst)
    q = G(M, D, U8)
    prev, nxt, dq = emit_buffers(0.9 * float(y0.float().abs().max()))      # a stale amax: some values clamp
    y1, mean1, rstd1 = run_ln_fwd(ops, M, D, BF, BF, False, worst, emit=(q.t, fmt, prev.vec, nxt.vec, dq.vec))
    assert torch.equal(y0, y1) and torch.equal(mean0, mean1) and torch.equal(rstd0, rstd1)
    check_emission(y1, q, fmt, prev, nxt, dq, True)
    return worst


def emitting_packed_backward(ops, M, D, fmt):
    worst = {}
    a = run_ln_bwd(ops, M, D, (BF, BF, BF), False, True, "deferred", worst)
    assert a["packed"]
    q = G(M, D, U8)
    prev, nxt, dq = emit_buffers(1.1 * float(a["dx"].float().abs().max()))
    b = run_ln_bwd(ops, M, D, (BF, BF, BF), False, True, "deferred", worst, emit=(q.t, fmt, prev.vec, nxt.vec, dq.vec))
    assert torch.equal(a["dx"], b["dx"]) and torch.equal(a["params"], b["params"])
    check_emission(b["dx"], q, fmt, prev, nxt, dq, False)
    return worst


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("D", [260, 516])
def test_fp8_emission_at_masked_widths(ops, D, fmt):
    worst = emitting_forward(ops, 37, D, fmt)
    report(f"ln fwd + fp8 copy D={D} fmt {fmt}", worst)
    worst = emitting_packed_backward(ops, 37, D, fmt)
    report(f"packed ln bwd + fp8 copy D={D} fmt {fmt}", worst)


@pytest.mark.parametrize("M,D", R.LN_LONG_EMIT)
def test_layernorm_forward_emitting_capped_grid(ops, M, D):
    """M = 8197 with an fp8 copy: 2050 row quads on a grid capped at 2048 blocks, so two blocks' waves take a second row."""
    report(f"ln fwd + fp8 copy M={M} D={D}", emitting_forward(ops, M, D, 0))


# ------------------------------------------------------------------------------------------------ the fold alone
@pytest.mark.parametrize("rows", R.FOLD_ROWS)
def test_param_fold(ops, rows):
    count = 3
    for D in R.FOLD_D:
        gen = torch.Generator().manual_seed(rows * 131 + D)
        stride = rows * 2 * D + 24
        pc = torch.full((count, stride), float("nan"))
        pc[:, :rows * 2 * D] = torch.randn(count, rows * 2 * D, generator=gen) * (1.0 + torch.arange(rows * 2 * D) % 7)
        part = G(count, stride, F32, pc)
        offs = [[0, D], [5 * D + 8, 3 * D], [2 * D, 7 * D + 16]]
        goff = torch.tensor(offs, dtype=torch.long, device="cuda")
        prev = prior(8 * D + 64, 4)
        res = []
        for _ in range(2):
            flat = V(8 * D + 64, prev)
            ops.ln_param_reduce_rows(count, rows, D, part.t, goff, flat.vec)
            torch.cuda.synchronize()
            assert part.outside_intact() and flat.outside_intact() and torch.equal(part.bits().cpu(), pc.view(torch.int32))
            res.append(flat.vec.cpu())
        assert torch.equal(res[0], res[1]), "two runs differ"
        worst, keep = {}, torch.ones(flat.n, dtype=torch.bool)
        for k in range(count):
            rows_k = pc[k, :rows * 2 * D].view(rows, 2 * D)
            for h, off in enumerate(offs[k]):
                want, bound = R.fold_ref(rows_k[:, h * D:(h + 1) * D], prev[off:off + D])
                within(worst, "dgamma" if h == 0 else "dbeta", res[0][off:off + D], want, bound)
                keep[off:off + D] = False
        assert torch.equal(res[0][keep], prev[keep]), "the fold wrote outside dgamma / dbeta"
        report(f"fold rows={rows} D={D}", worst)


# ------------------------------------------------------------------------------------------------ BatchNorm(token axis) + ReLU
def run_bn(ops, N, L, Hp, dtype, worst, special=False, off8=False):
    o = R.bn_inputs(N, L, Hp, dtype, special)
    fast = R.bn_fast(dtype, Hp) and not off8
    u, gamma, beta = G(N * L, Hp, dtype, o["u"], off8), V(L, o["gamma"]), V(L, o["beta"])
    ins = dict(u=(u, o["u"]), gamma=(gamma, o["gamma"]), beta=(beta, o["beta"]))
    # two training calls in a row
    rm, rv, nbt = V(L, o["run_mean"]), V(L, o["run_var"]), torch.zeros(1, dtype=torch.long, device="cuda")
    f = R.bn_fwd_ref(o["u"], o["gamma"], o["beta"], N, L, Hp, o["run_mean"], o["run_var"], fast=fast)
    f2 = R.bn_fwd_ref(o["u"], o["gamma"], o["beta"], N, L, Hp, f["run_mean"], f["run_var"], fast=fast)
    mom = R.f32(R.BN_MOMENTUM)
    steps = ((f, f["e_run_mean"], f["e_run_var"]), (f2, f2["e_run_mean"] + (1 - mom) * f["e_run_mean"], f2["e_run_var"] + (1 - mom) * f["e_run_var"]))
    for call, (fr, e_rm, e_rv) in enumerate(steps):
        r, mean, rstd = G(N * L, Hp, dtype, None, off8), V(L), V(L)
        ops.bnrelu_fwd(u.t, gamma.vec, beta.vec, r.t, mean.vec, rstd.vec, N, L, running_mean=rm.vec, running_var=rv.vec, nbt=nbt)
        settle(ins, dict(r=r, mean=mean, rstd=rstd, run_mean=rm, run_var=rv))
        within(worst, "r", r.t, fr["r"], R.finish(fr["r"], fr["e_r"], dtype))
        within(worst, "mean", mean.vec, fr["mean"], fr["b_mean"])
        within(worst, "rstd", rstd.vec, fr["rstd"], fr["b_rstd"])
        within(worst, "run_mean", rm.vec, fr["run_mean"], e_rm)
        within(worst, "run_var", rv.vec, fr["run_var"], e_rv)
        assert int(nbt) == call + 1
    out = dict(r=r.t.clone(), e_r=R.finish(f["r"], f["e_r"], dtype))
    # backward, on parameter gradients that already hold something
    mean_c, rstd_c = f["mean"].float(), f["rstd"].float()
    b = R.bn_bwd_ref(o["u"], o["dr"], o["gamma"], o["beta"], mean_c, rstd_c, N, L, Hp, fast)
    assert b["margin"] > 1.0
    dr, du, mean, rstd = G(N * L, Hp, dtype, o["dr"], off8), G(N * L, Hp, dtype, None, off8), V(L, mean_c), V(L, rstd_c)
    prev_g, prev_b = prior(L, 5), prior(L, 6)
    dg, db = V(L, prev_g), V(L, prev_b)
    ops.bnrelu_bwd(u.t, dr.t, gamma.vec, beta.vec, mean.vec, rstd.vec, du.t, dg.vec, db.vec, N, L)
    settle(dict(ins, dr=(dr, o["dr"]), mean=(mean, mean_c), rstd=(rstd, rstd_c)), dict(du=du, dgamma=dg, dbeta=db))
    within(worst, "du", du.t, b["du"], R.finish(b["du"], b["e_du"], dtype))
    within(worst, "dgamma", dg.vec, prev_g.double() + b["dgamma"], R.param_bound(b["depth"], b["abs_g"], b["e_g"], prev_g))
    within(worst, "dbeta", db.vec, prev_b.double() + b["dbeta"], R.param_bound(b["depth"], b["abs_b"], 0.0, prev_b))
    out.update(du=du.t.clone(), e_du=R.finish(b["du"], b["e_du"], dtype))
    # eval: the given running statistics; nothing but r, mean and rstd may change
    fe = R.bn_fwd_ref(o["u"], o["gamma"], o["beta"], N, L, Hp, o["run_mean"], o["run_var"], training=False)
    rm, rv, nbt = V(L, o["run_mean"]), V(L, o["run_var"]), torch.full((1,), 7, dtype=torch.long, device="cuda")
    r, mean, rstd = G(N * L, Hp, dtype, None, off8), V(L), V(L)
    ops.bnrelu_fwd(u.t, gamma.vec, beta.vec, r.t, mean.vec, rstd.vec, N, L, running_mean=rm.vec, running_var=rv.vec, nbt=nbt, training=False)
    settle(dict(ins, run_mean=(rm, o["run_mean"]), run_var=(rv, o["run_var"])), dict(r=r, mean=mean, rstd=rstd))
    assert int(nbt) == 7
    within(worst, "eval r", r.t, fe["r"], R.finish(fe["r"], fe["e_r"], dtype))
    assert torch.equal(mean.vec.cpu(), o["run_mean"])
    within(worst, "eval rstd", rstd.vec, fe["rstd"], fe["b_rstd"])
    return out


@pytest.mark.parametrize("Hp,N", R.BN_GEOMS)
def test_bnrelu(ops, Hp, N):
    for dtype in (BF, F32):
        worst = {}
        for L in R.BN_L:
            run_bn(ops, N, L, Hp, dtype, worst)
        kind = "fast" if R.bn_fast(dtype, Hp) else "generic"
        report(f"bnrelu Hp={Hp} N={N} {dtype} ({kind} kernels)", worst)


@pytest.mark.parametrize("Hp,N", [(2048, 5), (64, 129), (8, 5), (8192, 5)])
def test_bnrelu_misaligned_operands_take_the_generic_kernels(ops, Hp, N):
    """bf16 operands 8 bytes off a 16-byte boundary: bn_fast_ok's fall-back.  Held to the generic kernels' bound, and to the aligned run
    within the two bounds' sum."""
    worst_a, worst_m = {}, {}
    a = run_bn(ops, N, 5, Hp, BF, worst_a)
    m = run_bn(ops, N, 5, Hp, BF, worst_m, off8=True)
    for k in ("r", "du"):
        diff = (a[k].double() - m[k].double()).abs().cpu()
        assert bool((diff <= a["e_" + k] + m["e_" + k]).all()), k
    report(f"bnrelu Hp={Hp} N={N} bf16 misaligned (generic kernels)", worst_m)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_bnrelu_far_shift(ops, dtype):
    """Channel 1's first value, the one-pass kernel's shift, is a 20-sigma outlier; channel 2's mean lies 50 sigma from zero."""
    Hp, N, L = R.BN_SPECIAL
    worst = {}
    run_bn(ops, N, L, Hp, dtype, worst, special=True)
    report(f"bnrelu far shift Hp={Hp} N={N} L={L} {dtype}", worst)


def test_bnrelu_refusals(ops):
    u, r, mean, rstd, gamma = G(4, 8, BF, 1.0), G(4, 8, BF), V(2), V(2), V(2, 1.0)
    with pytest.raises(RuntimeError):      # eval mode without running statistics
        ops.bnrelu_fwd(u.t, gamma.vec, gamma.vec, r.t, mean.vec, rstd.vec, 2, 2, training=False)
    u1, r1 = G(1, 1, F32, 1.0), G(1, 1, F32)
    with pytest.raises(RuntimeError):      # one value per channel (N = 1, Hp = 1)
        ops.bnrelu_fwd(u1.t, gamma.vec[:1], gamma.vec[:1], r1.t, mean.vec[:1], rstd.vec[:1], 1, 1)
    torch.cuda.synchronize()
    for b in (r, r1, mean, rstd):
        assert b.untouched()                   # refused before any launch
