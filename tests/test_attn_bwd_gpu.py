"""Every attention-backward kernel family against fp64, element by element, in guarded buffers (tests/attn_bwd_ref.py has the bounds, the
fp64 references and the geometry tables; tests/test_attn_bwd_cpu.py checks the bounds themselves without a GPU).  For each table entry,
forward and backward run through ops.attn_fwd / ops.attn_bwd with sentinel guards before and behind every operand and output; then: guards
intact, inputs unchanged bit for bit, no output element unwritten or NaN, the forward bound and |lse err| <= 1e-3, the backward bound
against the fp64 backward with the kernel's own forward results, the backward bound against the autograd gradient, and the same bits from
a second run.  The fp8 copy of dqkv (csmae_attn_bwd_q) is checked at one ragged shape per resident family.

Families and how they are reached: the four LDS-resident backward kernels by (T, head_dim) (launch_bwd_bf16), the streaming kernels just
past each resident limit and, at resident shapes, through csmae_attn_stream_mode(2); the any-length bf16 kernels at head_dim % 8 != 0 and,
at streamable shapes, through mode 0; the fp32 kernels up to their LDS limits and the any-length fp32 ones beyond.  Not covered: the
tuning-aid kernels that only a CSMAE_DEBUG option read once per process selects (attn_bwd_2pass at T > 64, attn_bwd_2sweep,
attn_bwd_4waves), and T > 4097.

Worst max |err| / bound per family over its table (no factor; the tests allow 2 bound + 1e-6), measured on an MI355X:
  family                  dq     dk     dv    of the allowance   against autograd
  attn_bwd_bf16           1.40   1.32   1.40   0.70               0.70
  attn_bwd1p2_bf16        1.10   1.09   1.11   0.56               0.56
  attn_bwd1p_bf16<NW=4>   1.39   1.07   0.97   0.69               0.48
  attn_bwd1p_bf16<NW=8>   1.02   1.03   0.74   0.51               0.37
  attn_bwd_stream         0.99   1.09   0.93   0.55               0.46
  attn_bwd_any<bf16_t>    1.89   1.90   1.93   0.96               0.96   (one output rounding, held to its exact worst case 2^-8)
  attn_bwd_f32            0.03   0.02   0.02   0.01               0.02
  attn_bwd_any<float>     0.01   0.01   0.01   0.01               0.01
No family needed a term beyond those counted in tests/attn_bwd_ref.py, and no kernel defect showed.
Needs an MI355X."""
import pytest
import torch

import attn_bwd_ref as R
from norm_ref import Guarded

pytestmark = pytest.mark.gpu

_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from csmae_hip import ops as o
    import csmae_hip
    csmae_hip.load()
    return o


class stream_mode:
    """`with stream_mode(ops, m):` — csmae_attn_stream_mode(m) inside, the previous mode restored on the way out."""

    def __init__(self, ops, mode):
        self.ops, self.mode = ops, mode

    def __enter__(self):
        self.prev = self.ops.attn_stream_mode(self.mode)

    def __exit__(self, *exc):
        self.ops.attn_stream_mode(self.prev)


def operands(B, T, H, hd, dtype):
    qkv, dout = R.inputs(B, T, H, hd)
    return qkv.to(dtype), dout.to(dtype)


def run_guarded(ops, geom, dtype):
    """Forward and backward of one geometry in guarded buffers: (out, lse [B, H, T], dqkv) after the guard, input and coverage checks."""
    B, T, H, hd = geom
    D = H * hd
    qkv_c, dout_c = operands(B, T, H, hd, dtype)
    qkv = Guarded(B * T, 3 * D, dtype, fill=qkv_c)
    dout = Guarded(B * T, D, dtype, fill=dout_c)
    out, lse, dqkv = Guarded(B * T, D, dtype), Guarded(B * H, T, torch.float32), Guarded(B * T, 3 * D, dtype)
    ops.attn_fwd(qkv.t, out.t, lse.t, B, T, H, hd)
    ops.attn_bwd(qkv.t, out.t, dout.t, lse.t, dqkv.t, B, T, H, hd)
    torch.cuda.synchronize()
    for name, gb in (("qkv", qkv), ("dout", dout), ("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert gb.outside_intact(), f"{geom} {name}: an element outside the tensor was written"
    for name, gb, src in (("qkv", qkv, qkv_c), ("dout", dout, dout_c)):
        assert torch.equal(gb.bits().cpu(), src.view(_INT[dtype])), f"{geom} {name}: an input was changed"
    for name, gb in (("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert gb.unwritten() == 0, f"{geom} {name}: {gb.unwritten()} elements were left unwritten"
        assert not bool(torch.isnan(gb.t.float()).any()), f"{geom} {name}: NaN"
    return out.t, lse.t.view(B, H, T), dqkv.t


def check_case(ops, geom, dtype, scheme, family):
    B, T, H, hd = geom
    out, lse, dqkv = run_guarded(ops, geom, dtype)
    again = run_guarded(ops, geom, dtype)
    for x, y, name in zip((out, lse, dqkv), again, ("out", "lse", "dqkv")):
        assert torch.equal(x.view(_INT[x.dtype]), y.view(_INT[y.dtype])), f"{geom} {name}: two runs differ"
    qkv_c, dout_c = operands(B, T, H, hd, dtype)
    qkv, dout = qkv_c.cuda(), dout_c.cuda()
    fwd = R.reference(qkv, dout, B, T, H, hd)
    ref, lse_ref, pabsv, _ = fwd
    err = (out.double() - ref).abs()
    unit = R.fwd_unit(ref, pabsv, T, hd, scheme)
    f_excess, f_ratio = float((err / (R.FWD_FACTOR * unit + R.ABS_FLOOR)).max()), float((err / unit.clamp_min(1e-300)).max())
    lse_err = float((lse.double() - lse_ref).abs().max())
    given, auto, line = R.check_backward(qkv, dout, out, lse, dqkv, B, T, H, hd, scheme, fwd)
    print(f"BWD family={family} geom={geom} fwd={f_ratio:.3f} lse_err={lse_err:.2e} " + " ".join(f"{n}={given[n][1]:.3f}" for n in R.TENSORS) +
          f" excess={R.worst(given):.3f} autograd_excess={R.worst(auto):.3f}")
    if dtype == torch.bfloat16:     # the forward bound as tests/attn_stream_ref.py states it
        assert R.S.fwd_excess(out, ref, pabsv)[0] <= 1.0, (family, geom)
    assert f_excess <= 1.0, (family, geom, f_excess, f_ratio)
    assert lse_err <= 1e-3, (family, geom, lse_err)
    assert R.worst(given) <= 1.0, (family, geom, given, line)
    assert R.worst(auto) <= 1.0, (family, geom, auto, line)


@pytest.mark.parametrize("entry", R.RESIDENT, ids=[R.geom_id(e) for e in R.RESIDENT])
def test_resident_backward(ops, entry):
    import csmae_hip as C
    *geom, kind = entry
    B, T, H, hd = geom
    assert R.resident_bwd_kernel(T, hd) == kind
    with stream_mode(ops, 1):
        assert ops.attn_resident(ops.BF16, T, hd) and ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_RESIDENT
        check_case(ops, tuple(geom), torch.bfloat16, R.SCHEME_OF[kind], kind)


@pytest.mark.parametrize("entry", R.STREAMING, ids=[R.geom_id(e) for e in R.STREAMING])
def test_streaming_backward(ops, entry):
    import csmae_hip as C
    *geom, mode = entry
    B, T, H, hd = geom
    assert (R.S.TILE, R.S.OWN) == (C.ATTN_STREAM_TILE, C.ATTN_STREAM_OWN)
    with stream_mode(ops, mode):
        assert ops.attn_resident(ops.BF16, T, hd) == (mode == 2) and ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_STREAM
        check_case(ops, tuple(geom), torch.bfloat16, R.SCHEME_OF[R.STREAM], R.STREAM)


@pytest.mark.parametrize("entry", R.ANY, ids=[R.geom_id(e) for e in R.ANY])
def test_any_length_backward(ops, entry):
    import csmae_hip as C
    *geom, mode = entry
    B, T, H, hd = geom
    with stream_mode(ops, mode):
        assert not ops.attn_resident(ops.BF16, T, hd) and ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_ANY
        check_case(ops, tuple(geom), torch.bfloat16, R.SCHEME_OF[R.ANY_BF16], R.ANY_BF16)


@pytest.mark.parametrize("geom", R.FP32, ids=[R.geom_id(e) for e in R.FP32])
def test_fp32_backward(ops, geom):
    import csmae_hip as C
    B, T, H, hd = geom
    kind = R.f32_bwd_kernel(T, hd)
    for mode in (1, 2):            # the stream mode does not reach the fp32 route
        with stream_mode(ops, mode):
            assert ops.attn_route(ops.F32, T, hd) == C.ATTN_ROUTE_F32
    check_case(ops, geom, torch.float32, R.SCHEME_OF[kind], kind)


# one ragged shape per resident family, a partial head_dim in each
EMIT = [(2, 33, 3, 24, R.TWO_PASS), (1, 97, 3, 24, R.ONE_PASS_2KP), (1, 97, 1, 40, R.ONE_PASS_4), (1, 257, 3, 24, R.ONE_PASS_8)]


@pytest.mark.parametrize("entry", EMIT, ids=[R.geom_id(e) for e in EMIT])
def test_backward_emits_the_fp8_copy_of_a_separate_quantisation_pass(ops, entry):
    """csmae_attn_bwd_q at ragged shapes, with test_attention_emits_the_fp8_copies_of_a_separate_quantisation_pass's assertions: the e5m2 bytes
    are csmae_fp8_quantize's of the plain kernel's dqkv with the same previous-step amax, the recorded amax is the tensor's, the bf16 result
    is the plain kernel's, and with skip_out the bf16 tensor is not touched."""
    *geom, kind = entry
    B, T, H, hd = geom
    D = H * hd
    assert ops.attn_resident(ops.BF16, T, hd) and R.resident_bwd_kernel(T, hd) == kind
    qkv_c, dout_c = operands(B, T, H, hd, torch.bfloat16)
    qkv, dout = qkv_c.cuda(), dout_c.cuda()
    out = torch.empty(B * T, D, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, T, device="cuda")
    ref = torch.empty(B * T, 3 * D, device="cuda", dtype=torch.bfloat16)
    fmt = ops.FP8_E5M2
    with stream_mode(ops, 1):
        ops.attn_fwd(qkv, out, lse, B, T, H, hd)
        ops.attn_bwd(qkv, out, dout, lse, ref, B, T, H, hd)
        prev = torch.zeros(ops.FP8_SLOTS, device="cuda")
        prev[7] = float(ref.float().abs().max()) * 0.8      # a stale amax: some values clamp
        nxt, dq = torch.zeros(ops.FP8_SLOTS, device="cuda"), torch.zeros(1, device="cuda")
        q, got = Guarded(B * T, 3 * D, torch.uint8, fill=0), Guarded(B * T, 3 * D, torch.bfloat16)
        ops.attn_bwd(qkv, out, dout, lse, got.t, B, T, H, hd, emit=(q.t, fmt, prev, nxt, dq))
        torch.cuda.synchronize()
        assert q.outside_intact() and got.outside_intact()
        assert torch.equal(got.t.view(torch.int16), ref.view(torch.int16))
        want_q, want_next, want_dq = torch.zeros_like(q.t), torch.zeros(ops.FP8_SLOTS, device="cuda"), torch.zeros(1, device="cuda")
        ops.fp8_quantize(ref, want_q, prev, want_dq, fmt=fmt, amax_next=want_next)
        assert torch.equal(q.t, want_q)
        assert float(nxt.max()) == float(ref.float().abs().max()) == float(want_next.max())
        assert float(dq) == float(want_dq)
        q2, keep = Guarded(B * T, 3 * D, torch.uint8, fill=0), Guarded(B * T, 3 * D, torch.bfloat16)
        nxt.zero_()
        ops.attn_bwd(qkv, out, dout, lse, keep.t, B, T, H, hd, emit=(q2.t, fmt, prev, nxt, dq), skip_out=True)
        torch.cuda.synchronize()
        assert torch.equal(q2.t, want_q) and q2.outside_intact() and keep.untouched() and float(nxt.max()) == float(want_next.max())
