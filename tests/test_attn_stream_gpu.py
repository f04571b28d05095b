"""The streaming MFMA attention kernels (csrc/attention_stream.hip) and their routing: route answers, parity against fp64 in NaN-guarded
buffers around the kernels' tile sizes, the derived forward bound (tests/attn_stream_ref.py), agreement with the LDS-resident family,
bitwise reproducibility, stream ordering through the launch-carried event, and two model steps whose attention takes the new route.
Needs an MI355X."""
import pytest
import torch

import attn_bwd_ref as BR
import attn_stream_ref as R

pytestmark = pytest.mark.gpu


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


# (T, head_dim) of the resident entries of ATT in tests/test_ops_gpu.py ...
RESIDENT = [(50, 64), (197, 32), (17, 32), (5, 64), (65, 80), (257, 32), (33, 16), (224, 64), (129, 32), (97, 64), (96, 32), (160, 32)]
# ... and of the four presets' encoder / decoder blocks (ViT-B/16 and ViT-L/16 at 224^2: 50 x 64, 197 x 32; ViT-L/16 at 256^2: 65 x 64, 257 x 32; ViT-H/14: 65 x 80, 257 x 32)
RESIDENT += [(65, 64)]
STREAMED = [(401, 64), (577, 80), (300, 32), (1025, 32), (225, 64), (100, 96), (40, 128), (1370, 64), (8192, 128)]


def test_route(ops):
    import csmae_hip as C
    prev = ops.attn_stream_mode(1)
    try:
        assert ops.attn_stream_mode() == 1            # (a query leaves the mode alone)
        for T, hd in RESIDENT:
            assert ops.attn_resident(ops.BF16, T, hd)
            assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_RESIDENT, (T, hd)
        for T, hd in STREAMED:
            assert not ops.attn_resident(ops.BF16, T, hd)
            assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_STREAM, (T, hd)
        assert ops.attn_route(ops.BF16, 300, 20) == C.ATTN_ROUTE_ANY      # head_dim % 8 != 0: the any-length kernels, as before
        with pytest.raises(RuntimeError):
            ops.attn_route(ops.BF16, 8193, 32)                            # refused, as csmae_attn_fwd refuses it
        for T, hd in RESIDENT + STREAMED:
            assert ops.attn_route(ops.F32, T, hd) == C.ATTN_ROUTE_F32
        assert ops.attn_stream_mode(0) == 1
        for T, hd in STREAMED:
            assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_ANY, (T, hd)
        for T, hd in RESIDENT:
            assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_RESIDENT, (T, hd)
        assert ops.attn_stream_mode(2) == 0
        for T, hd in RESIDENT + STREAMED:
            assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_STREAM, (T, hd)
            assert ops.attn_resident(ops.BF16, T, hd) == ((T, hd) in RESIDENT)   # csmae_attn_resident keeps its meaning
        assert ops.attn_route(ops.BF16, 300, 20) == C.ATTN_ROUTE_ANY
        assert ops.attn_route(ops.F32, 300, 32) == C.ATTN_ROUTE_F32
    finally:
        ops.attn_stream_mode(prev)


def test_binding_constants_are_the_kernels(ops):
    import csmae_hip as C
    assert (C.ATTN_STREAM_TILE, C.ATTN_STREAM_OWN) == (R.TILE, R.OWN)


class Guarded:
    """A contiguous [rows, cols] tensor inside a larger allocation, NaN guard rows before and behind it (a multiple of 16 bytes each)."""

    def __init__(self, rows, cols, dtype, fill=None):
        es = torch.empty(0, dtype=dtype).element_size()
        g = 3
        while (g * cols * es) % 16:
            g += 1
        self.g, self.rows = g, rows
        self.base = torch.full((rows + 2 * g, cols), float("nan"), dtype=dtype, device="cuda")
        self.t = self.base[g:g + rows]
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0
        if fill is not None:
            self.t.copy_(fill)
        self.bits = torch.int16 if es == 2 else torch.int32
        self.before = self.base[:g].view(self.bits).clone()
        self.behind = self.base[g + rows:].view(self.bits).clone()

    def guards_intact(self):
        return torch.equal(self.base[:self.g].view(self.bits), self.before) and torch.equal(self.base[self.g + self.rows:].view(self.bits), self.behind)


def run_guarded(ops, B, T, H, hd):
    """Forward and backward of one geometry in guarded, NaN-prefilled buffers; returns (out, lse, dqkv) after checking guards and coverage."""
    D = H * hd
    qkv_c, dout_c = R.inputs(B, T, H, hd)
    qkv = Guarded(B * T, 3 * D, torch.bfloat16, qkv_c.cuda())
    dout = Guarded(B * T, D, torch.bfloat16, dout_c.cuda())
    out = Guarded(B * T, D, torch.bfloat16)
    lse = Guarded(B * H, T, torch.float32)
    dqkv = Guarded(B * T, 3 * D, torch.bfloat16)
    ops.attn_fwd(qkv.t, out.t, lse.t, B, T, H, hd)
    ops.attn_bwd(qkv.t, out.t, dout.t, lse.t, dqkv.t, B, T, H, hd)
    torch.cuda.synchronize()
    for name, gb in (("qkv", qkv), ("dout", dout), ("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert gb.guards_intact(), f"{name}: a guard row was written"
    for name, gb in (("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert not bool(torch.isnan(gb.t).any()), f"{name}: an element was left unwritten (or a guard row was read)"
    return out.t, lse.t.view(B, H, T), dqkv.t


def check_against_fp64(geom, out, lse, dqkv, what):
    B, T, H, hd = geom
    qkv_c, dout_c = R.inputs(B, T, H, hd)
    qkv, dout = qkv_c.cuda(), dout_c.cuda()
    ref, lse_ref, pabsv, grad = R.reference(qkv, dout, B, T, H, hd)
    excess, ratio = R.fwd_excess(out, ref, pabsv)
    lse_err = float((lse.double() - lse_ref).abs().max())
    gscale = float(grad.abs().max())
    gerr = (dqkv.double() - grad).abs()
    gtol = 2e-2 * max(gscale, 1.0) + 2e-2 * grad.abs()
    gworst = float((gerr / gtol).max())
    print(f"{what} {geom}: forward max |err| / (2^-9 (sum P|V| + |ref|)) = {ratio:.3f} (bound ratio {excess:.3f}), |lse err| = {lse_err:.2e}, "
          f"backward max err / tol = {gworst:.3f} (max |grad| {gscale:.3g})")
    assert excess <= 1.0, (what, geom, excess, ratio)
    assert lse_err <= 1e-3, (what, geom, lse_err)
    assert gworst <= 1.0, (what, geom, gworst)
    # the per-element backward bounds of tests/attn_bwd_ref.py (both families round P, dS and the output to bf16 once: its "mfma" scheme):
    # against the fp64 backward with the kernel's own out and lse, and against the autograd gradient
    given, auto, line = BR.check_backward(qkv, dout, out, lse, dqkv, B, T, H, hd, "mfma", (ref, lse_ref, pabsv, grad))
    print(f"{what} {geom}: {line}")
    assert BR.worst(given) <= 1.0, (what, geom, given)
    assert BR.worst(auto) <= 1.0, (what, geom, auto)


# T one below, at and one above one and two streamed tiles (ATTN_STREAM_TILE = 64) and one and two owned blocks (ATTN_STREAM_OWN = 128:
# four waves x two 16-row blocks), then 1, 5 and the sequence lengths of large inputs; every head_dim bucket edge and the narrow head 8.
PARITY = [(2, 1, 2, 32), (2, 5, 2, 64), (2, 63, 2, 8), (2, 64, 2, 32), (2, 65, 2, 80), (2, 127, 2, 64), (2, 128, 2, 96), (2, 129, 2, 128),
          (2, 255, 2, 32), (2, 256, 2, 64), (2, 257, 2, 80), (3, 257, 2, 8), (2, 289, 2, 32), (2, 289, 3, 96), (2, 577, 2, 32), (3, 577, 2, 80),
          (2, 1025, 2, 32), (2, 1025, 2, 64), (2, 1025, 2, 128), (2, 1370, 2, 64), (1, 1370, 3, 96), (1, 4097, 2, 128), (2, 4097, 2, 8),
          (1, 4097, 1, 64)]


@pytest.mark.parametrize("geom", PARITY)
def test_parity_in_guarded_buffers(ops, geom):
    import csmae_hip as C
    B, T, H, hd = geom
    assert R.TILE == C.ATTN_STREAM_TILE and R.OWN == C.ATTN_STREAM_OWN
    with stream_mode(ops, 1):
        default_streams = ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_STREAM
    with stream_mode(ops, 1 if default_streams else 2):    # (shapes the resident kernels take are reached through mode 2)
        assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_STREAM
        out, lse, dqkv = run_guarded(ops, B, T, H, hd)
    check_against_fp64(geom, out, lse, dqkv, "streaming")


@pytest.mark.parametrize("geom", [(2, 197, 2, 32), (3, 50, 2, 64), (1, 65, 2, 80)])
def test_streaming_agrees_with_the_resident_family(ops, geom):
    """Both families on one shape (mode 2 against mode 1): each meets the fp64 checks, and they agree with each other within the same
    tolerances — the forward bound and test_attention_fwd_bwd's backward tolerance, the resident result in the reference's place."""
    import csmae_hip as C
    B, T, H, hd = geom
    with stream_mode(ops, 1):
        assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_RESIDENT
        out_r, lse_r, dqkv_r = run_guarded(ops, B, T, H, hd)
    with stream_mode(ops, 2):
        assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_STREAM
        out_s, lse_s, dqkv_s = run_guarded(ops, B, T, H, hd)
    check_against_fp64(geom, out_r, lse_r, dqkv_r, "resident")
    check_against_fp64(geom, out_s, lse_s, dqkv_s, "streaming")
    qkv_c, dout_c = R.inputs(B, T, H, hd)
    _, _, pabsv, _ = R.reference(qkv_c.cuda(), dout_c.cuda(), B, T, H, hd, backward=False)
    excess, ratio = R.fwd_excess(out_s, out_r.double(), pabsv)
    gr = dqkv_r.double()
    gworst = float(((dqkv_s.double() - gr).abs() / (2e-2 * max(float(gr.abs().max()), 1.0) + 2e-2 * gr.abs())).max())
    lse_err = float((lse_s - lse_r).abs().max())
    print(f"streaming against resident {geom}: forward ratio {ratio:.3f}, |lse diff| {lse_err:.2e}, backward err / tol {gworst:.3f}")
    assert excess <= 1.0 and lse_err <= 1e-3 and gworst <= 1.0, (geom, excess, lse_err, gworst)


@pytest.mark.parametrize("geom", [(2, 577, 2, 32), (1, 1025, 1, 64)])
def test_two_runs_give_the_same_bits(ops, geom):
    import csmae_hip as C
    B, T, H, hd = geom
    with stream_mode(ops, 1):
        assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_STREAM
        a = run_guarded(ops, B, T, H, hd)
        b = run_guarded(ops, B, T, H, hd)
    for x, y, name in zip(a, b, ("out", "lse", "dqkv")):
        assert torch.equal(x, y), (geom, name)


def test_launch_carried_event_orders_a_second_stream_behind_streaming_backward(ops):
    """csmae_next_launch_event in front of a streaming attn_bwd, csmae_flush_launch_event behind it (ops.launch_done): a second stream that
    waits for the event sees the whole dqkv — the event rides on the one launch that holds both backward passes, or the flush records it
    (the pattern of test_launch_carried_event_orders_a_second_stream in tests/test_ops_gpu.py)."""
    import csmae_hip as C
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    ev = torch.cuda.Event()
    ev.record()                                   # (torch creates the HIP event at its first record)
    spin = torch.empty(64 << 20, device="cuda")   # a long kernel in front, so that the launch is still queued when the second stream starts waiting
    B, T, H, hd = 8, 577, 16, 32
    D = H * hd
    with stream_mode(ops, 1):
        assert ops.attn_route(ops.BF16, T, hd) == C.ATTN_ROUTE_STREAM
        qkv_c, dout_c = R.inputs(B, T, H, hd)
        qkv, dout = qkv_c.cuda(), dout_c.cuda()
        out = torch.empty(B * T, D, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(B, H, T, device="cuda")
        ops.attn_fwd(qkv, out, lse, B, T, H, hd)
        want = torch.empty(B * T, 3 * D, device="cuda", dtype=torch.bfloat16)
        ops.attn_bwd(qkv, out, dout, lse, want, B, T, H, hd)
        got = torch.zeros_like(want)
        torch.cuda.synchronize()
        for _ in range(3):
            got.zero_()
            spin.fill_(1.0)
            with ops.launch_done(ev, main.cuda_stream):
                ops.attn_bwd(qkv, out, dout, lse, got, B, T, H, hd)
            side.wait_event(ev)
            with torch.cuda.stream(side):
                seen = got.clone()
            side.synchronize()
            assert torch.equal(seen, want)
        torch.cuda.synchronize()


MICRO = dict(dim_model=128, encoder_num_layers=2, encoder_num_heads=2, decoder_embed_dim=64, decoder_num_layers=2, decoder_num_heads=2)


@pytest.mark.parametrize("S,N,mask_ratio,enc_T", [(320, 2, 0.75, 101), (512, 1, 0.5, 513)])
def test_large_inputs_bf16_tracks_fp32(ops, S, N, mask_ratio, enc_T):
    """MAE_ViT_MsLdCeCd at 320^2 (decoder T = 401, head_dim 32) and at 512^2 with mask_ratio 0.5 (encoder T = 513, head_dim 64; decoder T = 1025):
    the bf16 step, its attention on the streaming route, against the fp32 engine with test_odd_geometries_bf16_tracks_fp32's assertions —
    loss within 2e-2, gradient cosine > 0.98 on every parameter that has a gradient."""
    import csmae_hip as C
    import models_mae
    p = 16
    L = (S // p) ** 2
    with stream_mode(ops, 1):
        assert ops.attn_route(ops.BF16, L + 1, MICRO["decoder_embed_dim"] // MICRO["decoder_num_heads"]) == C.ATTN_ROUTE_STREAM
        assert int(L * (1 - mask_ratio)) + 1 == enc_T
        enc_route = ops.attn_route(ops.BF16, enc_T, MICRO["dim_model"] // MICRO["encoder_num_heads"])
        assert enc_route == (C.ATTN_ROUTE_STREAM if enc_T > 224 else C.ATTN_ROUTE_RESIDENT)
        torch.manual_seed(11)
        m = models_mae.MAE_ViT_MsLdCeCd(**MICRO, input_size=S, patch_size=str(p), mask_ratio=mask_ratio, predictor_hidden_size=128).cuda().train()
        g = torch.Generator().manual_seed(12)
        imgs = torch.randn(N, 3, S, S, generator=g).cuda()
        dr = dict(noise=[torch.rand(N, L, generator=g), torch.rand(N, L, generator=g)], box=(S // 9, S // 5, (S * 2) // 3, (S * 5) // 8))
        res = {}
        for dt in (torch.float32, torch.bfloat16):
            m.compute_dtype = dt
            m.zero_grad(set_to_none=True)
            m._test_draws = dict(dr)
            loss = m(imgs, mask_ratio=mask_ratio)[0]
            loss.backward()
            res[dt] = (float(loss.detach()), {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None})
    lf, gf = res[torch.float32]
    lb, gb = res[torch.bfloat16]
    assert abs(lb - lf) <= 2e-2 * abs(lf), (lb, lf)
    assert gf.keys() == gb.keys()
    for n in gf:
        assert torch.isfinite(gb[n]).all(), n
        if gf[n].norm() > 1e-7:
            cos = torch.nn.functional.cosine_similarity(gf[n].flatten().double(), gb[n].flatten().double(), dim=0)
            assert cos > 0.98, (n, float(cos))
