"""Tensor-level launchers for the C ABI (include/csmae.h).  Every function only enqueues HIP kernels on
torch's current stream; all tensors must live on the GPU, be contiguous in their last dim, and are owned
by PyTorch.  No function here computes anything with torch ops."""
from __future__ import annotations

import ctypes

import torch

from . import BF16, EPI_ATOMIC, EPI_DGELU, EPI_GELU, EPI_NONE, EPI_RESID, F32, LOSS_KINDS, check, load
from . import EPI_DGELU_Q8 as _EPI_DGELU_Q8, EPI_GELU_Q8 as _EPI_GELU_Q8   # (private here: __all__ below is every public name of this module)

_DT = {torch.float32: F32, torch.bfloat16: BF16}
_timer = None
_Q8 = {EPI_GELU: _EPI_GELU_Q8, EPI_DGELU: _EPI_DGELU_Q8}


class KernelTimer:
    """HIP-event timing of individual launches on the stream they are enqueued on (bench.py roofline leg)."""

    def __init__(self):
        self.records, self._e0 = [], None

    def __enter__(self):
        global _timer
        _timer = self
        return self

    def __exit__(self, *a):
        global _timer
        _timer = None

    def begin(self):
        self._e0 = torch.cuda.Event(enable_timing=True)
        self._e0.record()

    def end(self, kind, work):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.records.append((kind, work, self._e0, e1))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, work, e0, e1 in self.records:
            d = out.setdefault(kind, dict(ms=0.0, work=0.0, launches=0))
            d["ms"] += e0.elapsed_time(e1)
            d["work"] += work
            d["launches"] += 1
        return out


def dt(t: torch.Tensor) -> int:
    return _DT[t.dtype]


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("csmae_hip ops need GPU tensors: the MI355X path has no CPU fallback")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _s(st):
    """the `st` argument of every launcher: a raw stream handle, or None for torch's current stream"""
    return st if st is not None else stream()


def _begin():
    """Start of a timed launch: `t = _begin()`, the launch, `if t: t.end(kind, work)`.  Returns the active KernelTimer (start event recorded) or None."""
    if _timer is not None:
        _timer.begin()
    return _timer


def _epi(epilogue, aux):
    """gelu' as one byte per element: a uint8 `aux` turns the GELU / DGELU epilogue into its _Q8 code"""
    if aux is not None and aux.dtype == torch.uint8:
        return _Q8[epilogue]
    return epilogue


_masked = {}


def cu_masked_stream(lo: int, hi: int, total_cus: int = None):
    """A torch stream whose kernels run only on the compute units of mask bits [lo, hi) (csmae_stream_create_cu_mask: bit i is CU i / 8 of
    XCD i % 8, so a range whose ends are multiples of 8 is the same CUs in every XCD).  Cached per range: queues are a finite resource."""
    if total_cus is None:
        total_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    key = (lo, hi, total_cus, torch.cuda.current_device())
    s = _masked.get(key)
    if s is None:
        if not _masked:
            import atexit
            atexit.register(_destroy_masked)
        if not (0 <= lo < hi <= total_cus):
            raise ValueError(f"cu_masked_stream: empty or out-of-range CU range [{lo}, {hi}) of {total_cus}")
        words = (total_cus + 31) // 32
        bits = ((1 << (hi - lo)) - 1) << lo
        mask = (ctypes.c_uint32 * words)(*[(bits >> (32 * w)) & 0xFFFFFFFF for w in range(words)])
        h = ctypes.c_void_p()
        check(load().csmae_stream_create_cu_mask(words, ctypes.cast(mask, ctypes.c_void_p), ctypes.cast(ctypes.byref(h), ctypes.c_void_p)), "csmae_stream_create_cu_mask")
        s = _masked[key] = torch.cuda.ExternalStream(h.value)
    return s


def _destroy_masked():
    for s in _masked.values():
        try:
            load().csmae_stream_destroy(s.cuda_stream)
        except Exception:
            pass
    _masked.clear()


class launch_done:
    """`with launch_done(ev, st): <one op>` — the op's kernel carries the torch event `ev` as its own completion signal (csmae_next_launch_event)
    instead of a marker packet recorded behind it on stream `st`; ops whose launch site does not support that get the plain record.  `ev` must
    have been recorded once before (torch creates the HIP event at its first record).
    Contract (csrc: every CSMAE_LAUNCH site): the event goes to the FIRST CSMAE_LAUNCH kernel issued inside the block, so the wrapped ABI call
    must issue that kernel LAST — a call that launched anything behind it (a split-K fold, a trailing quantisation) would release the waiter
    before its output is complete.  True of the three users (csmae_gemm / csmae_gemm_fp8: pipelined kernel last, quantisation passes in
    front through plain launches; csmae_attn_bwd: one kernel)."""

    def __init__(self, ev, st):
        self.h, self.st = ev.cuda_event, st

    def __enter__(self):
        check(load().csmae_next_launch_event(self.h), "csmae_next_launch_event")

    def __exit__(self, *exc):
        rc = load().csmae_flush_launch_event(self.st)
        if exc[0] is None:   # (an exception already on its way out of the body is the one to report: never replace it with the flush's)
            check(rc, "csmae_flush_launch_event")
        return False


def gemm(a, b, out, *, trans_a=False, trans_b=False, bias=None, epilogue=EPI_NONE, aux=None, resid=None, splitk=1, st=None):
    """out[M,N] (+)= A(m,k) B(k,n).  a: [M,K] ([K,M] if trans_a); b: [N,K] ([K,N] if trans_b)."""
    K, M = (a.shape[0], a.shape[1]) if trans_a else (a.shape[1], a.shape[0])
    Kb, N = (b.shape[0], b.shape[1]) if trans_b else (b.shape[1], b.shape[0])
    assert K == Kb and out.shape[0] == M and out.shape[1] == N, (a.shape, b.shape, out.shape, trans_a, trans_b)
    assert a.dtype == b.dtype and a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1
    assert resid is None or resid.dtype == out.dtype, "the residual epilogue reads its addend in the output's dtype"
    epilogue = _epi(epilogue, aux)
    t = _begin()
    check(load().csmae_gemm(dt(a), int(trans_a), int(trans_b), M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), dt(out), _p(bias), epilogue,
                            _p(aux), aux.stride(0) if aux is not None else 0, _p(resid), resid.stride(0) if resid is not None else 0, splitk, _s(st)), "csmae_gemm")
    if t:
        t.end(("gemm_bf16" if a.dtype == torch.bfloat16 else "gemm_f32") + ("_T" if trans_a else "_N") + ("N" if trans_b else "T"), 2.0 * M * N * K)
    return out


def gemm_route(a, b, out, *, trans_a=False, trans_b=False, epilogue=EPI_NONE, aux=None, splitk=1):
    """The kernel gemm() would launch with these arguments (csmae_gemm_route, no launch): a bf16 tile configuration 0..6 or ROUTE_F32."""
    K, M = (a.shape[0], a.shape[1]) if trans_a else (a.shape[1], a.shape[0])
    N = b.shape[1] if trans_b else b.shape[0]
    epilogue = _epi(epilogue, aux)
    rc = load().csmae_gemm_route(dt(a), int(trans_a), int(trans_b), M, N, K, a.stride(0), b.stride(0), out.stride(0), epilogue, splitk)
    check(min(rc, 0), "csmae_gemm_route")
    return rc


def gemm_ks_route(a, bk, b_plain, out, *, epilogue=EPI_NONE, aux=None):
    """The kernel gemm_ks() would launch with these arguments (csmae_gemm_ks_route): ROUTE_KSLAB, or gemm_route() of its plain-weight fallback."""
    M, K = a.shape
    N = b_plain.shape[0]
    epilogue = _epi(epilogue, aux)
    rc = load().csmae_gemm_ks_route(dt(a), M, N, K, _p(a), a.stride(0), _p(bk), N, b_plain.stride(0), _p(out), out.stride(0), epilogue)
    check(min(rc, 0), "csmae_gemm_ks_route")
    return rc


def gemm_ks(a, bk, b_plain, out, *, bias=None, epilogue=EPI_NONE, aux=None, resid=None, st=None):
    """out[M,N] = a[M,K] W^T (+ epilogue) with W [N,K] given twice: `bk` its K-slab mirror (flat bf16, Wk[K/32][N][32], weights_kslab) for the
    two-workgroups-per-CU kernel, `b_plain` in torch's layout for the shapes that kernel does not take."""
    M, K = a.shape
    N = b_plain.shape[0]
    assert b_plain.shape[1] == K and out.shape == (M, N) and a.stride(1) == 1 and out.stride(1) == 1 and b_plain.stride(1) == 1
    assert resid is None or resid.dtype == out.dtype
    assert bk.dtype == torch.bfloat16 and bk.is_contiguous() and bk.numel() >= N * K, "gemm_ks: the K-slab mirror is a flat bf16 tensor of N * K elements"
    epilogue = _epi(epilogue, aux)
    t = _begin()
    check(load().csmae_gemm_ks(dt(a), M, N, K, _p(a), a.stride(0), _p(bk), N, _p(b_plain), b_plain.stride(0), _p(out), out.stride(0), dt(out), _p(bias), epilogue,
                               _p(aux), aux.stride(0) if aux is not None else 0, _p(resid), resid.stride(0) if resid is not None else 0, _s(st)), "csmae_gemm_ks")
    if t:
        t.end(("gemm_bf16" if a.dtype == torch.bfloat16 else "gemm_f32") + "_NT", 2.0 * M * N * K)
    return out


def gemm_ln_supported(M, N, K):
    """True when csmae_gemm_ln_fwd / _bwd take the shape (whole output rows in one workgroup: N <= 512, N % 64 == 0, K % 64 == 0)."""
    return load().csmae_gemm_ln_supported(M, N, K) == 1


def gemm_ln_fwd(a, bk, bias, resid, x_out, gamma, beta, y, mean, rstd, eps=1e-6, st=None):
    """x_out = a W^T + bias + resid; y = LayerNorm(x_out) * gamma + beta; mean / rstd of x_out — one kernel (csmae_gemm_ln_fwd).  `bk`: the K-slab
    mirror of W [N, K] (flat bf16, N * K elements); a, resid, x_out, y bf16 [M, .]."""
    M, K = a.shape
    N = x_out.shape[1]
    assert a.dtype == resid.dtype == x_out.dtype == y.dtype == bk.dtype == torch.bfloat16 and bk.is_contiguous() and bk.numel() >= N * K
    assert resid.shape == x_out.shape == y.shape == (M, N) and a.stride(1) == resid.stride(1) == x_out.stride(1) == y.stride(1) == 1
    assert mean.dtype == rstd.dtype == torch.float32 and mean.numel() >= M and rstd.numel() >= M and gamma.numel() == beta.numel() == N
    t = _begin()
    check(load().csmae_gemm_ln_fwd(M, N, K, _p(a), a.stride(0), _p(bk), N, _p(bias), _p(resid), resid.stride(0), _p(x_out), x_out.stride(0), _p(gamma), _p(beta),
                                   eps, _p(y), y.stride(0), _p(mean), _p(rstd), _s(st)), "csmae_gemm_ln_fwd")
    if t:
        t.end("gemm_bf16_NT", 2.0 * M * N * K)


def gemm_ln_bwd(dy, w, x, mean, rstd, gamma, dres_in, dx_out, partial_ws=None, st=None):
    """dx_out = LayerNorm'(dy w; x, mean, rstd, gamma) + dres_in (w [K, N]: the layer's weight as torch stores it); partial_ws receives ceil(M / 128)
    partial rows [2, N] of dgamma / dbeta for ln_param_reduce_rows — one kernel (csmae_gemm_ln_bwd)."""
    M, K = dy.shape
    N = w.shape[1]
    assert w.shape[0] == K and x.shape == dx_out.shape == (M, N) and (dres_in is None or dres_in.shape == (M, N))
    assert dy.dtype == w.dtype == x.dtype == dx_out.dtype == torch.bfloat16 and (dres_in is None or dres_in.dtype == torch.bfloat16)
    assert dy.stride(1) == w.stride(1) == x.stride(1) == dx_out.stride(1) == 1 and mean.dtype == rstd.dtype == torch.float32
    t = _begin()
    check(load().csmae_gemm_ln_bwd(M, N, K, _p(dy), dy.stride(0), _p(w), w.stride(0), _p(x), x.stride(0), _p(mean), _p(rstd), _p(gamma), _p(dres_in),
                                   dres_in.stride(0) if dres_in is not None else 0, _p(dx_out), dx_out.stride(0), _p(partial_ws),
                                   partial_ws.numel() if partial_ws is not None else 0, _s(st)), "csmae_gemm_ln_bwd")
    if t:
        t.end("gemm_bf16_NN", 2.0 * M * N * K)


def weights_kslab(desc, src, dst, max_blocks=64, st=None):
    """K-slab mirrors (csmae.h csmae_gemm_ks) of the weights in desc (int64 [count, 3] on the device: flat offset, out, in) from the bf16 mirror."""
    check(load().csmae_weights_kslab(desc.shape[0], _p(desc), max_blocks, _p(src), _p(dst), _s(st)), "csmae_weights_kslab")


def gemm_dw(dy, x, dw, workspace, db=None, st=None):
    """dw[out,in] (fp32, contiguous) += dy[tokens,out]^T x[tokens,in] via split-K slabs in `workspace` (fp32); db[out] += colsum(dy)."""
    K, M = dy.shape
    N = x.shape[1]
    assert x.shape[0] == K and dw.shape == (M, N) and dw.is_contiguous() and dy.dtype == x.dtype
    t = _begin()
    check(load().csmae_gemm_dw(dt(dy), M, N, K, _p(dy), dy.stride(0), _p(x), x.stride(0), _p(dw), _p(db), _p(workspace), workspace.numel(), _s(st)), "csmae_gemm_dw")
    if t:
        t.end(("gemm_bf16" if dy.dtype == torch.bfloat16 else "gemm_f32") + "_TN", 2.0 * M * N * K)


# ---- fp8 MFMA path (BASELINE.json configs[4])
FP8_E4M3, FP8_E5M2 = 0, 1


def fp8_quantize(src, dst, amax, dq, fmt=FP8_E4M3, transpose=False, amax_next=None, st=None):
    """dst (uint8: OCP fp8 bytes) = fp8(src * FMAX / amax), per-tensor scale on the device, `dq` receives the de-quantisation factor.
    `amax` / `amax_next` are 64-slot partial maxima (FP8_SLOTS floats, zeroed by the caller before they are written).  Current scaling
    (amax_next None): `amax` first receives max|src|.  Delayed scaling: `amax` is the previous step's and is only read; this step's
    max|src| is folded into `amax_next`.
    transpose: dst is [cols, rows] (weight mirror for dX)."""
    rows, cols = src.shape
    assert dst.dtype == torch.uint8 and dst.shape == ((cols, rows) if transpose else (rows, cols)) and src.stride(1) == 1 and dst.stride(1) == 1
    s = _s(st)
    if amax_next is None:
        check(load().csmae_fp8_amax(dt(src), rows, cols, _p(src), src.stride(0), _p(amax), s), "csmae_fp8_amax")
    check(load().csmae_fp8_quantize(dt(src), fmt, int(transpose), rows, cols, _p(src), src.stride(0), _p(dst), dst.stride(0), _p(amax), _p(dq),
                                    _p(amax_next), s), "csmae_fp8_quantize")


FP8_SLOTS = 64   # an amax is 64 partial maxima (see csrc/fp8.hip)


def fp8_weights(desc, p, w8, w8t, amax, dq, st=None):
    """All fp8 weight mirrors in three launches: desc int64 [count, 3] = (offset in p / w8 / w8t, out, in); amax [count, 64] zeroed, dq [count]."""
    check(load().csmae_fp8_weights(desc.shape[0], _p(desc), _p(p), _p(w8), _p(w8t), _p(amax), _p(dq), _s(st)), "csmae_fp8_weights")


def gemm_fp8(a8, b8, out, dq_a, dq_b, *, a_fmt=FP8_E4M3, bias=None, epilogue=EPI_NONE, aux=None, resid=None, emit=None, skip_out=False, st=None):
    """out[M,N] = dq_a * dq_b * a8[M,K] b8[N,K]^T (+ epilogue): both operands K-contiguous fp8 bytes (uint8 tensors).
    emit = (q_out uint8 [M,N], fmt, amax_prev [64], amax_next [64], dq [1]): the epilogue also writes `out` as fp8 bytes for the next GEMM.
    skip_out (with emit): `out` only names shape / dtype / row stride — the kernel writes the fp8 copy (and the gelu' codes) and not the bf16 tensor."""
    assert not skip_out or emit is not None
    M, K = a8.shape
    N = b8.shape[0]
    assert a8.dtype == torch.uint8 and b8.dtype == torch.uint8 and b8.shape[1] == K and out.shape == (M, N)
    assert resid is None or resid.dtype == out.dtype
    epilogue = _epi(epilogue, aux)
    q_out, *q_rest = _emit_args(emit)   # (csmae_gemm_fp8 takes the copy's row stride behind its pointer)
    t = _begin()
    check(load().csmae_gemm_fp8(a_fmt, M, N, K, _p(a8), a8.stride(0), _p(b8), b8.stride(0), None if skip_out else _p(out), out.stride(0), dt(out), _p(bias), epilogue,
                                _p(aux), aux.stride(0) if aux is not None else 0, _p(resid), resid.stride(0) if resid is not None else 0,
                                _p(dq_a), _p(dq_b), q_out, emit[0].stride(0) if emit else 0, *q_rest, _s(st)), "csmae_gemm_fp8")
    if t:
        t.end("gemm_fp8_NT", 2.0 * M * N * K)
    return out


def _dw_group_args(self, products, workspace, dy, x, dw, db):
    """What DwGroup and DwGroup8 share: the host arrays of device pointers and sizes of a grouped weight-gradient launch, after self.K is set.
    dy, x, dw, db: where a product tuple holds those tensors."""
    VP, LL = ctypes.c_void_p * len(products), ctypes.c_longlong * len(products)
    self.n, self.keep = len(products), (products, workspace)
    self.dY, self.X, self.dW, self.dB = (VP(*[_p(q[i]) for q in products]) for i in (dy, x, dw, db))
    self.ldy, self.ldx = LL(*[q[dy].stride(0) for q in products]), LL(*[q[x].stride(0) for q in products])
    self.M, self.N = LL(*[q[dw].shape[0] for q in products]), LL(*[q[dw].shape[1] for q in products])
    self.flops = sum(2.0 * q[dw].shape[0] * q[dw].shape[1] * self.K for q in products)
    self.ws, self.ws_n = _p(workspace), workspace.numel()


class DwGroup:
    """Argument block of one grouped weight-gradient launch (csmae_gemm_dw_group): the host arrays of device pointers are built once
    — the engine's workspace and gradient buffers do not move — and re-used every step."""

    def __init__(self, products, workspace):
        """products: [(dy [K, >=M], x [K, >=N], dw [M, N] fp32 contiguous, db [M] fp32 or None)] with one K."""
        self.K = products[0][0].shape[0]
        self.dtype = dt(products[0][0])
        for dy, x, dw, db in products:
            assert dy.shape[0] == self.K and x.shape[0] == self.K and dw.is_contiguous() and dy.dtype == x.dtype and dy.stride(1) == 1 and x.stride(1) == 1
        _dw_group_args(self, products, workspace, 0, 1, 2, 3)

    def launch(self, slots=0, st=None):
        t = _begin()
        check(load().csmae_gemm_dw_group(self.dtype, self.n, self.K, self.dY, self.ldy, self.X, self.ldx, self.dW, self.dB, self.M, self.N, slots,
                                         self.ws, self.ws_n, _s(st)), "csmae_gemm_dw_group")
        if t:
            t.end(("gemm_bf16" if self.dtype == BF16 else "gemm_f32") + "_TN", self.flops)


class DwGroup8:
    """Argument block of one grouped fp8 weight-gradient launch (csmae_gemm_dw_group_fp8): products [(dy8 [K, >=M] uint8 e5m2, dq_y [1], x8 [K, >=N] uint8 e4m3,
    dq_x [1], dw [M, N] fp32 contiguous, db [M] fp32 or None)] over one K."""

    def __init__(self, products, workspace):
        self.K = products[0][0].shape[0]
        for dy, dqy, x, dqx, dw, db in products:
            assert dy.dtype == x.dtype == torch.uint8 and dy.shape[0] == x.shape[0] == self.K and dy.stride(1) == x.stride(1) == 1 and dw.is_contiguous()
            assert dqy.dtype == dqx.dtype == torch.float32 and dqy.numel() >= 1 and dqx.numel() >= 1
        _dw_group_args(self, products, workspace, 0, 2, 4, 5)
        self.dqy, self.dqx = ((ctypes.c_void_p * self.n)(*[_p(q[i]) for q in products]) for i in (1, 3))

    def launch(self, slots=0, st=None):
        t = _begin()
        check(load().csmae_gemm_dw_group_fp8(self.n, self.K, self.dY, self.ldy, self.dqy, self.X, self.ldx, self.dqx, self.dW, self.dB, self.M, self.N, slots,
                                             self.ws, self.ws_n, _s(st)), "csmae_gemm_dw_group_fp8")
        if t:
            t.end("gemm_fp8_TN", self.flops)


def attn_resident(dtype_code, T, hd):
    """True when (dtype, T, head_dim) runs the LDS-resident MFMA attention kernels (the ones that can emit an fp8 copy of their output)."""
    return load().csmae_attn_resident(dtype_code, T, hd) == 1


def attn_route(dtype_code, T, hd):
    """The kernel family attn_fwd() / attn_bwd() would run for (dtype, T, head_dim) under the current attn_stream_mode (csmae_attn_route, no launch):
    ATTN_ROUTE_RESIDENT, ATTN_ROUTE_STREAM, ATTN_ROUTE_ANY or ATTN_ROUTE_F32; raises for an unsupported dtype or geometry."""
    rc = load().csmae_attn_route(dtype_code, T, hd)
    if rc < 0:
        raise RuntimeError(f"csmae_attn_route: dtype {dtype_code}, T {T}, head_dim {hd} unsupported ({rc})")
    return rc


def attn_stream_mode(mode=-1):
    """Set which bf16 shapes take the streaming MFMA attention kernels — 0: none (the scalar any-length kernels run what is not LDS-resident), 1: what
    is not resident (default), 2: every shape with head_dim % 8 == 0 — and return the previous mode; any other value only queries."""
    return load().csmae_attn_stream_mode(mode)


def attn_fwd(qkv, out, lse, B, T, H, hd, emit=None, st=None):
    """emit = (q_out uint8 [B*T, H*hd], fmt, amax_prev [64], amax_next [64], dq [1]): also write `out` as fp8 bytes for attn.proj's GEMM."""
    if emit is None:
        check(load().csmae_attn_fwd(dt(qkv), B, T, H, hd, _p(qkv), _p(out), _p(lse), _s(st)), "csmae_attn_fwd")
    else:
        check(load().csmae_attn_fwd_q(dt(qkv), B, T, H, hd, _p(qkv), _p(out), _p(lse), *_emit_args(emit), _s(st)), "csmae_attn_fwd_q")


def attn_bwd(qkv, out, dout, lse, dqkv, B, T, H, hd, emit=None, skip_out=False, st=None):
    """skip_out (with emit): only the fp8 copy of dqkv is written."""
    assert not skip_out or emit is not None
    if emit is None:
        check(load().csmae_attn_bwd(dt(qkv), B, T, H, hd, _p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), _s(st)), "csmae_attn_bwd")
    else:
        check(load().csmae_attn_bwd_q(dt(qkv), B, T, H, hd, _p(qkv), _p(out), _p(dout), _p(lse), None if skip_out else _p(dqkv), *_emit_args(emit), _s(st)),
              "csmae_attn_bwd_q")


def _emit_args(emit):
    """emit = (q_out uint8, fmt, amax_prev [64], amax_next [64], dq [1]) or None -> the five trailing C arguments"""
    if emit is None:
        return None, 0, None, None, None
    return _p(emit[0]), emit[1], _p(emit[2]), _p(emit[3]), _p(emit[4])


def layernorm_fwd(x, gamma, beta, y, mean, rstd, y32=None, eps=1e-6, emit=None, skip_out=False, st=None):
    """skip_out (with emit): only the fp8 copy of y (and the row statistics) is written."""
    M, D = x.shape
    assert not skip_out or emit is not None
    check(load().csmae_layernorm_fwd(dt(x), dt(y), M, D, _p(x), _p(gamma), _p(beta), eps, None if skip_out else _p(y), _p(y32), _p(mean), _p(rstd), *_emit_args(emit),
                                     _s(st)), "csmae_layernorm_fwd")


def layernorm_bwd(dy, x, mean, rstd, gamma, dx_out, dgamma, dbeta, dres_in=None, dx_lp=None, partial_ws=None, emit=None, st=None):
    """x, dres_in and dx_out share one dtype (the residual stream's).  dgamma=None with a workspace: the parameter-gradient partial
    rows stay in `partial_ws` for ln_param_reduce."""
    M, D = x.shape
    assert dx_out.dtype == x.dtype and (dres_in is None or dres_in.dtype == x.dtype)
    lp = dt(dx_lp) if dx_lp is not None else dt(dy)
    check(load().csmae_layernorm_bwd(dt(dy), dt(x), lp, M, D, _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dres_in), _p(dx_out), _p(dx_lp), _p(dgamma), _p(dbeta),
                                     _p(partial_ws), partial_ws.numel() if partial_ws is not None else 0, *_emit_args(emit), _s(st)), "csmae_layernorm_bwd")


def ln_param_reduce(count, M, D, partials, goff, gbase, st=None):
    """partials [>= count, slice] fp32 (row k = LayerNorm k's partial rows), goff [count, 2] int64 offsets of dgamma / dbeta in gbase."""
    check(load().csmae_ln_param_reduce(count, M, D, _p(partials), partials.stride(0), partials.shape[1], _p(gbase), _p(goff), _s(st)), "csmae_ln_param_reduce")


def ln_param_reduce_rows(count, rows, D, partials, goff, gbase, st=None):
    """The same fold for LayerNorms whose partial rows were left by gemm_ln_bwd: `rows` = ceil(M / 128) rows per LayerNorm."""
    check(load().csmae_ln_param_reduce_rows(count, rows, D, _p(partials), partials.stride(0), _p(gbase), _p(goff), _s(st)), "csmae_ln_param_reduce_rows")


def bnrelu_fwd(u, gamma, beta, r, mean, rstd, N, L, running_mean=None, running_var=None, nbt=None, eps=1e-5, momentum=0.1, training=True, st=None):
    check(load().csmae_bnrelu_fwd(dt(u), N, L, u.shape[1], _p(u), _p(gamma), _p(beta), eps, momentum, _p(r), _p(mean), _p(rstd),
                                  _p(running_mean), _p(running_var), _p(nbt), int(training), _s(st)), "csmae_bnrelu_fwd")


def bnrelu_bwd(u, dr, gamma, beta, mean, rstd, du, dgamma, dbeta, N, L, st=None):
    check(load().csmae_bnrelu_bwd(dt(u), N, L, u.shape[1], _p(u), _p(dr), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(du), _p(dgamma),
                                  _p(dbeta), _s(st)), "csmae_bnrelu_bwd")


def crop_resize(src, dst, box, st=None):
    S = src.shape[-1]
    check(load().csmae_crop_resize(src.numel() // (S * S), S, _p(src), _p(dst), _p(box), _s(st)), "csmae_crop_resize")


def mask_sort(noise, keep, ids_restore, mask, ids_keep, ids_shuffle=None, st=None):
    rows, L = noise.shape
    check(load().csmae_mask_sort(rows, L, keep, _p(noise), _p(ids_restore), _p(mask), _p(ids_keep), _p(ids_shuffle), _s(st)), "csmae_mask_sort")


def patch_gather(img0, img1, ids_keep, out, N, C, S, p, keep, st=None):
    check(load().csmae_patch_gather(dt(out), out.shape[0], keep, N, C, S, p, _p(img0), _p(img1), _p(ids_keep), _p(out), out.stride(0), _s(st)), "csmae_patch_gather")


def embed_assemble(tok, pos, cls, ids_keep, x, B2, keep, st=None):
    check(load().csmae_embed_assemble(dt(x), B2, keep, x.shape[-1], _p(tok), _p(pos), _p(cls), _p(ids_keep), _p(x), _s(st)), "csmae_embed_assemble")


def embed_assemble_bwd(dx, dtok, dcls, B2, keep, st=None):
    check(load().csmae_embed_assemble_bwd(dt(dx), dt(dtok), B2, keep, dx.shape[-1], _p(dx), _p(dtok), _p(dcls), _s(st)), "csmae_embed_assemble_bwd")


def unshuffle_fwd(z, mask_token, dpos, ids_restore, xd, B2, L, keep, st=None):
    check(load().csmae_unshuffle_fwd(dt(xd), B2, L, keep, xd.shape[-1], _p(z), _p(mask_token), _p(dpos), _p(ids_restore), _p(xd), _s(st)), "csmae_unshuffle_fwd")


def unshuffle_bwd(dxd, ids_restore, dz, dmask_token, B2, L, keep, st=None):
    check(load().csmae_unshuffle_bwd(dt(dxd), dt(dz), B2, L, keep, dxd.shape[-1], _p(dxd), _p(ids_restore), _p(dz), _p(dmask_token), _s(st)), "csmae_unshuffle_bwd")


def rows_gather(src, dst, group, gstride, off, st=None):
    check(load().csmae_rows_gather(dt(dst), dst.shape[0], dst.shape[1], _p(src), group, gstride, off, _p(dst), _s(st)), "csmae_rows_gather")


def rows_gather_idx(x, ids, keep, out, st=None):
    """out[n, k, :] = x[n, ids[n, k], :] for k < keep (x [N, L, D] fp32, ids [N, >= keep] int32, out [N, keep, D] fp32)."""
    N, L, D = x.shape
    assert x.dtype == out.dtype == torch.float32 and ids.dtype == torch.int32 and x.is_contiguous() and out.is_contiguous() and ids.stride(1) == 1
    assert out.shape == (N, keep, D) and ids.shape[0] == N and ids.shape[1] >= keep
    check(load().csmae_rows_gather_idx(N, L, keep, D, _p(x), _p(ids), ids.stride(0), _p(out), _s(st)), "csmae_rows_gather_idx")
    return out


def rows_scatter_add2(a, scale_a, off_a, b, scale_b, off_b, dst, group, gstride, st=None):
    """dst[view(r) + off_a] += scale_a * a[r]; dst[view(r) + off_b] += scale_b * b[r]   (view(r) = (r // group) * gstride + r % group)."""
    assert a.shape == b.shape and a.dtype == b.dtype and dst.dtype == torch.float32
    check(load().csmae_rows_scatter_add2(dt(a), a.shape[0], a.shape[1], _p(a), scale_a, off_a, _p(b), scale_b, off_b, group, gstride, _p(dst),
                                         _s(st)), "csmae_rows_scatter_add2")


def spec_fixup(g, bufs, tmp, dgamma, dbeta, st=None):
    """The speculative cross-decoder backward's fix-up (csmae.h csmae_spec_fixup): dgamma / dbeta += g * tmp[0] / tmp[1]; the three bf16 tensors *= g (no-op for g == 1)."""
    b0, b1, b2 = bufs
    assert all(b.dtype == torch.bfloat16 and b.is_contiguous() for b in bufs) and tmp.shape[0] == 2 and tmp.dtype == torch.float32
    check(load().csmae_spec_fixup(_p(g), _p(b0), b0.numel(), _p(b1), b1.numel(), _p(b2), b2.numel(), _p(tmp[0]), _p(tmp[1]), _p(dgamma), _p(dbeta), tmp.shape[1],
                                  _s(st)), "csmae_spec_fixup")


def rows_scatter_add(src, dst, group, gstride, off, scale=1.0, st=None):
    check(load().csmae_rows_scatter_add(dt(src), src.shape[0], src.shape[1], _p(src), scale, group, gstride, off, _p(dst), _s(st)), "csmae_rows_scatter_add")


def target_minmax(img0, img1, scratch, out, B2, N, C, S, p, norm_pix, st=None):
    check(load().csmae_target_minmax(int(norm_pix), B2, N, C, S, p, _p(img0), _p(img1), _p(scratch), _p(out), _s(st)), "csmae_target_minmax")


def recon_loss_fwd(kind, norm_pix, img0, img1, pred, minmax, rowloss, B2, N, C, S, p, mask=None, st=None):
    """pred: fp32 or bf16 [B2 * (L + 1), >= P]; mask (optional, [B2 * L] fp32): patches with mask 0 are skipped (rowloss 0)."""
    check(load().csmae_recon_loss_fwd(LOSS_KINDS[kind], int(norm_pix), dt(pred), B2, N, C, S, p, _p(img0), _p(img1), _p(pred), pred.stride(0), _p(minmax),
                                      _p(mask), _p(rowloss), _s(st)), "csmae_recon_loss_fwd")


def recon_loss_bwd(kind, norm_pix, img0, img1, pred, minmax, mask, losses, gout, vscale, dpred, B2, N, C, S, p, extra=None, st=None):
    check(load().csmae_recon_loss_bwd(LOSS_KINDS[kind], int(norm_pix), dt(dpred), dt(pred), B2, N, C, S, p, _p(img0), _p(img1), _p(pred), pred.stride(0), _p(minmax),
                                      _p(mask), _p(losses), _p(gout), vscale, _p(extra), _p(dpred), dpred.stride(0), _s(st)), "csmae_recon_loss_bwd")


# ---- ssim family (MAE_ViT_Shared.py:165-267)
def ssim_workspace_floats(B2, C, S, p, levels):
    n = ctypes.c_longlong(0)
    check(load().csmae_ssim_workspace_floats(B2, C, S, p, levels, ctypes.byref(n)), "csmae_ssim_workspace_floats")
    return n.value


def ssim_fwd(levels, norm_pix, img0, img1, pred, mask, ws, terms, B2, N, C, S, p, flags=0, st=None):
    check(load().csmae_ssim_fwd(levels, flags, int(norm_pix), B2, N, C, S, p, _p(img0), _p(img1), _p(pred), pred.stride(0), _p(mask), _p(ws), _p(terms),
                                _s(st)), "csmae_ssim_fwd")


def ssim_apply(pure, views, weight, recon_scale, terms, losses, st=None):
    check(load().csmae_ssim_apply(int(pure), views, weight, recon_scale, _p(terms), _p(losses), _s(st)), "csmae_ssim_apply")


def ssim_bwd(levels, pred, mask, gout, scale, ws, extra, B2, N, C, S, p, st=None):
    check(load().csmae_ssim_bwd(levels, B2, N, C, S, p, _p(pred), pred.stride(0), _p(mask), _p(gout), scale, _p(ws), _p(extra), _s(st)), "csmae_ssim_bwd")


def pair_loss_fwd(kind, rows, D, a, aview, t, tview, partial, st=None):
    check(load().csmae_pair_loss_fwd(LOSS_KINDS[kind], rows, D, _p(a), *aview, _p(t), *tview, _p(partial), _s(st)), "csmae_pair_loss_fwd")


def pair_loss_bwd(kind, rows, D, a, aview, t, tview, gout, coef, da_lp=None, da_acc=None, dt_acc=None, lp_dtype=F32, st=None):
    lp = dt(da_lp) if da_lp is not None else lp_dtype
    check(load().csmae_pair_loss_bwd(LOSS_KINDS[kind], lp, rows, D, _p(a), *aview, _p(t), *tview, _p(gout), coef, _p(da_lp), _p(da_acc), _p(dt_acc),
                                     _s(st)), "csmae_pair_loss_bwd")


def ntxent_fwd(latent, z, inv_norm, E, neg, rowloss, N, Te, keep, tau=0.5, eps=1e-8, st=None):
    check(load().csmae_ntxent_fwd(N, Te, keep, latent.shape[-1], _p(latent), tau, eps, _p(z), _p(inv_norm), _p(E), _p(neg), _p(rowloss), _s(st)), "csmae_ntxent_fwd")


def ntxent_bwd(z, inv_norm, E, neg, gout, dpool, N, tau=0.5, eps=1e-8, st=None):
    check(load().csmae_ntxent_bwd(N, z.shape[-1], _p(z), _p(inv_norm), _p(E), _p(neg), tau, eps, _p(gout), _p(dpool), _s(st)), "csmae_ntxent_bwd")


def latent_grad_finish(dlat, dpool, inv_keep, dlat_lp, B2, Te, st=None):
    lp = dt(dlat_lp) if dlat_lp is not None else F32
    check(load().csmae_latent_grad_finish(lp, B2, Te, dlat.shape[-1], _p(dlat), _p(dpool), inv_keep, _p(dlat_lp), _s(st)), "csmae_latent_grad_finish")


def loss_finalize(per_view, views, rowloss, mask, recon_scale, losses, cd_partial=None, cd_scale=0.0, e_partial=None, e_scale=0.0,
                  ce_rowloss=None, ce_rows=0, st=None):
    check(load().csmae_loss_finalize(per_view, views, _p(rowloss), _p(mask), recon_scale, _p(cd_partial), cd_scale, _p(e_partial), e_scale,
                                     _p(ce_rowloss), ce_rows, _p(losses), _s(st)), "csmae_loss_finalize")


def adamw(tile_off, tile_cnt, tile_wd, p, g, m, v, lr, beta1, beta2, eps, step, p_lp=None, gate=None, tile_ks=None, p_ks=None, st=None):
    """One fused AdamW step over the tiles; `step` (1-based) sets the bias corrections 1 - beta^step; a non-finite `gate` (device
    scalar) turns the launch into a no-op.  tile_ks (int64 [ntiles, 3]: weight offset, N, K; K = 0 none) + p_ks: also write the K-slab mirrors."""
    check(load().csmae_adamw(tile_off.numel(), _p(tile_off), _p(tile_cnt), _p(tile_wd), _p(p), _p(g), _p(m), _p(v), float(lr), float(beta1), float(beta2), float(eps),
                             1.0 - beta1 ** step, 1.0 - beta2 ** step, _p(p_lp), _p(gate), _p(tile_ks), _p(p_ks), _s(st)), "csmae_adamw")


def adamw_fp8(tile8, wd, p, g, m, v, lr, beta1, beta2, eps, step, p_lp, gate, w8, w8t, amax_prev, amax_next, dq, st=None):
    """The fused AdamW step over 64 x 64 sub-blocks of fp8-mirrored weights (tile8 int64 [ntiles, 6]), writing W8 / W8^T with delayed scaling (csmae_adamw_fp8)."""
    check(load().csmae_adamw_fp8(tile8.shape[0], _p(tile8), float(wd), _p(p), _p(g), _p(m), _p(v), float(lr), float(beta1), float(beta2), float(eps), 1.0 - beta1 ** step,
                                 1.0 - beta2 ** step, _p(p_lp), _p(gate), _p(w8), _p(w8t), _p(amax_prev), _p(amax_next), _p(dq), _s(st)), "csmae_adamw_fp8")


def gate_accumulate(loss, slot, accumulate, st=None):
    check(load().csmae_gate_accumulate(_p(loss), _p(slot), int(accumulate), _s(st)), "csmae_gate_accumulate")


def clip_grad_norm(g, max_norm, scratch, out, st=None):
    """out[0] = ||g||_2, out[1] = min(1, max_norm / (norm + 1e-6)); g *= out[1] in place (max_norm <= 0: norm only)."""
    check(load().csmae_clip_grad_norm(g.numel(), _p(g), float(max_norm), _p(scratch), _p(out), _s(st)), "csmae_clip_grad_norm")


def augment_u8(src, meta, mean, inv_std, dst, st=None):
    """src [N, Hmax, Wmax, C] uint8, meta [N, 8] int32 {H, W, i, j, h, w, hflip, vflip}, dst [N, C, S, S] fp32 (util/datasets.py:120-136)."""
    N, Hmax, Wmax, C = src.shape
    assert src.dtype == torch.uint8 and src.is_contiguous() and meta.dtype == torch.int32 and meta.shape == (N, 8) and dst.shape[:2] == (N, C)
    check(load().csmae_augment_u8(N, C, Hmax, Wmax, dst.shape[-1], _p(src), _p(meta), _p(mean), _p(inv_std), _p(dst), _s(st)), "csmae_augment_u8")


def eval_u8(src, meta, mean, inv_std, dst, st=None):
    """src [N, Hmax, Wmax, C] uint8, meta [N, 8] int32 {H, W, Hr, Wr, top, left, 0, 0} (util.gpu_input.eval_transform_params), dst [N, C, S, S]
    fp32: the eval transform of util/datasets.py:140-158."""
    N, Hmax, Wmax, C = src.shape
    assert src.dtype == torch.uint8 and src.is_contiguous() and meta.dtype == torch.int32 and meta.shape == (N, 8) and dst.shape[:2] == (N, C)
    assert dst.dtype == torch.float32 and dst.is_contiguous() and dst.shape[-1] == dst.shape[-2]
    check(load().csmae_eval_u8(N, C, Hmax, Wmax, dst.shape[-1], _p(src), _p(meta), _p(mean), _p(inv_std), _p(dst), _s(st)), "csmae_eval_u8")


def _u16_args(src, meta, band, mean, inv_std, dst):
    """The argument list the two multispectral launchers share: src [N, Hmax, Wmax, Cin] uint16, meta [N, 8] int32, band [Cout] int32 ON THE HOST
    (the library reads and checks it before the launch), mean / inv_std [Cout] fp32, dst [N, Cout, S, S] fp32."""
    N, Hmax, Wmax, Cin = src.shape
    Cout = band.numel()
    assert src.dtype == torch.uint16 and src.is_contiguous() and meta.dtype == torch.int32 and meta.shape == (N, 8) and meta.is_contiguous()
    assert band.dtype == torch.int32 and not band.is_cuda and band.is_contiguous(), "band is a host int32 tensor"
    assert mean.dtype == inv_std.dtype == torch.float32 and mean.numel() == inv_std.numel() == Cout
    assert dst.dtype == torch.float32 and dst.is_contiguous() and dst.shape[0] == N and dst.shape[1] == Cout and dst.shape[-1] == dst.shape[-2]
    return N, Cin, Cout, Hmax, Wmax, dst.shape[-1], _p(src), _p(meta), band.data_ptr(), _p(mean), _p(inv_std), _p(dst)


def augment_u16(src, meta, band, mean, inv_std, dst, st=None):
    """The training transform of multispectral tiles (util/datasets.py:489-564): src [N, Hmax, Wmax, Cin] uint16 in raw units, meta [N, 8] int32
    {H, W, i, j, h, w, hflip, vflip}, band [Cout] host int32 (source band of each output channel, bit 8 = masked), dst [N, Cout, S, S] fp32."""
    check(load().csmae_augment_u16(*_u16_args(src, meta, band, mean, inv_std, dst), _s(st)), "csmae_augment_u16")


def eval_u16(src, meta, band, mean, inv_std, dst, st=None):
    """The eval transform of multispectral tiles: as augment_u16 with meta {H, W, Hr, Wr, top, left, 0, 0} (util.gpu_input.eval_transform_params)."""
    check(load().csmae_eval_u16(*_u16_args(src, meta, band, mean, inv_std, dst), _s(st)), "csmae_eval_u16")


def cast_bf16(src, dst, st=None):
    check(load().csmae_cast_f32_to_bf16(src.numel(), _p(src), _p(dst), _s(st)), "csmae_cast_f32_to_bf16")


def cast_f32(src, dst, st=None):
    check(load().csmae_cast_bf16_to_f32(src.numel(), _p(src), _p(dst), _s(st)), "csmae_cast_bf16_to_f32")


def colsum(x, out, st=None):
    check(load().csmae_colsum(dt(x), x.shape[0], x.shape[1], _p(x), x.stride(0), _p(out), _s(st)), "csmae_colsum")


# ---- linear probing (csrc/classify.hip): everything behind the last transformer block, fp32
def _f32c(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), "linear-probe kernels take contiguous fp32 tensors"


def probe_pool_fwd(x, gamma, beta, feat, global_pool, eps=1e-6, st=None):
    """feat [N, D] = LayerNorm(mean of tokens 1.. of x [N, T, D]) (global_pool) or LayerNorm(x[:, 0]); x fp32 or bf16."""
    N, T, D = x.shape
    assert x.is_contiguous() and feat.shape == (N, D) and gamma.numel() == D and beta.numel() == D
    _f32c(gamma, beta, feat)
    check(load().csmae_probe_pool_fwd(dt(x), int(bool(global_pool)), N, T, D, _p(x), _p(gamma), _p(beta), float(eps), _p(feat), _s(st)), "csmae_probe_pool_fwd")
    return feat


def bn1d_fwd(feat, fbn, running_mean, running_var, nbt=None, eps=1e-6, momentum=0.1, training=True, st=None):
    """BatchNorm1d(D, affine=False) over the batch axis of feat [N, D]; training moves the running statistics in place."""
    N, D = feat.shape
    if training and N == 1:   # (torch.nn.functional.batch_norm's refusal, before anything is launched)
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(feat.shape)}")
    assert fbn.shape == feat.shape and running_mean.numel() == D and running_var.numel() == D and (nbt is None or nbt.dtype == torch.int64)
    _f32c(feat, fbn, running_mean, running_var)
    check(load().csmae_bn1d_fwd(N, D, _p(feat), float(eps), float(momentum), _p(fbn), _p(running_mean), _p(running_var), _p(nbt), int(bool(training)),
                                _s(st)), "csmae_bn1d_fwd")
    return fbn


def head_linear_fwd(x, w, b, logits, st=None):
    """logits [N, K] = x [N, D] w[K, D]^T + b."""
    (N, D), K = x.shape, w.shape[0]
    assert w.shape == (K, D) and logits.shape == (N, K) and (b is None or b.numel() == K)
    _f32c(x, w, b, logits)
    check(load().csmae_head_linear_fwd(N, D, K, _p(x), _p(w), _p(b), _p(logits), _s(st)), "csmae_head_linear_fwd")
    return logits


def head_linear_bwd(dlogits, x, dw, db=None, accumulate=False, gscale=None, st=None):
    """dw [K, D] (+)= gscale dlogits^T x, db [K] (+)= gscale sum_n dlogits (gscale: device scalar or None)."""
    (N, K), D = dlogits.shape, x.shape[1]
    assert x.shape == (N, D) and dw.shape == (K, D) and (db is None or db.numel() == K)
    _f32c(dlogits, x, dw, db, gscale)
    check(load().csmae_head_linear_bwd(N, D, K, _p(dlogits), _p(x), _p(gscale), _p(dw), _p(db), int(bool(accumulate)), _s(st)), "csmae_head_linear_bwd")


def softmax_ce(logits, labels, loss, dlogits=None, counts=None, gout=None, accumulate_counts=False, scratch=None, st=None):
    """loss[0] = mean cross-entropy; dlogits = gout (softmax - onehot) / N; counts [2] (+)= top-1 / top-5 hits.  labels int64 [N]."""
    N, K = logits.shape
    assert labels.dtype == torch.int64 and labels.numel() == N and labels.is_contiguous() and (dlogits is None or dlogits.shape == logits.shape)
    _f32c(logits, loss, dlogits, counts, gout)
    if scratch is None:
        scratch = torch.empty(3 * N, device=logits.device, dtype=torch.float32)
    assert scratch.numel() >= 3 * N
    check(load().csmae_softmax_ce(N, K, _p(logits), _p(labels), _p(gout), _p(scratch), _p(loss), _p(dlogits), _p(counts), int(bool(accumulate_counts)),
                                  _s(st)), "csmae_softmax_ce")


LARS_NORM_FLOATS = 128   # scratch floats per tensor of a csmae_lars_step launch


def lars_table(params, grads, mus):
    """Device table of csmae_lars_step: one row {p, g, mu addresses, numel, ndim > 1} per tensor (contiguous fp32 on the GPU)."""
    rows = []
    for p, g, mu in zip(params, grads, mus):
        _f32c(p, g, mu)
        assert g.shape == p.shape and mu.shape == p.shape
        rows.append([_p(p), _p(g), _p(mu), p.numel(), int(p.dim() > 1)])
    return torch.tensor(rows, dtype=torch.int64).to(params[0].device)


def lars_step(table, norms, lr, weight_decay, momentum, trust_coefficient, gate=None, st=None):
    n = table.shape[0]
    assert table.dtype == torch.int64 and table.shape[1] == 5 and table.is_contiguous() and norms.numel() >= n * LARS_NORM_FLOATS
    _f32c(norms, gate)
    check(load().csmae_lars_step(n, _p(table), float(lr), float(weight_decay), float(momentum), float(trust_coefficient), _p(norms), _p(gate), _s(st)), "csmae_lars_step")


# ---- end-to-end fine-tuning (csrc/classify.hip)
def probe_pool_bwd(x, dfeat, gamma, dres, dgamma, dbeta, global_pool, eps=1e-6, accumulate=False, partial=None, st=None):
    """Reverse of probe_pool_fwd: dres [N, T, D] (the dtype of x, every element written) from dfeat [N, D]; dgamma / dbeta [D] (+)= over the batch."""
    N, T, D = x.shape
    if global_pool and T < 2:   # (the forward's refusal, before anything is launched)
        raise ValueError(f"global_pool averages tokens 1 .. T-1: T = {T} leaves nothing to average")
    assert x.is_contiguous() and dres.is_contiguous() and dres.shape == x.shape and dres.dtype == x.dtype and dfeat.shape == (N, D)
    assert gamma.numel() == D and dgamma.numel() == D and dbeta.numel() == D
    _f32c(dfeat, gamma, dgamma, dbeta, partial)
    if partial is None:
        partial = torch.empty(2 * N * D, device=x.device, dtype=torch.float32)
    assert partial.numel() >= 2 * N * D
    check(load().csmae_probe_pool_bwd(dt(x), int(bool(global_pool)), N, T, D, _p(x), _p(dfeat), _p(gamma), float(eps), _p(dres), _p(partial), _p(dgamma),
                                      _p(dbeta), int(bool(accumulate)), _s(st)), "csmae_probe_pool_bwd")
    return dres


def head_linear_dx(dlogits, w, dx, gscale=None, st=None):
    """dx [N, D] = gscale dlogits [N, K] w [K, D] (gscale: device scalar or None)."""
    (N, K), D = dlogits.shape, w.shape[1]
    assert w.shape == (K, D) and dx.shape == (N, D)
    _f32c(dlogits, w, dx, gscale)
    check(load().csmae_head_linear_dx(N, D, K, _p(dlogits), _p(w), _p(gscale), _p(dx), _s(st)), "csmae_head_linear_dx")
    return dx


def soft_ce(logits, target, loss, dlogits=None, gout=None, scratch=None, st=None):
    """loss[0] = mean soft-target cross-entropy against dense targets [N, K]; dlogits = gout (softmax sum(target) - target) / N."""
    N, K = logits.shape
    assert target.shape == (N, K) and (dlogits is None or dlogits.shape == logits.shape)
    _f32c(logits, target, loss, dlogits, gout)
    if scratch is None:
        scratch = torch.empty(N, device=logits.device, dtype=torch.float32)
    assert scratch.numel() >= N
    check(load().csmae_soft_ce(N, K, _p(logits), _p(target), _p(gout), _p(scratch), _p(loss), _p(dlogits), _s(st)), "csmae_soft_ce")


def mixup_target(labels, target, lam=1.0, smoothing=0.0, st=None):
    """target [N, K] = lam onehot(y) + (1 - lam) onehot(y flipped), label-smoothed (timm mixup_target); lam = 1: plain label smoothing."""
    N, K = target.shape
    assert labels.dtype == torch.int64 and labels.numel() == N and labels.is_contiguous()
    _f32c(target)
    check(load().csmae_mixup_target(N, K, _p(labels), float(lam), float(smoothing), _p(target), _s(st)), "csmae_mixup_target")
    return target


def mixup_cutmix(x, out, lam=1.0, box=None, st=None):
    """out[n] = lam x[n] + (1 - lam) x[N-1-n] (box None), or x[n] with box = (yl, yh, xl, xh) copied from x[N-1-n].  Out of place, N even."""
    N, C, H, W = x.shape
    if N % 2:   # (timm's assertion, before anything is launched)
        raise ValueError(f"Batch size should be even when using this (got {N})")
    assert out.shape == x.shape and out.data_ptr() != x.data_ptr()
    _f32c(x, out)
    yl, yh, xl, xh = (0, 0, 0, 0) if box is None else (int(v) for v in box)
    check(load().csmae_mixup_cutmix(int(box is not None), N, C, H, W, _p(x), _p(out), float(lam), yl, yh, xl, xh, _s(st)), "csmae_mixup_cutmix")
    return out


def pos_embed_grad(dres, dpos, accumulate=False, st=None):
    """dpos [T, D] fp32 (+)= sum over the batch of dres [N, T, D] (fp32 or bf16)."""
    N, T, D = dres.shape
    assert dres.is_contiguous() and dpos.numel() == T * D
    _f32c(dpos)
    check(load().csmae_pos_embed_grad(dt(dres), N, T, D, _p(dres), _p(dpos), int(bool(accumulate)), _s(st)), "csmae_pos_embed_grad")


# ---- k-NN evaluation (csrc/knn.hip)
def l2_normalize(src, dst, eps=1e-12, st=None):
    """dst [rows, D] (contiguous, fp32 or bf16) = src[r] / max(||src[r]||, eps); src fp32 [rows, D], rows may be strided."""
    rows, D = src.shape
    assert src.dtype == torch.float32 and src.stride(1) == 1 and dst.shape == (rows, D) and dst.is_contiguous()
    check(load().csmae_l2_normalize(dt(src), dt(dst), rows, D, _p(src), src.stride(0), float(eps), _p(dst), _s(st)), "csmae_l2_normalize")
    return dst


def knn_select(sim, val, idx, base=0, Bc=None, st=None):
    """Merge the similarity tile sim[:, :Bc] (fp32, rows may be strided; bank rows base .. base+Bc-1) into the best-k lists val / idx [Q, k]
    (fp32 / int32, contiguous; a fresh search starts from (-inf, -1)).  k outside [1, 64] is refused."""
    Q, k = val.shape
    Bc = sim.shape[1] if Bc is None else int(Bc)
    assert sim.dtype == torch.float32 and sim.shape[0] == Q and sim.stride(1) == 1 and 0 < Bc <= sim.shape[1]
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and idx.shape == val.shape and val.is_contiguous() and idx.is_contiguous()
    t = _begin()
    check(load().csmae_knn_select(Q, Bc, k, _p(sim), sim.stride(0), int(base), _p(val), _p(idx), _s(st)), "csmae_knn_select")
    if t:
        t.end("knn_select", 4.0 * Q * Bc)   # work: the bytes of the tile


def knn_vote(val, idx, bank_labels, num_classes, T, top5, votes=None, counts=None, query_labels=None, accumulate_counts=False, st=None):
    """votes [Q, K] (optional) = the exp(val / T)-weighted votes of the neighbours' labels, top5 [Q, 5] int32 the best classes (ties to the lower
    id, -1 behind the K-th); with query_labels (int64) counts [2] (+)= top-1 / top-5 hits."""
    Q, k = val.shape
    K = int(num_classes)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and idx.shape == val.shape and val.is_contiguous() and idx.is_contiguous()
    assert bank_labels.dtype == torch.int64 and bank_labels.is_contiguous() and top5.dtype == torch.int32 and top5.shape == (Q, 5) and top5.is_contiguous()
    assert votes is None or votes.shape == (Q, K)
    assert query_labels is None or (query_labels.dtype == torch.int64 and query_labels.numel() == Q and query_labels.is_contiguous() and counts is not None)
    _f32c(votes, counts)
    check(load().csmae_knn_vote(Q, k, K, _p(val), _p(idx), _p(bank_labels), 1.0 / float(T), _p(votes), _p(top5), _p(counts), _p(query_labels),
                                int(bool(accumulate_counts)), _s(st)), "csmae_knn_vote")


# ---- per-image reconstruction scores (csrc/recon_eval.hip)
def recon_eval_workspace_floats(N, C, S):
    n = ctypes.c_longlong(0)
    check(load().csmae_recon_eval_workspace_floats(N, C, S, ctypes.byref(n)), "csmae_recon_eval_workspace_floats")
    return n.value


def recon_eval(img, pred, mean, std, p, out=None, st=None, ws=None):
    """out [N, 4] fp32 = per image {sum (X - Y)^2, sum |X - Y|, ssim(X, Y), 0} with X = img * std + mean and Y = the un-patchified pred * std + mean.
    img: fp32 [N, C, S, S] contiguous.  pred: fp32 or bf16 [N, L, p*p*C], or any view of that shape whose last dimension is dense (wider rows,
    a cls row in front of each image's rows cut off by slicing): its strides are what the kernel walks.  mean, std: fp32 [C] on the device.
    ws: recon_eval_workspace_floats(N, C, S) fp32 (allocated here when None).  The library refuses S < 11, S % p != 0 and any other dtype of pred before it launches anything."""
    N, C, S, S2 = img.shape
    p = int(p)
    assert img.dtype == torch.float32 and img.is_contiguous() and S == S2 and p > 0
    assert pred.dim() == 3 and pred.shape == (N, (S // p) ** 2, p * p * C) and pred.stride(2) == 1, (tuple(pred.shape), pred.stride(), S, p, C)
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and mean.numel() == C and std.numel() == C and mean.is_contiguous() and std.is_contiguous()
    if out is None:
        out = torch.empty(N, 4, device=img.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape == (N, 4) and out.is_contiguous()
    floats = recon_eval_workspace_floats(N, C, S)
    part = ws if ws is not None else torch.empty(floats, device=img.device, dtype=torch.float32)
    assert part.dtype == torch.float32 and part.is_contiguous() and part.numel() >= floats
    t = _begin()
    check(load().csmae_recon_eval(_DT.get(pred.dtype, -1), N, C, S, p, _p(img), _p(pred), pred.stride(1), pred.stride(0), _p(mean), _p(std), _p(part), _p(out),
                                  _s(st)), "csmae_recon_eval")
    if t:
        t.end("recon_eval", (4.0 + pred.element_size()) * N * C * S * S)   # work: the bytes of both operands
    return out


# ---- reconstruction contact sheets (csrc/recon_panel.hip)
def recon_panel(img, pred, mask, mean, std, p, panels=(0, 1, 2), gap=2, bands=None, out=None, st=None):
    """out [N, S, W, 3] uint8, W = K S + (K - 1) gap: per image one RGB row of the K = len(panels) panels, `gap` white pixels between neighbours.
    Panel codes: 0 X, 1 X (1 - m), 2 Y, 3 Y m, 4 X (1 - m) + Y m with X = img * std + mean, Y = the un-patchified pred * std + mean, m = mask of the
    pixel's patch; a value v becomes the byte int(min(max(255 v, 0), 255)).  img, pred, mean, std: as recon_eval takes them.  mask: fp32 [N, L]
    contiguous, 1 = removed.  bands: the channels shown as red, green, blue; None = (0, 1, 2), or (0, 0, 0) for C = 1.  The library refuses
    S % p != 0, 1 > K > 5, a code outside [0, 4], a band outside [0, C), gap < 0 and any other dtype of pred before it launches anything."""
    N, C, S, S2 = img.shape
    p = int(p)
    assert img.dtype == torch.float32 and img.is_contiguous() and S == S2 and p > 0
    assert pred.dim() == 3 and pred.shape == (N, (S // p) ** 2, p * p * C) and pred.stride(2) == 1, (tuple(pred.shape), pred.stride(), S, p, C)
    assert mask.dtype == torch.float32 and mask.shape == (N, (S // p) ** 2) and mask.is_contiguous(), (tuple(mask.shape), mask.dtype)
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and mean.numel() == C and std.numel() == C and mean.is_contiguous() and std.is_contiguous()
    codes = [int(c) for c in panels]
    K, gap = len(codes), int(gap)
    br, bg, bb = (int(b) for b in (bands if bands is not None else ((0, 0, 0) if C == 1 else (0, 1, 2))))
    W = K * S + (K - 1) * gap
    if out is None:
        out = torch.empty(N, S, max(W, 0), 3, device=img.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.shape == (N, S, W, 3) and out.is_contiguous(), (tuple(out.shape), out.dtype, (N, S, W, 3))
    codes = (codes + [0] * 5)[:max(K, 5)]
    t = _begin()
    check(load().csmae_recon_panel(_DT.get(pred.dtype, -1), N, C, S, p, _p(img), _p(pred), pred.stride(1), pred.stride(0), _p(mask), _p(mean), _p(std), br, bg, bb,
                                   codes[0], codes[1], codes[2], codes[3], codes[4], K, gap, _p(out), _s(st)), "csmae_recon_panel")
    if t:
        t.end("recon_panel", 3.0 * W * S * N + (4.0 + pred.element_size()) * N * min(C, 3) * S * S)   # work: the bytes written + the shown planes of both operands
    return out


# ---- linear segmentation probe (csrc/segment.hip)
SEG_CE_SCRATCH_FLOATS = 2048   # scratch floats of a csmae_seg_ce launch


def seg_token_norm(x, gamma, beta, out, eps=1e-6, st=None):
    """out [N L, D] fp32 = LayerNorm of the L patch tokens of x [N, L + 1, D] (fp32 or bf16, contiguous); the cls row of each image is dropped."""
    N, T, D = x.shape
    assert x.is_contiguous() and out.shape == (N * (T - 1), D) and gamma.numel() == D and beta.numel() == D
    _f32c(gamma, beta, out)
    check(load().csmae_seg_token_norm(dt(x), N, T, D, _p(x), _p(gamma), _p(beta), float(eps), _p(out), _s(st)), "csmae_seg_token_norm")
    return out


def seg_ce(pl, labels, loss, count, dpl=None, conf=None, scratch=None, gscale=None, pred=None, st=None):
    """Mean cross-entropy of the patch logits pl [N, G, G, K] (fp32), upsampled bilinearly (align_corners=False) to the S x S labels [N, S, S] (uint8,
    255 = ignored; None only with pred): loss [1] fp32, count [1] int64 = the valid pixels.  With no valid pixel the loss is 0 and the gradient all
    zeros (torch.nn.functional.cross_entropy gives NaN there).  dpl [N, G, G, K] (optional) = gscale d loss / d pl (gscale: device scalar or None),
    every element written.  conf [K, K] int64 (optional) += the confusion counts, rows = true class, columns = argmax class; the caller zeroes it.
    pred [N, S, S] uint8 (optional) = the argmax class of every pixel.  The library refuses K outside [2, 64], S / G not in {4, 8, 14, 16} and
    S != G (S / G) before it launches anything."""
    N, G, G2, K = pl.shape
    S = (labels if labels is not None else pred).shape[-1]
    assert G == G2 and G > 0 and (labels is not None or pred is not None)
    for t in (labels, pred):
        assert t is None or (t.dtype == torch.uint8 and t.shape == (N, S, S) and t.is_contiguous()), "labels / pred: contiguous uint8 [N, S, S]"
    assert loss.numel() >= 1 and count.dtype == torch.int64 and count.numel() >= 1 and count.is_contiguous()
    assert dpl is None or (dpl.shape == pl.shape and labels is not None)
    assert conf is None or (conf.dtype == torch.int64 and conf.shape == (K, K) and conf.is_contiguous())
    _f32c(pl, loss, dpl, gscale)
    if scratch is None:
        scratch = torch.empty(SEG_CE_SCRATCH_FLOATS, device=pl.device, dtype=torch.float32)
    _f32c(scratch)
    assert scratch.numel() >= SEG_CE_SCRATCH_FLOATS
    p = S // G
    t = _begin()
    check(load().csmae_seg_ce(N, G, p, K, S, _p(pl), _p(labels), _p(scratch), _p(loss), _p(count), _p(conf), _p(pred), _s(st)), "csmae_seg_ce")
    if dpl is not None:
        check(load().csmae_seg_ce_bwd(N, G, p, K, S, _p(pl), _p(labels), _p(count), _p(gscale), _p(dpl), _s(st)), "csmae_seg_ce_bwd")
    if t:
        t.end("seg_ce", float(N) * S * S + 4.0 * pl.numel() * (1 if dpl is None else 3))   # work: the label bytes + the logits (read again and written by the backward)


# ---- overlay sheets, argmax map and per-image counts of the segmentation probe (csrc/seg_panel.hip)
def seg_panel(img, pl, labels, mean, std, palette, panes=(0, 3, 4), alpha=0.5, gap=2, bands=None, ignore_rgb=(224, 224, 192), out=None, pred=None, stats=None,
              st=None):
    """out [N, S, W, 3] uint8, W = P S + (P - 1) gap: per image one RGB row of the P = len(panes) panes, `gap` white pixels between neighbours.
    Pane codes: 0 image, 1 gt, 2 pred, 3 gt_over, 4 pred_over, 5 errors (include/csmae.h states each byte).  img [N, C, S, S] fp32 contiguous,
    normalised; mean, std fp32 [C]; pl [N, G, G, K] fp32 patch logits, S = G p, upsampled bilinearly as seg_ce does; labels uint8 [N, S, S] (255 =
    ignored) or None; palette uint8 [K, 3] on the device; alpha: the overlay's weight, taken as a8 = round(256 alpha); bands: the channels shown as
    red, green, blue (None = (0, 1, 2), or (0, 0, 0) for C = 1).  pred [N, S, S] uint8 (optional) = the argmax class of every pixel; stats [N, K, 3]
    int32 (optional, needs labels) = per image and class (intersection, label area, prediction area), overwritten.  The library refuses K outside
    [2, 64], S / G not in {4, 8, 14, 16}, S != G (S / G), 1 > P > 6, a code outside [0, 5], a pane 1, 3, 5 or stats without labels, a band outside
    [0, C), gap < 0, alpha outside [0, 1] and N S W 3 >= 2^31 before it launches anything."""
    N, C, S, S2 = img.shape
    assert img.dtype == torch.float32 and img.is_contiguous() and S == S2
    assert pl.dim() == 4 and pl.shape[0] == N and pl.shape[1] == pl.shape[2] and pl.shape[1] > 0, (tuple(pl.shape), N)
    G, K = pl.shape[1], pl.shape[3]
    _f32c(pl)
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and mean.numel() == C and std.numel() == C and mean.is_contiguous() and std.is_contiguous()
    assert palette.dtype == torch.uint8 and palette.shape == (K, 3) and palette.is_contiguous(), (tuple(palette.shape), palette.dtype, K)
    for t in (labels, pred):
        assert t is None or (t.dtype == torch.uint8 and t.shape == (N, S, S) and t.is_contiguous()), "labels / pred: contiguous uint8 [N, S, S]"
    assert stats is None or (stats.dtype == torch.int32 and stats.shape == (N, K, 3) and stats.is_contiguous()), "stats: contiguous int32 [N, K, 3]"
    codes = [int(c) for c in panes]
    P, gap = len(codes), int(gap)
    br, bg, bb = (int(b) for b in (bands if bands is not None else ((0, 0, 0) if C == 1 else (0, 1, 2))))
    ir, ig, ib = (int(v) for v in ignore_rgb)
    a8 = int(round(256.0 * float(alpha)))
    W = P * S + (P - 1) * gap
    if out is None:
        out = torch.empty(N, S, max(W, 0), 3, device=img.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.shape == (N, S, W, 3) and out.is_contiguous(), (tuple(out.shape), out.dtype, (N, S, W, 3))
    codes = (codes + [0] * 6)[:max(P, 6)]
    t = _begin()
    check(load().csmae_segpanel(N, C, S, G, S // G, K, _p(img), _p(mean), _p(std), br, bg, bb, _p(pl), _p(labels), _p(palette), ir, ig, ib, a8, codes[0], codes[1],
                                 codes[2], codes[3], codes[4], codes[5], P, gap, _p(out), _p(pred), _p(stats), _s(st)), "csmae_segpanel")
    if t:
        # work: the bytes written + the shown planes of the image + the labels + the logits
        t.end("seg_panel", 3.0 * W * S * N + 4.0 * N * min(C, 3) * S * S + (0 if labels is None else N * S * S) + (0 if pred is None else N * S * S) + 4.0 * pl.numel())
    return out


__all__ =[n for n in dir() if not n.startswith("_")]
