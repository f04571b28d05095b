"""What the attention-backward tests share (tests/test_attn_bwd_gpu.py, tests/test_attn_bwd_cpu.py, and check_against_fp64 of
tests/test_attn_stream_gpu.py): the fp64 backward that takes the forward results the kernel was handed, per-element bounds counted from the
kernels, the bound against the independent autograd gradient, fp32 emulations of the kernels' arithmetic with seeded defects, and the
geometry tables with the kernel that takes each entry.

fp64 backward with the GIVEN forward results (the idiom of norm_ref.ln_bwd_ref).  From the rounded qkv and dout and the out / lse the kernel
reads:  P = exp(s - lse),  D_i = sum_d dO_id out_id,  dS = P (dO V^T - D) scale,  dQ = dS K,  dK = dS^T Q,  dV = P^T dO.  The reference
shares every input of the kernel, so what is left is what the backward itself rounds.

Rounding points, read from the kernels (u = 2^-9: one round-to-nearest bf16 rounding, (__bf16)x in pack2bf, csrc/common.h; w = 2^-24):
  every bf16 MFMA family — attn_bwd_bf16 (two passes), attn_bwd1p_bf16 with four and with eight waves, attn_bwd1p2_bf16 (csrc/attention.hip)
  and attn_bwd_stream (csrc/attention_stream.hip) — has the SAME scheme:
    - s: fp32 MFMA over head_dim exact bf16 products;  p = exp2(s c2 - lse LOG2E) (v_exp_f32, 1 ulp):  relative error of p before it is
      rounded  e_p = w ((hd + 4) sum_d |q||k| scale + 3 |lse|) + EXP_REL;
    - dP = dO V^T: fp32 MFMA, hd w sum |dO||V|;  D_i: a chain of hd fp32 additions of exact products, hd w sum |dO||out|;
    - dS = p (dP - D) scale: three fp32 operations, then ONE bf16 rounding — pack_pair in the two-pass and streaming kernels; pack2bf on
      the way into the wave's LDS patch in the single-pass kernels, where the SAME rounded values feed dK (pack_pair / the dsp words) and,
      read back transposed, dQ: the trip through LDS adds no rounding of its own.  P is rounded to bf16 once (pack_pair / the pp words);
    - dQ, dK, dV: fp32 MFMA accumulation of exact products over T, and in the single-pass kernels the fp32 read-modify-write of the dQ
      accumulator in LDS once per key pair (at most 9 more additions): depth (T + 47) w sum |terms| covers padded rows and those adds;
    - ONE bf16 rounding of the output (st4<bf16_t>).
    so  |dV err| <= u (sum_i P_ij |dO_id| + |dV|),  |dQ err| <= u (sum_j |dS_ij||K_jd| + |dQ|),  |dK err| <= u (sum_i |dS_ij||Q_id| + |dK|)
    plus the fp32 terms above.  The streaming backward recomputes S, dP and D in each pass with the same operations: no further term.
  attn_bwd_any<bf16_t> (head_dim % 8 != 0, and everything not resident under csmae_attn_stream_mode(0)): fp32 throughout (expf), u only in
    the output rounding;  attn_bwd_f32 and attn_bwd_any<float>: w everywhere.  Same formulae with the inner u set to zero.
The tests allow attn_stream_ref.FWD_FACTOR = 2 times the bound plus 1e-6, the forward's convention, and nothing else.  (bf16 keeps 8
significant bits, so one rounding can lose up to 2^-8 |x|: with u = 2^-9 the factor 2 is what makes the bound hold in the worst case, not
slack — a single output rounding, as in attn_bwd_any<bf16_t>, reaches 0.97 of the allowance.)

Bound against the independent fp64 autograd gradient (attn_stream_ref.reference): the bound above plus what the forward's own error
propagates —  |dD_i| <= sum_d (forward bound of out)_id |dO_id|  and the relative error expm1(|lse err|_i) of P:
    |dS' - dS*| <= |dS'| e_l + P' (1 + e_l) scale |dD|,  carried through the three products.
"""
import torch

import attn_stream_ref as S
from attn_stream_ref import FWD_FACTOR, U_BF16, inputs, reference  # noqa: F401  (re-exported for the two test files)
from gemm_bounds import U32

LOG2E = 1.4426950408889634
EXP_REL = 2.0 ** -22        # v_exp_f32 / expf: 1 ulp by the ISA manual and HIP's math table; two allowed
ABS_FLOOR = 1e-6            # the forward convention's absolute term

# scheme -> (u of P and dS, u of the output)
SCHEMES = {"mfma": (U_BF16, U_BF16), "scalar_bf16": (0.0, U_BF16), "scalar_f32": (0.0, U32)}
TENSORS = ("dq", "dk", "dv")


def cdiv(a, b):
    return -(-a // b)


def heads(x, B, T, H, hd):
    """[B*T, H*hd] -> [B, H, T, hd]"""
    return x.reshape(B, T, H, hd).permute(0, 2, 1, 3)


def split_qkv(x, B, T, H, hd):
    return x.reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)


def join_qkv(dq, dk, dv, B, T, H, hd):
    """three [B, H, T, hd] -> [B*T, 3*H*hd]"""
    return torch.stack((dq, dk, dv), 0).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * H * hd)


def tensor_of(x, i, D):
    """columns of dq (0), dk (1) or dv (2) inside a [B*T, 3D] tensor"""
    return x[:, i * D:(i + 1) * D]


# ------------------------------------------------------------------------------------------------ fp64 reference and bounds
def bwd_given_forward(qkv, dout, out, lse, B, T, H, hd, scheme):
    """fp64 backward of the rounded operands with the GIVEN out [B*T, D] and lse [B, H, T] (any float dtype, on the operands' device).
    Returns grad [B*T, 3D], its per-element bound (no factor, no floor), and the intermediates autograd_extra() needs."""
    u_in, u_out = SCHEMES[scheme]
    q, k, v = split_qkv(qkv.double(), B, T, H, hd)
    g, o = heads(dout.double(), B, T, H, hd), heads(out.double(), B, T, H, hd)
    L = lse.double().reshape(B, H, T)
    scale = hd ** -0.5
    P = torch.exp((q @ k.transpose(-2, -1)) * scale - L[..., None])
    dP = g @ v.transpose(-2, -1)
    Dl = (g * o).sum(-1)
    dS = P * (dP - Dl[..., None]) * scale
    aq, ak, ag = q.abs(), k.abs(), g.abs()
    e_prel = U32 * ((hd + 4) * (aq @ ak.transpose(-2, -1)) * scale + 3 * L.abs()[..., None]) + EXP_REL
    e_dp = hd * U32 * (ag @ v.abs().transpose(-2, -1))
    e_D = hd * U32 * (ag * o.abs()).sum(-1)
    e_pre = dS.abs() * (e_prel + 3 * U32) + P * scale * (e_dp + e_D[..., None])
    e_dS = u_in * dS.abs() + (1 + u_in) * e_pre
    e_P = u_in * P + (1 + u_in) * P * e_prel
    depth = (T + 47) * U32
    grads = (dS @ k, dS.transpose(-2, -1) @ q, P.transpose(-2, -1) @ g)
    errs = (e_dS @ ak + depth * (dS.abs() @ ak), e_dS.transpose(-2, -1) @ aq + depth * (dS.abs().transpose(-2, -1) @ aq),
            e_P.transpose(-2, -1) @ ag + depth * (P.transpose(-2, -1) @ ag))
    bounds = [u_out * (G.abs() + e) + e for G, e in zip(grads, errs)]
    return dict(grad=join_qkv(*grads, B, T, H, hd), bound=join_qkv(*bounds, B, T, H, hd), P=P, dS=dS, aq=aq, ak=ak, ag=ag, scale=scale,
                geom=(B, T, H, hd))


def fwd_unit(ref, pabsv, T, hd, scheme):
    """The forward's per-element unit  u (sum P|V| + |ref|): u = 2^-9 for a bf16 output (attn_stream_ref), and the fp32 accumulation over T
    keys and hd columns, which is all an fp32 output has."""
    return (SCHEMES[scheme][1] + (T + hd + 8) * U32) * (pabsv + ref.abs())


def autograd_extra(G, fwd_bound_out, lse_err):
    """What the forward's error adds to |kernel - autograd gradient|: fwd_bound_out [B*T, D] is the bound the forward output is held to,
    lse_err [B, H, T] = |lse given - lse fp64|."""
    B, T, H, hd = G["geom"]
    e_l = torch.expm1(lse_err.double().reshape(B, H, T))[..., None]
    dD = (heads(fwd_bound_out.double(), B, T, H, hd) * G["ag"]).sum(-1)[..., None]
    e = G["dS"].abs() * e_l + G["P"] * (1 + e_l) * G["scale"] * dD
    return join_qkv(e @ G["ak"], e.transpose(-2, -1) @ G["aq"], (G["P"] * e_l).transpose(-2, -1) @ G["ag"], B, T, H, hd)


def excess(got, want, bound, extra=None):
    """Per tensor (dq, dk, dv): (max err / (FWD_FACTOR bound [+ extra] + 1e-6), max err / bound).  The bound holds when the first is <= 1;
    the second is the figure the factor is judged by.  A NaN anywhere gives inf."""
    D = got.shape[1] // 3
    out = {}
    for i, name in enumerate(TENSORS):
        err = (tensor_of(got, i, D).double() - tensor_of(want, i, D)).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        b = tensor_of(bound, i, D)
        allowed = FWD_FACTOR * b + ABS_FLOOR + (tensor_of(extra, i, D) if extra is not None else 0.0)
        out[name] = (float((err / allowed).max()), float((err / b.clamp_min(1e-300)).max()))
    return out


def check_backward(qkv, dout, out, lse, dqkv, B, T, H, hd, scheme, fwd=None):
    """Both backward bounds of one result, operands on one device.  fwd = (ref, lse_ref, pabsv, grad) of attn_stream_ref.reference when the
    caller has it.  Returns (given-forward excess per tensor, autograd excess per tensor, a line for the log)."""
    ref, lse_ref, pabsv, grad = fwd if fwd is not None else reference(qkv, dout, B, T, H, hd)
    G = bwd_given_forward(qkv, dout, out, lse, B, T, H, hd, scheme)
    given = excess(dqkv, G["grad"], G["bound"])
    fb = FWD_FACTOR * fwd_unit(ref, pabsv, T, hd, scheme) + ABS_FLOOR
    extra = autograd_extra(G, fb, (lse.double().reshape(B, H, T) - lse_ref).abs())
    auto = excess(dqkv, grad, G["bound"], extra)
    line = ", ".join(f"{n} {given[n][1]:.3f} ({given[n][0]:.3f}; autograd {auto[n][0]:.3f})" for n in TENSORS)
    return given, auto, "backward max err / bound (against 2 bound + 1e-6; against autograd): " + line


def worst(ex):
    return max(v[0] for v in ex.values())


# ------------------------------------------------------------------------------------------------ fp32 emulations (CPU self-check)
DEFECTS = ("dq_drop_last_key", "dkv_drop_last_query", "dkv_drop_last_tile", "delta_zero_row", "delta_stale_row", "dp_drop_kslice",
           "scale_missing_key_tile", "pad_rows_live", "sample1_head_offset")


def defect_applies(defect, B, T, H, hd, pad):
    if defect in ("dq_drop_last_key", "dkv_drop_last_query", "delta_stale_row"):
        return T >= 2
    if defect == "dkv_drop_last_tile":
        return T > 16
    if defect in ("delta_zero_row", "scale_missing_key_tile"):
        return True
    if defect == "dp_drop_kslice":           # the last 32-column k step of dP = dO V^T (for a partial head_dim: its masked tail)
        return hd > 32
    if defect == "pad_rows_live":            # needs padded query rows, and rows of another sample behind this one's
        return pad > 0 and T % pad != 0 and B >= 2
    if defect == "sample1_head_offset":
        return B >= 2
    raise ValueError(defect)


def emulate_fwd(qkv, B, T, H, hd, scheme):
    """(out, lse) a forward kernel of the scheme hands the backward: attn_stream_ref's emulation for the MFMA families, plain fp32 softmax
    attention with one output rounding for the scalar kernels."""
    if scheme == "mfma":
        return S.emulate_stream_fwd(qkv, B, T, H, hd)
    q, k, v = split_qkv(qkv.float(), B, T, H, hd)
    s = (q * torch.tensor(hd ** -0.5)) @ k.transpose(-2, -1)
    att = torch.softmax(s, dim=-1)
    out = (att @ v).transpose(1, 2).reshape(B * T, H * hd).to(torch.bfloat16 if scheme == "scalar_bf16" else torch.float32)
    return out, torch.logsumexp(s, dim=-1)


def emulate_bwd(qkv, dout, out, lse, B, T, H, hd, scheme, pad=0, defect=None):
    """The backward's arithmetic in fp32 torch.  mfma: rows padded with zeros to a multiple of `pad` (16: the two-pass kernel's tiles, 32:
    the single-pass kernels' tile pairs, 64: a streamed tile), lse in the log2 domain with +inf on padded rows, P and dS rounded to bf16
    before the three products, one bf16 output rounding.  scalar_*: no padding, no inner rounding, expf.
    Defects (the smallest things a tile kernel gets wrong):
      dq_drop_last_key / dkv_drop_last_query / dkv_drop_last_tile: the last key missing from dQ; the last query, or the last 16-query
        tile, missing from dK and dV;
      delta_zero_row / delta_stale_row: D_i of the last query zero, or the first query's;
      dp_drop_kslice: the last 32-column k step missing from dP;
      scale_missing_key_tile: dS of keys 0..15 not multiplied by scale;
      pad_rows_live: the guards of padded query rows missing — they hold the rows that follow the sample in memory and a finite lse (0)
        instead of +inf, so P is not zero there (with zero-padded operands a finite lse alone changes nothing: p multiplies dO = 0);
      sample1_head_offset: K of every sample behind the first read at the first sample's rows."""
    assert defect is None or defect_applies(defect, B, T, H, hd, pad), defect
    mfma = scheme == "mfma"
    Tp = cdiv(T, pad) * pad if (mfma and pad) else T
    f = torch.float32
    scale = torch.tensor(hd ** -0.5, dtype=f)

    def rows(x):   # [B*T, H*hd] -> [B, H, Tp, hd], zero rows behind the sample (pad_rows_live: the rows that follow it in memory)
        flat = torch.cat((x.to(f), torch.zeros(Tp, x.shape[1])), 0)
        idx = torch.arange(B)[:, None] * T + torch.arange(Tp)[None, :]
        t = flat[idx]
        if defect != "pad_rows_live":
            t[:, T:] = 0.0
        return t.reshape(B, Tp, H, hd).permute(0, 2, 1, 3)

    D3 = H * hd
    q, k, v = (rows(qkv[:, i * D3:(i + 1) * D3]) for i in range(3))
    g, o = rows(dout), rows(out)
    if defect == "pad_rows_live":
        k, v = k.clone(), v.clone()
        k[:, :, T:] = 0.0
        v[:, :, T:] = 0.0
    if defect == "sample1_head_offset":
        k = k[:1].expand(B, -1, -1, -1)
    L = torch.full((B, H, Tp), 0.0 if defect == "pad_rows_live" else float("inf"))
    L[:, :, :T] = lse.to(f).reshape(B, H, T)
    Dl = (o * g).sum(-1)
    if defect == "delta_zero_row":
        Dl[:, :, T - 1] = 0.0
    if defect == "delta_stale_row":
        Dl[:, :, T - 1] = Dl[:, :, 0]
    a = q @ k.transpose(-2, -1)
    if mfma:
        p = torch.exp2(a * (scale * torch.tensor(LOG2E, dtype=f)) - (L * torch.tensor(LOG2E, dtype=f))[..., None])
    else:
        p = torch.exp(a * scale - L[..., None])
    lo = 32 * ((hd - 1) // 32) if defect == "dp_drop_kslice" else hd
    dp = g[..., :lo] @ v[..., :lo].transpose(-2, -1)
    ds = p * (dp - Dl[..., None])
    tile = torch.ones(Tp)
    if defect == "scale_missing_key_tile":
        tile[:16] = 1.0 / scale
    ds = ds * scale * tile
    if mfma:
        p, ds = p.to(torch.bfloat16).to(f), ds.to(torch.bfloat16).to(f)
    nk = T - 1 if defect == "dq_drop_last_key" else Tp
    nq = T - 1 if defect == "dkv_drop_last_query" else (16 * ((T - 1) // 16) if defect == "dkv_drop_last_tile" else Tp)
    dq = ds[..., :nk] @ k[..., :nk, :]
    dk = ds[..., :nq, :].transpose(-2, -1) @ q[..., :nq, :]
    dv = p[..., :nq, :].transpose(-2, -1) @ g[..., :nq, :]
    odt = torch.float32 if scheme == "scalar_f32" else torch.bfloat16
    return join_qkv(dq[..., :T, :], dk[..., :T, :], dv[..., :T, :], B, T, H, hd).to(odt)


# ------------------------------------------------------------------------------------------------ geometry tables
# Mirrors of the dispatch in csrc/attention.hip.  DISPATCH_BF16: head_dim bucket 32 / 64 / 96, key-fragment count NKF by T.
TWO_PASS, ONE_PASS_4, ONE_PASS_2KP, ONE_PASS_8 = "attn_bwd_bf16", "attn_bwd1p_bf16<NW=4>", "attn_bwd1p2_bf16", "attn_bwd1p_bf16<NW=8>"
STREAM, ANY_BF16, F32, ANY_F32 = "attn_bwd_stream", "attn_bwd_any<bf16_t>", "attn_bwd_f32", "attn_bwd_any<float>"
SCHEME_OF = {TWO_PASS: "mfma", ONE_PASS_4: "mfma", ONE_PASS_2KP: "mfma", ONE_PASS_8: "mfma", STREAM: "mfma", ANY_BF16: "scalar_bf16",
             F32: "scalar_f32", ANY_F32: "scalar_f32"}
PAD_OF = {TWO_PASS: 16, ONE_PASS_4: 32, ONE_PASS_2KP: 32, ONE_PASS_8: 32, STREAM: 64, ANY_BF16: 0, F32: 0, ANY_F32: 0}
LDS_LIMIT = 160 * 1024


def bf16_resident(T, hd):
    return hd % 8 == 0 and T <= 288 and (hd <= 32 or (hd <= 64 and T <= 224) or (hd <= 96 and T <= 96))


def resident_bwd_kernel(T, hd):
    """launch_bwd_bf16 without the CSMAE_DEBUG tuning aids."""
    assert bf16_resident(T, hd)
    HD = 32 if hd <= 32 else (64 if hd <= 64 else 96)
    nkf = 2 if T <= 32 else (4 if T <= 64 else (6 if T <= 96 else (14 if T <= 224 else 18)))
    tp = nkf * 16
    lds = 2 * tp * (HD + 8) * 2 + tp * (HD + 4) * 4 + 4 * 32 * HD * 2 + 2 * tp * 4       # AttnBwd1p<HD, NKF>::LDS
    if HD <= 32 and 6 <= nkf <= 16 and lds <= LDS_LIMIT:
        return ONE_PASS_2KP
    if nkf >= 18 and lds + 4 * 32 * HD * 2 <= LDS_LIMIT:
        return ONE_PASS_8
    if lds <= LDS_LIMIT and nkf >= 6:
        return ONE_PASS_4
    return TWO_PASS


def f32_bwd_kernel(T, hd):
    """attn_bwd_impl's fp32 branch: the LDS-resident fp32 kernel while its four images and two statistics rows fit."""
    return ANY_F32 if (4 * T * (hd + 1) + 2 * T) * 4 > LDS_LIMIT or hd > 96 else F32


def f32_fwd_resident(T, hd):
    """attn_fwd_impl's fp32 branch."""
    return not (2 * T * (hd + 1) * 4 > LDS_LIMIT or hd > 96)


def f32_fwd_limit(hd):
    """Largest T whose K and V images fit the forward fp32 kernel's LDS."""
    return LDS_LIMIT // (2 * (hd + 1) * 4)


def f32_bwd_limit(hd):
    return LDS_LIMIT // ((4 * (hd + 1) + 2) * 4)


# (B, T, H, head_dim, kernel).  Resident T edges: 1, 15..17, 31..33, 63..65, 95..97, 223..225, 287, 288; every head_dim bucket edge
# (8, 16, 24, 32 | 40, 64 | 72, 88, 96) in every family that takes it, each partial head_dim at a ragged T; B*H odd, = 1, H = 3; and B*H = 21
# for pair_remap (32-wide buckets, 16 workgroups and more: blocks 0..15 are dealt in pairs, 16..20 are not).
RESIDENT = [
    (1, 1, 1, 16, TWO_PASS), (2, 15, 3, 8, TWO_PASS), (1, 16, 3, 64, TWO_PASS), (2, 17, 3, 24, TWO_PASS), (3, 31, 1, 40, TWO_PASS),
    (1, 32, 1, 96, TWO_PASS), (1, 33, 3, 72, TWO_PASS), (3, 63, 1, 88, TWO_PASS), (2, 64, 2, 32, TWO_PASS), (1, 1, 3, 72, TWO_PASS),
    (3, 17, 7, 32, TWO_PASS),
    (1, 65, 3, 24, ONE_PASS_2KP), (3, 95, 1, 8, ONE_PASS_2KP), (2, 96, 2, 32, ONE_PASS_2KP), (1, 97, 1, 16, ONE_PASS_2KP),
    (1, 129, 3, 32, ONE_PASS_2KP), (1, 223, 1, 24, ONE_PASS_2KP), (1, 224, 3, 8, ONE_PASS_2KP), (3, 65, 7, 16, ONE_PASS_2KP),
    (1, 65, 3, 40, ONE_PASS_4), (3, 95, 1, 64, ONE_PASS_4), (1, 96, 1, 40, ONE_PASS_4), (1, 97, 3, 64, ONE_PASS_4), (2, 129, 2, 64, ONE_PASS_4),
    (1, 223, 1, 40, ONE_PASS_4), (1, 224, 1, 64, ONE_PASS_4), (1, 65, 1, 72, ONE_PASS_4), (3, 95, 1, 88, ONE_PASS_4), (1, 96, 3, 96, ONE_PASS_4),
    (1, 225, 3, 8, ONE_PASS_8), (3, 257, 1, 16, ONE_PASS_8), (1, 287, 1, 24, ONE_PASS_8), (1, 288, 1, 32, ONE_PASS_8), (7, 225, 3, 8, ONE_PASS_8),
]
# (B, T, H, head_dim, csmae_attn_stream_mode that reaches the kernel).  Streaming: just past every resident limit (289 | 225 at head_dim 40..64 |
# 97 at 72..96 | head_dim 128) in the default mode, and resident shapes through mode 2 around ATTN_STREAM_TILE = 64 and ATTN_STREAM_OWN = 128
# with the partial head_dims (tests/test_attn_stream_gpu.py's PARITY holds the long sequences).
STREAMING = [
    (1, 289, 3, 32, 1), (1, 289, 1, 96, 1), (2, 225, 1, 64, 1), (1, 97, 1, 72, 1), (1, 1, 1, 128, 1), (1, 225, 1, 40, 1),
    (1, 1, 3, 16, 2), (1, 63, 3, 24, 2), (1, 64, 1, 40, 2), (3, 65, 1, 72, 2), (1, 127, 1, 88, 1), (1, 128, 1, 8, 2), (1, 129, 3, 16, 2),
    (1, 191, 1, 128, 1), (1, 193, 1, 104, 1),
]
# The any-length bf16 kernels: head_dim % 8 != 0 (4, 20, and one per wider bucket) whatever the mode, and streamable shapes through mode 0.
# T around the forward's 256 queries per workgroup.
ANY = [
    (2, 17, 3, 4, 1), (1, 257, 1, 20, 1), (3, 1, 1, 20, 1), (1, 256, 1, 36, 1), (1, 255, 1, 68, 1), (1, 33, 3, 100, 1), (2, 5, 1, 124, 1),
    (1, 289, 3, 32, 0), (1, 97, 1, 128, 0), (2, 225, 1, 64, 0), (1, 100, 1, 96, 0), (1, 40, 2, 128, 0),
]
# fp32 (parity mode): the LDS-resident fp32 kernels up to their limits (forward and backward differ), the any-length ones beyond and at
# head_dim > 96.
FP32 = [
    (1, 1, 1, 32), (2, 17, 3, 24), (3, 65, 1, 40), (2, 50, 1, 64), (1, 97, 3, 4), (1, 33, 1, 100), (1, 40, 2, 128),
    (1, f32_bwd_limit(96), 1, 96), (1, f32_bwd_limit(96) + 1, 1, 96), (1, f32_fwd_limit(96), 1, 96), (1, f32_fwd_limit(96) + 1, 1, 96),
    (1, f32_bwd_limit(20), 1, 20), (1, f32_bwd_limit(20) + 1, 1, 20),
]

RESIDENT_T_EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 223, 224, 225, 287, 288)
HD_EDGES = (8, 16, 24, 32, 40, 64, 72, 88, 96)


def geom_id(e):
    return "x".join(str(v) for v in e[:4]) + ("" if len(e) == 4 else f"-{e[4]}".replace(" ", ""))
