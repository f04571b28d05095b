"""What the streaming-attention tests share (tests/test_attn_stream_gpu.py, tests/test_attn_stream_cpu.py): the seeded inputs, the fp64 reference
with its autograd, the derived forward bound, and a torch emulation of the streaming forward kernel's rounding points.

Forward bound.  The kernel (csrc/attention_stream.hip) rounds P to bf16 once (relative error <= 2^-9), rounds the output once (relative error
<= 2^-9) and keeps everything else — scores, exponentials, the running sum l (from the un-rounded p), the rescaled accumulators — in fp32, so
    |out - ref| <= 2^-9 (sum_j P_ij |V_jd| + |ref_id|)
up to fp32 terms.  The tests allow FWD_FACTOR = 2 times that plus 1e-6, elementwise.  The emulation below, run on CPU
(tests/test_attn_stream_cpu.py prints the figures), reaches a maximum of |err| / (2^-9 (sum P|V| + |ref|)) of 0.48 at (T, hd) = (577, 32) and
0.37 at (1370, 64), against 42 / 60 with the last key tile dropped and 196 / 160 with one rescale left out: the factor 2 — twice the worst case
of the derivation, four times what random data reaches — is kept as derived; it is far from hiding either bug (both asserted there)."""
import torch

TILE = 64           # ATTN_STREAM_TILE: rows of one streamed tile (csrc/attention_common.h)
OWN = 128           # ATTN_STREAM_OWN: rows a workgroup owns
FWD_FACTOR = 2.0
U_BF16 = 2.0 ** -9  # relative error of one round-to-nearest bf16 rounding


def inputs(B, T, H, hd):
    """qkv [B*T, 3*H*hd] and dout [B*T, H*hd], bf16, seeded by the geometry (CPU tensors)."""
    g = torch.Generator().manual_seed(1000 * T + 10 * hd + B + H)
    D = H * hd
    return torch.randn(B * T, 3 * D, generator=g).to(torch.bfloat16), torch.randn(B * T, D, generator=g).to(torch.bfloat16)


def reference(qkv, dout, B, T, H, hd, backward=True):
    """fp64 softmax attention on the bf16-rounded inputs (on the inputs' device): out [B*T, D], lse [B, H, T], sum_j P_ij |V_jd| [B*T, D] and,
    with `backward`, dqkv [B*T, 3D] from autograd."""
    D = H * hd
    x = qkv.double().requires_grad_(backward)
    q, k, v = x.reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * hd ** -0.5
    att = torch.softmax(s, dim=-1)
    out = (att @ v).transpose(1, 2).reshape(B * T, D)
    lse = torch.logsumexp(s.detach(), dim=-1)
    pabsv = (att.detach() @ v.detach().abs()).transpose(1, 2).reshape(B * T, D)
    grad = None
    if backward:
        out.backward(dout.double())
        grad = x.grad
    return out.detach(), lse, pabsv, grad


def fwd_excess(out, ref, pabsv):
    """max over elements of |out - ref| / (FWD_FACTOR 2^-9 (sum P|V| + |ref|) + 1e-6): the bound holds when this is <= 1.  Also returns the
    maximum of |out - ref| / (2^-9 (sum P|V| + |ref|)), the figure the factor is judged by."""
    err = (out.double() - ref).abs()
    unit = U_BF16 * (pabsv + ref.abs())
    return float((err / (FWD_FACTOR * unit + 1e-6)).max()), float((err / unit.clamp_min(1e-30)).max())


def emulate_stream_fwd(qkv, B, T, H, hd, drop_last_tile=False, no_rescale_tile=None):
    """The streaming forward's arithmetic in torch: key tiles of TILE rows, online softmax in the log2 domain, fp32 everywhere except P (rounded
    to bf16 before P V; l sums the un-rounded p) and the bf16 output.  drop_last_tile / no_rescale_tile inject the two bugs the bound has to see:
    the last key tile never processed, and the O accumulator not rescaled by exp2(m_old - m_new) at tile `no_rescale_tile`."""
    D = H * hd
    q, k, v = qkv.float().reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    c2 = hd ** -0.5 * 1.4426950408889634
    m = torch.full((B, H, T, 1), float("-inf"))
    l = torch.zeros(B, H, T, 1)
    o = torch.zeros(B, H, T, hd)
    nt = -(-T // TILE)
    for it in range(nt - 1 if drop_last_tile else nt):
        kt, vt = k[:, :, it * TILE:(it + 1) * TILE], v[:, :, it * TILE:(it + 1) * TILE]
        s = q @ kt.transpose(-2, -1)
        mn = torch.maximum(m, s.amax(dim=-1, keepdim=True) * c2)
        alpha = torch.exp2(m - mn)
        p = torch.exp2(s * c2 - mn)
        l = l * alpha + p.sum(dim=-1, keepdim=True)
        o = (o if it == no_rescale_tile else o * alpha) + p.to(torch.bfloat16).float() @ vt
        m = mn
    out = (o / l).to(torch.bfloat16).transpose(1, 2).reshape(B * T, D)
    lse = ((m + torch.log2(l)) * 0.6931471805599453).squeeze(-1)
    return out, lse
