"""Helpers of the token-plumbing tests (test_tokens_gpu.py) and of their CPU self-check (test_tokens_cpu.py): guarded buffers for the five
dtypes csrc/tokens.hip touches, one plain reference per entry point written from the operation's definition (the kernel file's header
comments and include/csmae.h), fp32 emulations with seeded defects, and the geometry tuples both test files walk.

Contracts (what the reference is, and what the comparison is):

Bit-exact
  - mask_sort: ids_shuffle is the stable ascending argsort of the noise (rank(i) = #{j : n[j] < n[i] or (n[j] == n[i] and j < i)}, so
    -0.0 == 0.0 as in torch.argsort(stable=True)), ids_restore its inverse permutation, mask = rank >= keep, ids_keep the first `keep` of
    ids_shuffle.  Tie rows included.
  - patch_gather: an fp32 output equals the source element, a bf16 output its round-to-nearest-even bf16; pad columns [P, ld) are +0.
  - embed_assemble, unshuffle_fwd: one fp32 addition of two fp32 operands, then for a bf16 stream one RNE rounding.
  - embed_assemble_bwd dtok, unshuffle_bwd dz, rows_gather, rows_gather_idx: a copy (one RNE rounding into bf16).  dz starts as the sentinel
    and every element must be written; with keep == L dmask_token keeps its prior content bit for bit.
  - spec_fixup buffers: g == 1 leaves all three bit-identical (NaN payloads and sentinel-valued elements included); otherwise each element
    is bf16_rne(fp32(x) * g).

Fused or unfused
  - rows_scatter_add, rows_scatter_add2, spec_fixup dgamma / dbeta: dst + src * scale in fp32.  The compiler may contract it to an fma, so
    each element must equal, bit for bit, fl(dst + fl(src * scale)) or fma(src, scale, dst) (fma32 below: exact product and TwoSum in
    fp64, rounded to odd, then to fp32 - no double rounding).  Rows outside the view keep their content exactly.

Counted sum bound (fp64 reference)
  - dcls: sample group sg adds its cdiv(B2, 32) samples in a row, block folds the 32 groups onto the prior content in a row:
    depth = cdiv(B2, 32) + 32.
  - dmask_token: row group g adds its cdiv(L, 8) rows in a row, 8 LDS partials in a row, then one atomic per sample onto the prior content in
    any order: depth = cdiv(L, 8) + 8 + B2.  (The order of those atomics is not fixed: two runs of the same binary on the same data can
    differ in the last bit of a dmask_token element - seen in the flagship benchmark as one mask_token element one ulp apart after 40
    steps - so this output is held to the bound, which covers every order, and not to bits.)
  - |err| <= depth * 2^-24 * (sum |terms| + |prior|) + 2^-24 |result|.  No global-maximum tolerance.
    Worst error / bound of the honest fp32 emulations over every geometry of this file (test_tokens_cpu.py prints them):
    dcls 0.073 (order 0), 0.080 (order 1); dmask_token 0.195 (order 0), 0.207 (order 1).

crop_resize (fp64 reference of the same filter: triangle filter, support max(scale, 1) = 1 for a box inside the image, window
[int(c - 0.5), int(c + 1.5)) clipped to the box, weights renormalised, horizontal pass first)
  - centre c~ = fl(fl(in / out) * (o + 0.5)): two roundings, |c~ - c| <= 2 u c;
  - a window edge fl(fl(c~ -+ 1) + 0.5): two more roundings of a magnitude <= c + 1.5, so a tap that is in one window and not in the other has a
    true weight <= 2 u c + 2 u (c + 1.5): the result is continuous across the boundary;
  - a tap's weight 1 - |fl(fl((k + lo) - c~) + 0.5)|: (k + lo) is exact, the difference and the sum are <= 2 in magnitude (2 u each), the final
    subtraction u: 5 u;
    so every un-normalised weight is off by at most e_w = 4 u c + 8 u;
  - the window total (>= 0.5: the nearest tap alone weighs that much; 1 away from the box's edges) adds the taps' errors and two additions;
    the division rounds once: |dw^_k| <= (e_w + w^_k (3 e_w + 2 u tot)) / tot + u w^_k <= 2 e_w (1 + 3 w^_k) + 5 u w^_k;
  - out = sum_a wy_a sum_b wx_b v_ab: first order in the weights' errors plus their product, and 3 + 3 additions and 2 multiplications per
    term: 8 u sum wy wx |v|.
  The candidate taps of an output are the four positions floor(c - 0.5) - 1 .. + 2 inside the box (either window is among them).
  The full-image box is an exact identity (weights 1 and 0) and is compared by bits.  Worst error / bound of the fp32 emulation over every
  geometry of this file: 0.118 (the oracle and the crop golden, which evaluate the filter in fp32 too: 0.082).  A box larger than the image would read outside the plane, so the kernel's down-sampling branch cannot be
  reached by a valid call and is not tested.
"""
import functools

import numpy as np
import torch

import norm_ref
from gemm_bounds import SENTINEL, U32

BF, F32, U8, I32, I64 = torch.bfloat16, torch.float32, torch.uint8, torch.int32, torch.int64
# integer outputs hold ranks, token ids and box coordinates: all >= 0, so a negative sentinel cannot be a result
INT_SENTINEL = {I32: -0x5A5A5A5B, I64: -0x5A5A5A5A5A5A5A5B}
_INT = {BF: torch.int16, F32: torch.int32, U8: torch.uint8, I32: torch.int32, I64: torch.int64}
cdiv = norm_ref.cdiv


class Guarded(norm_ref.Guarded):
    """norm_ref.Guarded for any shape (a zero-sized view is guards only) and for int32 / int64 as well: the view sits 16-byte aligned
    between two runs of sentinel elements, prefilled with the sentinel unless `fill` is given.  `snapshot` keeps the bits of an input."""

    def __init__(self, shape, dtype, fill=None, device="cuda"):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        es = torch.empty(0, dtype=dtype).element_size()
        q = 16 // es
        cols = shape[-1]
        g = cdiv(max(2 * cols, q), q) * q
        n = int(np.prod(shape))
        self.shape, self.rows, self.cols, self.dtype, self.g, self.start, self.n = shape, n // cols if cols else 0, cols, dtype, g, g, n
        self.sentinel = INT_SENTINEL[dtype] if dtype in INT_SENTINEL else SENTINEL[dtype]
        self.ibase = torch.full((g + n + g + q,), self.sentinel, dtype=_INT[dtype], device=device)
        assert self.ibase.data_ptr() % 16 == 0
        self.base = self.ibase.view(dtype)
        self.t = self.base[g:g + n].view(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0 and (n == 0 or self.t.data_ptr() == self.ibase.data_ptr() + g * es)
        if fill is not None:
            fill = fill if torch.is_tensor(fill) else torch.full(shape, fill)
            if fill.dtype == _INT[dtype] and fill.dtype != dtype:
                self.ibase[g:g + n].copy_(fill.reshape(-1))      # raw bits of a float type
            else:
                self.t.copy_(fill.to(dtype).reshape(shape))
        self.snap = self.bits().clone()

    def bits(self):
        return self.ibase[self.start:self.start + self.n].view(self.shape)

    def unchanged(self):
        return torch.equal(self.bits(), self.snap)


def bits_of(t):
    """The bit pattern of a CPU tensor as integers (bf16 -> int16, fp32 -> int32)."""
    return t.contiguous().view(_INT[t.dtype])


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ geometry tuples
MASK_ROWS = (1, 3)
MASK_L = (1, 2, 63, 64, 65, 255, 256, 257, 1024)
MASK_L_LIMIT = 16384                 # the largest L csmae_mask_sort accepts: 64 KiB of dynamic LDS
MASK_NOISE = ("uniform", "four", "equal", "zeros")
PATCH_GEOMS = ((1, 8, 2), (3, 32, 16), (4, 28, 14), (13, 16, 8), (3, 8, 1))   # (C, S, p)
PATCH_N = (1, 2)
PATCH_PADS = (0, 1, 8, 40)
EMBED_D = (4, 8, 64, 516, 1024, 1028)
EMBED_KEEP = (0, 1, 5)
EMBED_B2 = (1, 3)
EMBED_L = 7
EMBED_BWD_B2 = (1, 31, 32, 33, 513, 1100)
EMBED_BWD_D = (4, 8, 12, 64, 772)
EMBED_BWD_KEEP = (0, 1, 3)
BWD_ROUTES = ((F32, F32), (F32, BF), (BF, BF))                                # (gradient in, gradient out)
UNSH_B2 = (1, 3)
UNSH_LD = tuple((9, d) for d in (4, 64, 508, 512, 516, 1024, 1028)) + tuple((l, 516) for l in (1, 7, 8, 196))
ROWS_CASES = ((1, 8), (5, 8), (4097, 8), (5, 4), (5, 516))                    # (rows, D); 4097: one past the grid cap
ROWS_CASES2 = ((1, 8), (5, 8), (8193, 8), (5, 4), (5, 516))
ROWS_FORMS = ("engine", "group1", "off0")
SCALES = (1.0, 0.5, -1.0, 0.3)
IDX_D = (1, 7, 8, 516)
IDX_GEOMS = ((3, 5, 1, 4), (8, 1100, 1025, 1030))                              # (N, L, keep, ids_ld): N keep = 3 and 8200
SPEC_G = (1.0, 0.5, -3.0, 0.0)
SPEC_SIZES = (8, 8000, 1024 * 256 * 8 + 8)                                    # the last: a second grid-stride trip of one uint4
SPEC_L = (1, 255, 256, 257, 2048)
CROP_S = (8, 12, 60, 64, 260)
CROP_PLANES = (1, 3)


def mask_keeps(L):
    return tuple(sorted({0, 1, L // 4, L - 1, L} & set(range(L + 1))))


def patch_keeps(L):
    return tuple(sorted({1, max(L // 4, 1), L}))


def unsh_keeps(L):
    return tuple(sorted({0, 1, L // 4, L} & set(range(L + 1))))


def _factor(rows):
    return {1: (1, 1), 5: (1, 5), 4097: (17, 241), 8193: (3, 2731)}[rows]     # rows = N * L


def rows_view(form, rows):
    """(group, gstride, off_a, off_b, storage rows) of a row view.  engine: the decoder embedding [2 N, L + 1, D] without its cls rows,
    off_a the original's half, off_b the crop's (what rows_gather / rows_scatter_add use).  The two views are disjoint in every form."""
    if form == "engine":
        N, L = _factor(rows)
        return L, L + 1, 1, N * (L + 1) + 1, 2 * N * (L + 1)
    if form == "group1":
        return 1, 2, 1, 0, 2 * rows + 1
    if form == "off0":
        return 3, 7, 3, 0, cdiv(rows, 3) * 7
    raise ValueError(form)


def storage_rows(rows, group, gstride, off):
    """view row r -> storage row (r / group) * gstride + off + r % group"""
    r = torch.arange(rows)
    return (r // group) * gstride + off + r % group


def crop_boxes(S):
    """(i, j, h, w): the full image, 1 x 1 at each corner, one row, one column, the bottom-right quadrant, four seeded boxes inside the image."""
    g = torch.Generator().manual_seed(4000 + S)
    out = [(0, 0, S, S), (0, 0, 1, 1), (0, S - 1, 1, 1), (S - 1, 0, 1, 1), (S - 1, S - 1, 1, 1), (S // 3, 0, 1, S), (0, S // 3, S, 1),
           (S - S // 2, S - S // 2, S // 2, S // 2)]
    for _ in range(4):
        h, w = (int(torch.randint(1, S + 1, (1,), generator=g)) for _ in range(2))
        i, j = int(torch.randint(0, S - h + 1, (1,), generator=g)), int(torch.randint(0, S - w + 1, (1,), generator=g))
        out.append((i, j, h, w))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ mask_sort
@functools.lru_cache(maxsize=None)
def mask_noise(rows, L, kind):
    g = torch.Generator().manual_seed(100 + 7 * rows + 13 * L)
    if kind == "uniform":
        return torch.rand(rows, L, generator=g)
    if kind == "four":
        return torch.randint(0, 4, (rows, L), generator=g).float() * 0.25
    if kind == "equal":
        return torch.full((rows, L), 0.5)
    z = torch.zeros(rows, L)                               # "zeros": +0.0 and -0.0 mixed: one tie class
    z[torch.rand(rows, L, generator=g) < 0.5] = -0.0
    return z


def mask_sort_ref(noise, keep, defect=None):
    """From the definition: rank(i) = #{j : n[j] < n[i] or (n[j] == n[i] and j < i)}.  Returns ids_restore (int64), mask (fp32),
    ids_keep (int32 [rows, keep]), ids_shuffle (int32)."""
    n = noise.numpy()
    rows, L = n.shape
    rank = np.empty((rows, L), dtype=np.int64)
    j = np.arange(L)
    for r in range(rows):
        for i0 in range(0, L, 1024):
            i = np.arange(i0, min(i0 + 1024, L))
            v = n[r, i][:, None]
            tie = (j[None, :] > i[:, None]) if defect == "tie_reversed" else (j[None, :] < i[:, None])
            rank[r, i] = ((n[r][None, :] < v) | ((n[r][None, :] == v) & tie)).sum(1)
    shuffle = np.empty((rows, L), dtype=np.int32)
    np.put_along_axis(shuffle, rank, np.broadcast_to(np.arange(L, dtype=np.int32), (rows, L)), 1)
    mask = (rank > keep) if defect == "rank_gt_keep" else (rank >= keep)
    return torch.from_numpy(rank), torch.from_numpy(mask.astype(np.float32)), torch.from_numpy(shuffle[:, :keep].copy()), torch.from_numpy(shuffle)


# ------------------------------------------------------------------------------------------------ patch_gather
@functools.lru_cache(maxsize=None)
def patch_inputs(C, S, p, N, keep, views):
    L = (S // p) ** 2
    g = torch.Generator().manual_seed(200 + C + 3 * S + 5 * p + 7 * N + 11 * keep + views)
    imgs = [torch.randn(N, C, S, S, generator=g) for _ in range(views)]
    ids = torch.randint(0, L, (views * N * keep,), generator=g, dtype=torch.int32)     # with replacement: duplicates
    ids[0], ids[-1] = 0, L - 1
    if ids.numel() > 2:
        ids[1] = ids[0]
    return imgs, ids.reshape(views * N, keep)


def patch_gather_ref(imgs, ids, p, ld, dtype, defect=None):
    """out[n2 * keep + t][c p p + ph p + pw] = view(n2 / N)[n2 % N][c][gh p + ph][gw p + pw], token ids[n2, t] = gh G + gw; pads +0."""
    if defect == "view1_reads_img0":
        imgs = [imgs[0]] * len(imgs)
    x = torch.cat(imgs)
    B, C, S, _ = x.shape
    G, P = S // p, C * p * p
    l = ids.long()
    gh, gw = (l % G, l // G) if defect == "gh_gw_swapped" else (l // G, l % G)
    e = torch.arange(P)
    c, ph, pw = e // (p * p), (e % (p * p)) // p, e % p
    n2 = torch.arange(B)[:, None, None]
    val = x[n2, c[None, None, :], gh[:, :, None] * p + ph[None, None, :], gw[:, :, None] * p + pw[None, None, :]]     # [B, keep, P]
    out = torch.full((B * ids.shape[1], ld), 1.0 if defect == "pad_not_zeroed" else 0.0)
    out[:, :P] = val.reshape(-1, P)
    return out.to(dtype)


# ------------------------------------------------------------------------------------------------ embed_assemble
@functools.lru_cache(maxsize=None)
def embed_inputs(B2, keep, D):
    g = torch.Generator().manual_seed(300 + B2 + 3 * keep + 5 * D)
    tok, pos, cls = torch.randn(B2 * keep, D, generator=g), torch.randn(EMBED_L + 1, D, generator=g), torch.randn(D, generator=g)
    ids = torch.randint(0, EMBED_L, (B2, keep), generator=g, dtype=torch.int32)
    if keep:
        ids[0, 0], ids[-1, -1] = 0, EMBED_L - 1
    return tok, pos, cls, ids


def embed_assemble_ref(tok, pos, cls, ids, dtype, defect=None):
    """x[n2, 0] = cls + pos[0];  x[n2, 1 + t] = tok[n2 keep + t] + pos[1 + ids[n2, t]]"""
    B2, keep = ids.shape
    D = tok.shape[1]
    x = torch.empty(B2, keep + 1, D)
    x[:, 0] = cls + pos[0]
    x[:, 1:] = tok.reshape(B2, keep, D) + pos[ids.long() + (0 if defect == "pos_without_plus1" else 1)]
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def embed_bwd_inputs(B2, keep, D, in_dtype):
    g = torch.Generator().manual_seed(400 + B2 + 3 * keep + 5 * D)
    dx = (torch.randn(B2, keep + 1, D, generator=g) * (0.5 + torch.rand(B2, 1, 1, generator=g))).to(in_dtype)
    return dx, torch.randn(D, generator=g) * 2.0 + 0.5


def sum_bound(depth, terms_abs, prior, result):
    return depth * U32 * (terms_abs + prior.double().abs()) + U32 * result.abs()


def embed_bwd_ref(dx, prior, out_dtype):
    """dtok[n2 keep + t] = dx[n2, 1 + t] (one rounding);  dcls = prior + sum_n2 dx[n2, 0] in fp64, and its bound."""
    B2, T, D = dx.shape
    c = dx[:, 0].double()
    dcls = prior.double() + c.sum(0)
    return dx[:, 1:].reshape(B2 * (T - 1), D).float().to(out_dtype), dcls, sum_bound(cdiv(B2, 32) + 32, c.abs().sum(0), prior, dcls)


def _chain(acc, terms, order):
    """acc + terms[0] + terms[1] ... in fp32, one addition at a time (order 1: backwards)."""
    for k in (range(len(terms)) if order == 0 else range(len(terms) - 1, -1, -1)):
        acc = acc + terms[k]
    return acc


def embed_bwd_emu(dx, prior, out_dtype, order=0, defect=None):
    """embed_assemble_bwd_kernel in fp32 torch: (dtok, dcls).  The cls workgroup: 4 column units x 32 sample groups; group sg adds samples
    sg, sg + 32, ...; the groups are folded onto the prior content in a row.  The token workgroups stride over the samples by the grid."""
    B2, T, D = dx.shape
    c = dx[:, 0].float()
    nb = (B2 // 32) * 32 if defect == "drop_ragged_sample_group" else B2
    parts = [_chain(torch.zeros(D), list(c[sg:nb:32]), order) for sg in range(32)]
    dcls = _chain(torch.zeros(D) if defect == "prior_overwritten" else prior.clone(), parts, order)
    if defect == "drop_last_column_unit" and (D // 4) % 4:
        lost = (D // 4) // 4 * 16
        dcls[lost:] = prior[lost:]
    dtok = dx[:, 1:].float().to(out_dtype).clone()
    if defect == "drop_grid_tail" and B2 > 512:
        dtok[512:] = float("nan")        # (never written)
    return dtok.reshape(B2 * (T - 1), D), dcls


# ------------------------------------------------------------------------------------------------ unshuffle
@functools.lru_cache(maxsize=None)
def unsh_inputs(B2, L, keep, Dd):
    g = torch.Generator().manual_seed(500 + B2 + 3 * L + 5 * keep + 7 * Dd)
    z, mt, dpos = torch.randn(B2, keep + 1, Dd, generator=g), torch.randn(Dd, generator=g), torch.randn(L + 1, Dd, generator=g)
    ids_restore = torch.argsort(torch.rand(B2, L, generator=g), dim=1)       # a permutation per sample
    dxd = torch.randn(B2, L + 1, Dd, generator=g) * (0.5 + torch.rand(B2, 1, 1, generator=g))
    return z, mt, dpos, ids_restore, dxd, torch.randn(Dd, generator=g) * 2.0 + 0.5


def unshuffle_fwd_ref(z, mt, dpos, ids_restore, dtype, defect=None):
    """xd[n, 0] = z[n, 0] + dpos[0];  xd[n, 1 + j] = (r = ids_restore[n, j]) < keep ? z[n, 1 + r] : mask_token;  + dpos[1 + j]"""
    B2, T, Dd = z.shape
    keep, L = T - 1, ids_restore.shape[1]
    flat = torch.cat([z.reshape(-1, Dd), torch.zeros(1, Dd)])               # (a defective r == keep reads the next sample's cls row)
    r = ids_restore
    kept = (r <= keep) if defect == "r_le_keep" else (r < keep)
    row = torch.arange(B2)[:, None] * T + 1 + r
    src = torch.where(kept[:, :, None], flat[torch.where(kept, row, torch.zeros_like(row))], mt.expand(B2, L, Dd))
    xd = torch.empty(B2, L + 1, Dd)
    xd[:, 0] = z[:, 0] + dpos[0]
    xd[:, 1:] = src + dpos[1:]
    return xd.to(dtype)


def unshuffle_bwd_ref(dxd, ids_restore, keep, prior, out_dtype):
    """dz[n, 0] = dxd[n, 0]; dz[n, 1 + r] = dxd[n, 1 + j] where r = ids_restore[n, j] < keep; dmask_token = prior + the other rows, fp64."""
    B2, T, Dd = dxd.shape
    L = T - 1
    dz = torch.full((B2, keep + 1, Dd), float("nan"))
    dz[:, 0] = dxd[:, 0].float()
    masked = torch.zeros(Dd, dtype=torch.float64)
    absm = torch.zeros(Dd, dtype=torch.float64)
    for n in range(B2):
        r = ids_restore[n]
        k = r < keep
        dz[n, 1 + r[k]] = dxd[n, 1:][k].float()
        masked += dxd[n, 1:][~k].double().sum(0)
        absm += dxd[n, 1:][~k].double().abs().sum(0)
    dm = prior.double() + masked
    return dz.to(out_dtype), dm, sum_bound(cdiv(L, 8) + 8 + B2, absm, prior, dm)


def unshuffle_bwd_emu(dxd, ids_restore, keep, prior, order=0, defect=None):
    """dmask_token of unshuffle_bwd_kernel in fp32 torch: per sample, row group g adds the masked rows among j = g, g + 8, ...; the 8 partials
    are added in a row; one atomic per sample onto the prior content (order 1: every chain backwards)."""
    B2, T, Dd = dxd.shape
    L = T - 1
    dm = torch.zeros(Dd) if defect == "prior_overwritten" else prior.clone()
    sums = []
    for n in range(B2):
        r = ids_restore[n]
        masked = (r > keep) if defect == "r_le_keep" else (r >= keep)
        rows = dxd[n, 1:].float() * masked[:, None]
        parts = [_chain(torch.zeros(Dd), list(rows[g::8]), order) for g in range(8)]
        s = _chain(parts[0] if order == 0 else parts[7], parts[1:] if order == 0 else parts[:7], order)
        if defect == "stale_partials" and Dd > 512:      # the second trip's fold reads the first trip's partials of groups 1..7
            stale = _chain(parts[0], parts[1:], 0)
            s = s.clone()
            w = min(Dd - 512, 512)
            s[512:512 + w] = parts[0][512:512 + w] + (stale - parts[0])[:w]
        sums.append(s)
    return _chain(dm, sums, order)


# ------------------------------------------------------------------------------------------------ row views
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for fp32 tensors: the product is exact in fp64, the sum is rounded to odd in fp64 (TwoSum gives the
    exact residual), and 53 >= 2 * 24 + 2 bits make the final rounding to fp32 the correct one."""
    p = a.double().numpy() * b.double().numpy()
    cc = c.double().numpy()
    s = p + cc
    bb = s - p
    e = (p - (s - bb)) + (cc - bb)                      # exact: p + cc == s + e
    bits = s.view(np.int64).copy()
    inexact = e != 0
    toward_zero = inexact & ((e > 0) != (s > 0))        # the exact sum is smaller in magnitude than s: step back one ulp
    bits[toward_zero] -= 1
    bits[inexact] |= 1
    return torch.from_numpy(bits.view(np.float64).astype(np.float32))


def axpy_both(dst, src, scale):
    """The two fp32 evaluations of dst + src * scale: (unfused, fused)."""
    s = torch.tensor(scale, dtype=torch.float32)
    x = src.float()
    return dst + x * s, fma32(x, s.expand_as(x), dst)


def one_of(got, a, b):
    """Elements of got that equal neither a nor b, bit for bit."""
    g = bits_of(got)
    return int(((g != bits_of(a)) & (g != bits_of(b))).sum())


@functools.lru_cache(maxsize=None)
def rows_inputs(rows, D, nstore, dtype):
    g = torch.Generator().manual_seed(600 + rows + 3 * D + 5 * nstore)
    return (torch.randn(rows, D, generator=g).to(dtype), torch.randn(rows, D, generator=g).to(dtype), torch.randn(nstore, D, generator=g),
            torch.randn(nstore, D, generator=g))


def rows_gather_ref(store, rows, group, gstride, off, dtype, cap=4096, defect=None):
    out = store[storage_rows(rows, group, gstride, off)].to(dtype)
    if defect == "drop_grid_tail":
        out[cap:] = float("nan")
    return out


def rows_scatter_add_emu(src, dst, scale, group, gstride, off, cap=4096, defect=None):
    """(unfused, fused) results of dst[view(r)] += scale src[r]; rows outside the view are dst's."""
    rows = src.shape[0] if defect != "drop_grid_tail" else min(src.shape[0], cap)
    idx = storage_rows(rows, group, gstride, off)
    base = torch.zeros_like(dst[idx]) if defect == "prior_overwritten" else dst[idx]
    u, f = axpy_both(base, src[:rows], scale)
    ou, of = dst.clone(), dst.clone()
    ou[idx], of[idx] = u, f
    return ou, of


def rows_scatter_add2_emu(a, sa, off_a, b, sb, off_b, dst, group, gstride, defect=None):
    if defect == "offsets_exchanged":
        off_a, off_b = off_b, off_a
    u1, f1 = rows_scatter_add_emu(a, dst, sa, group, gstride, off_a, 8192, defect)
    u2, f2 = rows_scatter_add_emu(b, dst, sb, group, gstride, off_b, 8192, defect)
    ia, ib = storage_rows(a.shape[0], group, gstride, off_a), storage_rows(a.shape[0], group, gstride, off_b)
    assert not set(ia.tolist()) & set(ib.tolist()), "the two views overlap"
    u1[ib], f1[ib] = u2[ib], f2[ib]
    return u1, f1


@functools.lru_cache(maxsize=None)
def idx_inputs(N, L, keep, ids_ld, D):
    g = torch.Generator().manual_seed(700 + N + 3 * L + 5 * D)
    ids = torch.randint(0, L, (N, ids_ld), generator=g, dtype=torch.int32)
    ids[0, 0], ids[-1, keep - 1] = L - 1, 0
    return torch.randn(N, L, D, generator=g), ids


def rows_gather_idx_ref(x, ids, keep, defect=None):
    """out[n, k, :] = x[n, ids[n, k], :] for k < keep"""
    out = x[torch.arange(x.shape[0])[:, None], ids[:, :keep].long()].clone()
    if defect == "drop_grid_tail":
        out.reshape(-1, x.shape[2])[8192:] = float("nan")
    return out


# ------------------------------------------------------------------------------------------------ spec_fixup
@functools.lru_cache(maxsize=None)
def spec_inputs(L, g):
    """Three bf16 tensors of SPEC_SIZES elements (as int16 bit patterns), tmp [2, L], dgamma / dbeta priors.  For g == 1 the tensors hold
    arbitrary bit patterns (NaN payloads, infinities, the guard sentinel); otherwise finite values."""
    gen = torch.Generator().manual_seed(800 + L)
    bufs = []
    for k, n in enumerate(SPEC_SIZES):
        if g == 1.0:
            b = torch.randint(-32768, 32768, (n,), generator=gen, dtype=torch.int32).to(torch.int16)
            b[::5] = torch.tensor(SENTINEL[BF], dtype=torch.int16)
        else:
            b = bits_of((torch.randn(n, generator=gen) * 3.0).to(BF)).clone()
        bufs.append(b)
    return bufs, torch.randn(2, L, generator=gen), torch.randn(L, generator=gen), torch.randn(L, generator=gen)


def spec_fixup_emu(bufs, g, defect=None):
    """The three tensors after the call (int16 bit patterns): untouched for g == 1, else bf16_rne(fp32(x) * g)."""
    out = []
    for b in bufs:
        n = b.numel()
        if g == 1.0 and defect != "g1_rescales":
            out.append(b.clone())
            continue
        y = bits_of((b.view(BF).float() * torch.tensor(g, dtype=torch.float32)).to(BF)).clone()
        if defect == "drop_grid_tail":
            y[1024 * 256 * 8:] = b[1024 * 256 * 8:]
        out.append(y)
    return out


# ------------------------------------------------------------------------------------------------ crop_resize
@functools.lru_cache(maxsize=None)
def crop_planes(planes, S):
    return torch.randn(planes, S, S, generator=torch.Generator().manual_seed(900 + planes + 3 * S)) * 2.0 + 0.3


def _axis64(n_in, n_out):
    """Exact (fp64) normalised weights [n_out, n_in] of one axis, the bound of their fp32 evaluation, and that of the candidate taps."""
    o = torch.arange(n_out, dtype=torch.float64)
    scale = n_in / n_out
    c = scale * (o + 0.5)
    sup = max(scale, 1.0)
    k = torch.arange(n_in, dtype=torch.float64)
    lo = torch.floor(c - sup + 0.5).clamp_min(0)
    hi = torch.floor(c + sup + 0.5).clamp_max(n_in)
    x = (k[None, :] + 0.5 - c[:, None]) / sup
    w = (1.0 - x.abs()).clamp_min(0.0) * ((k[None, :] >= lo[:, None]) & (k[None, :] < hi[:, None]))
    tot = w.sum(1, keepdim=True)
    wn = w / tot
    e_w = (4 * U32 * c + 8 * U32)[:, None]
    first = torch.floor(c - 0.5)[:, None] - 1
    cand = (k[None, :] >= first) & (k[None, :] <= first + 3)
    return wn, (2 * e_w * (1 + 3 * wn) + 5 * U32 * wn) * cand


def crop_ref64(planes, box):
    """fp64 crop + anti-aliased bilinear resize back to S x S, horizontal pass first, and the per-element bound of its fp32 evaluation."""
    i, j, h, w = box
    S = planes.shape[-1]
    V = planes[:, i:i + h, j:j + w].double()
    wy, ay = _axis64(h, S)
    wx, ax = _axis64(w, S)
    out = wy @ (V @ wx.t())
    A = V.abs()
    bound = ay @ (A @ wx.t()) + wy @ (A @ ax.t()) + ay @ (A @ ax.t()) + 8 * U32 * (wy @ (A @ wx.t()))
    return out, bound


def _axis32(n_in, n_out):
    """fp32 taps of one axis as ATen's separable filter forms them: (lo, n, weights [n_out, 3]) - float32 numpy, one operation at a time."""
    f = np.float32
    o = np.arange(n_out, dtype=np.float32)
    scale = f(n_in) / f(n_out)
    assert scale <= 1.0
    c = scale * (o + f(0.5))
    lo = np.maximum(((c - f(1.0)) + f(0.5)).astype(np.int32), 0)
    hi = np.minimum(((c + f(1.0)) + f(0.5)).astype(np.int32), n_in)
    n = np.minimum(hi - lo, 8)
    assert n.max() <= 3
    w = np.zeros((n_out, 3), dtype=np.float32)
    tot = np.zeros(n_out, dtype=np.float32)
    for k in range(3):
        a = np.abs(((lo + k).astype(np.float32) - c) + f(0.5))
        wk = np.where((a < 1) & (k < n), f(1.0) - a, f(0.0)).astype(np.float32)
        w[:, k] = wk
        tot = tot + wk
    return lo, n, w / tot[:, None]


def crop_emu32(planes, box):
    """The same filter in fp32, one operation at a time: sum_a wy_a (sum_b wx_b v_ab), taps in ascending order."""
    i, j, h, w = box
    V = planes[:, i:i + h, j:j + w].numpy()
    S = planes.shape[-1]
    ylo, yn, wy = _axis32(h, S)
    xlo, xn, wx = _axis32(w, S)
    out = np.zeros((V.shape[0], S, S), dtype=np.float32)
    for a in range(3):
        ya = np.minimum(ylo + a, h - 1)
        hs = np.zeros((V.shape[0], S, S), dtype=np.float32)
        for b in range(3):
            xb = np.minimum(xlo + b, w - 1)
            hs = hs + np.where(b < xn, wx[:, b], np.float32(0))[None, None, :] * V[:, ya][:, :, xb]
        out = out + np.where(a < yn, wy[:, a], np.float32(0))[None, :, None] * hs
    return torch.from_numpy(out)


def ratio(got, want, bound):
    """Worst |got - want| / bound (inf where a NaN sits)."""
    r = (got.double() - want).abs() / bound.clamp_min(1e-300)
    return float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max()) if r.numel() else 0.0


def diff_bits(got, want):
    """Number of elements whose bit patterns differ."""
    return int((bits_of(got) != bits_of(want)).sum()) if got.dtype in (BF, F32) else int((got != want).sum())
