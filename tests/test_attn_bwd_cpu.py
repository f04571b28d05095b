"""CPU-only self-check of the attention-backward bounds (tests/attn_bwd_ref.py) that tests/test_attn_bwd_gpu.py and check_against_fp64 hold
the kernels to — the role tests/test_norm_bounds_cpu.py plays for the norm bounds.  On the GPU test's own seeded inputs, at one geometry
per kernel family (its padding and rounding scheme): the honest fp32 emulation of the kernel's arithmetic meets the bound against the fp64
backward with the given forward results and the bound against the autograd gradient; every seeded defect that applies to the geometry
breaks the first.  The geometry tables are checked against the mirrors of the dispatch, and every edge the tables promise is in them.

Figures of this file (printed with -s).  Honest emulation, max |err| / bound per family (dq, dk, dv), no factor — the tests allow
2 bound + 1e-6, and u = 2^-9 is half of what one bf16 rounding can lose, so ratios up to 2 are honest:
  attn_bwd_bf16 (2, 17, 3, 40) 1.34, 1.31, 1.08;  attn_bwd1p2_bf16 (2, 197, 2, 32) 0.93, 0.72, 0.73;
  attn_bwd1p_bf16<NW=4> (2, 97, 1, 72) 0.96, 0.89, 0.86;  attn_bwd1p_bf16<NW=8> (2, 257, 1, 24) 0.79, 0.79, 0.60;
  attn_bwd_stream (2, 289, 1, 64) 0.74, 0.98, 0.61;  attn_bwd_any<bf16_t> (2, 50, 3, 20) 1.92, 1.94, 1.94 (one output rounding held to its
  exact worst case);  attn_bwd_f32 / attn_bwd_any<float> (2, 50, 1, 40) 0.011, 0.010, 0.016.
Of the allowance the honest emulations take at most 0.67 (MFMA families), 0.97 (any-length bf16) and 0.008 (fp32); of the autograd
allowance 0.54, 0.97, 0.008.  The smallest seeded defect — D_i of the last query row zeroed at (2, 257, 1, 24), one row of 257 — reaches
6.4 times the allowance (stale D_i there: 9.8); the same two defects reach 18 to 450 at the other MFMA geometries; a dropped key 14 to 112,
a dropped query or tile 16 to 116, a missing k step of dP 111 to 364, a missing scale 227 to 776, live padded rows above 3e4, a wrong
sample offset 158 to 1.5e3; every defect above 700 in the scalar kernels."""
import pytest
import torch

import attn_bwd_ref as R

# one geometry per family: (B, T, H, head_dim, kernel); B >= 2 and a ragged T everywhere, a partial head_dim above 32 where the family takes one
CASES = [(2, 17, 3, 40, R.TWO_PASS), (2, 197, 2, 32, R.ONE_PASS_2KP), (2, 97, 1, 72, R.ONE_PASS_4), (2, 257, 1, 24, R.ONE_PASS_8),
         (2, 289, 1, 64, R.STREAM), (2, 50, 3, 20, R.ANY_BF16), (2, 50, 1, 40, R.F32)]
IDS = [R.geom_id(c) for c in CASES]


def _setup(case):
    B, T, H, hd, kind = case
    scheme = R.SCHEME_OF[kind]
    qkv, dout = R.inputs(B, T, H, hd)
    if scheme == "scalar_f32":
        qkv, dout = qkv.float(), dout.float()
    out, lse = R.emulate_fwd(qkv, B, T, H, hd, scheme)
    return qkv, dout, out, lse, scheme, R.PAD_OF[kind]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_honest_emulation_meets_both_bounds(case):
    B, T, H, hd, kind = case
    qkv, dout, out, lse, scheme, pad = _setup(case)
    dqkv = R.emulate_bwd(qkv, dout, out, lse, B, T, H, hd, scheme, pad)
    given, auto, line = R.check_backward(qkv, dout, out, lse, dqkv, B, T, H, hd, scheme)
    print(f"{kind} {case[:4]}: {line}")
    assert R.worst(given) <= 1.0, (case, given)
    assert R.worst(auto) <= 1.0, (case, auto)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_applicable_defect_breaks_the_given_forward_bound(case):
    B, T, H, hd, kind = case
    qkv, dout, out, lse, scheme, pad = _setup(case)
    G = R.bwd_given_forward(qkv, dout, out, lse, B, T, H, hd, scheme)
    for defect in R.DEFECTS:
        if not R.defect_applies(defect, B, T, H, hd, pad):
            continue
        dqkv = R.emulate_bwd(qkv, dout, out, lse, B, T, H, hd, scheme, pad, defect)
        ex = R.excess(dqkv, G["grad"], G["bound"])
        print(f"{kind} {case[:4]} {defect}: " + ", ".join(f"{n} {ex[n][0]:.3g}" for n in R.TENSORS))
        assert R.worst(ex) > 1.0, (case, defect, ex)


def test_every_seeded_defect_meets_a_geometry():
    for d in R.DEFECTS:
        assert any(R.defect_applies(d, B, T, H, hd, R.PAD_OF[kind]) for B, T, H, hd, kind in CASES), d
    assert {kind for *_, kind in CASES} | {R.ANY_F32} == set(R.SCHEME_OF)          # (attn_bwd_any<float> is attn_bwd_f32's arithmetic)


def test_a_defect_changes_only_what_it_names():
    """The emulation's defects are as small as they claim: dropping the last key from dQ leaves dK and dV alone, a stale D_i touches
    nothing of dV."""
    B, T, H, hd, kind = CASES[0]
    qkv, dout, out, lse, scheme, pad = _setup(CASES[0])
    D = H * hd
    honest = R.emulate_bwd(qkv, dout, out, lse, B, T, H, hd, scheme, pad)
    a = R.emulate_bwd(qkv, dout, out, lse, B, T, H, hd, scheme, pad, "dq_drop_last_key")
    assert torch.equal(a[:, D:], honest[:, D:]) and not torch.equal(a[:, :D], honest[:, :D])
    b = R.emulate_bwd(qkv, dout, out, lse, B, T, H, hd, scheme, pad, "delta_stale_row")
    assert torch.equal(b[:, 2 * D:], honest[:, 2 * D:]) and not torch.equal(b[:, :2 * D], honest[:, :2 * D])


def test_tables_name_the_kernel_the_dispatch_picks():
    for B, T, H, hd, kind in R.RESIDENT:
        assert R.bf16_resident(T, hd) and R.resident_bwd_kernel(T, hd) == kind, (T, hd, kind)
    for B, T, H, hd, mode in R.STREAMING:
        assert hd % 8 == 0 and R.bf16_resident(T, hd) == (mode == 2), (T, hd, mode)
    for B, T, H, hd, mode in R.ANY:
        assert (hd % 8 != 0 and mode == 1) or (hd % 8 == 0 and mode == 0 and not R.bf16_resident(T, hd)), (T, hd, mode)
    kinds = {R.f32_bwd_kernel(T, hd) for _, T, _, hd in R.FP32}
    assert kinds == {R.F32, R.ANY_F32}
    assert {R.f32_fwd_resident(T, hd) for _, T, _, hd in R.FP32} == {True, False}
    # the LDS limits, by formula: the last shape inside and the first beyond, for both kernels
    for hd in (96, 20):
        t = R.f32_bwd_limit(hd)
        assert R.f32_bwd_kernel(t, hd) == R.F32 and R.f32_bwd_kernel(t + 1, hd) == R.ANY_F32
        assert (1, t, 1, hd) in R.FP32 and (1, t + 1, 1, hd) in R.FP32
    t = R.f32_fwd_limit(96)
    assert R.f32_fwd_resident(t, 96) and not R.f32_fwd_resident(t + 1, 96) and (1, t, 1, 96) in R.FP32 and (1, t + 1, 1, 96) in R.FP32


def test_tables_cover_every_edge():
    res_T = {T for _, T, _, _, _ in R.RESIDENT}
    assert set(R.RESIDENT_T_EDGES) <= res_T and max(res_T) <= 288
    by_kind = {}
    for B, T, H, hd, kind in R.RESIDENT:
        by_kind.setdefault(kind, []).append((B, T, H, hd))
    assert set(by_kind) == {R.TWO_PASS, R.ONE_PASS_2KP, R.ONE_PASS_4, R.ONE_PASS_8}
    # every family meets each T edge and head_dim edge it can take
    for kind, geoms in by_kind.items():
        for T in R.RESIDENT_T_EDGES:
            if any(R.bf16_resident(T, hd) and R.resident_bwd_kernel(T, hd) == kind for hd in R.HD_EDGES):
                assert any(g[1] == T for g in geoms), (kind, T)
        for hd in R.HD_EDGES:
            if any(R.bf16_resident(T, hd) and R.resident_bwd_kernel(T, hd) == kind for T in R.RESIDENT_T_EDGES):
                assert any(g[3] == hd for g in geoms), (kind, hd)
        # each partial head_dim (a masked tail inside its bucket) meets a ragged T
        for hd in {g[3] for g in geoms if g[3] not in (32, 64, 96)}:
            assert any(g[3] == hd and g[1] % 16 for g in geoms), (kind, hd)
        bh = {g[0] * g[2] for g in geoms}
        assert 1 in bh and any(n % 2 and n > 1 for n in bh) and any(g[2] == 3 for g in geoms), kind
    # pair_remap deals blocks in pairs from 16 workgroups of a 32-wide bucket on: an odd count above 16 in each such family
    for kind in (R.TWO_PASS, R.ONE_PASS_2KP, R.ONE_PASS_8):
        assert any(g[0] * g[2] > 16 and (g[0] * g[2]) % 2 and g[3] <= 32 for g in by_kind[kind]), kind
    st_T = {T for _, T, *_ in R.STREAMING}
    assert {289, R.S.TILE - 1, R.S.TILE, R.S.TILE + 1, R.S.OWN - 1, R.S.OWN, R.S.OWN + 1} <= st_T
    assert {hd for _, _, _, hd, _ in R.STREAMING} >= set(R.HD_EDGES) | {128}
    any_hd = {hd for _, _, _, hd, _ in R.ANY}
    assert {4, 20, 128} <= any_hd and {0, 1} == {m for *_, m in R.ANY}
    for table in (R.RESIDENT, R.STREAMING, R.ANY, R.FP32):
        assert len(set(table)) == len(table)
