"""CPU self-check of the token-plumbing tests (tests/tokens_ref.py; no GPU needed): the references agree with independent constructions
(torch.argsort, torch.gather, unfold, autograd of the cat / gather / + pos graph, the oracle's crop_resize and the crop golden), the honest
fp32 emulations meet every contract on every geometry tuple, each seeded defect breaks a contract on at least one tuple (the smallest
violation is printed: a ratio for the bounded contracts, a count of differing elements for the exact ones), and the host side of every
entry point of csrc/tokens.hip refuses bad arguments before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tokens_ref as R
from tokens_ref import BF, F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ references vs independent constructions
def test_mask_sort_reference_is_the_stable_argsort():
    for rows in R.MASK_ROWS:
        for L in R.MASK_L + (4100,):
            for kind in R.MASK_NOISE:
                noise = R.mask_noise(rows, L, kind)
                stable = torch.argsort(noise, dim=1, stable=True)
                for keep in R.mask_keeps(L):
                    ids_restore, mask, ids_keep, ids_shuffle = R.mask_sort_ref(noise, keep)
                    assert torch.equal(ids_shuffle.long(), stable), (rows, L, kind)
                    assert torch.equal(ids_restore, torch.argsort(stable, dim=1))
                    assert torch.equal(ids_keep.long(), stable[:, :keep]) and ids_keep.shape == (rows, keep)
                    want = torch.ones(rows, L)
                    want.scatter_(1, stable[:, :keep], 0.0)
                    assert torch.equal(mask, want)


def test_patch_gather_reference_is_unfold():
    for C, S, p in R.PATCH_GEOMS:
        L, P = (S // p) ** 2, C * p * p
        for N in R.PATCH_N:
            for views in (1, 2):
                for keep in R.patch_keeps(L):
                    imgs, ids = R.patch_inputs(C, S, p, N, keep, views)
                    cols = torch.nn.functional.unfold(torch.cat(imgs), kernel_size=p, stride=p).transpose(1, 2)        # [B, L, P]
                    want = torch.gather(cols, 1, ids.long().unsqueeze(-1).expand(-1, -1, P)).reshape(-1, P)
                    for pad in R.PATCH_PADS:
                        got = R.patch_gather_ref(imgs, ids, p, P + pad, F32)
                        assert torch.equal(got[:, :P], want) and R.diff_bits(got[:, P:], torch.zeros(got.shape[0], pad)) == 0
                    got = R.patch_gather_ref(imgs, ids, p, P + 8, BF)
                    assert R.diff_bits(got[:, :P], want.to(BF)) == 0


def test_embed_and_unshuffle_references_are_the_autograd_graph():
    for B2 in R.EMBED_B2:
        for keep in R.EMBED_KEEP:
            tok, pos, cls, ids = R.embed_inputs(B2, keep, 64)
            tr = tok.clone().requires_grad_(True)
            cr = cls.clone().requires_grad_(True)
            x = torch.cat([(cr + pos[0]).expand(B2, 1, 64), tr.reshape(B2, keep, 64) + pos[1:][ids.long()]], dim=1)
            assert R.diff_bits(R.embed_assemble_ref(tok, pos, cls, ids, F32), x.detach()) == 0
            dx, prior = R.embed_bwd_inputs(B2, keep, 64, F32)
            x.backward(dx)
            dtok, dcls, bound = R.embed_bwd_ref(dx, prior, F32)
            assert R.diff_bits(dtok, tr.grad) == 0
            assert R.ratio(cr.grad + prior, dcls, bound) <= 1.0
    for B2 in R.UNSH_B2:
        for L, Dd in ((9, 64), (196, 516), (1, 4)):
            for keep in R.unsh_keeps(L):
                z, mt, dpos, ids_restore, dxd, prior = R.unsh_inputs(B2, L, keep, Dd)
                zr, mtr = z.clone().requires_grad_(True), mt.clone().requires_grad_(True)
                seq = torch.cat([zr[:, 1:], mtr.expand(B2, L - keep, Dd)], dim=1)
                seq = torch.gather(seq, 1, ids_restore.unsqueeze(-1).expand(-1, -1, Dd))
                ref = torch.cat([zr[:, :1], seq], dim=1) + dpos
                assert R.diff_bits(R.unshuffle_fwd_ref(z, mt, dpos, ids_restore, F32), ref.detach()) == 0
                ref.backward(dxd)
                dz, dm, bound = R.unshuffle_bwd_ref(dxd, ids_restore, keep, prior, F32)
                assert R.diff_bits(dz, zr.grad) == 0, "every dz element is written, and to the autograd value"
                assert R.ratio(mtr.grad + prior, dm, bound + R.U32 * dm.abs()) <= 1.0


def test_row_view_references_are_slices_and_gathers():
    for rows, D in R.ROWS_CASES:
        N, L = R._factor(rows)
        group, gstride, off_a, off_b, nstore = R.rows_view("engine", rows)
        src, _, store, _ = R.rows_inputs(rows, D, nstore, F32)
        emb = store.reshape(2 * N, L + 1, D)
        assert torch.equal(R.rows_gather_ref(store, rows, group, gstride, off_b, F32), emb[N:, 1:].reshape(rows, D))
        assert torch.equal(R.rows_gather_ref(store, rows, group, gstride, off_a, F32), emb[:N, 1:].reshape(rows, D))
        want = emb.clone()
        want[N:, 1:] += 0.5 * src.reshape(N, L, D)
        assert torch.equal(R.rows_scatter_add_emu(src, store, 0.5, group, gstride, off_b)[0], want.reshape(-1, D))
    for N, L, keep, ids_ld in R.IDX_GEOMS:
        x, ids = R.idx_inputs(N, L, keep, ids_ld, 7)
        assert torch.equal(R.rows_gather_idx_ref(x, ids, keep), torch.gather(x, 1, ids[:, :keep].long().unsqueeze(-1).expand(-1, -1, 7)))


def test_fma32_rounds_once():
    g = torch.Generator().manual_seed(1)
    a, b, c = (torch.randn(200000, generator=g) for _ in range(3))
    c = c * torch.tensor(2.0) ** torch.randint(-30, 30, (200000,), generator=g)
    got = R.fma32(a, b, c)
    import math
    if hasattr(math, "fma"):
        want = torch.tensor([math.fma(float(x), float(y), float(z)) for x, y, z in zip(a[:20000], b[:20000], c[:20000])], dtype=torch.float64).float()
        assert torch.equal(got[:20000], want)
    # a tie of the double rounding: 1 + 2^-24 + 2^-60 must round up, 1 + 2^-24 - 2^-60 down... in fp32 products: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24
    x = torch.tensor([1.0 + 2.0 ** -12])
    assert float(R.fma32(x, x, torch.tensor([2.0 ** -60]))) == 1.0 + 2.0 ** -11 + 2.0 ** -23
    assert float(R.fma32(x, x, torch.tensor([-2.0 ** -60]))) == 1.0 + 2.0 ** -11
    assert float(R.fma32(x, x, torch.tensor([0.0]))) == 1.0 + 2.0 ** -11          # the tie itself: to even
    exact = (a.double() * b.double() + c.double())
    assert bool(((got.double() - exact).abs() <= R.U32 * exact.abs() + 1e-300).all())


def test_crop_reference_against_the_oracle_and_the_golden():
    import csmae_oracle as O
    d = np.load(os.path.join(ROOT, "tests", "golden", "crop.npz"))
    imgs = torch.from_numpy(d["imgs64"])
    worst = 0.0
    for n, box in enumerate(d["boxes64"]):
        box = tuple(int(v) for v in box)
        ref, bound = R.crop_ref64(imgs.reshape(-1, 64, 64), box)
        for got in (torch.from_numpy(d[f"out64_{n}"]), O.crop_resize(imgs, box, 64)):
            r = R.ratio(got.reshape(-1, 64, 64), ref, bound)
            worst = max(worst, r)
            assert r <= 1.0, (box, r)
    big = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(int(d["seed224"][0])))
    for n, box in enumerate(d["boxes224"]):
        box = tuple(int(v) for v in box)
        ref, bound = R.crop_ref64(big.reshape(-1, 224, 224), box)
        idx = torch.from_numpy(d["idx224"])
        r = R.ratio(torch.from_numpy(d[f"val224_{n}"]), ref.reshape(-1)[idx], bound.reshape(-1)[idx])
        worst = max(worst, r)
        assert r <= 1.0, (box, r)
    for S in (8, 12, 60):
        for box in R.crop_boxes(S):
            pl = R.crop_planes(3, S)
            ref, bound = R.crop_ref64(pl, box)
            r = R.ratio(O.crop_resize(pl[None], box, S)[0], ref, bound)
            worst = max(worst, r)
            assert r <= 1.0, (S, box, r)
    print(f"crop_resize: oracle / golden vs the fp64 reference, worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ honest emulations meet the contracts
def test_crop_emulation_meets_the_bound_and_the_identity():
    worst = 0.0
    for S in R.CROP_S:
        for planes in R.CROP_PLANES:
            pl = R.crop_planes(planes, S)
            for box in R.crop_boxes(S):
                ref, bound = R.crop_ref64(pl, box)
                emu = R.crop_emu32(pl, box)
                r = R.ratio(emu, ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, (S, box, r)
                if box == (0, 0, S, S):
                    assert R.diff_bits(emu, pl) == 0 and torch.equal(ref, pl.double())
    print(f"crop_resize: fp32 emulation, worst err / bound {worst:.3f}")


def _dcls_cases():
    for route in R.BWD_ROUTES:
        for B2 in R.EMBED_BWD_B2:
            for D in R.EMBED_BWD_D:
                for keep in R.EMBED_BWD_KEEP:
                    yield route, B2, D, keep


def _dmask_cases():
    for route in R.BWD_ROUTES:
        for B2 in R.UNSH_B2:
            for L, Dd in R.UNSH_LD:
                for keep in R.unsh_keeps(L):
                    yield route, B2, L, Dd, keep


def test_sum_emulations_meet_the_counted_bounds():
    worst = {}
    for route, B2, D, keep in _dcls_cases():
        if keep != R.EMBED_BWD_KEEP[-1] or route[1] == BF and route[0] == F32:
            continue
        dx, prior = R.embed_bwd_inputs(B2, keep, D, route[0])
        dtok, dcls, bound = R.embed_bwd_ref(dx, prior, route[1])
        for order in (0, 1):
            etok, ecls = R.embed_bwd_emu(dx, prior, route[1], order)
            assert R.diff_bits(etok, dtok) == 0
            r = R.ratio(ecls, dcls, bound)
            worst["dcls", order] = max(worst.get(("dcls", order), 0.0), r)
            assert r <= 1.0, (B2, D, r)
    for route, B2, L, Dd, keep in _dmask_cases():
        if route[1] == BF and route[0] == F32:
            continue
        z, mt, dpos, ids_restore, dxd, prior = R.unsh_inputs(B2, L, keep, Dd)
        dxd = dxd.to(route[0])
        dz, dm, bound = R.unshuffle_bwd_ref(dxd, ids_restore, keep, prior, route[1])
        assert not bool(torch.isnan(dz.float()).any()), "the reference writes every dz element"
        for order in (0, 1):
            em = R.unshuffle_bwd_emu(dxd, ids_restore, keep, prior, order)
            if keep == L:
                assert R.diff_bits(em, prior) == 0
            r = R.ratio(em, dm, bound)
            worst["dmask_token", order] = max(worst.get(("dmask_token", order), 0.0), r)
            assert r <= 1.0, (B2, L, Dd, keep, r)
    print("counted sums: worst err / bound of the fp32 emulations " + ", ".join(f"{k} order {o}: {v:.3f}" for (k, o), v in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------ seeded defects
def _mask_defect(defect):
    for rows in R.MASK_ROWS:
        for L in R.MASK_L:
            for kind in R.MASK_NOISE:
                noise = R.mask_noise(rows, L, kind)
                for keep in R.mask_keeps(L):
                    yield sum(R.diff_bits(a, b) for a, b in zip(R.mask_sort_ref(noise, keep, defect), R.mask_sort_ref(noise, keep)))


def _patch_defect(defect):
    for C, S, p in R.PATCH_GEOMS:
        for N in R.PATCH_N:
            for views in (1, 2):
                for keep in R.patch_keeps((S // p) ** 2):
                    imgs, ids = R.patch_inputs(C, S, p, N, keep, views)
                    for pad in R.PATCH_PADS:
                        for dt in (F32, BF):
                            ld = C * p * p + pad
                            yield R.diff_bits(R.patch_gather_ref(imgs, ids, p, ld, dt, defect), R.patch_gather_ref(imgs, ids, p, ld, dt))


def _embed_defect(defect):
    for D in R.EMBED_D:
        for keep in R.EMBED_KEEP:
            for B2 in R.EMBED_B2:
                i = R.embed_inputs(B2, keep, D)
                yield R.diff_bits(R.embed_assemble_ref(*i, BF, defect), R.embed_assemble_ref(*i, BF))


def _unsh_fwd_defect(defect):
    for _, B2, L, Dd, keep in _dmask_cases():
        z, mt, dpos, ids_restore, _, _ = R.unsh_inputs(B2, L, keep, Dd)
        yield R.diff_bits(R.unshuffle_fwd_ref(z, mt, dpos, ids_restore, F32, defect), R.unshuffle_fwd_ref(z, mt, dpos, ids_restore, F32))


def _embed_bwd_defect(defect):
    for route, B2, D, keep in _dcls_cases():
        if route != (F32, F32):
            continue
        dx, prior = R.embed_bwd_inputs(B2, keep, D, F32)
        dtok, dcls, bound = R.embed_bwd_ref(dx, prior, F32)
        etok, ecls = R.embed_bwd_emu(dx, prior, F32, 0, defect)
        if defect == "drop_grid_tail":
            yield R.diff_bits(etok, dtok)
        else:
            r = R.ratio(ecls, dcls, bound)
            yield r if r > 1.0 else 0


def _unsh_bwd_defect(defect):
    for route, B2, L, Dd, keep in _dmask_cases():
        if route != (F32, F32):
            continue
        _, _, _, ids_restore, dxd, prior = R.unsh_inputs(B2, L, keep, Dd)
        _, dm, bound = R.unshuffle_bwd_ref(dxd, ids_restore, keep, prior, F32)
        em = R.unshuffle_bwd_emu(dxd, ids_restore, keep, prior, 0, defect)
        r = R.ratio(em, dm, bound)
        yield (r if r > 1.0 else 0) if keep < L else R.diff_bits(em, prior)


def _rows_defect(defect):
    for form in R.ROWS_FORMS:
        for rows, D in R.ROWS_CASES2:
            group, gstride, off_a, off_b, nstore = R.rows_view(form, rows)
            a, b, store, _ = R.rows_inputs(rows, D, nstore, F32)
            if defect == "offsets_exchanged":
                want = R.rows_scatter_add2_emu(a, 0.3, off_a, b, -1.0, off_b, store, group, gstride)
                got = R.rows_scatter_add2_emu(a, 0.3, off_a, b, -1.0, off_b, store, group, gstride, defect)
                yield R.one_of(got[0], *want)
                continue
            yield R.diff_bits(R.rows_gather_ref(store, rows, group, gstride, off_b, F32, 8192, defect), R.rows_gather_ref(store, rows, group, gstride, off_b, F32))
            yield R.one_of(R.rows_scatter_add_emu(a, store, 0.3, group, gstride, off_b, 8192, defect)[0], *R.rows_scatter_add_emu(a, store, 0.3, group, gstride, off_b))
    if defect == "drop_grid_tail":
        for N, L, keep, ids_ld in R.IDX_GEOMS:
            x, ids = R.idx_inputs(N, L, keep, ids_ld, 8)
            yield R.diff_bits(R.rows_gather_idx_ref(x, ids, keep, defect), R.rows_gather_idx_ref(x, ids, keep))


def _spec_defect(defect):
    for g in R.SPEC_G:
        bufs = R.spec_inputs(R.SPEC_L[0], g)[0]
        yield sum(int((a != b).sum()) for a, b in zip(R.spec_fixup_emu(bufs, g, defect), R.spec_fixup_emu(bufs, g)))


DEFECTS = [("gh_gw_swapped", _patch_defect), ("pos_without_plus1", _embed_defect), ("view1_reads_img0", _patch_defect), ("pad_not_zeroed", _patch_defect),
           ("tie_reversed", _mask_defect), ("rank_gt_keep", _mask_defect), ("r_le_keep", _unsh_fwd_defect), ("r_le_keep", _unsh_bwd_defect),
           ("drop_last_column_unit", _embed_bwd_defect), ("stale_partials", _unsh_bwd_defect), ("drop_ragged_sample_group", _embed_bwd_defect),
           ("drop_grid_tail", _embed_bwd_defect), ("drop_grid_tail", _rows_defect), ("drop_grid_tail", _spec_defect),
           ("prior_overwritten", _embed_bwd_defect), ("prior_overwritten", _unsh_bwd_defect), ("prior_overwritten", _rows_defect),
           ("offsets_exchanged", _rows_defect), ("g1_rescales", _spec_defect)]


@pytest.mark.parametrize("defect,walk", DEFECTS, ids=[f"{d}-{w.__name__[1:-7]}" for d, w in DEFECTS])
def test_seeded_defect_is_caught(defect, walk):
    found = [v for v in walk(defect) if v]
    assert found, f"{defect}: no geometry tuple shows it"
    print(f"{defect} ({walk.__name__[1:-7]}): caught on {len(found)} tuples, smallest violation {min(found):.4g}")


def test_honest_walks_report_nothing():
    for walk in (_mask_defect, _patch_defect, _embed_defect, _unsh_fwd_defect, _embed_bwd_defect, _unsh_bwd_defect, _rows_defect, _spec_defect):
        assert not any(walk(None)), walk.__name__


# ------------------------------------------------------------------------------------------------ host-side refusals
ERR_ARG, ERR_UNSUPPORTED = -1, -3
PTR = 0x10000      # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused before any launch


@pytest.fixture(scope="module")
def lib():
    import csmae_hip
    assert os.path.exists(csmae_hip.LIB_PATH), "run `make` / __graft_entry__.build() first"
    lib = ctypes.CDLL(csmae_hip.LIB_PATH)
    lib.csmae_last_error.restype = ctypes.c_char_p
    for name, sig in csmae_hip._SIGNATURES.items():
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = ctypes.c_int
    return lib


REFUSALS = [   # (entry point, arguments, status)
    ("csmae_mask_sort", (1, 16385, 4, PTR, PTR, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_mask_sort", (1, 16, 17, PTR, PTR, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_mask_sort", (0, 16, 4, PTR, PTR, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_patch_gather", (0, 4, 2, 2, 3, 30, 16, PTR, PTR, PTR, PTR, 768, None), ERR_ARG),      # S % p != 0
    ("csmae_patch_gather", (0, 4, 2, 2, 3, 32, 16, PTR, PTR, PTR, PTR, 767, None), ERR_ARG),      # ld < P
    ("csmae_patch_gather", (0, 8, 2, 2, 3, 32, 16, PTR, None, PTR, PTR, 768, None), ERR_ARG),     # two views, img1 = NULL
    ("csmae_patch_gather", (0, 4, 0, 2, 3, 32, 16, PTR, PTR, PTR, PTR, 768, None), ERR_ARG),      # keep = 0
    ("csmae_patch_gather", (0, 4, 2, 2, 3, 32, 0, PTR, PTR, PTR, PTR, 768, None), ERR_ARG),       # p = 0: refused, not a division by zero
    ("csmae_patch_gather", (0, 4, 2, 2, 0, 32, 16, PTR, PTR, PTR, PTR, 768, None), ERR_ARG),      # C = 0
    ("csmae_patch_gather", (0, 4, 2, 2, 3, 0, 16, PTR, PTR, PTR, PTR, 768, None), ERR_ARG),       # S = 0
    ("csmae_patch_gather", (7, 4, 2, 2, 3, 32, 16, PTR, PTR, PTR, PTR, 768, None), ERR_UNSUPPORTED),
    ("csmae_embed_assemble", (0, 2, 3, 6, PTR, PTR, PTR, PTR, PTR, None), ERR_ARG),               # D % 4 != 0
    ("csmae_embed_assemble", (7, 2, 3, 8, PTR, PTR, PTR, PTR, PTR, None), ERR_UNSUPPORTED),
    ("csmae_embed_assemble_bwd", (0, 0, 2, 3, 6, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_embed_assemble_bwd", (1, 0, 2, 3, 8, PTR, PTR, PTR, None), ERR_UNSUPPORTED),          # bf16 in, fp32 out
    ("csmae_unshuffle_fwd", (0, 2, 16, 17, 8, PTR, PTR, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_unshuffle_fwd", (0, 2, 16, 4, 6, PTR, PTR, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_unshuffle_fwd", (7, 2, 16, 4, 8, PTR, PTR, PTR, PTR, PTR, None), ERR_UNSUPPORTED),
    ("csmae_unshuffle_bwd", (0, 0, 2, 16, 17, 8, PTR, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_unshuffle_bwd", (0, 0, 2, 16, 4, 6, PTR, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_unshuffle_bwd", (1, 0, 2, 16, 4, 8, PTR, PTR, PTR, PTR, None), ERR_UNSUPPORTED),      # bf16 in, fp32 out
    ("csmae_rows_gather", (0, 4, 6, PTR, 2, 3, 1, PTR, None), ERR_ARG),
    ("csmae_rows_gather", (0, 4, 8, PTR, 0, 3, 1, PTR, None), ERR_ARG),
    ("csmae_rows_gather", (7, 4, 8, PTR, 2, 3, 1, PTR, None), ERR_UNSUPPORTED),
    ("csmae_rows_scatter_add", (0, 4, 6, PTR, 1.0, 2, 3, 1, PTR, None), ERR_ARG),
    ("csmae_rows_scatter_add", (7, 4, 8, PTR, 1.0, 2, 3, 1, PTR, None), ERR_UNSUPPORTED),
    ("csmae_rows_scatter_add2", (0, 4, 8, PTR, 1.0, 5, PTR, 1.0, 5, 2, 3, PTR, None), ERR_ARG),   # off_a == off_b
    ("csmae_rows_scatter_add2", (0, 4, 6, PTR, 1.0, 1, PTR, 1.0, 5, 2, 3, PTR, None), ERR_ARG),
    ("csmae_rows_scatter_add2", (7, 4, 8, PTR, 1.0, 1, PTR, 1.0, 5, 2, 3, PTR, None), ERR_UNSUPPORTED),
    ("csmae_rows_gather_idx", (2, 16, 17, 8, PTR, PTR, 17, PTR, None), ERR_ARG),                  # keep > L
    ("csmae_rows_gather_idx", (2, 16, 4, 8, PTR, PTR, 3, PTR, None), ERR_ARG),                    # ids_ld < keep
    ("csmae_spec_fixup", (PTR, PTR, 12, PTR, 8, PTR, 8, PTR, PTR, PTR, PTR, 4, None), ERR_ARG),   # n % 8 != 0
    ("csmae_spec_fixup", (PTR, PTR, 8, PTR + 8, 8, PTR, 8, PTR, PTR, PTR, PTR, 4, None), ERR_ARG),   # a misaligned tensor
    ("csmae_spec_fixup", (PTR, PTR, 8, PTR, 8, PTR, 8, PTR, PTR, PTR, PTR, 0, None), ERR_ARG),
    ("csmae_crop_resize", (1, 1025, PTR, PTR, PTR, None), ERR_ARG),
    ("csmae_crop_resize", (0, 64, PTR, PTR, PTR, None), ERR_ARG),
]


@pytest.mark.parametrize("name,args,status", REFUSALS, ids=[f"{n[6:]}-{i}" for i, (n, _, _) in enumerate(REFUSALS)])
def test_host_refuses_bad_arguments_before_any_launch(lib, name, args, status):
    assert getattr(lib, name)(*args) == status
    msg = lib.csmae_last_error().decode()
    assert name in msg, msg
