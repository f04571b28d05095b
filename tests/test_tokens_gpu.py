"""csrc/tokens.hip in guarded buffers against the plain references of tests/tokens_ref.py (whose docstring states the contracts): every
operand and output sits between sentinel guards; after each launch the guards are intact, the inputs unchanged, no output element is left
unwritten, and the contract holds per element - bit equality for everything that copies, one of the two fp32 evaluations for dst + src * scale,
a counted bound against fp64 for the two sums and for crop_resize.  Each test prints "exact" or its worst error / bound ratio (-s shows them).
crop_resize's down-sampling branch needs a box larger than the image, which would read outside the plane: no valid call reaches it, so it
is not tested.  Needs an MI355X."""
import functools

import pytest
import torch

import tokens_ref as R
from tokens_ref import BF, F32, I32, I64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from csmae_hip import ops as o
    import csmae_hip
    csmae_hip.load()
    return o


def G(shape, dtype, fill=None):
    return R.Guarded(shape, dtype, fill, "cuda")


def settle(ins, outs, accs=()):
    """After a launch: every guard intact, every input unchanged bit for bit, no output element left unwritten."""
    torch.cuda.synchronize()
    for b in ins:
        assert b.outside_intact() and b.unchanged(), f"an input of shape {b.shape} was written"
    for b in outs:
        assert b.outside_intact(), f"written outside the output of shape {b.shape}"
        assert b.unwritten() == 0, f"{b.unwritten()} elements of the output of shape {b.shape} left unwritten"
    for b in accs:
        assert b.outside_intact(), f"written outside the accumulator of shape {b.shape}"


def exact(got, want, what):
    n = R.diff_bits(got.t.cpu(), want.reshape(got.shape))
    assert n == 0, f"{what}: {n} of {got.n} elements differ from the reference"


def bounded(worst, name, got, want, bound, what):
    r = R.ratio(got.t.cpu(), want, bound)
    worst[name] = max(worst.get(name, 0.0), r)
    assert r <= 1.0, f"{what}: {name} err / bound {r:.3f}"


# ------------------------------------------------------------------------------------------------ mask_sort
@functools.lru_cache(maxsize=None)
def mask_ref(rows, L, kind, keep):
    return R.mask_sort_ref(R.mask_noise(rows, L, kind), keep)


def run_mask_sort(ops, rows, L, kind, keep, shuffle):
    noise = G((rows, L), F32, R.mask_noise(rows, L, kind))
    ids_restore, mask, ids_keep = G((rows, L), I64), G((rows, L), F32), G((rows, keep), I32)
    ids_shuffle = G((rows, L), I32) if shuffle else None
    ops.mask_sort(noise.t, keep, ids_restore.t, mask.t, ids_keep.t, ids_shuffle.t if shuffle else None)
    settle([noise], [ids_restore, mask, ids_keep] + ([ids_shuffle] if shuffle else []))
    want = mask_ref(rows, L, kind, keep)
    what = f"mask_sort rows {rows} L {L} {kind} keep {keep}"
    for b, w, name in zip((ids_restore, mask, ids_keep, ids_shuffle), want, ("ids_restore", "mask", "ids_keep", "ids_shuffle")):
        if b is not None:
            exact(b, w, f"{what} {name}")


@pytest.mark.parametrize("L", R.MASK_L)
def test_mask_sort(ops, L):
    for rows in R.MASK_ROWS:
        for kind in R.MASK_NOISE:
            for keep in R.mask_keeps(L):
                for shuffle in (True, False):
                    run_mask_sort(ops, rows, L, kind, keep, shuffle)
    print(f"mask_sort L {L}: exact")


def test_mask_sort_at_the_accepted_limit(ops):
    """L = 16384: 64 KiB of dynamic LDS, the largest row csmae_mask_sort accepts."""
    run_mask_sort(ops, 2, R.MASK_L_LIMIT, "uniform", R.MASK_L_LIMIT // 4, True)
    print(f"mask_sort L {R.MASK_L_LIMIT}: exact")


# ------------------------------------------------------------------------------------------------ patch_gather
@pytest.mark.parametrize("geom", R.PATCH_GEOMS, ids=lambda g: "C%d-S%d-p%d" % g)
def test_patch_gather(ops, geom):
    C, S, p = geom
    L, P = (S // p) ** 2, C * p * p
    for N in R.PATCH_N:
        for views in (1, 2):
            for keep in R.patch_keeps(L):
                imgs, ids = R.patch_inputs(C, S, p, N, keep, views)
                for pad in R.PATCH_PADS:
                    for dt in (F32, BF):
                        im = [G(i.shape, F32, i) for i in imgs]
                        idb = G(ids.shape, I32, ids)
                        out = G((views * N * keep, P + pad), dt)
                        ops.patch_gather(im[0].t, im[1].t if views == 2 else None, idb.t, out.t, N, C, S, p, keep)
                        settle(im + [idb], [out])
                        exact(out, R.patch_gather_ref(imgs, ids, p, P + pad, dt), f"patch_gather {geom} N {N} views {views} keep {keep} pad {pad} {dt}")
    print(f"patch_gather {geom}: exact")


# ------------------------------------------------------------------------------------------------ embed_assemble
@pytest.mark.parametrize("D", R.EMBED_D)
def test_embed_assemble(ops, D):
    for keep in R.EMBED_KEEP:
        for B2 in R.EMBED_B2:
            tok, pos, cls, ids = R.embed_inputs(B2, keep, D)
            for dt in (F32, BF):
                ins = [G(tok.shape, F32, tok), G(pos.shape, F32, pos), G(cls.shape, F32, cls), G(ids.shape, I32, ids)]
                x = G((B2, keep + 1, D), dt)
                ops.embed_assemble(ins[0].t, ins[1].t, ins[2].t, ins[3].t, x.t, B2, keep)
                settle(ins, [x])
                exact(x, R.embed_assemble_ref(tok, pos, cls, ids, dt), f"embed_assemble D {D} keep {keep} B2 {B2} {dt}")
    print(f"embed_assemble D {D}: exact")


@functools.lru_cache(maxsize=None)
def embed_bwd_ref(B2, keep, D, din, dout):
    return R.embed_bwd_ref(*R.embed_bwd_inputs(B2, keep, D, din), dout)


@pytest.mark.parametrize("B2", R.EMBED_BWD_B2)
def test_embed_assemble_bwd(ops, B2):
    worst = {}
    for din, dout in R.BWD_ROUTES:
        for D in R.EMBED_BWD_D:
            for keep in R.EMBED_BWD_KEEP:
                dx, prior = R.embed_bwd_inputs(B2, keep, D, din)
                dtok, dcls, bound = embed_bwd_ref(B2, keep, D, din, dout)
                dxb, tokb, clsb = G(dx.shape, din, dx), G((B2 * keep, D), dout), G((D,), F32, prior)
                ops.embed_assemble_bwd(dxb.t, tokb.t, clsb.t, B2, keep)
                settle([dxb], [tokb], [clsb])
                what = f"embed_assemble_bwd {din}->{dout} B2 {B2} D {D} keep {keep}"
                exact(tokb, dtok, what + " dtok")
                bounded(worst, "dcls", clsb, dcls, bound, what)
    print(f"embed_assemble_bwd B2 {B2}: dtok exact, dcls worst err / bound {worst['dcls']:.3f}")


# ------------------------------------------------------------------------------------------------ unshuffle
@functools.lru_cache(maxsize=None)
def unsh_bwd_ref(B2, L, keep, Dd, din, dout):
    i = R.unsh_inputs(B2, L, keep, Dd)
    return R.unshuffle_bwd_ref(i[4].to(din), i[3], keep, i[5], dout)


@pytest.mark.parametrize("LD", R.UNSH_LD, ids=lambda g: "L%d-Dd%d" % g)
def test_unshuffle_fwd_bwd(ops, LD):
    L, Dd = LD
    worst = {}
    for B2 in R.UNSH_B2:
        for keep in R.unsh_keeps(L):
            z, mt, dpos, ids_restore, dxd, prior = R.unsh_inputs(B2, L, keep, Dd)
            for dt in (F32, BF):
                ins = [G(z.shape, F32, z), G(mt.shape, F32, mt), G(dpos.shape, F32, dpos), G(ids_restore.shape, I64, ids_restore)]
                xd = G((B2, L + 1, Dd), dt)
                ops.unshuffle_fwd(ins[0].t.reshape(-1, Dd), ins[1].t, ins[2].t, ins[3].t, xd.t, B2, L, keep)
                settle(ins, [xd])
                exact(xd, R.unshuffle_fwd_ref(z, mt, dpos, ids_restore, dt), f"unshuffle_fwd B2 {B2} L {L} keep {keep} Dd {Dd} {dt}")
            for din, dout in R.BWD_ROUTES:
                dz, dm, bound = unsh_bwd_ref(B2, L, keep, Dd, din, dout)
                gb, ib = G(dxd.shape, din, dxd), G(ids_restore.shape, I64, ids_restore)
                dzb, dmb = G((B2 * (keep + 1), Dd), dout), G((Dd,), F32, prior)
                ops.unshuffle_bwd(gb.t, ib.t, dzb.t, dmb.t, B2, L, keep)
                settle([gb, ib], [dzb], [dmb])
                what = f"unshuffle_bwd {din}->{dout} B2 {B2} L {L} keep {keep} Dd {Dd}"
                exact(dzb, dz, what + " dz")
                if keep == L:
                    exact(dmb, prior, what + " dmask_token keeps its content")
                bounded(worst, "dmask_token", dmb, dm, bound, what)
    print(f"unshuffle L {L} Dd {Dd}: xd, dz exact, dmask_token worst err / bound {worst['dmask_token']:.3f}")


# ------------------------------------------------------------------------------------------------ row views
@pytest.mark.parametrize("form", R.ROWS_FORMS)
def test_rows_gather_and_scatter_add(ops, form):
    for rows, D in R.ROWS_CASES:
        group, gstride, _, off, nstore = R.rows_view(form, rows)
        for dt in (F32, BF):
            src, _, store, _ = R.rows_inputs(rows, D, nstore, dt)
            sb, out = G(store.shape, F32, store), G((rows, D), dt)
            ops.rows_gather(sb.t, out.t, group, gstride, off)
            settle([sb], [out])
            exact(out, R.rows_gather_ref(store, rows, group, gstride, off, dt), f"rows_gather {form} rows {rows} D {D} {dt}")
            for scale in R.SCALES:
                srcb, dst = G(src.shape, dt, src), G(store.shape, F32, store)
                ops.rows_scatter_add(srcb.t, dst.t, group, gstride, off, scale=scale)
                settle([srcb], [], [dst])
                n = R.one_of(dst.t.cpu(), *R.rows_scatter_add_emu(src, store, scale, group, gstride, off))
                assert n == 0, f"rows_scatter_add {form} rows {rows} D {D} {dt} scale {scale}: {n} elements are neither fl(dst + fl(src scale)) nor the fma"
    print(f"rows_gather, rows_scatter_add {form}: exact")


@pytest.mark.parametrize("form", R.ROWS_FORMS)
def test_rows_scatter_add2(ops, form):
    for rows, D in R.ROWS_CASES2:
        group, gstride, off_a, off_b, nstore = R.rows_view(form, rows)
        for dt in (F32, BF):
            a, b, store, _ = R.rows_inputs(rows, D, nstore, dt)
            for k, sa in enumerate(R.SCALES):
                sb = R.SCALES[(k + 1) % len(R.SCALES)]
                ab, bb, dst = G(a.shape, dt, a), G(b.shape, dt, b), G(store.shape, F32, store)
                ops.rows_scatter_add2(ab.t, sa, off_a, bb.t, sb, off_b, dst.t, group, gstride)
                settle([ab, bb], [], [dst])
                n = R.one_of(dst.t.cpu(), *R.rows_scatter_add2_emu(a, sa, off_a, b, sb, off_b, store, group, gstride))
                assert n == 0, f"rows_scatter_add2 {form} rows {rows} D {D} {dt} scales {sa}, {sb}: {n} elements are neither evaluation"
    print(f"rows_scatter_add2 {form}: exact")


@pytest.mark.parametrize("D", R.IDX_D)
def test_rows_gather_idx(ops, D):
    for N, L, keep, ids_ld in R.IDX_GEOMS:
        x, ids = R.idx_inputs(N, L, keep, ids_ld, D)
        xb, ib, out = G(x.shape, F32, x), G(ids.shape, I32, ids), G((N, keep, D), F32)
        ops.rows_gather_idx(xb.t, ib.t, keep, out.t)
        settle([xb, ib], [out])
        exact(out, R.rows_gather_idx_ref(x, ids, keep), f"rows_gather_idx D {D} N {N} keep {keep}")
    print(f"rows_gather_idx D {D}: exact")


# ------------------------------------------------------------------------------------------------ spec_fixup
@pytest.mark.parametrize("g", R.SPEC_G)
def test_spec_fixup(ops, g):
    for k, L in enumerate(R.SPEC_L):
        bufs, tmp, dg, db = R.spec_inputs(L, g)
        bufs = bufs[k % 3:] + bufs[:k % 3]                       # every tensor slot meets every size
        gb, tb = G((1,), F32, torch.tensor([g])), G(tmp.shape, F32, tmp)
        bb = [G(b.shape, BF, b) for b in bufs]
        dgb, dbb = G(dg.shape, F32, dg), G(db.shape, F32, db)
        ops.spec_fixup(gb.t, [b.t for b in bb], tb.t, dgb.t, dbb.t)
        settle([gb, tb], [], bb + [dgb, dbb])
        for b, want in zip(bb, R.spec_fixup_emu(bufs, g)):
            n = int((b.bits().cpu() != want).sum())
            assert n == 0, f"spec_fixup g {g} L {L}: {n} of {b.n} elements of a tensor differ"
        for b, prior, t in ((dgb, dg, tmp[0]), (dbb, db, tmp[1])):
            n = R.one_of(b.t.cpu(), *R.axpy_both(prior, t, g))
            assert n == 0, f"spec_fixup g {g} L {L}: {n} dgamma / dbeta elements are neither evaluation"
    print(f"spec_fixup g {g}: exact")


# ------------------------------------------------------------------------------------------------ crop_resize
@functools.lru_cache(maxsize=None)
def crop_ref(planes, S, box):
    return R.crop_ref64(R.crop_planes(planes, S), box)


@pytest.mark.parametrize("S", R.CROP_S)
def test_crop_resize(ops, S):
    worst = {}
    for planes in R.CROP_PLANES:
        pl = R.crop_planes(planes, S)
        for box in R.crop_boxes(S):
            src, bx, dst = G(pl.shape, F32, pl), G((4,), I32, torch.tensor(box, dtype=torch.int32)), G(pl.shape, F32)
            ops.crop_resize(src.t, dst.t, bx.t)
            settle([src, bx], [dst])
            if box == (0, 0, S, S):
                exact(dst, pl, f"crop_resize S {S} planes {planes}: the full image is the identity")
            ref, bound = crop_ref(planes, S, box)
            bounded(worst, "out", dst, ref, bound, f"crop_resize S {S} planes {planes} box {box}")
    print(f"crop_resize S {S}: identity exact, worst err / bound {worst['out']:.3f}")
