"""The multispectral input kernels (`csmae_augment_u16` / `csmae_eval_u16`, csrc/multispectral.hip) and the loader around them (util/ms_input.py)
against the float64 chain of tests/ms_input_ref.py, in NaN-prefilled buffers with guard elements before and behind the output.

Tolerance, per image and band: |out - oracle| <= 1e-5 * max(1, max |oracle|) over the band's plane.  It follows from the arithmetic, not from a
measurement: the kernel makes a few dozen fp32 roundings (weights, two fma chains, the normalisation) on values no larger than the plane's
largest, 6e-8 relative each; the bound leaves about a tenfold margin."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ms_input_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64
MASKED, DROPPED = (10,), (0, 9)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import csmae_hip
    from csmae_hip import ops as o
    csmae_hip.load()
    return o


def pack(tiles):
    from util.ms_input import pack_uint16
    return pack_uint16([torch.from_numpy(np.array(t)) for t in tiles]).data


def run_guarded(ops, train, tiles, metas, S, masked=(), dropped=(), data=None):
    """The kernel on a padded batch, its output inside a NaN-prefilled buffer with NaN guards: every element written, every guard intact."""
    band, mean, inv_std = R.plan(masked, dropped)
    N, Cout = len(tiles), band.numel()
    n = N * Cout * S * S
    buf = torch.full((GUARD + n + GUARD,), NAN, device="cuda")
    out = buf[GUARD:GUARD + n].view(N, Cout, S, S)
    src = (pack(tiles) if data is None else data).cuda()
    (ops.augment_u16 if train else ops.eval_u16)(src, torch.tensor(metas, dtype=torch.int32).cuda(), band, mean.cuda(), inv_std.cuda(), out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "a guard element was written"
    assert not bool(torch.isnan(out).any()), "an output element was left unwritten"
    return out.cpu()


def check(out, oracles, what):
    worst = 0.0
    for n, ora in enumerate(oracles):
        assert out[n].shape == ora.shape
        for k in range(ora.shape[0]):
            err = float((out[n, k].double() - ora[k]).abs().max())
            bound = 1e-5 * max(1.0, float(ora[k].abs().max()))
            worst = max(worst, err / bound)
            assert err <= bound, (what, n, k, err, bound)
    print(f"{what}: worst error / bound = {worst:.3f}")


@functools.lru_cache(maxsize=None)
def tile(seed, H, W):
    t = R.tile(seed, H, W)
    t.setflags(write=False)
    return t


def test_identity_pins_band_order_and_normalisation(ops):
    tiles = [tile(20 + n, 8, 8) for n in range(3)]
    band, mean, inv_std = R.plan()
    for train, meta in ((True, (8, 8, 0, 0, 8, 8, 0, 0)), (False, (8, 8, 8, 8, 0, 0, 0, 0))):
        out = run_guarded(ops, train, tiles, [meta] * 3, 8)
        for n, t in enumerate(tiles):
            want = (torch.from_numpy(t.astype(np.float32)).permute(2, 0, 1) - mean[:, None, None]) * inv_std[:, None, None]   # fp32 throughout
            ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -23
            assert bool(((out[n] - want).abs() <= 2 * ulp).all()), (train, n, float(((out[n] - want).abs() / ulp).max()))


def test_upscale_and_flips(ops):
    tiles = [tile(30, 9, 7), tile(31, 12, 12), tile(32, 12, 12)]
    S = 16
    for flips, metas in enumerate([
            [(9, 7, 0, 0, 5, 4, 0, 0), (12, 12, 7, 6, 5, 6, 1, 0), (12, 12, 0, 3, 12, 9, 0, 1)],      # boxes at the top-left, bottom-right, full height
            [(9, 7, 2, 0, 7, 7, 1, 1), (12, 12, 0, 0, 12, 12, 1, 1), (12, 12, 4, 0, 3, 12, 1, 0)]]):   # bottom edge + full width, the whole tile, left + right edge
        out = run_guarded(ops, True, tiles, metas, S)
        check(out, [R.oracle_train(t, m, S) for t, m in zip(tiles, metas)], f"upscale {flips}")


def test_downscale_and_the_tap_limit(ops):
    from util.gpu_input import EVAL_MAX_TAPS, eval_transform_params
    t = tile(40, 40, 33)
    tiles = [t, t, t]
    metas = [(40, 33, 0, 0, 40, 33, 0, 0), (40, 33, 0, 0, 40, 33, 1, 0), (40, 33, 3, 2, 36, 30, 0, 1)]
    for S in (16, 2):     # 2.5 and 20 source pixels per output pixel: 11 and up to 40 taps (the whole box)
        check(run_guarded(ops, True, tiles, metas, S), [R.oracle_train(t, m, S) for m in metas], f"train downscale S={S}")
    for S in (16, 2):     # S = 2 resizes 40 -> 2 rows: 4 * 40 // 2 + 1 = 81 taps, the most this tile can ask for within the limit
        meta = eval_transform_params(40, 33, S)
        check(run_guarded(ops, False, tiles, [meta] * 3, S), [R.oracle_eval(t, meta, S)] * 3, f"eval downscale S={S}")
    assert 4 * 40 // 2 + 1 <= EVAL_MAX_TAPS < 4 * 40 // 1 + 1
    with pytest.raises(ValueError, match="taps"):     # one step further (40 -> 1 row, 161 taps) is refused on the host, as for u8
        eval_transform_params(40, 33, 1)
    # ... and the limit itself: 95 rows -> 4 is exactly EVAL_MAX_TAPS taps
    tall = tile(41, 95, 5)
    assert 4 * 95 // 4 + 1 == EVAL_MAX_TAPS
    meta = (95, 5, 4, 4, 0, 0, 0, 0)
    check(run_guarded(ops, False, [tall] * 3, [meta] * 3, 4), [R.oracle_eval(tall, meta, 4)] * 3, "eval 96 taps")


def test_masked_and_dropped_bands(ops):
    tiles = [tile(50, 9, 7), tile(51, 12, 12), tile(52, 12, 12)]
    S = 16
    metas = [(9, 7, 1, 1, 7, 5, 1, 0), (12, 12, 0, 0, 12, 12, 0, 1), (12, 12, 2, 3, 8, 9, 0, 0)]
    poisoned = pack(tiles).clone()
    pv = poisoned.view(torch.int16)
    for b in DROPPED:
        pv[..., b] = -1          # 65535 in every source value of a dropped band
    kept = [b for b in range(13) if b not in DROPPED]
    for train, ms in ((True, metas), (False, None)):
        if not train:
            from util.gpu_input import eval_transform_params
            ms = [eval_transform_params(t.shape[0], t.shape[1], S) for t in tiles]
        out = run_guarded(ops, train, tiles, ms, S, MASKED, DROPPED, data=poisoned)
        k = kept.index(MASKED[0])
        assert bool((out[:, k] == 0.0).all()), "the masked channel is not exactly 0"
        oracle = (R.oracle_train if train else R.oracle_eval)
        oras = [oracle(t, m, S, MASKED, DROPPED) for t, m in zip(tiles, ms)]
        assert all(bool((o[k] == 0.0).all()) for o in oras)
        check(out, oras, f"bands train={train}")
        clean = run_guarded(ops, train, tiles, ms, S, MASKED, DROPPED)
        assert torch.equal(clean, out), "a dropped band's values reached the output"


@pytest.mark.parametrize("S,sizes", [(16, [(20, 14), (14, 20), (20, 20)]), (64, [(64, 64)] * 3)])
def test_eval_geometry(ops, S, sizes):
    from util.gpu_input import eval_transform_params
    tiles = [tile(60 + n, h, w) for n, (h, w) in enumerate(sizes)]
    metas = [eval_transform_params(h, w, S) for h, w in sizes]
    if S == 64:
        assert metas[0] == (64, 64, 73, 73, 4, 4, 0, 0)
    else:
        assert metas[0][2:4] == (25, 18) and metas[1][2:4] == (18, 25)    # both branches of the shorter-side rule
    check(run_guarded(ops, False, tiles, metas, S), [R.oracle_eval(t, m, S) for t, m in zip(tiles, metas)], f"eval S={S}")


def test_argument_checks(ops):
    import csmae_hip
    lib = csmae_hip.load()
    S = 8
    src = torch.zeros(1, 8, 8, 13, dtype=torch.uint16).cuda()
    meta = torch.tensor([(8, 8, 0, 0, 8, 8, 0, 0)], dtype=torch.int32).cuda()
    band, mean, inv_std = R.plan()
    mean, inv_std = mean.cuda(), inv_std.cuda()
    buf = torch.full((GUARD + 13 * S * S + GUARD,), NAN, device="cuda")
    out = buf[GUARD:GUARD + 13 * S * S]

    for fn in (lib.csmae_augment_u16, lib.csmae_eval_u16):
        def call(Cin=13, Cout=13, band=band, Wmax=8, fn=fn):
            return fn(1, Cin, Cout, 8, Wmax, S, src.data_ptr(), meta.data_ptr(), band.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), out.data_ptr(), ops.stream())
        bad = band.clone()
        bad[4] = 13
        flagged = band.clone()
        flagged[4] = 0x200 | 4
        for kw, word in ((dict(Cout=0), "band counts"), (dict(Cin=14, Cout=13), "band counts"), (dict(Cin=5, Cout=6), "band counts"), (dict(band=bad), "band[4]"),
                         (dict(Cin=12, Cout=13), "band counts"), (dict(band=flagged), "band[4]"), (dict(Wmax=1000), "does not fit")):
            assert call(**kw) != 0, kw
            assert word in lib.csmae_last_error().decode(), (kw, lib.csmae_last_error().decode())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote to dst"
    bad = band.clone()
    bad[12] = 13
    for op in (ops.augment_u16, ops.eval_u16):
        with pytest.raises(csmae_hip.CsmaeError, match=r"band\[12\]"):
            op(src, meta, bad, mean, inv_std, out.view(1, 13, S, S))
        with pytest.raises(csmae_hip.CsmaeError, match="band counts"):
            op(torch.zeros(1, 8, 4, 14, dtype=torch.uint16).cuda(), meta, band, mean, inv_std, out.view(1, 13, S, S))
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------------------------------------ through the loader and a driver
def write_tiles(folder, sizes, labels, seed=70):
    tiles = [R.tile(seed + n, h, w) for n, (h, w) in enumerate(sizes)]
    for n, t in enumerate(tiles):
        R.write_tiff(str(folder / f"t{n}.tif"), t, planar=bool(n % 2), compression=8 if n % 3 == 0 else 1)
    (folder / "list.txt").write_text("".join(f"t{n}.tif {lab}\n" for n, lab in enumerate(labels)))
    return tiles, str(folder / "list.txt")


def test_through_the_loader(ops, tmp_path):
    import argparse

    from util.gpu_input import eval_transform_params, sample_transform_params
    from util.ms_input import build_eurosat_loader
    sizes, labels = [(9, 7), (12, 12), (16, 11), (10, 10), (8, 13)], [4, 0, 2, 2, 1]
    tiles, lst = write_tiles(tmp_path, sizes, labels)
    S = 8
    args = argparse.Namespace(batch_size=2, input_size=S, num_workers=0, masked_bands=list(MASKED), dropped_bands=list(DROPPED))
    loader = build_eurosat_loader(lst, False, args, torch.device("cuda"))
    assert len(loader.dataset) == 5 and len(loader) == 3 and loader.augment.in_chans == 11
    got, seen = [], []
    for x, y in loader:
        assert x.is_cuda and x.dtype == torch.float32 and x.shape[1:] == (11, S, S)
        got.append(x.cpu().clone())
        seen += y.tolist()
    assert [g.shape[0] for g in got] == [2, 2, 1] and seen == labels
    check(torch.cat(got), [R.oracle_eval(t, eval_transform_params(t.shape[0], t.shape[1], S), S, MASKED, DROPPED) for t in tiles], "loader eval")

    # training: the draws of a seeded run, replayed on the host in the order the loader makes them (sampler first, then batch by batch)
    class Index(torch.utils.data.Dataset):
        def __len__(self):
            return 5

        def __getitem__(self, i):
            return i

    for seed in (0, 1):
        torch.manual_seed(seed)
        order, params = [], []
        replay = torch.utils.data.DataLoader(Index(), sampler=torch.utils.data.RandomSampler(Index()), batch_size=2, num_workers=0, drop_last=True, collate_fn=list)
        for idx in replay:
            order += idx
            params += [sample_transform_params(*sizes[i]) for i in idx]
        loader = build_eurosat_loader(lst, True, args, torch.device("cuda"))
        torch.manual_seed(seed)
        got, seen = [], []
        for x, y in loader:
            got.append(x.cpu().clone())
            seen += y.tolist()
        assert len(order) == 4 and seen == [labels[i] for i in order]
        check(torch.cat(got), [R.oracle_train(tiles[i], p, S, MASKED, DROPPED) for i, p in zip(order, params)], f"loader train seed {seed}")


def test_through_main_linprobe(ops, tmp_path):
    import main_linprobe
    tiles, lst = write_tiles(tmp_path, [(64, 64)] * 8, [0, 1] * 4, seed=90)
    out = tmp_path / "out"
    main_linprobe.main(main_linprobe.get_args_parser().parse_args(
        ["--dataset_type", "euro_sat", "--dropped_bands", "0", "9", "--train_path", lst, "--test_path", lst, "--nb_classes", "2", "--embed_dim", "64", "--depth", "2",
         "--num_heads", "2", "--input_size", "32", "--batch_size", "4", "--epochs", "1", "--num_workers", "0", "--output_dir", str(out),
         "--device", "cuda:0"]))
    lines = [json.loads(ln) for ln in open(os.path.join(out, "log.jsonl")).read().splitlines()]
    assert len(lines) == 1 and np.isfinite(lines[0]["test_acc1"]) and np.isfinite(lines[0]["train_loss"]) and 0.0 <= lines[0]["test_acc1"] <= 100.0
