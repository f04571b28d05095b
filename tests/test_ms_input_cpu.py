"""CPU-side checks of the multispectral input path: the TIFF reader against a writer of the test's own, the EuroSAT tile list, the band plan,
the packing pair, and the wiring of `--dataset_type euro_sat` into the drivers.  No kernel is launched."""
import os
import re

import numpy as np
import pytest
import torch

import ms_input_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ read_tiff
@pytest.mark.parametrize("form", ["chunky", "planar", "deflate", "deflate_32946", "big_endian", "two_strips", "planar_strips_big"])
def test_read_tiff_round_trips(form, tmp_path):
    from util.tiff import read_tiff
    want = R.tile(1, 9, 7)
    kw = dict(chunky={}, planar=dict(planar=True), deflate=dict(compression=8), deflate_32946=dict(compression=32946), big_endian=dict(order=">"),
              two_strips=dict(rows_per_strip=5), planar_strips_big=dict(planar=True, rows_per_strip=4, order=">", compression=8))[form]
    path = str(tmp_path / f"{form}.tif")
    R.write_tiff(path, want, **kw)
    got = read_tiff(path)
    assert got.dtype == np.uint16 and got.shape == (9, 7, 13) and got.flags["C_CONTIGUOUS"] and (got == want).all()


def test_read_tiff_8_bit_and_pil(tmp_path):
    from PIL import Image

    from util.tiff import read_tiff
    rgb = np.random.default_rng(2).integers(0, 256, size=(6, 11, 3), dtype=np.uint8)
    R.write_tiff(str(tmp_path / "rgb.tif"), rgb, geo=False)
    got = read_tiff(str(tmp_path / "rgb.tif"))
    assert got.dtype == np.uint8 and (got == rgb).all()
    # a 1-band 16-bit file written by PIL against PIL's own read
    one = R.tile(3, 10, 8, 1)[:, :, 0]
    Image.fromarray(one).save(str(tmp_path / "pil.tif"))
    with Image.open(str(tmp_path / "pil.tif")) as im:
        pil = np.asarray(im)
    got = read_tiff(str(tmp_path / "pil.tif"))
    assert got.shape == (10, 8, 1) and (got[:, :, 0] == pil).all() and (pil == one).all()


def test_read_tiff_refusals(tmp_path):
    from util.tiff import read_tiff
    a = R.tile(4, 9, 7)
    cases = [(dict(tiled=True), "322"), (dict(compression=5), r"259\) = 5"), (dict(predictor=2), r"317\) = 2")]
    for k, (kw, word) in enumerate(cases):
        path = str(tmp_path / f"bad{k}.tif")
        R.write_tiff(path, a, **kw)
        with pytest.raises(ValueError, match=word):
            read_tiff(path)
    big = tmp_path / "big.tif"
    big.write_bytes(b"II" + (43).to_bytes(2, "little") + bytes(12))
    with pytest.raises(ValueError, match="43"):
        read_tiff(str(big))
    junk = tmp_path / "junk.tif"
    junk.write_bytes(b"not a tiff at all")
    with pytest.raises(ValueError, match="not a TIFF"):
        read_tiff(str(junk))
    R.write_tiff(str(tmp_path / "f.tif"), a)
    raw = bytearray((tmp_path / "f.tif").read_bytes())
    at = raw.index((339).to_bytes(2, "little") + (3).to_bytes(2, "little"))   # the SampleFormat entry: point it at 13 x 3 (IEEE float)
    off = int.from_bytes(raw[at + 8:at + 12], "little")
    raw[off:off + 26] = (3).to_bytes(2, "little") * 13
    (tmp_path / "f.tif").write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="339"):
        read_tiff(str(tmp_path / "f.tif"))


# ------------------------------------------------------------------------------------------------ EuroSatDataset and packing
def test_eurosat_dataset_and_packing(tmp_path):
    from util.gpu_input import PackedBatch
    from util.ms_input import EuroSatDataset, collate_uint16
    sub = tmp_path / "tiles"
    sub.mkdir()
    tiles = [R.tile(10, 9, 7), R.tile(11, 12, 12), R.tile(12, 8, 10)]
    R.write_tiff(str(sub / "a.tif"), tiles[0])
    np.save(str(sub / "b.npy"), tiles[1])
    R.write_tiff(str(tmp_path / "c.tiff"), tiles[2], planar=True, compression=8)
    R.write_tiff(str(sub / "rgb.tif"), R.tile(13, 5, 5, 3))
    lst = tmp_path / "train.txt"
    lst.write_text(f"tiles/a.tif 3\ntiles/b.npy 0\n{tmp_path / 'c.tiff'} 7\ntiles/rgb.tif 1\n")
    ds = EuroSatDataset(str(lst))
    assert len(ds) == 4
    for i in range(3):
        got, label = ds[i]
        assert got.dtype == torch.uint16 and got.shape == tiles[i].shape and (got.numpy() == tiles[i]).all() and label == (3, 0, 7)[i]
    with pytest.raises(ValueError, match="rgb.tif"):
        ds[3]
    batch, labels = collate_uint16([ds[i] for i in range(3)])
    assert isinstance(batch, PackedBatch) and batch.data.shape == (3, 12, 12, 13) and batch.data.dtype == torch.uint16
    assert batch.sizes.tolist() == [[9, 7], [12, 12], [8, 10]] and labels.tolist() == [3, 0, 7]
    for n, t in enumerate(tiles):
        h, w = t.shape[:2]
        data = batch.data[n].numpy()
        assert (data[:h, :w] == t).all() and int(data[h:].astype(np.int64).sum()) == 0 and int(data[:, w:].astype(np.int64).sum()) == 0
    with pytest.raises(FileNotFoundError):
        EuroSatDataset(str(tmp_path / "nope.txt"))


# ------------------------------------------------------------------------------------------------ band plan
def test_band_plan():
    import argparse

    from util import ms_input as M
    assert M.EUROSAT_MEAN == tuple(R.MEAN) and M.EUROSAT_STD == tuple(R.STD)
    band, mean, inv_std = M.band_plan([10], [0, 9])
    kept = [1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12]
    assert band == [1, 2, 3, 4, 5, 6, 7, 8, 10 | 0x100, 11, 12] and len(band) == 11
    assert mean == [R.MEAN[b] for b in kept] and inv_std == [1.0 / R.STD[b] for b in kept]
    rb, rm, ri = R.plan(masked=[10], dropped=[0, 9])
    assert torch.equal(torch.tensor(band, dtype=torch.int32), rb) and torch.equal(torch.tensor(mean, dtype=torch.float32), rm)
    assert torch.equal(torch.tensor(inv_std, dtype=torch.float32), ri)
    assert M.band_plan(None, None)[0] == list(range(13))
    assert M.eurosat_channels(argparse.Namespace(masked_bands=[10], dropped_bands=[0, 9], input_channels=None)) == 11
    assert M.eurosat_channels(argparse.Namespace(masked_bands=None, dropped_bands=None, input_channels=13)) == 13
    for masked, dropped, word in (([13], None, "masked_bands"), (None, [-1], "dropped_bands"), ([3], [3, 4], "both"), (None, list(range(13)), "all 13")):
        with pytest.raises(ValueError, match=word):
            M.band_plan(masked, dropped)
    with pytest.raises(ValueError, match="input_channels"):
        M.eurosat_channels(argparse.Namespace(masked_bands=None, dropped_bands=[0, 9], input_channels=13))


def test_kernel_limits_match_the_host():
    """The u16 kernels hold as many taps as the u8 kernels and the host check (so eval_transform_params refuses for both), and the row limit of
    util.ms_input is the kernel's."""
    from util import gpu_input, ms_input
    src = open(os.path.join(ROOT, "cross-scale-mae_amd", "csrc", "multispectral.hip")).read()
    assert int(re.search(r"#define MS_MAX_TAPS (\d+)", src).group(1)) == gpu_input.EVAL_MAX_TAPS
    assert int(re.search(r"#define MS_MAX_ROW_FLOATS (\d+)", src).group(1)) == ms_input.MAX_ROW_VALUES
    assert int(re.search(r"#define MS_MAX_BANDS (\d+)", src).group(1)) == ms_input.EUROSAT_BANDS


# ------------------------------------------------------------------------------------------------ wiring
def test_build_loaders_refuses_conflicting_input_channels(tmp_path):
    import main_linprobe
    from util.downstream import build_loaders
    missing = str(tmp_path / "nope.txt")
    a = main_linprobe.get_args_parser().parse_args(["--dataset_type", "euro_sat", "--input_channels", "13", "--dropped_bands", "0", "9", "--train_path", missing,
                                                    "--test_path", missing])
    with pytest.raises(ValueError, match="input_channels"):
        build_loaders(a, torch.device("cpu"))
    a = main_linprobe.get_args_parser().parse_args(["--dataset_type", "euro_sat", "--input_channels", "3", "--train_path", missing, "--test_path", missing])
    with pytest.raises(ValueError, match="input_channels"):
        build_loaders(a, torch.device("cpu"))
    # the other types keep 3 channels when the flag is not given
    a = main_linprobe.get_args_parser().parse_args(["--dataset_type", "rgb", "--train_path", missing, "--test_path", missing])
    with pytest.raises(FileNotFoundError):
        build_loaders(a, torch.device("cpu"))
    assert a.input_channels == 3


@pytest.mark.parametrize("driver", ["main_linprobe", "main_finetune", "main_knn", "main_pretrain"])
def test_drivers_reach_the_eurosat_list(driver, tmp_path, monkeypatch):
    """euro_sat on a missing list file fails at the read of the list, not at a refusal of the dataset type."""
    mod = __import__(driver)
    parse = mod.get_args_parser().parse_args
    missing = str(tmp_path / "nope.txt")
    flags = ["--dataset_type", "euro_sat", "--dropped_bands", "0", "9", "--train_path", missing, "--output_dir", str(tmp_path / "out")]
    if driver == "main_pretrain":
        monkeypatch.delenv("RANK", raising=False)
        monkeypatch.delenv("WORLD_SIZE", raising=False)
        flags += ["--device", "cpu", "--output_dir_base", str(tmp_path)]
    else:
        flags += ["--test_path", missing]
    a = parse(flags)
    with pytest.raises(FileNotFoundError):
        mod.main(a)
    assert a.input_channels == 11
    with pytest.raises(ValueError, match="input_channels"):
        mod.main(parse(flags + ["--input_channels", "13"]))


@pytest.mark.parametrize("driver", ["main_linprobe", "main_knn"])
def test_other_multiband_types_still_raise(driver, tmp_path):
    mod = __import__(driver)
    for kind in ("sentinel", "naip", "smart", "spacenetv1", "resisc45"):
        with pytest.raises(NotImplementedError, match=kind):
            mod.main(mod.get_args_parser().parse_args(["--dataset_type", kind, "--output_dir", str(tmp_path)]))
    import main_pretrain
    for kind in ("naip", "coco"):
        with pytest.raises(NotImplementedError, match=kind):
            main_pretrain.main(main_pretrain.get_args_parser().parse_args(["--dataset_type", kind, "--device", "cpu"]))
