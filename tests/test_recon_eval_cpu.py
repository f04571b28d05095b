"""CPU self-checks of the reconstruction-evaluation tests and of the host-side pieces of the feature: the float64 reference of recon_eval_ref.py
against the oracle's ssim, its bounds against an fp32 emulation of the kernel with and without seeded defects, util.misc's seed / glob helpers,
util.viz.add_noise, the refusals of util.metrics.batch_metrics and the flags of main_recon_eval.py."""
import os
import random

import numpy as np
import pytest
import torch

import recon_eval_ref as R


def test_float64_ssim_matches_oracle():
    import csmae_oracle as O
    for shape in ((2, 3, 11, 11), (3, 3, 48, 16), (2, 1, 74, 2), (5, 4, 96, 8)):
        o = R.inputs(*shape)
        X, Y, _, _ = R.operands64(o["img"], o["pred"], o["mean"], o["std"], shape[3])
        got = R.ssim_planes(X, Y).mean(1)
        for n in range(shape[0]):
            want = O.ssim(torch.from_numpy(X[n:n + 1]), torch.from_numpy(Y[n:n + 1]), data_range=1).item()
            assert abs(got[n] - want) <= 1e-12, (shape, n, got[n], want)


def test_patchify_roundtrip_follows_the_element_definition():
    N, C, S, p = 2, 3, 12, 4
    planes = np.arange(N * C * S * S, dtype=np.float64).reshape(N, C, S, S)
    rows = R.patchify(planes, p)
    for (n, c, y, x) in ((0, 0, 0, 0), (1, 2, 5, 10), (0, 1, 11, 3)):
        assert rows[n, (y // p) * (S // p) + x // p, ((y % p) * p + x % p) * C + c] == planes[n, c, y, x]
    assert (R.unpatchify(rows, C, S, p) == planes).all()


@pytest.mark.parametrize("shape", [(2, 3, 11, 11), (3, 3, 48, 16), (2, 1, 74, 2), (5, 4, 96, 8)])
def test_honest_emulation_is_inside_the_bounds(shape):
    o = R.inputs(*shape)
    ref = R.reference(o["img"], o["pred"], o["mean"], o["std"], shape[3])
    assert R.violations(R.emulate(o["img"], o["pred"], o["mean"], o["std"], shape[3]).numpy(), ref) == []
    bf = o["pred"].bfloat16()
    ref = R.reference(o["img"], bf.float(), o["mean"], o["std"], shape[3])
    assert R.violations(R.emulate(o["img"], bf, o["mean"], o["std"], shape[3]).numpy(), ref) == []


@pytest.mark.parametrize("defect,shape,expect", [
    ("drop_last_rows", (2, 3, 11, 11), "sse"), ("drop_last_rows", (3, 3, 48, 16), "sae"), ("drop_last_cols", (3, 3, 48, 16), "sse"),
    ("drop_last_cols", (2, 1, 74, 2), "sae"), ("overlap_twice", (3, 3, 48, 16), "sse"), ("overlap_twice", (2, 1, 74, 2), "sae"),
    ("swap_elem_order", (3, 3, 48, 16), "ssim"), ("swap_elem_order", (5, 4, 96, 8), "sse"), ("cls_as_patch0", (3, 3, 48, 16), "ssim"),
    ("cls_as_patch0", (2, 1, 74, 2), "sae")])
def test_bounds_reject_seeded_defects(defect, shape, expect):
    o = R.inputs(*shape)
    ref = R.reference(o["img"], o["pred"], o["mean"], o["std"], shape[3])
    bad = R.violations(R.emulate(o["img"], o["pred"], o["mean"], o["std"], shape[3], defect=defect).numpy(), ref)
    assert expect in bad, (defect, shape, bad)


def test_bounds_reject_unsigned_ssim():
    """Y = 1 - X: the structure term is negative, so a clamped (nonnegative) score is far from the signed one."""
    N, C, S, p = 2, 3, 48, 16
    o = R.inputs(N, C, S, p)
    X, _, _, _ = R.operands64(o["img"], o["pred"], o["mean"], o["std"], p)
    m, s = o["mean"].double().numpy()[None, :, None, None], o["std"].double().numpy()[None, :, None, None]
    pred = torch.from_numpy(R.patchify((1.0 - X - m) / s, p)).float()
    ref = R.reference(o["img"], pred, o["mean"], o["std"], p)
    assert (ref["ssim"] < 0).all()
    assert R.violations(R.emulate(o["img"], pred, o["mean"], o["std"], p).numpy(), ref) == []
    assert "ssim" in R.violations(R.emulate(o["img"], pred, o["mean"], o["std"], p, defect="unsigned_ssim").numpy(), ref)


def test_sum_depth_counts_the_fold():
    assert R.tiles_x(11) == 1 and R.tiles_x(42) == 1 and R.tiles_x(43) == 2 and R.tiles_x(74) == 2 and R.tiles_x(544) == 17
    assert R.sum_depth(3, 128) == 17 + 1 + 6 and R.sum_depth(3, 544) == 17 + 14 + 6


# ------------------------------------------------------------------------------------------------ util.misc
def test_seed_str_to_int():
    from util.misc import seed_str_to_int
    assert seed_str_to_int("") == 0
    assert seed_str_to_int("0-0") == 48 + 45 + 48
    assert seed_str_to_int("12-3") == 49 + 50 + 45 + 51
    assert seed_str_to_int("3-12") == seed_str_to_int("12-3")      # (the reference's seeds collide like this; kept)


def test_glob_helper(tmp_path):
    from util.misc import glob_helper
    for sub, name in (("a", "1.jpg"), ("a", "2.jpg"), ("a/b", "3.jpg"), ("c", "4.jpg"), ("c", "5.png")):
        (tmp_path / sub).mkdir(parents=True, exist_ok=True)
        (tmp_path / sub / name).write_bytes(b"x")
    pattern = f"{tmp_path}/**/*.jpg"
    every = list(glob_helper(pattern))
    assert sorted(os.path.basename(f) for f in every) == ["1.jpg", "2.jpg", "3.jpg", "4.jpg"]
    assert list(glob_helper(pattern, max_samples=2)) == every[:2]
    assert list(glob_helper(pattern, max_samples=9, plot_every=3)) == every       # (foreign keyword arguments are ignored)
    walk = list(glob_helper(pattern, max_samples=3, random_walk=True, walk_seed=5))
    assert len(walk) == 3 and len(set(walk)) == 3 and set(walk) <= set(every)
    assert walk == list(glob_helper(pattern, max_samples=3, random_walk=True, walk_seed=5))
    random.seed(5)
    import glob
    assert walk == random.sample(glob.glob(pattern, recursive=True), 3)
    with pytest.raises(AssertionError, match="max_samples"):
        list(glob_helper(pattern, random_walk=True))
    with pytest.raises(AssertionError, match="walkseed"):
        list(glob_helper(pattern, walk_seed=1))


# ------------------------------------------------------------------------------------------------ util.viz.add_noise
def test_add_noise():
    from util.viz import add_noise
    x = torch.full((3, 16, 16), 0.5)
    g = add_noise(x, "gaussian", 0.25, generator=torch.Generator().manual_seed(3))
    assert g.shape == x.shape and g.dtype == x.dtype and 0.15 < float((g - x).std()) < 0.35
    assert torch.equal(g, add_noise(x, "gaussian", 0.25, generator=torch.Generator().manual_seed(3)))
    assert not torch.equal(g, add_noise(x, "gaussian", 0.25, generator=torch.Generator().manual_seed(4)))
    po = add_noise(x, "poisson", 2.0, generator=torch.Generator().manual_seed(3)) - x
    assert bool((po >= 0).all()) and bool((po == po.round()).all()) and 1.5 < float(po.mean()) < 2.5
    sp = add_noise(x, "s&p", 0.3, generator=torch.Generator().manual_seed(3)) - x
    assert set(sp.unique().tolist()) == {0.0, 1.0} and 0.2 < float(sp.mean()) < 0.4
    arr = add_noise(np.zeros((4, 4, 3)), "gaussian", 0.1)                         # arrays become tensors, as in the reference
    assert isinstance(arr, torch.Tensor) and arr.shape == (4, 4, 3) and arr.dtype == torch.float64
    assert add_noise(x, "s&p", 0.0).equal(x)
    with pytest.raises(ValueError, match="noise type"):
        add_noise(x, "speckle", 0.1)


# ------------------------------------------------------------------------------------------------ util.metrics.batch_metrics
def test_batch_metrics_refusals():
    from util import metrics
    img, pred = torch.zeros(2, 3, 32, 32), torch.zeros(2, 4, 768)
    with pytest.raises(ValueError, match="calc_metric"):
        metrics.batch_metrics(img, pred, 16, ["mse", "ms_ssim"])
    with pytest.raises(ValueError, match="unknown metric"):
        metrics.batch_metrics(img, pred, 16, ["psnr"])
    with pytest.raises(RuntimeError, match="MI355X only") as e:
        metrics.batch_metrics(img, pred, 16, ["ssim"])
    with pytest.raises(RuntimeError, match="MI355X only") as e2:
        metrics.calc_ssim(img, img)
    assert str(e.value) == str(e2.value)


def test_eval_seed_and_synthetic_images():
    from util import viz
    from util.misc import seed_str_to_int
    assert viz.eval_seed(7, 2) == seed_str_to_int("7-2")
    ds = viz.SyntheticEvalImages(3, 32, 2)
    assert len(ds) == 6
    (a, sa), (b, sb), (c, sc) = ds[2], ds[3], ds[4]
    assert a.shape == (3, 32, 32) and a.dtype == torch.float32
    assert torch.equal(a, b) and not torch.equal(a, c) and (sa, sb, sc) == (viz.eval_seed(1, 0), viz.eval_seed(1, 1), viz.eval_seed(2, 0))


# ------------------------------------------------------------------------------------------------ main_recon_eval.py
def test_driver_flags(monkeypatch):
    import main_recon_eval as M
    a = M.get_args_parser().parse_args(["--chkpt_dirs", "A", "B"])
    assert a.chkpt_dirs == ["A", "B"] and a.metrics is None and a.noise is None and not a.random_crop and a.num_runs_each == 5 and a.batch_size == 64
    assert a.dataset_type == "folder" and a.max_samples is None
    a = M.get_args_parser().parse_args(["--chkpt_basedir", "/x", "--chkpt_dirs", "A", "--data_dir", "/d", "--metrics", "ssim", "sad", "--num_runs_each", "2",
                                        "--noise", "gaussian", "0.25", "--random_crop", "--batch_size", "3", "--max_samples", "7", "--output_dir", "/o",
                                        "--dataset_type", "synthetic", "--synthetic_len", "6"])
    assert (a.chkpt_basedir, a.data_dir, a.metrics, a.num_runs_each, a.random_crop, a.batch_size, a.max_samples, a.output_dir, a.dataset_type, a.synthetic_len) == \
        ("/x", "/d", ["ssim", "sad"], 2, True, 3, 7, "/o", "synthetic", 6)
    assert M.parse_noise(a.noise) == ("gaussian", 0.25) and M.parse_noise(None) is None
    with pytest.raises(ValueError, match="--noise"):
        M.parse_noise(["speckle", "1"])
    with pytest.raises(SystemExit):
        M.get_args_parser().parse_args(["--chkpt_dirs", "A", "--metrics", "ms_ssim"])
    with pytest.raises(SystemExit):
        M.get_args_parser().parse_args([])                                          # --chkpt_dirs is required
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one process"):
        M.main(M.get_args_parser().parse_args(["--chkpt_dirs", "A"]))
    mtrs = {"mse": {"A": [1.0, 3.0]}, "ssim": {"A": [0.5, 0.5]}}
    assert M.summarize(mtrs, "A") == {"mse_mean": 2.0, "mse_std": 1.0, "ssim_mean": 0.5, "ssim_std": 0.0}
