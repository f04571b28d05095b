"""GPU tests of the batched reconstruction evaluation (csrc/recon_eval.hip, util.metrics.batch_metrics, util.viz.run_eval, main_recon_eval.py)
against the float64 references and bounds of recon_eval_ref.py, in guarded buffers."""
import argparse
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import recon_eval_ref as R
from gemm_bounds import U32

pytestmark = pytest.mark.gpu
MICRO = dict(dim_model=128, encoder_num_layers=2, encoder_num_heads=2, decoder_embed_dim=64, decoder_num_layers=2, decoder_num_heads=2)
NAMES = ["mse", "mae", "l1", "l2", "ssim"]
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import csmae_hip
    from csmae_hip import ops as o
    csmae_hip.load()
    return o


@functools.lru_cache(maxsize=None)
def reference(shape, bf16):
    o = R.inputs(*shape)
    pred = o["pred"].bfloat16().float() if bf16 else o["pred"]
    return R.reference(o["img"], pred, o["mean"], o["std"], shape[3])


def device_pred(pred, layout):
    """The prediction on the GPU: contiguous fp32; a view with a cls row in front of each image's rows and 8 pad columns, both NaN; or bf16."""
    if layout == "fp32":
        return pred.cuda()
    if layout == "bf16":
        return pred.bfloat16().cuda()
    N, L, P = pred.shape
    buf = torch.full((N, L + 1, P + 8), NAN, device="cuda")
    buf[:, 1:, :P] = pred.cuda()
    return buf[:, 1:, :P]


def run_guarded(ops, img, pred, mean, std, p):
    """ops.recon_eval with `out` and the workspace inside sentinel-guarded buffers -> [N, 4] on the CPU (the guards are checked here)."""
    N, C, S, _ = img.shape
    floats = ops.recon_eval_workspace_floats(N, C, S)
    assert floats == N * C * R.tiles_x(S) ** 2 * 3
    gout, gws = R.Guarded(N, 4, torch.float32), R.Guarded(1, floats, torch.float32)
    got = ops.recon_eval(img, pred, mean, std, p, out=gout.t, ws=gws.vec)
    torch.cuda.synchronize()
    assert got.data_ptr() == gout.t.data_ptr()
    assert gout.outside_intact() and gws.outside_intact(), "recon_eval wrote outside out / the workspace"
    assert gout.unwritten() == 0 and gws.unwritten() == 0, "recon_eval left part of out / the workspace unwritten"
    return gout.t.cpu()


# ------------------------------------------------------------------------------------------------ the kernel against float64
@pytest.mark.parametrize("layout", ["fp32", "strided", "bf16"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_float64(ops, shape, layout):
    N, C, S, p = shape
    o = R.inputs(*shape)
    ref = reference(shape, layout == "bf16")
    img, mean, std = o["img"].cuda(), o["mean"].cuda(), o["std"].cuda()
    got = run_guarded(ops, img, device_pred(o["pred"], layout), mean, std, p).double().numpy()
    err = np.abs(got[:, :3] - np.stack([ref["sse"], ref["sae"], ref["ssim"]], 1))
    print(f"recon_eval {shape} {layout}: sse err/bound {float((err[:, 0] / ref['b_sse']).max()):.3f}  sae err/bound {float((err[:, 1] / ref['b_sae']).max()):.3f}  "
          f"worst ssim err {float(err[:, 2].max()):.3e}")
    if layout == "fp32":   # the parent's kernel on the same inputs, image by image (recorded in recon_eval_ref.py, not asserted here)
        from util import metrics
        X, Y, _, _ = R.operands64(o["img"], o["pred"], o["mean"], o["std"], p)
        worst = max(abs(metrics.calc_ssim(torch.from_numpy(X[n:n + 1]).float().cuda(), torch.from_numpy(Y[n:n + 1]).float().cuda(), num_channels=C) - ref["ssim"][n])
                    for n in range(N))
        print(f"calc_ssim {shape}: worst ssim err {worst:.3e}")
    assert R.violations(got, ref) == []


# ------------------------------------------------------------------------------------------------ pixel ownership
@pytest.mark.parametrize("S,p", [(42, 7), (48, 16), (74, 2), (128, 16)])
def test_every_pixel_is_counted_once(ops, S, p):
    """Y = X except one pixel: sse = d^2 and sae = |d| exactly (d = 0.25, mean 0, std 1, X on a 2^-10 grid so that X + d is exact)."""
    C = 3
    X = (torch.rand(1, C, S, S, generator=torch.Generator().manual_seed(S)) * 1024).floor() / 1024
    mean, std = torch.zeros(C).cuda(), torch.ones(C).cuda()
    for (y, x) in ((0, 0), (S - 1, S - 1), (31, 32), (S - 11, S - 10), (S - 1, 0)):
        for c in (0, C - 1):
            Y = X.clone()
            Y[0, c, y, x] += 0.25
            pred = torch.from_numpy(R.patchify(Y.numpy(), p))
            got = run_guarded(ops, X.cuda(), pred.cuda(), mean, std, p)
            assert got[0, 0].item() == 0.0625 and got[0, 1].item() == 0.25 and got[0, 3].item() == 0.0, ((y, x, c), got)


# ------------------------------------------------------------------------------------------------ identities
def test_identities(ops):
    shape = (3, 3, 48, 16)
    o = R.inputs(*shape)
    img, mean, std = o["img"].cuda(), o["mean"].cuda(), o["std"].cuda()
    same = torch.from_numpy(R.patchify(o["img"].numpy(), 16)).cuda()
    got = run_guarded(ops, img, same, mean, std, 16)
    assert bool((got[:, 0] == 0).all()) and bool((got[:, 1] == 0).all()) and bool(((got[:, 2] - 1).abs() <= R.SSIM_ATOL).all()), got
    X, _, _, _ = R.operands64(o["img"], o["pred"], o["mean"], o["std"], 16)
    m, s = o["mean"].double().numpy()[None, :, None, None], o["std"].double().numpy()[None, :, None, None]
    inv = torch.from_numpy(R.patchify((1.0 - X - m) / s, 16)).float()
    got = run_guarded(ops, img, inv.cuda(), mean, std, 16)
    assert bool((got[:, 2] < 0).all()), got
    assert R.violations(got.double().numpy(), R.reference(o["img"], inv, o["mean"], o["std"], 16)) == []


def test_rows_do_not_depend_on_the_batch(ops):
    shape = (5, 4, 96, 8)
    o = R.inputs(*shape)
    img, pred, mean, std = o["img"].cuda(), o["pred"].cuda(), o["mean"].cuda(), o["std"].cuda()
    bits = lambda t: t.contiguous().view(torch.int32)   # noqa: E731
    whole = bits(run_guarded(ops, img, pred, mean, std, 8))
    for n in range(5):
        assert torch.equal(bits(run_guarded(ops, img[n:n + 1].contiguous(), pred[n:n + 1].contiguous(), mean, std, 8))[0], whole[n]), n
    rev = bits(run_guarded(ops, img.flip(0).contiguous(), pred.flip(0).contiguous(), mean, std, 8))
    assert torch.equal(rev.flip(0), whole)


def test_mean_agrees_with_calc_metric(ops):
    """Both kernels may be 1e-4 from the oracle, so their gap can reach twice that."""
    from util import metrics
    shape = (4, 3, 128, 16)
    o = R.inputs(*shape)
    got = ops.recon_eval(o["img"].cuda(), o["pred"].cuda(), o["mean"].cuda(), o["std"].cuda(), 16)
    X, Y, _, _ = R.operands64(o["img"], o["pred"], o["mean"], o["std"], 16)
    parent = metrics.calc_metric(torch.from_numpy(X).float().cuda(), torch.from_numpy(Y).float().cuda(), "ssim")
    assert abs(float(got[:, 2].double().mean()) - parent) <= 2e-4, (got[:, 2], parent)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("S,p,dtype,match", [(10, 5, torch.float32, "11-tap"), (12, 5, torch.float32, "does not tile"), (16, 8, torch.int8, "fp32 or bf16")])
def test_refusals_launch_nothing(ops, S, p, dtype, match):
    import csmae_hip
    C = 3
    img = torch.zeros(1, C, S, S, device="cuda")
    pred = torch.zeros(1, (S // p) ** 2, p * p * C, device="cuda", dtype=dtype)
    mean, std = torch.zeros(C).cuda(), torch.ones(C).cuda()
    gout, gws = R.Guarded(1, 4, torch.float32), R.Guarded(1, 64, torch.float32)
    with pytest.raises(csmae_hip.CsmaeError, match=match):
        ops.recon_eval(img, pred, mean, std, p, out=gout.t, ws=gws.vec)
    lib = csmae_hip.load()
    rc = lib.csmae_recon_eval(csmae_hip.F32 if dtype == torch.float32 else 5, 1, C, S, p, img.data_ptr(), pred.data_ptr(), p * p * C, (S // p) ** 2 * p * p * C,
                              mean.data_ptr(), std.data_ptr(), gws.vec.data_ptr(), gout.t.data_ptr(), ops.stream())
    assert rc != 0 and match in lib.csmae_last_error().decode()
    assert lib.csmae_recon_eval(csmae_hip.F32, 1, 0, 32, 16, img.data_ptr(), pred.data_ptr(), 768, 3072, mean.data_ptr(), std.data_ptr(), gws.vec.data_ptr(),
                                gout.t.data_ptr(), ops.stream()) != 0            # C < 1
    assert lib.csmae_recon_eval(csmae_hip.F32, 1, 3, 32, 16, img.data_ptr(), pred.data_ptr(), 768, 3072, None, std.data_ptr(), gws.vec.data_ptr(),
                                gout.t.data_ptr(), ops.stream()) != 0            # a null pointer
    n = ctypes.c_longlong(-1)
    assert lib.csmae_recon_eval_workspace_floats(1, C, 10, ctypes.byref(n)) != 0 and n.value == -1
    torch.cuda.synchronize()
    assert gout.untouched() and gws.untouched()


# ------------------------------------------------------------------------------------------------ util.metrics.batch_metrics
def test_batch_metrics(ops):
    from util import metrics
    shape = (3, 3, 48, 16)
    N, C, S, p = shape
    o = R.inputs(*shape)
    ref = reference(shape, False)
    names = NAMES + ["ssd", "sad"]
    got = metrics.batch_metrics(o["img"].cuda(), o["pred"].cuda(), p, names, mean=o["mean"].numpy(), std=o["std"].numpy())
    assert list(got) == names
    for v in got.values():
        assert v.is_cuda and v.dtype == torch.float32 and v.shape == (N,)
    g = {k: v.double().cpu().numpy() for k, v in got.items()}
    cnt = C * S * S
    assert (np.abs(g["l2"] - ref["sse"]) <= ref["b_sse"]).all() and (np.abs(g["l1"] - ref["sae"]) <= ref["b_sae"]).all()
    assert (np.abs(g["mse"] - ref["sse"] / cnt) <= ref["b_sse"] / cnt + U32 * ref["sse"] / cnt).all()     # (one more rounding: the division)
    assert (np.abs(g["mae"] - ref["sae"] / cnt) <= ref["b_sae"] / cnt + U32 * ref["sae"] / cnt).all()
    assert (np.abs(g["ssim"] - ref["ssim"]) <= R.SSIM_ATOL).all()
    assert (g["ssd"] == g["l2"]).all() and (g["sad"] == g["l1"]).all()
    one = metrics.batch_metrics(o["img"].cuda(), o["pred"].cuda(), p, "ssim", mean=o["mean"].cuda(), std=o["std"].cuda())
    assert list(one) == ["ssim"] and torch.equal(one["ssim"], got["ssim"])
    with pytest.raises(ValueError, match="calc_metric"):
        metrics.batch_metrics(o["img"].cuda(), o["pred"].cuda(), p, ["ms_ssim"])


# ------------------------------------------------------------------------------------------------ util.viz.run_eval end to end
def micro_model(seed):
    import models_mae
    torch.manual_seed(seed)
    return models_mae.MAE_ViT_Baseline(**MICRO, input_size=64, patch_size="16", mask_ratio=0.75).cuda().eval()


def write_jpegs(folder, n):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(11)
    yy, xx = np.meshgrid(np.arange(40), np.arange(52), indexing="ij")
    for i in range(n):
        a = np.stack([127 + 90 * np.sin(0.1 * (i + 1) * yy + 0.07 * (c + 1) * xx + i) + 20 * rng.standard_normal((40, 52)) for c in range(3)], -1)
        Image.fromarray(a.clip(0, 255).astype(np.uint8)).save(os.path.join(folder, f"img_{i}.jpg"), quality=95)


@pytest.mark.parametrize("use_noise,random_crop", [(None, False), (("gaussian", 0.25), True)])
def test_run_eval_end_to_end(ops, tmp_path, use_noise, random_crop):
    from util import viz
    from util.misc import glob_helper
    write_jpegs(str(tmp_path / "data" / "sub"), 5)
    models = {"first": micro_model(1), "second": micro_model(2)}
    runs, bs = 2, 3
    kw = dict(use_noise=use_noise, num_runs_each=runs, batch_size=bs, random_crop=random_crop, num_workers=0)
    mtrs = viz.run_eval(models, str(tmp_path / "data"), **kw)
    assert list(mtrs) == NAMES
    for name in NAMES:
        assert list(mtrs[name]) == ["first", "second"]
        for v in mtrs[name].values():
            assert len(v) == 5 and all(isinstance(f, float) for f in v)
    assert mtrs == viz.run_eval(models, str(tmp_path / "data"), do_plot_metrics_comp=False, **kw)       # identical floats; plot arguments are ignored
    one = viz.run_eval(models["first"], str(tmp_path / "data"), comp_metrics="ssim", max_samples=2, **kw)
    assert list(one) == ["ssim"] and list(one["ssim"]) == ["model"] and len(one["ssim"]["model"]) == 2     # (other batches: not compared with the run above)

    # the same batches again, scored by the float64 reference
    paths = list(glob_helper(f"{tmp_path}/data/**/*.jpg"))
    ds = viz.EvalImages(paths, 64, runs, random_crop=random_crop)
    items = [ds[k] for k in range(len(ds))]
    assert [s for _, s in items] == [viz.eval_seed(i, r) for i in range(5) for r in range(runs)]
    mean, std = R.channel_stats(3)
    for model_name, model in models.items():
        want = {k: [] for k in ("sse", "sae", "ssim", "b_sse", "b_sae")}
        for b0 in range(0, len(items), bs):
            imgs = torch.stack([x for x, _ in items[b0:b0 + bs]])
            seeds = [s for _, s in items[b0:b0 + bs]]
            dev_imgs = viz.eval_noise(imgs.cuda(), seeds, use_noise)
            if use_noise is not None:
                assert not torch.equal(dev_imgs.cpu(), imgs) and torch.equal(dev_imgs, viz.eval_noise(imgs.cuda(), seeds, use_noise))
            noise, box = viz.mask_draws(model, seeds, dev_imgs.device)
            with torch.no_grad():
                _, pred, mask = model._run(dev_imgs, model.mask_ratio, noise, box)[:3]
                for j, s in enumerate(seeds):                                         # the batched mask of a row is the seeded batch-1 mask
                    assert torch.equal(mask[j], model(dev_imgs[j:j + 1], mask_ratio=model.mask_ratio, mask_seed=s)[2][0]), (b0, j)
            ref = R.reference(dev_imgs.cpu(), pred.float().cpu(), mean, std, 16)
            for k in want:
                want[k].append(ref[k])
        w = {k: np.concatenate(v).reshape(5, runs).mean(1) for k, v in want.items()}
        cnt = 3 * 64 * 64
        g = {k: np.asarray(mtrs[k][model_name]) for k in NAMES}
        assert (np.abs(g["l2"] - w["sse"]) <= w["b_sse"]).all() and (np.abs(g["l1"] - w["sae"]) <= w["b_sae"]).all(), model_name
        assert (np.abs(g["mse"] - w["sse"] / cnt) <= (w["b_sse"] + U32 * w["sse"]) / cnt).all(), model_name
        assert (np.abs(g["mae"] - w["sae"] / cnt) <= (w["b_sae"] + U32 * w["sae"]) / cnt).all(), model_name
        assert (np.abs(g["ssim"] - w["ssim"]) <= R.SSIM_ATOL).all(), model_name
    assert mtrs["ssim"]["first"] != mtrs["ssim"]["second"]


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_on_synthetic_images(ops, tmp_path):
    import main_recon_eval as M
    from util import misc
    kw = dict(MICRO, input_size=64, patch_size="16", mask_ratio=0.75)
    for seed, name in ((1, "run_a"), (2, "run_b")):
        m = micro_model(seed)
        args = argparse.Namespace(model="MAE_ViT_Baseline", output_dir=str(tmp_path / name), device="cuda", **kw)
        os.makedirs(args.output_dir)
        misc.save_model(args, 3, m, m, torch.optim.SGD(m.parameters(), lr=0.1), None)
    out = tmp_path / "eval"
    M.main(M.get_args_parser().parse_args(["--chkpt_basedir", str(tmp_path), "--chkpt_dirs", "run_a", "run_b", "--dataset_type", "synthetic", "--synthetic_len", "6",
                                           "--num_runs_each", "2", "--batch_size", "4", "--num_workers", "0", "--output_dir", str(out), "--noise", "s&p", "0.05"]))
    lines = [json.loads(ln) for ln in open(out / "log.txt").read().splitlines()]
    assert [ln["model"] for ln in lines] == ["run_a", "run_b"]
    for ln in lines:
        assert ln["n_images"] == 6 and ln["num_runs_each"] == 2 and ln["noise"] == ["s&p", 0.05]
        for name in NAMES:
            assert np.isfinite(ln[f"{name}_mean"]) and ln[f"{name}_std"] >= 0
        assert -1.0 <= ln["ssim_mean"] <= 1.0 and ln["mse_mean"] > 0
    rows = open(out / "per_image.csv").read().splitlines()
    assert rows[0] == "model,image," + ",".join(NAMES)
    assert [r.split(",")[0] for r in rows[1:]] == ["run_a"] * 6 + ["run_b"] * 6 and [int(r.split(",")[1]) for r in rows[1:]] == list(range(6)) * 2
    assert abs(np.mean([float(r.split(",")[-1]) for r in rows[1:7]]) - lines[0]["ssim_mean"]) < 1e-12
