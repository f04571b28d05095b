"""GPU tests of the reconstruction contact sheets (csrc/recon_panel.hip, util.viz.reconstruction_panels, util.recon_plot.plot_reconstruction, run_eval's panel_dir)
against the float64 reference and the decided / borderline rule of recon_panel_ref.py, in guarded buffers."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import recon_eval_ref as R
import recon_panel_ref as P
from gemm_bounds import U16

pytestmark = pytest.mark.gpu
MICRO = dict(dim_model=128, encoder_num_layers=2, encoder_num_heads=2, decoder_embed_dim=64, decoder_num_layers=2, decoder_num_heads=2)
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
def reference(case):
    o = P.case_inputs(case)
    return P.reference(o["img"], o["pred"], o["mask"], o["mean"], o["std"], case[0][3], case[1], case[2], o["bands"])


def device_pred(pred, strided):
    """The prediction on the GPU in its own dtype: dense, or a view with a cls row in front of each image's rows and 5 more columns, both NaN."""
    if not strided:
        return pred.cuda()
    N, L, Pn = pred.shape
    buf = torch.full((N, L + 1, Pn + 5), NAN, device="cuda", dtype=pred.dtype)
    buf[:, 1:, :Pn] = pred.cuda()
    return buf[:, 1:, :Pn]


def run_guarded(ops, o, pred, p, panels, gap, bands):
    """ops.recon_panel with `out` inside a sentinel-guarded buffer whose payload starts 8 bytes behind a 16-byte boundary (4-aligned, not 16-aligned),
    run twice over payloads prefilled with 0xA5 and with 0x5A: a byte the kernel leaves unwritten differs between the two.  -> uint8 [N, S, W, 3] numpy."""
    N, C, S, _ = o["img"].shape
    W = P.sheet_width(S, len(panels), gap)
    img, mask, mean, std = o["img"].cuda(), o["mask"].cuda(), o["mean"].cuda(), o["std"].cuda()
    got = []
    for fill in (0xA5, 0x5A):
        g = R.Guarded(1, N * S * W * 3, torch.uint8, off8=True, fill=fill)
        assert g.vec.data_ptr() % 16 == 8
        out = ops.recon_panel(img, pred, mask, mean, std, p, panels=panels, gap=gap, bands=bands, out=g.vec.view(N, S, W, 3))
        torch.cuda.synchronize()
        assert out.data_ptr() == g.vec.data_ptr()
        assert g.outside_intact(), "recon_panel wrote outside out"
        got.append(g.vec.view(N, S, W, 3).cpu().numpy().copy())
    assert (got[0] == got[1]).all(), f"{int((got[0] != got[1]).sum())} bytes of out were left unwritten"
    return got[0]


# ------------------------------------------------------------------------------------------------ the kernel against float64
@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_kernel_vs_float64(ops, case):
    shape, panels, gap, bf16, strided = case
    o, ref = P.case_inputs(case), reference(case)
    assert P.borderline_share(ref) <= P.BORDERLINE_CAP
    got = run_guarded(ops, o, device_pred(o["pred"], strided), shape[3], panels, gap, o["bands"])
    print(f"recon_panel {P.case_id(case)}: borderline share {P.borderline_share(ref):.2e}, borderline bytes that differ {P.differing_borderline_share(got, ref):.2e}")
    assert (got[ref["gap"]] == 255).all(), "a gap byte is not 255"
    assert P.violations(got, ref) == []


def test_default_bands_and_panels(ops):
    """bands=None is (0, 1, 2), or (0, 0, 0) for one channel; the defaults of ops.recon_panel are panels (0, 1, 2) and gap 2."""
    for case in (P.CASES[0], P.CASES[7]):
        o, p = P.case_inputs(case), case[0][3]
        img, mask, mean, std = o["img"].cuda(), o["mask"].cuda(), o["mean"].cuda(), o["std"].cuda()
        a = ops.recon_panel(img, o["pred"].cuda(), mask, mean, std, p)
        b = ops.recon_panel(img, o["pred"].cuda(), mask, mean, std, p, panels=(0, 1, 2), gap=2, bands=o["bands"])
        assert a.dtype == torch.uint8 and a.shape == (case[0][0], case[0][2], 3 * case[0][2] + 4, 3) and torch.equal(a, b)


def test_batch_independence(ops):
    case = P.CASES[11]   # (5, 3, 42, 7), panels (2, 2), gap 3: a sheet of 10962 bytes, so the images start at every alignment
    o, p = P.case_inputs(case), case[0][3]
    whole = run_guarded(ops, o, o["pred"].cuda(), p, case[1], case[2], o["bands"])
    for n in range(5):
        one = dict(o, img=o["img"][n:n + 1].contiguous(), mask=o["mask"][n:n + 1].contiguous())
        assert (run_guarded(ops, one, o["pred"][n:n + 1].contiguous().cuda(), p, case[1], case[2], o["bands"])[0] == whole[n]).all(), n
    rev = dict(o, img=o["img"].flip(0).contiguous(), mask=o["mask"].flip(0).contiguous())
    assert (run_guarded(ops, rev, o["pred"].flip(0).contiguous().cuda(), p, case[1], case[2], o["bands"])[::-1] == whole).all()


def test_nonfinite_inputs_are_defined(ops):
    """NaN, +inf, -inf planted in whole patches of the prediction give 0 / 255 / 0 in the y panel there and change no other byte; the x panel, which
    does not show the prediction, does not change at all."""
    case = P.CASES[8]    # (2, 4, 32, 8), bands (3, 1, 0): 16 patches per image
    N, C, S, p = case[0]
    o = P.case_inputs(case)
    panels, gap = (0, 2), 3
    clean = run_guarded(ops, o, o["pred"].cuda(), p, panels, gap, o["bands"])
    pred = o["pred"].clone()
    planted = {(0, 5): (NAN, 0), (1, 0): (float("inf"), 255), (1, 15): (float("-inf"), 0)}
    for (n, l), (v, _) in planted.items():
        pred[n, l] = v
    got = run_guarded(ops, o, pred.cuda(), p, panels, gap, o["bands"])
    G, x0 = S // p, S + gap
    touched = np.zeros(got.shape, dtype=bool)
    for (n, l), (_, byte) in planted.items():
        gh, gw = divmod(l, G)
        sl = (n, slice(gh * p, gh * p + p), slice(x0 + gw * p, x0 + gw * p + p))
        assert (got[sl] == byte).all(), ((n, l), got[sl])
        touched[sl] = True
    assert (got[~touched] == clean[~touched]).all()
    # a NaN mask value (any non-finite operand) still gives a defined byte in the panels that use the mask
    bad = dict(o, mask=o["mask"].clone())
    bad["mask"][0, 3] = NAN
    got = run_guarded(ops, bad, o["pred"].cuda(), p, (1, 4), gap, o["bands"])
    assert (got[0, 0:p, 3 * p:4 * p] == 0).all() and (got[0, 0:p, x0 + 3 * p:x0 + 4 * p] == 0).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    import csmae_hip
    lib = csmae_hip.load()
    C, S, p = 3, 32, 16
    L, Pn = (S // p) ** 2, p * p * C
    img = torch.zeros(1, C, S, S, device="cuda")
    pred = torch.zeros(1, L, Pn, device="cuda")
    mask, mean, std = torch.zeros(1, L, device="cuda"), torch.zeros(C).cuda(), torch.ones(C).cuda()
    g = R.Guarded(1, S * (3 * S + 4) * 3, torch.uint8, off8=True)
    base = dict(dt=csmae_hip.F32, N=1, C=C, S=S, p=p, img=img.data_ptr(), pred=pred.data_ptr(), ldp=Pn, stride=L * Pn, mask=mask.data_ptr(), mean=mean.data_ptr(),
                std=std.data_ptr(), br=0, bg=1, bb=2, c0=0, c1=1, c2=2, c3=0, c4=0, K=3, gap=2, out=g.vec.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return lib.csmae_recon_panel(a["dt"], a["N"], a["C"], a["S"], a["p"], a["img"], a["pred"], a["ldp"], a["stride"], a["mask"], a["mean"], a["std"], a["br"], a["bg"],
                                     a["bb"], a["c0"], a["c1"], a["c2"], a["c3"], a["c4"], a["K"], a["gap"], a["out"], ops.stream())

    refused = [(dict(img=None), "null"), (dict(pred=None), "null"), (dict(mask=None), "null"), (dict(mean=None), "null"), (dict(std=None), "null"), (dict(out=None), "null"),
               (dict(N=0), "N"), (dict(N=-1), "N"), (dict(p=12), "does not tile"), (dict(ldp=Pn - 1), "ldp"), (dict(N=2, stride=L * Pn - 1), "img_stride"),
               (dict(dt=5), "fp32 or bf16"), (dict(br=3), "band_r"), (dict(bg=-1), "band_g"), (dict(bb=C), "band_b"), (dict(K=0), "n_panels"), (dict(K=6), "n_panels"),
               (dict(c1=5), "panel1"), (dict(c2=-1), "panel2"), (dict(gap=-1), "gap"), (dict(S=1 << 15, K=1), "2^31 bytes"),
               (dict(N=1 << 40, stride=1 << 40), "grid")]
    for kw, word in refused:
        assert call(**kw) != 0, kw
        assert word in lib.csmae_last_error().decode(), (kw, lib.csmae_last_error().decode())
    assert call(c3=9, c4=-3) == 0          # codes behind n_panels are not read
    torch.cuda.synchronize()
    assert g.outside_intact() and g.unwritten() < g.n
    g2 = R.Guarded(1, S * (3 * S + 4) * 3, torch.uint8, off8=True)
    for kw, _ in refused:
        if "out" not in kw:
            assert call(out=g2.vec.data_ptr(), **kw) != 0
    torch.cuda.synchronize()
    assert g2.untouched(), "a refused call wrote to out"
    with pytest.raises(csmae_hip.CsmaeError, match="fp32 or bf16"):
        ops.recon_panel(img, pred.half(), mask, mean, std, p)
    with pytest.raises(csmae_hip.CsmaeError, match="panel0"):
        ops.recon_panel(img, pred, mask, mean, std, p, panels=(7,))


# ------------------------------------------------------------------------------------------------ util.viz
def micro_model(seed):
    import models_mae
    torch.manual_seed(seed)
    return models_mae.MAE_ViT_Baseline(**MICRO, input_size=64, patch_size="16", mask_ratio=0.75).cuda().eval()


def synthetic_images(n, size=64, runs=1):
    from util import viz
    ds = viz.SyntheticEvalImages(n, size, runs)
    return torch.stack([ds[k * runs][0] for k in range(n)])


def check_rule(got, v255, delta, what):
    """Decided / borderline as recon_panel_ref states it, on one panel: got uint8, v255 and delta float64 of the same shape."""
    tobyte = lambda t: np.floor(np.clip(t, 0.0, 255.0))   # noqa: E731
    lo, hi = tobyte(v255 - delta), tobyte(v255 + delta)
    print(f"{what}: {int((hi != lo).sum())} of {lo.size} bytes borderline, {int((got != tobyte(v255)).sum())} differ from the float64 byte")
    assert ((got >= lo) & (got <= hi)).all(), (what, int(((got < lo) | (got > hi)).sum()))


def test_reconstruction_panels_and_plot(ops, tmp_path):
    from PIL import Image
    from util import recon_plot, viz
    model, other = micro_model(1), micro_model(2)
    S, gap = 64, 2
    imgs = synthetic_images(3)
    seeds = [viz.eval_seed(i, 0) for i in range(3)]
    sheets = viz.reconstruction_panels(model, imgs.cuda(), seeds)
    assert sheets.is_cuda and sheets.dtype == torch.uint8 and sheets.shape == (3, S, viz.sheet_width(S, 3, gap), 3)
    got = sheets.cpu().numpy()
    assert (got[:, :, S:S + gap] == 255).all() and (got[:, :, 2 * S + gap:2 * S + 2 * gap] == 255).all()
    # ... against run_one_image's arrays converted by plot_image's rule.  x and xm: float64 arithmetic on the same fp32 input, so the kernel's own
    # delta (recon_panel_ref).  y: the single-image forward may round its bf16 prediction differently at batch size 1, so delta is widened by the
    # bf16 spacing of the prediction — 2 u16 |pred| std in image space, 2^-8 relative each way — times 255.
    for n in range(3):
        hwc = imgs[n].permute(1, 2, 0).double().numpy()
        x, xm, y, ym, pasted = (t[0].numpy() for t in viz.run_one_image(hwc, model, mask_seed=seeds[n]))
        a = np.abs(hwc * viz.image_std)
        stats = R.U32 * (a + viz.image_mean)     # the kernel reads the statistics rounded to fp32, run_one_image keeps them in float64
        d_x = 255.0 * (R.U32 * (a + np.abs(x)) + stats) + R.U32 * 255.0 * np.abs(x) * (1 + 4 * R.U32)
        check_rule(got[n, :, :S], 255.0 * x, d_x, ("x", n))
        check_rule(got[n, :, S + gap:2 * S + gap], 255.0 * xm, d_x, ("xm", n))
        b = np.abs(y - viz.image_mean)
        d_y = 255.0 * (R.U32 * (b + np.abs(y)) + R.U32 * (b + viz.image_mean) + 2 * U16 * b) + R.U32 * 255.0 * np.abs(y) * (1 + 4 * U16)
        check_rule(got[n, :, 2 * S + 2 * gap:], 255.0 * y, d_y, ("y", n))
    # a forward already made gives the same sheets, other panels and all
    pred, mask = viz.masked_forward(model, imgs.cuda(), seeds)
    assert torch.equal(viz.reconstruction_panels(model, imgs.cuda(), None, pred=pred, mask=mask), sheets)
    five = viz.reconstruction_panels(model, imgs.cuda(), seeds, panels=("xm_ym", "ym", "y", "xm", "x"), gap=0)
    assert five.shape == (3, S, 5 * S, 3) and torch.equal(five[:, :, 4 * S:], sheets[:, :, :S]) and torch.equal(five[:, :, 2 * S:3 * S], sheets[:, :, 2 * S + 2 * gap:])

    # plot_reconstruction: rows in dict order with a white gap between them; the PNG and the JSON
    models = {"first": model, "second": other}
    hwc = imgs[1].permute(1, 2, 0).double().numpy()
    sheet = recon_plot.plot_reconstruction(models, hwc, image_name="img 1", title="micro", savedir=str(tmp_path), save=True, mask_seed=seeds[1], captions=False)
    W = viz.sheet_width(S, 3, gap)
    assert sheet.dtype == np.uint8 and sheet.shape == (2 * S + gap, W, 3)
    first = viz.reconstruction_panels(model, imgs[1:2].cuda(), [seeds[1]])[0].cpu().numpy()      # (a batch of one, as plot_reconstruction runs it)
    second = viz.reconstruction_panels(other, imgs[1:2].cuda(), [seeds[1]])[0].cpu().numpy()
    assert (sheet[:S] == first).all() and (sheet[S:S + gap] == 255).all()
    assert (sheet[S + gap:] == second).all() and not (second == first).all()
    png = tmp_path / "micro" / "plot_img_micro_img_1.png"
    assert (np.asarray(Image.open(png).convert("RGB")) == sheet).all()
    meta = json.load(open(tmp_path / "micro" / "plot_img_micro_img_1.json"))
    assert meta["models"] == ["first", "second"] and meta["panels"] == ["x", "xm", "y"]
    from util import metrics
    want = float(metrics.batch_metrics(imgs[1:2].cuda(), viz.masked_forward(model, imgs[1:2].cuda(), [seeds[1]])[0], 16, ["ssim"])["ssim"][0])
    assert meta["scores"]["first"] == want
    cap = recon_plot.plot_reconstruction(models, hwc, mask_seed=seeds[1])
    assert cap.shape == (2 * (S + recon_plot.CAPTION_HEIGHT) + gap, W, 3) and (cap[recon_plot.CAPTION_HEIGHT:recon_plot.CAPTION_HEIGHT + S] == first).all()


def test_run_eval_writes_sheets(ops, tmp_path):
    from PIL import Image
    from util import viz
    models = {"first": micro_model(1), "second": micro_model(2)}
    runs = 2

    def images(size):
        return viz.SyntheticEvalImages(3, size, runs)
    kw = dict(use_noise=("gaussian", 0.1), num_runs_each=runs, batch_size=4, num_workers=0, images=images)
    plain = viz.run_eval(models, None, **kw)
    out = tmp_path / "panels"
    mtrs = viz.run_eval(models, None, panel_dir=str(out), panel_every=2, **kw)
    assert mtrs == plain
    assert sorted(os.listdir(out)) == ["img_000000.png", "img_000002.png"]
    S, gap = 64, 2
    sheet = np.asarray(Image.open(out / "img_000000.png").convert("RGB"))
    assert sheet.shape == (2 * S + gap, viz.sheet_width(S, 3, gap), 3)
    # image 0's row of the first batch as run_eval forms it (items 0 .. 3: both runs of images 0 and 1), under eval_seed(0, 0) and its noise
    ds = images(S)
    seeds = [ds[k][1] for k in range(4)]
    assert seeds[0] == viz.eval_seed(0, 0)
    batch = viz.eval_noise(torch.stack([ds[k][0] for k in range(4)]).cuda(), seeds, kw["use_noise"])
    for r, model in enumerate(models.values()):
        want = viz.reconstruction_panels(model, batch, seeds)[0].cpu().numpy()
        assert (sheet[r * (S + gap):r * (S + gap) + S] == want).all(), r
    assert (sheet[S:S + gap] == 255).all()
    every = viz.run_eval(models["first"], None, panel_dir=str(tmp_path / "all"), panels=("y",), **kw)
    assert sorted(os.listdir(tmp_path / "all")) == ["img_000000.png", "img_000001.png", "img_000002.png"] and every["ssim"]["model"] == plain["ssim"]["first"]
    assert np.asarray(Image.open(tmp_path / "all" / "img_000001.png")).shape == (S, S, 3)


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_writes_sheets(ops, tmp_path):
    import argparse

    from PIL import Image

    import main_recon_eval as M
    from util import misc
    kw = dict(MICRO, input_size=64, patch_size="16", mask_ratio=0.75)
    for seed, name in ((1, "run_a"), (2, "run_b")):
        m = micro_model(seed)
        args = argparse.Namespace(model="MAE_ViT_Baseline", output_dir=str(tmp_path / name), device="cuda", **kw)
        os.makedirs(args.output_dir)
        misc.save_model(args, 3, m, m, torch.optim.SGD(m.parameters(), lr=0.1), None)
    out = tmp_path / "eval"
    M.main(M.get_args_parser().parse_args(["--chkpt_basedir", str(tmp_path), "--chkpt_dirs", "run_a", "run_b", "--dataset_type", "synthetic", "--synthetic_len", "4",
                                           "--num_runs_each", "2", "--batch_size", "3", "--num_workers", "0", "--output_dir", str(out), "--panel_dir", str(out / "panels"),
                                           "--panels", "x", "xm", "xm_ym"]))
    assert sorted(os.listdir(out / "panels")) == [f"img_{i:06d}.png" for i in range(4)]
    for i in range(4):
        assert np.asarray(Image.open(out / "panels" / f"img_{i:06d}.png")).shape == (2 * 64 + 2, 3 * 64 + 4, 3)      # one row per checkpoint
    lines = [json.loads(ln) for ln in open(out / "log.txt").read().splitlines()]
    assert [ln.get("model") for ln in lines] == ["run_a", "run_b", None]
    assert lines[2] == dict(panel_dir=str(out / "panels"), panel_every=1, panels=["x", "xm", "xm_ym"], sheets=4)
    rows = open(out / "per_image.csv").read().splitlines()
    assert len(rows) == 1 + 2 * 4
