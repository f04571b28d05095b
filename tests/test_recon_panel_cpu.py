"""CPU self-checks of the contact-sheet tests and of the host-side pieces of the feature: the float64 reference of recon_panel_ref.py against a literal
restatement of util.viz.run_one_image + the reference's plot_image conversion, its decided / borderline rule against an fp32 emulation of the kernel
with and without seeded defects, the cap on borderline bytes for every case, the binding, the driver's flags, run_eval's new keywords and
plot_reconstruction's path rule on a stub model."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import recon_eval_ref as R
import recon_panel_ref as P


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(case):
        if case not in cache:
            o = P.case_inputs(case)
            cache[case] = P.reference(o["img"], o["pred"], o["mask"], o["mean"], o["std"], case[0][3], case[1], case[2], o["bands"])
        return cache[case]
    return get


def test_reference_restates_run_one_image():
    """The five arrays as util.viz.run_one_image builds them ([1, H, W, C], float64, the mask repeated over a patch's elements and un-patchified) and
    plot_image's torch.clip(image * 255, 0, 255).int(), on a tiny case; mean / std are the plot statistics."""
    N, C, S, p = 2, 3, 8, 4
    o = R.inputs(N, C, S, p)
    mask = P.masks(N, (S // p) ** 2)
    mean, std = o["mean"].double(), o["std"].double()
    ref = P.reference(o["img"], o["pred"], mask, o["mean"], o["std"], p, (0, 1, 2, 3, 4), 1, (0, 1, 2))
    for n in range(N):
        x = o["img"][n:n + 1].double().permute(0, 2, 3, 1)
        y = torch.from_numpy(R.unpatchify(o["pred"][n:n + 1].double().numpy(), C, S, p)).permute(0, 2, 3, 1)
        mk = mask[n:n + 1].double().unsqueeze(-1).repeat(1, 1, p * p * C)
        mk = torch.from_numpy(R.unpatchify(mk.numpy(), C, S, p)).permute(0, 2, 3, 1)
        x, y = x * std + mean, y * std + mean
        xm, ym = x * (1 - mk), y * mk
        for k, arr in enumerate((x, xm, y, ym, xm + ym)):
            want = torch.clip(arr * 255, 0, 255).int()[0].numpy()
            got = ref["byte"][n, :, k * (S + 1):k * (S + 1) + S]
            assert (got == want).all(), (n, k)
            assert np.abs(ref["v255"][n, :, k * (S + 1):k * (S + 1) + S] - (arr * 255)[0].numpy()).max() < 1e-12
    assert ref["gap"][:, :, S].all() and (ref["byte"][ref["gap"]] == 255).all() and not ref["borderline"][ref["gap"]].any()
    assert ref["byte"].shape == (N, S, 5 * S + 4, 3)


def test_cases_cover_every_axis_twice():
    for axis, values in ((1, (P.P1, P.P3, P.P5, P.P2)), (2, (0, 3)), (3, (False, True)), (4, (False, True))):
        for v in values:
            assert len({c[0] for c in P.CASES if c[axis] == v}) >= 2, (axis, v)
    assert {c[0] for c in P.CASES} == set(P.SHAPES)


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_borderline_cap_and_honest_emulation(refs, case):
    o, ref = P.case_inputs(case), refs(case)
    share = P.borderline_share(ref)
    assert share <= P.BORDERLINE_CAP, (P.case_id(case), share)
    got = P.emulate(o["img"], o["pred"], o["mask"], o["mean"], o["std"], case[0][3], case[1], case[2], o["bands"])
    assert P.violations(got, ref) == []
    S, K, gap = case[0][2], len(case[1]), case[2]
    assert got.shape == (case[0][0], S, K * S + (K - 1) * gap, 3) and P.sheet_width(S, K, gap) == got.shape[2]


@pytest.mark.parametrize("defect,case,expect", [
    ("round_nearest", P.CASES[0], "decided"), ("round_nearest", P.CASES[14], "decided"),
    ("mask_inverted", P.CASES[1], "decided"), ("mask_inverted", P.CASES[10], "decided"),
    ("bgr", P.CASES[2], "decided"), ("bgr", P.CASES[9], "decided"),
    ("bands_ignored", P.CASES[8], "decided"), ("bands_ignored", P.CASES[9], "decided"),
    ("gap_short", P.CASES[3], "gap"), ("gap_short", P.CASES[11], "decided"),
    ("channel_major", P.CASES[4], "decided"), ("channel_major", P.CASES[9], "decided"),
    ("cls_as_patch0", P.CASES[3], "decided"), ("cls_as_patch0", P.CASES[6], "decided"),
    ("no_clamp", P.CASES[13], "decided"), ("no_clamp", P.CASES[14], "decided")])
def test_rule_rejects_seeded_defects(refs, defect, case, expect):
    o = P.case_inputs(case)
    got = P.emulate(o["img"], o["pred"], o["mask"], o["mean"], o["std"], case[0][3], case[1], case[2], o["bands"], defect=defect)
    bad = P.violations(got, refs(case))
    assert expect in bad, (defect, P.case_id(case), bad)


def test_masks():
    m = P.masks(5, 36)
    assert set(m.unique().tolist()) == {0.0, 1.0} and bool((m[3] == 0).all()) and bool((m[4] == 1).all()) and 0.5 < float(m[:3].mean()) < 0.95
    assert bool((P.masks(2, 1)[1] == 1).all()) and bool((P.masks(2, 16)[1] == 0).all())


# ------------------------------------------------------------------------------------------------ the binding
def test_symbol_and_signature():
    import csmae_hip
    lib = ctypes.CDLL(csmae_hip.LIB_PATH)
    assert hasattr(lib, "csmae_recon_panel")
    I, L, Pt = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    assert csmae_hip._SIGNATURES["csmae_recon_panel"] == [I, L, I, I, I, Pt, Pt, L, L, Pt, Pt, Pt] + [I] * 10 + [Pt, Pt]
    assert "csmae_recon_panel" in csmae_hip._ADDED_WITHIN_ABI and csmae_hip.ABI_VERSION == 7


def test_recon_panel_refuses_cpu_tensors():
    from csmae_hip import ops
    img, pred, mask = torch.zeros(1, 3, 16, 16), torch.zeros(1, 1, 768), torch.zeros(1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.recon_panel(img, pred, mask, torch.zeros(3), torch.ones(3), 16)
    sig = inspect.signature(ops.recon_panel)
    assert list(sig.parameters) == ["img", "pred", "mask", "mean", "std", "p", "panels", "gap", "bands", "out", "st"]
    assert (sig.parameters["panels"].default, sig.parameters["gap"].default, sig.parameters["bands"].default) == ((0, 1, 2), 2, None)


# ------------------------------------------------------------------------------------------------ util.viz
def test_panel_codes_and_run_eval_signature():
    from util import viz
    assert viz.PANEL_CODES == {"x": 0, "xm": 1, "y": 2, "ym": 3, "xm_ym": 4} and tuple(viz.PANEL_CODES) == P.NAMES
    assert viz.panel_codes(("xm_ym", "y", 0)) == [4, 2, 0] and viz.panel_codes("ym") == [3]
    with pytest.raises(ValueError, match="unknown panel"):
        viz.panel_codes(("x", "diff"))
    par = inspect.signature(viz.run_eval).parameters
    assert par["panel_dir"].default is None and par["panel_every"].default is None and par["panels"].default == ("x", "xm", "y")
    assert "plot_every" not in par and "do_plot_image_comp" not in par
    assert viz.sheet_width(64, 3, 2) == 196 and viz.sheet_width(224, 1, 7) == 224 and viz.sheet_width(20, 5, 0) == 100
    par = inspect.signature(viz.reconstruction_panels).parameters
    assert list(par) == ["model", "imgs", "seeds", "panels", "gap", "bands", "mean", "std", "pred", "mask"]
    a, b = np.zeros((4, 10, 3), np.uint8), np.full((4, 7, 3), 9, np.uint8)
    s = viz.stack_sheets([a, b], gap=2)
    assert s.shape == (10, 10, 3) and (s[:4] == 0).all() and (s[4:6] == 255).all() and (s[6:, :7] == 9).all() and (s[6:, 7:] == 255).all()
    assert viz.stack_sheets([a], gap=2) is not None and viz.stack_sheets([a], gap=2).shape == a.shape


class StubModel:
    def __init__(self, input_size, value):
        self.input_size, self.patch_size, self.input_channels, self.device, self.value = input_size, 4, 3, "cpu", value


def test_plot_reconstruction_path_rule(tmp_path, monkeypatch):
    """The forward, the scores and the kernel are replaced: what is checked is the stacking, the return value and where the files go."""
    from PIL import Image
    from util import recon_plot, viz
    seen = []

    def fake_forward(model, imgs, seeds):
        seen.append((model.value, tuple(imgs.shape), list(seeds)))
        return torch.zeros(1, 4, 48), torch.zeros(1, 4)

    def fake_panels(model, imgs, seeds, panels=("x", "xm", "y"), gap=2, bands=None, mean=None, std=None, pred=None, mask=None):
        assert pred is not None and mask is not None
        S = imgs.shape[-1]
        return torch.full((1, S, viz.sheet_width(S, len(panels), gap), 3), model.value, dtype=torch.uint8)

    monkeypatch.setattr(viz, "masked_forward", fake_forward)
    monkeypatch.setattr(viz, "reconstruction_panels", fake_panels)
    monkeypatch.setattr(viz.metrics, "batch_metrics", lambda img, pred, p, names, mean=None, std=None: {n: torch.tensor([0.25]) for n in names})
    models = {"first": StubModel(8, 10), "second": StubModel(8, 20)}
    img = np.zeros((8, 8, 3))
    sheet = recon_plot.plot_reconstruction(models, img, image_name="tile 7", title="Run A: clean", savedir=str(tmp_path), save=True, mask_seed=5, captions=False)
    assert sheet.dtype == np.uint8 and sheet.shape == (8 + 2 + 8, 28, 3)
    assert (sheet[:8] == 10).all() and (sheet[8:10] == 255).all() and (sheet[10:] == 20).all()
    assert seen == [(10, (1, 3, 8, 8), [5]), (20, (1, 3, 8, 8), [5])]
    sub = viz.title_to_fname("Run A: clean")
    png = tmp_path / sub / ("plot_img_" + viz.title_to_fname("Run A: clean - tile 7") + ".png")
    assert png.exists(), os.listdir(tmp_path)
    assert (np.asarray(Image.open(png).convert("RGB")) == sheet).all()
    meta = json.load(open(str(png)[:-4] + ".json"))
    assert meta["models"] == ["first", "second"] and meta["panels"] == ["x", "xm", "y"] and meta["metric"] == "ssim" and meta["scores"] == {"first": 0.25, "second": 0.25}
    # no image name: no sub-folder; no title: nothing saved; captions: a strip above each row, the rows unchanged below it
    recon_plot.plot_reconstruction(models, img, title="Run A", savedir=str(tmp_path / "flat"), save=True, mask_seed=5, captions=False)
    assert sorted(os.listdir(tmp_path / "flat")) == ["plot_img_Run_A.json", "plot_img_Run_A.png"]
    recon_plot.plot_reconstruction(models, img, savedir=str(tmp_path / "none"), save=True, mask_seed=5)
    assert not (tmp_path / "none").exists()
    cap = recon_plot.plot_reconstruction(models["first"], img, mask_seed=5, panels=("x", "y"), gap=3, show=True)
    assert cap.shape == (recon_plot.CAPTION_HEIGHT + 8, 8 + 3 + 8, 3) and (cap[recon_plot.CAPTION_HEIGHT:] == 10).all() and (cap[:recon_plot.CAPTION_HEIGHT] != 255).any()


# ------------------------------------------------------------------------------------------------ main_recon_eval.py
def test_driver_panel_flags():
    import main_recon_eval as M
    a = M.get_args_parser().parse_args(["--chkpt_dirs", "A"])
    assert a.panel_dir is None and a.panel_every is None and a.panels == ["x", "xm", "y"]
    a = M.get_args_parser().parse_args(["--chkpt_dirs", "A", "--panel_dir", "/o/p", "--panel_every", "4", "--panels", "x", "xm_ym", "ym"])
    assert (a.panel_dir, a.panel_every, a.panels) == ("/o/p", 4, ["x", "xm_ym", "ym"])
    from util import viz
    assert tuple(M.PANEL_CHOICES) == tuple(viz.PANEL_CODES)
    with pytest.raises(SystemExit):
        M.get_args_parser().parse_args(["--chkpt_dirs", "A", "--panels", "diff"])
