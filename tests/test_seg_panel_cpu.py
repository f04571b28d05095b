"""CPU-side checks of the overlay sheets of the segmentation probe: the float64 reference of tests/seg_panel_ref.py stays inside its caps on every
case and its rule catches every seeded defect of the fp32 emulation; the palette, the per-image scores, the palette PNG, the driver's flags and the
Python-side refusals of ops.seg_panel.  No kernel runs here."""
import os
import re

import numpy as np
import pytest
import torch

import recon_panel_ref as P
import seg_panel_ref as SP
import seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(o, defect=None, **kw):
    o = dict(o, **kw)
    ref = SP.reference(o["img"], o["pl"], o["labels"], o["mean"], o["std"], o["palette"], o["p"], o["panes"], o["gap"], o["bands"], o["a8"], o["ignore_rgb"])
    got = SP.emulate(o["img"], o["pl"], o["labels"], o["mean"], o["std"], o["palette"], o["p"], o["panes"], o["gap"], o["bands"], o["a8"], o["ignore_rgb"], defect=defect)
    return got, ref


def test_cases_cover_what_the_issue_lists():
    assert len(SP.COMBOS) == len(R.CASES) * len(SP.LABEL_PATTERNS) * len(SP.CHANNELS) == 75
    for case in R.CASES:
        mine = [c for c in SP.COMBOS if c[0] == case]
        assert {c[1] for c in mine} == set(R.PATTERNS) | {None} and {c[2] for c in mine} == {3, 1, 4}
        assert {c[3] for c in mine} == {0.0, 0.5, 1.0} and {c[4] for c in mine} == {0, 2}
        sets = {c[5] for c in mine}
        assert any(len(s) == 1 for s in sets) and (0, 1, 2, 3, 4, 5) in sets and any(len(s) == 6 for s in sets if not set(s) & set(SP.NEEDS_LABELS))
    for c in SP.COMBOS:
        assert c[1] is not None or not set(c[5]) & set(SP.NEEDS_LABELS), c
    assert P.BANDS[4] == (3, 1, 0) and P.BANDS[1] == (0, 0, 0)
    assert [SP.a8_of(a) for a in SP.ALPHAS] == [0, 128, 256]


@pytest.mark.parametrize("combo", SP.COMBOS, ids=SP.combo_id)
def test_reference_stays_inside_the_caps(combo):
    ref = SP.combo_reference(combo)
    assert SP.tie_share(ref) <= R.TIE_CAP, SP.tie_share(ref)
    assert SP.borderline_share(ref) <= P.BORDERLINE_CAP, SP.borderline_share(ref)
    N, G, p, K = combo[0]
    S, n = G * p, len(combo[5])
    assert ref["byte"].shape == (N, S, n * S + (n - 1) * combo[4], 3) and ref["byte"].dtype == np.uint8
    assert (ref["stats"] is None) == (combo[1] is None)
    if ref["stats"] is not None:
        lab = ref["labels"]
        assert (ref["stats"][:, :, 1].sum(1) == (lab < K).reshape(N, -1).sum(1)).all() and (ref["stats"][:, :, 2].sum(1) == ref["stats"][:, :, 1].sum(1)).all()
        assert (ref["stats"][:, :, 0] <= np.minimum(ref["stats"][:, :, 1], ref["stats"][:, :, 2])).all()


# combinations the defect hunt walks: every small case with labels, all six panes where the set allows, plus the unlabelled ones of one case
HUNT = tuple(c for c in SP.COMBOS if c[0] != (1, 14, 16, 16) and c[1] in ("random", "ignore30", None))


@pytest.mark.parametrize("combo", HUNT, ids=SP.combo_id)
def test_undisturbed_emulation_passes(combo):
    got, ref = run(SP.combo_inputs(combo))
    assert SP.violations(got, ref) == []
    assert SP.violations(got["out"], ref) == []


def test_violations_reports_every_seeded_defect():
    six = dict(panes=(0, 1, 2, 3, 4, 5), gap=2, a8=128)
    base = SP.combo_inputs(next(c for c in SP.COMBOS if c[0] == (3, 3, 8, 21) and c[1] == "ignore30" and c[2] == 3))
    stray = dict(base, labels=SP.with_stray_labels(base["labels"], 21))
    ties = dict(base, pl=SP.with_exact_ties(base["pl"]))
    special = {"stray_as_class": stray, "tie_highest": ties}
    for o in (stray, ties):                      # the planted inputs themselves are fine
        got, ref = run(o, **six)
        assert SP.violations(got, ref) == []
    assert bool(SP.reference(*(ties[k] for k in ("img", "pl", "labels", "mean", "std", "palette", "p")), (2,), 0, ties["bands"], 128)["tie"][0].all())
    found = {}
    for defect in SP.DEFECTS:
        got, ref = run(special.get(defect, base), defect=defect, **six)
        found[defect] = SP.violations(got, ref)
        assert found[defect], f"{defect}: not reported"
    # ... and by the check that is about it
    assert "tie" in found["tie_highest"] or "pred_tie" in found["tie_highest"]
    assert found["stats_count_ignored"] == ["stats"] and found["pred_area_all_pixels"] == ["stats"]
    assert "gap" in found["gap_short"] and "decided" in found["bgr"] and "decided" in found["blend_truncates"] and "pred" in found["align_corners"]
    # every defect that touches the bytes is also seen in the sheet alone, on at least one combination of the table
    for defect in ("align_corners", "blend_truncates", "bgr", "ignore_as_class", "errors_on_ignored", "gap_short"):
        hit = False
        for combo in HUNT:
            if combo[1] is None:
                continue
            got, ref = run(SP.combo_inputs(combo), defect=defect)
            hit = hit or bool(SP.violations(got["out"], ref))
        assert hit, defect


def test_borderline_and_tie_latitude_is_no_wider_than_stated():
    combo = next(c for c in SP.COMBOS if c[0] == (2, 2, 4, 5) and c[1] == "random" and c[2] == 3)
    o = dict(SP.combo_inputs(combo), panes=(0, 4, 2), gap=2, a8=128)
    got, ref = run(o)
    out = got["out"].copy()
    out[0, 0, 0, 0] = out[0, 0, 0, 0] ^ 1       # a decided byte off by one
    assert not ref["borderline"][0, 0, 0, 0] and "decided" in SP.violations(dict(got, out=out), ref)
    # at a tie pixel the second class is accepted only when every pane and pred show it
    t = dict(o, pl=SP.with_exact_ties(o["pl"]))
    got, ref = run(t)
    assert ref["tie"][0].all() and SP.violations(got, ref) == []
    second = SP.compose(SP.image_bytes(t["img"], t["mean"], t["std"], t["p"], t["bands"])[0], ref["arg2"], t["labels"].numpy(), 5, t["palette"], (0, 4, 2), 2, 128,
                        t["ignore_rgb"])
    mixed = got["out"].copy()
    S = ref["S"]
    mixed[0, :, 2 * (S + 2):] = second[0, :, 2 * (S + 2):]      # pane 2 shows class 1, pane 1 still class 0
    assert "tie" in SP.violations(mixed, ref)
    whole = got["out"].copy()
    whole[0] = second[0]
    assert SP.violations(whole, ref) == []
    assert "tie" in SP.violations(dict(out=whole, pred=got["pred"]), ref)   # ... and pred has to agree with the sheet


# ------------------------------------------------------------------------------------------------ util.seg_viz, util.metrics
def test_default_palette_is_the_voc_map():
    from util.seg_viz import default_palette, pane_codes
    pal = default_palette(8)
    assert pal.dtype == np.uint8 and pal.tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128], [0, 128, 128], [128, 128, 128]]
    big = default_palette(64)
    assert big.shape == (64, 3) and len({tuple(r) for r in big.tolist()}) == 64 and (big[:8] == pal).all() and big[8].tolist() == [64, 0, 0]
    assert (big == SP.voc_palette(64)).all()
    assert pane_codes(SP.PANES) == [0, 1, 2, 3, 4, 5] and pane_codes("errors") == [5] and pane_codes(("image", 4)) == [0, 4]
    with pytest.raises(ValueError, match="unknown pane"):
        pane_codes(["overlay"])


def test_per_image_scores_hand_built():
    from util.metrics import per_image_scores
    stats = np.zeros((3, 4, 3), dtype=np.int32)
    stats[0, 0] = (5, 7, 6)      # IoU 5 / 8
    stats[0, 1] = (3, 4, 6)      # IoU 3 / 7
    stats[0, 2] = (0, 2, 1)      # IoU 0 / 3; class 3 is absent
    stats[1, 3] = (9, 9, 9)      # one class, all right
    sc = per_image_scores(stats)  # image 2 has no valid pixel
    assert sc["valid"].tolist() == [13, 9, 0]
    assert np.allclose(sc["iou"][0, :3], [5 / 8, 3 / 7, 0.0], rtol=0, atol=1e-15) and np.isnan(sc["iou"][0, 3])
    assert abs(sc["mIoU"][0] - (5 / 8 + 3 / 7) / 3) < 1e-15 and abs(sc["pixel_acc"][0] - 8 / 13) < 1e-15
    assert sc["mIoU"][1] == 1.0 and sc["pixel_acc"][1] == 1.0 and np.isnan(sc["iou"][1, :3]).all() and sc["iou"][1, 3] == 1.0
    assert np.isnan(sc["mIoU"][2]) and np.isnan(sc["pixel_acc"][2]) and np.isnan(sc["iou"][2]).all()
    same = per_image_scores(torch.from_numpy(stats))
    assert all(np.array_equal(same[k], sc[k], equal_nan=True) for k in sc)
    # the sum over the images is the confusion matrix's diagonal, row sums and column sums: the pooled scores are miou_from_confusion's
    from util.metrics import miou_from_confusion
    cm = np.array([[5, 1, 0], [2, 3, 1], [0, 0, 4]])
    pooled = np.stack([np.diag(cm), cm.sum(1), cm.sum(0)], axis=1)[None]
    miou, per = miou_from_confusion(cm)
    sc = per_image_scores(pooled)
    assert np.allclose(sc["iou"][0], per, rtol=0, atol=1e-15) and abs(sc["mIoU"][0] - miou) < 1e-15
    with pytest.raises(ValueError):
        per_image_scores(np.zeros((2, 3)))


def test_write_mask_png_round_trips(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from util.seg_viz import default_palette, write_mask_png
    K = 21
    pal = default_palette(K)
    pred = torch.randint(0, K, (24, 40), generator=torch.Generator().manual_seed(3)).to(torch.uint8)
    path = str(tmp_path / "mask.png")
    write_mask_png(path, pred, pal)
    with Image.open(path) as im:
        assert im.mode == "P" and im.size == (40, 24)
        assert np.array_equal(np.asarray(im), pred.numpy())
        assert im.getpalette()[:3 * K] == pal.reshape(-1).tolist()
        assert np.array_equal(np.asarray(im.convert("RGB")), pal[pred.numpy()])
    write_mask_png(path, pred.numpy()[:5], torch.from_numpy(pal))
    with Image.open(path) as im:
        assert im.size == (40, 5)
    with pytest.raises(ValueError):
        write_mask_png(path, np.zeros((2, 3, 4)), pal)


# ------------------------------------------------------------------------------------------------ the driver, the binding
def test_driver_flags_default_off():
    import main_segprobe as M
    a = M.get_args_parser().parse_args([])
    new = ("panel_dir", "panel_every", "panes", "panel_alpha", "pred_dir", "per_image")
    assert not any(hasattr(a, k) for k in new), "a flag that is not given leaves the namespace (and the line the driver prints of it) as it was"
    assert not M.wants_outputs(a) and not M.wants_outputs(None)
    a = M.get_args_parser().parse_args("--panel_dir P --panel_every 3 --panes image errors gt pred --panel_alpha 0.25 --pred_dir Q --per_image".split())
    assert (a.panel_dir, a.panel_every, a.pred_dir, a.per_image, a.panel_alpha, a.panes) == ("P", 3, "Q", True, 0.25, ["image", "errors", "gt", "pred"])
    assert M.wants_outputs(a)
    for flags in (["--panel_dir", "P"], ["--pred_dir", "Q"], ["--per_image"]):
        assert M.wants_outputs(M.get_args_parser().parse_args(flags))
    assert not M.wants_outputs(M.get_args_parser().parse_args(["--panes", "gt", "--panel_every", "2", "--panel_alpha", "1"]))   # modifiers alone ask for nothing
    with pytest.raises(SystemExit):
        M.get_args_parser().parse_args(["--panes", "overlay"])
    from util.seg_viz import DEFAULT_PANES, PANE_CODES
    assert tuple(PANE_CODES) == M.PANE_CHOICES == SP.PANES and DEFAULT_PANES == M.DEFAULT_PANES == ("image", "gt_over", "pred_over")


def test_default_evaluate_takes_the_old_path():
    """Without the flags `evaluate` calls evaluate_batch(samples, labels, conf) exactly as before: no want_logits, no seg_panel."""
    import main_segprobe as M
    calls = []

    class Probe:
        num_classes = 3

        def eval(self):
            return self

        def evaluate_batch(self, *a, **kw):
            calls.append((len(a), kw))
            return torch.tensor(0.5), torch.tensor([4])

    batches = [(torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8))] * 2
    args = M.get_args_parser().parse_args([])
    for a in (args, None):
        calls.clear()
        stats = M.evaluate(batches, Probe(), torch.device("cpu"), a)
        assert calls == [(3, {}), (3, {})] and stats["loss"] == 0.5 and set(stats) == {"loss", "mIoU", "pixel_acc", "iou"}


def test_evaluate_batch_keeps_its_default_return():
    import inspect

    import models_seg
    sig = inspect.signature(models_seg.LinearSegProbe.evaluate_batch)
    assert list(sig.parameters) == ["self", "x", "labels", "conf", "want_logits"] and sig.parameters["want_logits"].default is False


def test_seg_panel_python_side_refusals():
    from csmae_hip import ops
    N, C, S, G, K = 2, 3, 8, 2, 5
    img, pl, labels = torch.zeros(N, C, S, S), torch.zeros(N, G, G, K), torch.zeros(N, S, S, dtype=torch.uint8)
    mean, std, pal = torch.zeros(C), torch.ones(C), torch.zeros(K, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_panel(img, pl, labels, mean, std, pal)
    bad = [dict(img=img.double()), dict(img=img[:, :, :, :6]), dict(pl=pl[:1]), dict(pl=pl.double()), dict(pl=torch.zeros(N, G, 3, K)), dict(labels=labels.long()),
           dict(labels=labels[:, :4]), dict(mean=torch.zeros(C + 1)), dict(std=std.double()), dict(palette=pal[:4]), dict(palette=pal.float()),
           dict(pred=torch.zeros(N, S, S)), dict(stats=torch.zeros(N, K, 3, dtype=torch.int64)), dict(stats=torch.zeros(N, K, 2, dtype=torch.int32)),
           dict(out=torch.zeros(N, S, 3 * S, 3, dtype=torch.uint8))]
    for kw in bad:
        a = dict(img=img, pl=pl, labels=labels, mean=mean, std=std, palette=pal)
        extra = {k: kw[k] for k in kw if k not in a}
        a.update({k: kw[k] for k in kw if k in a})
        with pytest.raises(AssertionError):
            ops.seg_panel(a["img"], a["pl"], a["labels"], a["mean"], a["std"], a["palette"], **extra)


def test_the_new_header_function_is_bound():
    import csmae_hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csmae.h")).read(), flags=re.S)
    assert re.search(r"int\s+csmae_segpanel\s*\(", text)
    assert "csmae_segpanel" in csmae_hip._SIGNATURES and "csmae_segpanel" in csmae_hip._ADDED_WITHIN_ABI
    assert hasattr(csmae_hip.load(), "csmae_segpanel")
    src = open(os.path.join(ROOT, "cross-scale-mae_amd", "csrc", "segment.hip")).read()
    common = open(os.path.join(ROOT, "cross-scale-mae_amd", "csrc", "seg_common.h")).read()
    for name in ("struct SegAxis", "seg_axis(int i", "struct SegPixel", "SegPixel seg_pixel("):
        assert name in common and name not in src, name
    for f in ("segment.hip", "seg_panel.hip"):
        assert '#include "seg_common.h"' in open(os.path.join(ROOT, "cross-scale-mae_amd", "csrc", f)).read()
