"""GPU tests of the overlay sheets of the segmentation probe (csrc/seg_panel.hip, ops.seg_panel, util.seg_viz, main_segprobe.py --panel_dir / --pred_dir /
--per_image) against the float64 reference and the decided / borderline / tie rule of seg_panel_ref.py, in guarded buffers.  Needs an MI355X."""
import csv
import os

import numpy as np
import pytest
import torch

import recon_eval_ref as E
import seg_panel_ref as SP
import seg_ref as R

pytestmark = pytest.mark.gpu
U8 = torch.uint8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import csmae_hip
    from csmae_hip import ops as o
    csmae_hip.load()
    return o


def guarded_bytes(n, fill):
    g = E.Guarded(1, n, U8, off8=True, fill=fill)
    assert g.vec.data_ptr() % 16 == 8
    return g


def run_guarded(ops, o, want_pred=True, want_stats=None, **kw):
    """ops.seg_panel with out, pred and stats inside sentinel-guarded buffers whose payloads start 8 bytes behind a 16-byte boundary, run twice over
    payloads prefilled with 0xA5 and with 0x5A: a byte the kernel leaves unwritten differs between the two.  -> dict(out, pred, stats) of numpy arrays."""
    o = dict(o, **kw)
    N, C, S, _ = o["img"].shape
    K, n = o["pl"].shape[-1], len(o["panes"])
    W = n * S + (n - 1) * o["gap"]
    want_stats = (o["labels"] is not None) if want_stats is None else want_stats
    dev = {k: o[k].cuda() for k in ("img", "pl", "mean", "std")}
    labels = None if o["labels"] is None else o["labels"].cuda()
    palette = torch.from_numpy(np.ascontiguousarray(o["palette"])).cuda()
    runs = []
    for fill in (0xA5, 0x5A):
        g = dict(out=guarded_bytes(N * S * W * 3, fill))
        if want_pred:
            g["pred"] = guarded_bytes(N * S * S, fill)
        if want_stats:
            g["stats"] = guarded_bytes(N * K * 3 * 4, fill)
        out = ops.seg_panel(dev["img"], dev["pl"], labels, dev["mean"], dev["std"], palette, panes=o["panes"], alpha=o["a8"] / 256.0, gap=o["gap"], bands=o["bands"],
                            ignore_rgb=o["ignore_rgb"], out=g["out"].vec.view(N, S, W, 3), pred=g["pred"].vec.view(N, S, S) if want_pred else None,
                            stats=g["stats"].vec.view(torch.int32).view(N, K, 3) if want_stats else None)
        torch.cuda.synchronize()
        assert out.data_ptr() == g["out"].vec.data_ptr()
        for name, b in g.items():
            assert b.outside_intact(), f"seg_panel wrote outside {name}"
        runs.append(dict(out=g["out"].vec.view(N, S, W, 3).cpu().numpy().copy(), pred=g["pred"].vec.view(N, S, S).cpu().numpy().copy() if want_pred else None,
                         stats=g["stats"].vec.view(torch.int32).view(N, K, 3).cpu().numpy().copy() if want_stats else None))
    for name in ("out", "pred", "stats"):
        if runs[0][name] is not None:
            assert (runs[0][name] == runs[1][name]).all(), f"{int((runs[0][name] != runs[1][name]).sum())} elements of {name} were left unwritten (or differ between two launches)"
    return runs[0]


def ref_of(o):
    return SP.reference(o["img"], o["pl"], o["labels"], o["mean"], o["std"], o["palette"], o["p"], o["panes"], o["gap"], o["bands"], o["a8"], o["ignore_rgb"])


def labelled(case, pattern="ignore30", C=3):
    return SP.combo_inputs(next(c for c in SP.COMBOS if c[0] == case and c[1] == pattern and c[2] == C))


# ------------------------------------------------------------------------------------------------ the kernel against float64
@pytest.mark.parametrize("combo", SP.COMBOS, ids=SP.combo_id)
def test_kernel_vs_float64(ops, combo):
    o, ref = SP.combo_inputs(combo), SP.combo_reference(combo)
    assert SP.tie_share(ref) <= R.TIE_CAP and SP.borderline_share(ref) <= SP.P.BORDERLINE_CAP
    got = run_guarded(ops, o)
    differ = float(((got["out"] != ref["byte"]) & ref["borderline"]).mean())
    print(f"seg_panel {SP.combo_id(combo)}: tie share {SP.tie_share(ref):.2e}, borderline share {SP.borderline_share(ref):.2e}, borderline bytes that differ {differ:.2e}")
    assert SP.violations(got, ref) == []
    keep = ~ref["tie"]
    assert (got["pred"].astype(np.int64)[keep] == ref["arg"][keep]).all(), "pred differs from the float64 argmax away from near-ties"


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "N%d-G%d-p%d-K%d" % c)
def test_stats_are_the_counts_of_pred(ops, case):
    from util.metrics import confusion_matrix
    N, G, p, K = case
    for pattern in ("random", "ignore30", "image_ignored", "all_ignored"):
        o = labelled(case, pattern)
        got = run_guarded(ops, o, panes=(2,), gap=0)
        lab = o["labels"].numpy()
        assert (got["stats"] == SP.count_stats(got["pred"], lab, K)).all(), pattern
        v = lab < K
        cm = confusion_matrix(lab[v], got["pred"][v], K)
        total = got["stats"].astype(np.int64).sum(0)
        assert (total[:, 0] == np.diag(cm)).all() and (total[:, 1] == cm.sum(1)).all() and (total[:, 2] == cm.sum(0)).all(), pattern


def test_stats_sum_agrees_with_seg_ce_conf(ops):
    """Away from near-ties (marked ignored on both sides, as seg_ref.conf_labels does) the sum over the images is seg_ce's confusion matrix."""
    N, G, p, K = case = (3, 3, 8, 21)
    o = labelled(case)
    tie = torch.from_numpy(SP.top_two(o["pl"], p)[2])
    labels = R.conf_labels(o["labels"], tie)
    got = run_guarded(ops, dict(o, labels=labels), panes=(5,), gap=0)
    conf = torch.zeros(K, K, device="cuda", dtype=torch.int64)
    ops.seg_ce(o["pl"].cuda(), labels.cuda(), torch.empty(1, device="cuda"), torch.empty(1, device="cuda", dtype=torch.int64), conf=conf)
    conf = conf.cpu().numpy()
    total = got["stats"].astype(np.int64).sum(0)
    assert (total[:, 0] == np.diag(conf)).all() and (total[:, 1] == conf.sum(1)).all() and (total[:, 2] == conf.sum(0)).all()


def test_stray_labels_stay_in_bounds_and_count_as_ignored(ops):
    N, G, p, K = case = (2, 2, 4, 5)
    o = labelled(case)
    o = dict(o, labels=SP.with_stray_labels(o["labels"], K), panes=(0, 1, 2, 3, 4, 5), gap=2, a8=128)
    got, ref = run_guarded(ops, o), ref_of(o)
    assert SP.violations(got, ref) == []
    lab = o["labels"].numpy()
    stray = (lab >= K) & (lab < 255)
    assert stray.sum() > 0 and int(got["stats"][:, :, 1].sum()) == int((lab < K).sum())
    S = ref["S"]
    gt = got["out"][:, :, S + 2:2 * S + 2]
    assert (gt[stray] == np.array(SP.IGNORE_RGB, dtype=np.uint8)).all(), "a stray label is shown as ignored in the gt pane"
    # ... exactly as if it had been 255
    same = run_guarded(ops, dict(o, labels=torch.where(torch.from_numpy(stray), torch.tensor(255, dtype=U8), o["labels"])))
    assert all((same[k] == got[k]).all() for k in ("out", "pred", "stats"))


@pytest.mark.parametrize("case", [(2, 2, 4, 5), (2, 4, 16, 64), (1, 14, 16, 16)], ids=lambda c: "N%d-G%d-p%d-K%d" % c)
def test_without_labels(ops, case):
    o = dict(labelled(case), labels=None, panes=(0, 2, 4), gap=2, a8=128)
    got, ref = run_guarded(ops, o), ref_of(o)
    assert got["stats"] is None and SP.violations(got, ref) == []
    # the panes that show no label do not depend on the labels
    with_labels = run_guarded(ops, dict(o, labels=labelled(case)["labels"]))
    assert (with_labels["out"] == got["out"]).all() and (with_labels["pred"] == got["pred"]).all()
    # ... and out alone is a complete call
    alone = run_guarded(ops, o, want_pred=False)
    assert (alone["out"] == got["out"]).all()


def test_exact_ties_take_the_lowest_index(ops):
    N, G, p, K = case = (3, 3, 8, 21)
    o = labelled(case)
    o = dict(o, pl=SP.with_exact_ties(o["pl"]), panes=(2, 4, 5), gap=0, a8=128)
    got, ref = run_guarded(ops, o), ref_of(o)
    assert ref["tie"][0].all() and (got["pred"][0] == 0).all()
    assert SP.violations(got, ref) == []


@pytest.mark.parametrize("case", [(2, 4, 16, 64), (1, 14, 16, 16)], ids=lambda c: "N%d-G%d-p%d-K%d" % c)
def test_two_launches_give_identical_bytes(ops, case):
    o = dict(labelled(case), panes=(0, 1, 2, 3, 4, 5), gap=2, a8=77)
    a, b = run_guarded(ops, o), run_guarded(ops, o)
    assert all((a[k] == b[k]).all() for k in ("out", "pred", "stats"))


def test_batch_independence(ops):
    case = (3, 3, 8, 21)
    o = dict(labelled(case), panes=(3, 5), gap=1, a8=100)     # a sheet row of 147 bytes: the images and bands start at every alignment
    whole = run_guarded(ops, o)
    for n in range(3):
        one = dict(o, img=o["img"][n:n + 1].contiguous(), pl=o["pl"][n:n + 1].contiguous(), labels=o["labels"][n:n + 1].contiguous())
        got = run_guarded(ops, one)
        assert all((got[k][0] == whole[k][n]).all() for k in ("out", "pred", "stats")), n


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "N%d-G%d-p%d-K%d" % c)
def test_pred_agrees_with_seg_ce(ops, case):
    N, G, p, K = case
    o = labelled(case, "random")
    got = run_guarded(ops, o, panes=(2,), gap=0)
    S = G * p
    pred = torch.empty(N, S, S, device="cuda", dtype=U8)
    ops.seg_ce(o["pl"].cuda(), None, torch.empty(1, device="cuda"), torch.empty(1, device="cuda", dtype=torch.int64), pred=pred)
    keep = ~SP.top_two(o["pl"], p)[2]
    assert (pred.cpu().numpy()[keep] == got["pred"][keep]).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    import csmae_hip
    lib = csmae_hip.load()
    N, C, G, p, K = 1, 3, 2, 16, 5
    S = G * p
    W = 3 * S + 4
    img, pl = torch.zeros(N, C, S, S, device="cuda"), torch.zeros(N, G, G, K, device="cuda")
    labels, pal = torch.zeros(N, S, S, device="cuda", dtype=U8), torch.zeros(K, 3, device="cuda", dtype=U8)
    mean, std = torch.zeros(C).cuda(), torch.ones(C).cuda()

    def buffers():
        return guarded_bytes(N * S * W * 3, None), guarded_bytes(N * S * S, None), guarded_bytes(N * K * 3 * 4, None)
    g = buffers()
    base = dict(N=N, C=C, S=S, G=G, p=p, K=K, img=img.data_ptr(), mean=mean.data_ptr(), std=std.data_ptr(), br=0, bg=1, bb=2, pl=pl.data_ptr(), labels=labels.data_ptr(),
                pal=pal.data_ptr(), ir=224, ig=224, ib=192, a8=128, c0=0, c1=3, c2=4, c3=0, c4=0, c5=0, n=3, gap=2, out=g[0].vec.data_ptr(), pred=g[1].vec.data_ptr(),
                stats=g[2].vec.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return lib.csmae_segpanel(a["N"], a["C"], a["S"], a["G"], a["p"], a["K"], a["img"], a["mean"], a["std"], a["br"], a["bg"], a["bb"], a["pl"], a["labels"], a["pal"],
                                   a["ir"], a["ig"], a["ib"], a["a8"], a["c0"], a["c1"], a["c2"], a["c3"], a["c4"], a["c5"], a["n"], a["gap"], a["out"], a["pred"], a["stats"],
                                   ops.stream())

    refused = [(dict(K=1), "K = 1"), (dict(K=65), "K = 65"), (dict(p=5, S=10), "patch size 5"), (dict(p=12, S=24), "patch size 12"), (dict(S=S + 1), "does not fit"),
               (dict(G=3), "does not fit"), (dict(n=0), "n_panes"), (dict(n=7), "n_panes"), (dict(c1=6), "pane1"), (dict(c2=-1), "pane2"),
               (dict(labels=None, stats=None), "labels, which are null"), (dict(labels=None, stats=None, c1=1, c2=2), "pane1"),
               (dict(labels=None, stats=None, c0=5, n=1), "pane0"), (dict(labels=None, c1=2, c2=4), "stats"), (dict(br=3), "band_r"), (dict(bg=-1), "band_g"),
               (dict(bb=C), "band_b"), (dict(gap=-1), "gap"), (dict(a8=-1), "a8"), (dict(a8=257), "a8"), (dict(N=1 << 20), "2^31"), (dict(N=0), "N"),
               (dict(img=None), "null"), (dict(pl=None), "null"), (dict(pal=None), "null"), (dict(out=None), "null"), (dict(ir=256), "ignore_rgb")]
    for kw, word in refused:
        assert call(**kw) != 0, kw
        assert word in lib.csmae_last_error().decode(), (kw, lib.csmae_last_error().decode())
    torch.cuda.synchronize()
    for b in g:
        assert b.untouched(), "a refused call wrote to an output"
    assert call(c3=9, c4=-3, c5=77) == 0          # codes behind n_panes are not read
    assert call(labels=None, stats=None, c1=2, pred=None) == 0
    torch.cuda.synchronize()
    assert all(b.outside_intact() for b in g) and all(b.unwritten() < b.n for b in g)
    with pytest.raises(csmae_hip.CsmaeError, match="pane0"):
        ops.seg_panel(img, pl, labels, mean, std, pal, panes=(7,))
    with pytest.raises(csmae_hip.CsmaeError, match="a8"):
        ops.seg_panel(img, pl, labels, mean, std, pal, alpha=1.5)
    with pytest.raises(csmae_hip.CsmaeError, match="null"):
        ops.seg_panel(img, pl, None, mean, std, pal)        # the default panes show the labels


# ------------------------------------------------------------------------------------------------ util.seg_viz and the driver
MICRO_FLAGS = ["--dataset_type", "synthetic", "--embed_dim", "128", "--depth", "2", "--num_heads", "2", "--input_size", "64", "--patch_size", "16", "--batch_size", "4",
               "--nb_classes", "3", "--synthetic_len", "8", "--device", "cuda", "--eval"]


def test_segmentation_panels_forward_or_given_logits(ops):
    import models_seg
    import models_vit
    from finetune_ref import VIT_MICRO
    from util import seg_viz
    torch.manual_seed(0)
    probe = models_seg.LinearSegProbe(models_vit.vit_base_patch16(num_classes=2, global_pool=False, **VIT_MICRO).cuda(), 3).eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 64, generator=g).cuda()
    labels = torch.randint(0, 3, (2, 64, 64), generator=g).to(U8).cuda()
    sheets = seg_viz.segmentation_panels(probe, x, labels)
    assert sheets.is_cuda and sheets.dtype == U8 and sheets.shape == (2, 64, 3 * 64 + 4, 3)
    _, pl = probe(x, labels)
    again = seg_viz.segmentation_panels(None, x, labels, patch_logits=pl)      # no forward: no probe needed
    assert torch.equal(again, sheets)
    assert seg_viz.segmentation_panels(probe, x, None, panes=("pred",), gap=0).shape == (2, 64, 64, 3)
    # against the float64 rule, with the plot statistics the function defaults to
    from util.viz import image_mean, image_std
    mean, std = torch.tensor(image_mean, dtype=torch.float32), torch.tensor(image_std, dtype=torch.float32)
    ref = SP.reference(x.cpu(), pl.cpu(), labels.cpu(), mean, std, SP.voc_palette(3), 16, (0, 3, 4), 2, (0, 1, 2), 128)
    assert SP.violations(sheets.cpu().numpy(), ref) == []


def test_driver_writes_sheets_masks_and_scores(ops, tmp_path, monkeypatch):
    from PIL import Image

    import main_segprobe as M
    seen = {}
    evaluate = M.evaluate

    def spy(loader, model, device, args=None):
        seen.update(loader=loader, model=model)
        return evaluate(loader, model, device, args)
    monkeypatch.setattr(M, "evaluate", spy)
    out = tmp_path / "with"
    stats = M.main(M.get_args_parser().parse_args(MICRO_FLAGS + ["--output_dir", str(out), "--panel_dir", str(out / "panels"), "--pred_dir", str(out / "pred"), "--per_image",
                                                                  "--panes", "image", "gt_over", "pred_over", "errors"]))
    names = [f"img_{i:06d}" for i in range(8)]          # two batches of four
    assert sorted(os.listdir(out / "panels")) == sorted(os.listdir(out / "pred")) == [n + ".png" for n in names]
    for n in names:
        assert np.asarray(Image.open(out / "panels" / (n + ".png"))).shape == (64, 4 * 64 + 3 * 2, 3)
    # the palette PNGs hold the class indices probe(x) gives, away from near-ties
    probe, loader = seen["model"], seen["loader"]
    x, labels = loader.samples, loader.targets
    from util.downstream import autocast
    with autocast(x.device):                            # (as the sweep runs its forward)
        pred = probe(x).cpu().numpy()
        _, pl = probe(x, labels)
    tie = SP.top_two(pl.cpu(), 16)[2]
    from util.seg_viz import default_palette
    for i, n in enumerate(names):
        with Image.open(out / "pred" / (n + ".png")) as im:
            assert im.mode == "P" and im.getpalette()[:9] == default_palette(3).reshape(-1).tolist()
            idx = np.asarray(im)
        assert idx.shape == (64, 64) and (idx[~tie[i % 4]] == pred[i % 4][~tie[i % 4]]).all(), n
    # per_image.csv: the valid-pixel-weighted pixel accuracy is the sweep's, up to the near-tie pixels
    rows = list(csv.reader(open(out / "per_image.csv")))
    assert rows[0] == ["index", "name", "valid", "pixel_acc", "mIoU", "iou_0", "iou_1", "iou_2"] and [r[1] for r in rows[1:]] == names
    assert [int(r[0]) for r in rows[1:]] == list(range(8))
    valid = np.array([int(r[2]) for r in rows[1:]], dtype=np.float64)
    acc = np.array([float(r[3]) for r in rows[1:]])
    assert valid.sum() == 2 * int((labels != 255).sum())
    n_tie = 2 * int(tie.sum())
    print(f"segprobe outputs: {int(valid.sum())} valid pixels, {n_tie} near-tie pixels, pixel_acc {stats['pixel_acc']:.4f}")
    assert abs((valid * acc).sum() - stats["pixel_acc"] / 100.0 * valid.sum()) <= n_tie + 1e-6 * valid.sum()
    assert all(0.0 <= float(r[4]) <= 1.0 for r in rows[1:])
    # the same call without the flags writes none of it and returns the same numbers
    plain_dir = tmp_path / "plain"
    plain = M.main(M.get_args_parser().parse_args(MICRO_FLAGS + ["--output_dir", str(plain_dir)]))
    assert plain == stats
    assert not any(f.endswith((".png", ".csv")) for _, _, fs in os.walk(plain_dir) for f in fs)
    # --panel_every, and --per_image alone
    third = tmp_path / "third"
    M.main(M.get_args_parser().parse_args(MICRO_FLAGS + ["--output_dir", str(third), "--panel_dir", str(third / "panels"), "--panel_every", "3"]))
    assert sorted(os.listdir(third / "panels")) == ["img_000000.png", "img_000003.png", "img_000006.png"] and not os.path.exists(third / "per_image.csv")
    assert np.asarray(Image.open(third / "panels" / "img_000003.png")).shape == (64, 3 * 64 + 4, 3)
