"""CPU-side checks of the segmentation probe: the mIoU arithmetic, the reference's interpolation weights and footprints (tests/seg_ref.py), the
seeds of the GPU cases (near-tie pixels within their cap), the folder dataset, the driver's parser and refusals, and the binding table."""
import os
import re

import numpy as np
import pytest
import torch

import seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_miou_hand_computed():
    from util.metrics import miou_from_confusion, pixel_accuracy_from_confusion
    cm = np.array([[5, 1, 0], [2, 3, 1], [0, 0, 4]])
    # IoU_0 = 5 / (5 + 1 + 2), IoU_1 = 3 / (3 + (2 + 1) + 1), IoU_2 = 4 / (4 + 0 + 1)
    want = np.array([5 / 8, 3 / 7, 4 / 5])
    miou, per = miou_from_confusion(cm)
    assert np.allclose(per, want, rtol=0, atol=1e-15) and abs(miou - want.mean()) < 1e-15
    assert abs(pixel_accuracy_from_confusion(cm) - 12 / 16) < 1e-15
    miou_t, per_t = miou_from_confusion(torch.from_numpy(cm))
    assert miou_t == miou and np.array_equal(per_t, per)
    # a class absent from truth and prediction has no IoU and is left out of the mean
    cm4 = np.zeros((4, 4), dtype=np.int64)
    cm4[:3, :3] = cm
    miou4, per4 = miou_from_confusion(cm4)
    assert abs(miou4 - want.mean()) < 1e-15 and np.isnan(per4[3]) and np.allclose(per4[:3], want)
    assert miou_from_confusion(np.zeros((3, 3)))[0] == 0.0 and pixel_accuracy_from_confusion(np.zeros((3, 3))) == 0.0
    with pytest.raises(ValueError):
        miou_from_confusion(np.zeros((2, 3)))


def test_miou_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from util.metrics import confusion_matrix, miou_from_confusion
    rng = np.random.default_rng(3)
    K = 6                                            # class 4 occurs nowhere
    y_true = rng.choice([0, 1, 2, 3, 5], size=4000)
    y_pred = np.where(rng.random(4000) < 0.6, y_true, rng.choice([0, 1, 2, 3, 5], size=4000))
    miou, per = miou_from_confusion(confusion_matrix(y_true, y_pred, K))
    want = metrics.jaccard_score(y_true, y_pred, labels=list(range(K)), average=None, zero_division=0)
    assert np.isnan(per[4]) and want[4] == 0
    present = [0, 1, 2, 3, 5]
    assert np.allclose(per[present], want[present], rtol=0, atol=1e-12)
    assert abs(miou - want[present].mean()) < 1e-12


@pytest.mark.parametrize("G,p", [(1, 4), (2, 4), (3, 8), (4, 16), (14, 16), (3, 14)])
def test_reference_weights_and_footprints(G, p):
    W = R.axis_weights(G, p)
    assert torch.allclose(W.sum(1), torch.ones(G * p, dtype=torch.float64), rtol=0, atol=1e-15), "the weights of a pixel sum to 1"
    assert bool((W >= 0).all())
    for g in range(G):
        rows = torch.nonzero(W[:, g] > 0).reshape(-1)
        assert rows.numel() <= 2 * p, "a cell is read by at most 2 p positions of an axis"
        assert int(rows.min()) >= max(p * g - p // 2, 0) and int(rows.max()) < min(p * g + 3 * p // 2, G * p), "the footprint range the gather kernel walks"
    # ... and the rule is torch's: the separable weights reproduce interpolate() in fp64
    x = torch.randn(2, G, G, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(G * 100 + p))
    want = R.upsample(x, p)
    got = torch.einsum("yg,xh,nghk->nyxk", W, W, x)
    assert torch.allclose(got, want, rtol=0, atol=1e-13)
    # the adjoint is the transpose
    X = torch.randn(2, G * p, G * p, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    assert torch.allclose(R.adjoint(X, G, p), torch.einsum("yg,xh,nyxk->nghk", W, W, X), rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", R.CASES)
def test_gpu_case_seeds_keep_near_ties_under_the_cap(case):
    """Condition of the exact confusion-matrix check, verified from the reference alone: at most 0.1 % of a case's pixels have fp64 top-two logits
    closer than 1e-4."""
    N, G, p, K = case
    for pattern in ("random", "ignore30"):
        ref = R.ce_case_ref(N, G, p, K, pattern)
        share = float(ref["tie"].double().mean())
        assert share <= R.TIE_CAP, (case, pattern, share)
        assert int(ref["conf"].sum()) == ref["count"] - int((ref["tie"] & (R.case_inputs(N, G, p, K, pattern)[1] != R.IGNORE)).sum())


def test_reference_empty_batch_and_bounds_are_finite():
    ref = R.ce_case_ref(2, 2, 4, 5, "all_ignored")
    assert ref["count"] == 0 and float(ref["loss"]) == 0.0 and not bool(ref["dpl"].any()) and int(ref["conf"].sum()) == 0
    ref = R.ce_case_ref(2, 2, 4, 5, "ignore30")
    assert 0 < float(ref["b_loss"]) < 1e-4 and bool((ref["b_dpl"] > 0).all()) and float(ref["b_dpl"].max()) < 1e-4
    y, b = R.ln_ref(*R.ln_inputs(2, 5, 70, torch.float32))
    assert y.shape == (8, 70) and bool((b > 0).all()) and float(b.max()) < 1e-4


def _write_pair(root, stem, size=(20, 30), mask=True, ext=".png"):
    from PIL import Image
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "masks"), exist_ok=True)
    rng = np.random.default_rng(len(stem))
    Image.fromarray(rng.integers(0, 255, size=size + (3,), dtype=np.uint8)).save(os.path.join(root, "images", stem + ext))
    m = rng.integers(0, 4, size=size, dtype=np.uint8)
    m[0, 0] = 255
    if mask:
        Image.fromarray(m, mode="L").save(os.path.join(root, "masks", stem + ".png"))
    return m


def test_folder_dataset_pairs_stems_and_refuses_a_missing_mask(tmp_path):
    pytest.importorskip("PIL")
    import main_segprobe as M
    root = str(tmp_path / "ok")
    masks = {stem: _write_pair(root, stem, ext=ext) for stem, ext in (("b_tile", ".png"), ("a_tile", ".jpg"))}
    ds = M.SegFolderDataset(root)
    assert [os.path.basename(i) for i, _ in ds.pairs] == ["a_tile.jpg", "b_tile.png"]
    assert [os.path.basename(m) for _, m in ds.pairs] == ["a_tile.png", "b_tile.png"]
    img, mask = ds[1]
    assert img.dtype == torch.uint8 and img.shape == (20, 30, 3) and mask.dtype == torch.uint8 and np.array_equal(mask.numpy(), masks["b_tile"])
    bad = str(tmp_path / "bad")
    _write_pair(bad, "x")
    _write_pair(bad, "y", mask=False)
    with pytest.raises(FileNotFoundError, match="y.png"):
        M.SegFolderDataset(bad)
    with pytest.raises(FileNotFoundError):
        M.SegFolderDataset(str(tmp_path / "nowhere"))


def test_label_transform_follows_the_eval_geometry():
    import main_segprobe as M
    from util.gpu_input import eval_transform_params
    # identity geometry: a 256 x 256 mask at S = 224 is resized to 256 (crop_pct 224 / 256) and centre-cropped
    m = torch.arange(256 * 256, dtype=torch.int64).reshape(256, 256) % 251
    out = M.label_eval_transform(m.to(torch.uint8), 224)
    assert eval_transform_params(256, 256, 224)[2:6] == (256, 256, 16, 16)
    assert torch.equal(out, m[16:240, 16:240].to(torch.uint8))
    # a 2 x down-scale picks the pixel under each output centre; the ignore value survives (nearest neighbour: no blending)
    m = torch.full((64, 128), 255, dtype=torch.uint8)
    m[:, :64] = 3
    out = M.label_eval_transform(m, 28)                # resize to 32 x 64, crop 28 x 28 at (2, 18)
    assert out.shape == (28, 28) and set(out.unique().tolist()) <= {3, 255}
    assert bool((out[:, :14] == 3).all()) and bool((out[:, 14:] == 255).all())


def test_driver_parser():
    import main_segprobe as M
    a = M.get_args_parser().parse_args([])
    assert (a.model, a.input_size, a.patch_size, a.nb_classes, a.batch_size, a.blr, a.dataset_type) == ("vit_base_patch16", 224, 16, 6, 64, 0.1, "folder")
    assert a.finetune == "" and a.transform_checkpoint_keys is False and a.lr is None and a.eval is False
    a = M.get_args_parser().parse_args("--dataset_type synthetic --model vit_large_patch16 --finetune ck.pth --transform_checkpoint_keys --input_size 64 "
                                       "--nb_classes 9 --batch_size 8 --epochs 2 --blr 0.5 --train_path A --test_path B".split())
    assert (a.dataset_type, a.model, a.finetune, a.input_size, a.nb_classes, a.batch_size, a.epochs, a.blr, a.train_path, a.test_path) == \
        ("synthetic", "vit_large_patch16", "ck.pth", 64, 9, 8, 2, 0.5, "A", "B")
    assert a.transform_checkpoint_keys is True
    with pytest.raises(SystemExit):
        M.get_args_parser().parse_args(["--dataset_type", "rgb"])


def test_driver_refuses_multi_gpu(monkeypatch):
    import main_segprobe as M
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        M.main(M.get_args_parser().parse_args(["--dataset_type", "synthetic"]))


def test_seg_ops_refuse_cpu_tensors():
    from csmae_hip import ops
    pl, labels = torch.zeros(1, 2, 2, 3), torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_ce(pl, labels, torch.zeros(1), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_token_norm(torch.zeros(1, 5, 8), torch.ones(8), torch.zeros(8), torch.zeros(4, 8))


def test_probe_refuses_what_the_kernels_do_not_hold():
    import models_seg
    import models_vit
    vit = models_vit.vit_base_patch16(img_size=32, patch_size=16, embed_dim=32, depth=1, num_heads=2, num_classes=2)
    with pytest.raises(NotImplementedError, match="ignore_index"):
        models_seg.LinearSegProbe(vit, 4, ignore_index=0)
    with pytest.raises(ValueError, match="num_classes"):
        models_seg.LinearSegProbe(vit, 65)
    probe = models_seg.LinearSegProbe(vit, 4)
    assert [n for n, p in probe.named_parameters() if p.requires_grad] == ["linear.weight", "linear.bias"]
    with pytest.raises(RuntimeError, match="no CPU fallback|only on an MI355X"):
        probe(torch.zeros(2, 3, 32, 32), torch.zeros(2, 32, 32, dtype=torch.uint8))


def test_every_new_header_function_is_bound():
    import csmae_hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csmae.h")).read(), flags=re.S)
    seg = re.findall(r"int\s+(csmae_seg_\w+)\s*\(", text)
    assert sorted(seg) == ["csmae_seg_ce", "csmae_seg_ce_bwd", "csmae_seg_token_norm"]
    for name in seg:
        assert name in csmae_hip._SIGNATURES and name in csmae_hip._ADDED_WITHIN_ABI, name
    assert re.search(r"^#define\s+CSMAE_SEG_IGNORE\s+255\s*$", text, flags=re.M) and csmae_hip.SEG_IGNORE == 255
    lib = csmae_hip.load()
    for name in seg:
        assert hasattr(lib, name)
