"""CPU-side checks of the fine-tuning surface: Mixup's host draws against timm 0.4.12's order and box arithmetic (restated in
finetune_ref.py), the dense-target algebra, layer-wise learning-rate decay groups, F1 from the confusion matrix, the command line, and the
refusals.  No kernel is launched."""
import numpy as np
import pytest
import torch

import finetune_ref as R
from finetune_ref import VIT_MICRO

# main_finetune.py:85-443 of the reference.  Two deliberate differences: --model (the reference's default names no models_vit factory) is left
# out, and --drop_path is 0.0 here (reference: 0.1) because drop-path is not implemented and a value above 0 raises.
REFERENCE_DEFAULTS = dict(
    batch_size=512, epochs=100, accum_iter=1, model_type=None, input_size=128, patch_size=16, clip_grad=None, weight_decay=0.05, lr=None, blr=1e-3,
    layer_decay=0.75, min_lr=1e-6, warmup_epochs=5, color_jitter=None, aa="rand-m9-mstd0.5-inc1", smoothing=0.1, reprob=0.25, remode="pixel", recount=1,
    resplit=False, mixup=0.8, cutmix=1.0, cutmix_minmax=None, mixup_prob=1.0, mixup_switch_prob=0.5, mixup_mode="batch", finetune="", use_psa=False,
    global_pool=True, train_path="./train_64.csv", test_path="/data2/HDD_16TB/fmow-rgb-preproc/val_224.csvv", dataset_type="rgb", masked_bands=None,
    dropped_bands=None, nb_classes=62, output_dir=None, output_dir_base="./out", val_img_path="./images/", log_dir="./output_dir", device="cuda:0", seed=0,
    resume=None, save_every=1, wandb_entity="utk-iccv23", wandb_project=None, wandb_id=None, start_epoch=0, eval=False, dist_eval=False, num_workers=10,
    pin_mem=True, world_size=1, dist_on_itp=False, dist_url="env://", transform_checkpoint_keys=False)
DROP_PATH_HERE = 0.0


def test_cli_parses_the_reference_defaults():
    import main_finetune
    import models_vit
    p = main_finetune.get_args_parser()
    args = p.parse_args([])
    for k, v in REFERENCE_DEFAULTS.items():
        assert getattr(args, k) == v, (k, getattr(args, k), v)
    assert args.drop_path == DROP_PATH_HERE and args.model in models_vit.__dict__ and int(args.local_rank) == 0
    assert p.parse_args(["--cls_token"]).global_pool is False and p.parse_args(["--resume", ""]).resume is None
    a = p.parse_args(["--dataset_type", "synthetic", "--cutmix_minmax", "0.2", "0.8", "--no_pin_mem", "--layer_decay", "0.65"])
    assert a.dataset_type == "synthetic" and a.cutmix_minmax == [0.2, 0.8] and a.pin_mem is False and a.layer_decay == 0.65


@pytest.mark.parametrize("alphas", [(0.8, 1.0), (0.8, 0.0), (0.0, 1.0)])
def test_mixup_draws_follow_timm_order(alphas):
    from util.mixup import Mixup
    shape = (8, 3, 30, 46)
    for prob, switch in ((1.0, 0.5), (0.6, 0.3)):
        m = Mixup(mixup_alpha=alphas[0], cutmix_alpha=alphas[1], prob=prob, switch_prob=switch, label_smoothing=0.1, num_classes=7)
        np.random.seed(1234)
        got = [m.params_per_batch(shape) for _ in range(40)]
        tail = np.random.rand()   # the generator must have advanced by exactly the same number of draws
        np.random.seed(1234)
        want = [R.timm_params_per_batch(shape, alphas[0], alphas[1], prob, switch) for _ in range(40)]
        assert got == want and tail == np.random.rand()
        assert any(b is not None for _, b in got) == (alphas[1] > 0) and any(b is None and lam < 1 for lam, b in got) == (alphas[0] > 0)


def test_cutmix_box_edges(monkeypatch):
    from util.mixup import Mixup, rand_bbox
    H, W = 30, 46

    def centre(cy, cx):
        draws = iter([cy, cx])
        monkeypatch.setattr(np.random, "randint", lambda lo, hi: next(draws))   # row first, then column

    for lam, cy, cx in ((1e-9, 15, 23), (1.0 - 1e-12, 15, 23), (0.5, 0, 0), (0.5, H - 1, W - 1), (0.3, 2, 44), (0.75, 29, 1)):
        centre(cy, cx)
        got = rand_bbox((3, H, W), lam)
        centre(cy, cx)
        want = tuple(int(v) for v in R.timm_rand_bbox((3, H, W), lam))
        assert got == want and all(isinstance(v, int) for v in got), (lam, cy, cx, got, want)
        yl, yh, xl, xh = got
        assert 0 <= yl <= yh <= H and 0 <= xl <= xh <= W
    centre(15, 23)
    assert rand_bbox((3, H, W), 1e-9) == (1, 29, 1, 45)               # lam -> 0: cut = int(size * 0.99..) = size - 1
    centre(15, 23)
    yl, yh, xl, xh = rand_bbox((3, H, W), 1.0 - 1e-12)                # lam -> 1: an empty box, the corrected lam is exactly 1
    assert (yh - yl) * (xh - xl) == 0
    centre(0, 0)
    assert rand_bbox((3, H, W), 0.5) == (0, 10, 0, 16)                # clipped at the top-left corner: cut = (21, 32), half = (10, 16)
    m = Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, num_classes=5)
    monkeypatch.setattr(np.random, "rand", lambda: 0.0)
    monkeypatch.setattr(np.random, "beta", lambda a, b: 0.5)
    centre(0, 0)
    lam, box = m.params_per_batch((2, 3, H, W))
    assert box == (0, 10, 0, 16) and lam == 1.0 - 160.0 / (H * W)


def test_mixup_refuses_what_is_not_implemented():
    from util.mixup import Mixup
    for kw in (dict(mode="elem"), dict(mode="pair"), dict(cutmix_minmax=(0.2, 0.8))):
        with pytest.raises(NotImplementedError):
            Mixup(**kw)
    m = Mixup(num_classes=5)
    with pytest.raises(ValueError, match="even"):
        m(torch.zeros(3, 3, 16, 16), torch.zeros(3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 16, 16), torch.zeros(2, dtype=torch.long))


def test_mixup_target_algebra():
    y = torch.tensor([0, 4, 2, 2, 1, 3])
    for K in (5, 62):
        for lam in (0.0, 0.3, 1.0):
            for s in (0.0, 0.1):
                t = R.mixup_target_ref(y, K, lam, s)
                assert torch.allclose(t.sum(1), torch.ones(6, dtype=torch.float64), atol=1e-14)
                assert torch.allclose(t, lam * R.mixup_target_ref(y, K, 1.0, s) + (1 - lam) * R.mixup_target_ref(y.flip(0), K, 1.0, s), atol=1e-15)
        smooth = R.mixup_target_ref(y, K, 1.0, 0.1)   # lam = 1: plain label smoothing, whose soft cross-entropy is LabelSmoothingCrossEntropy
        assert torch.allclose(smooth, 0.9 * torch.nn.functional.one_hot(y, K).double() + 0.1 / K, atol=1e-15)
        logits = R.rnd(6, K, seed=K).double()
        want = torch.nn.functional.cross_entropy(logits, y, label_smoothing=0.1)
        assert abs(float(R.soft_ce_ref(logits, smooth)) - float(want)) < 1e-12
        assert abs(float(R.soft_ce_ref(logits, R.mixup_target_ref(y, K))) - float(torch.nn.functional.cross_entropy(logits, y))) < 1e-12


def test_layer_decay_groups_on_the_micro_vit():
    import models_vit
    import util.lr_decay as lrd
    vit = models_vit.vit_base_patch16(num_classes=5, global_pool=True, **VIT_MICRO).finetune_mode()
    assert vit.no_weight_decay() == {"pos_embed", "cls_token"} and all(p.requires_grad for p in vit.parameters())
    L = len(vit.blocks) + 1
    groups = lrd.param_groups_lrd(vit, 0.05, no_weight_decay_list=vit.no_weight_decay(), layer_decay=0.75)
    names = lrd.param_group_names_lrd(vit, 0.05, no_weight_decay_list=vit.no_weight_decay(), layer_decay=0.75)
    assert names == [f"layer_{i}_{d}" for i in range(L + 1) for d in ("no_decay", "decay")] and len(groups) == 2 * (len(vit.blocks) + 2)
    by_id = {id(p): n for n, p in vit.named_parameters()}
    seen = []
    for name, g in zip(names, groups):
        layer = int(name.split("_")[1])
        assert g["lr_scale"] == 0.75 ** (L - layer) and g["weight_decay"] == (0.0 if name.endswith("no_decay") else 0.05)
        for p in g["params"]:
            n = by_id[id(p)]
            seen.append(n)
            assert lrd.get_layer_id_for_vit(n, L) == layer
            assert (p.ndim == 1 or n in ("pos_embed", "cls_token")) == name.endswith("no_decay"), n
    assert sorted(seen) == sorted(by_id.values())
    first = [by_id[id(p)] for p in groups[0]["params"]]
    assert {"pos_embed", "cls_token", "patch_embed.proj.bias"} == set(first) and [by_id[id(p)] for p in groups[1]["params"]] == ["patch_embed.proj.weight"]
    assert {by_id[id(p)] for p in groups[-2]["params"] + groups[-1]["params"]} == {"fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"}
    assert [lrd.get_layer_id_for_vit(n, 13) for n in ("cls_token", "pos_embed", "patch_embed.proj.weight", "blocks.0.norm1.weight", "blocks.11.mlp.fc2.bias",
                                                      "norm.weight", "fc_norm.bias", "head.weight")] == [0, 0, 0, 1, 12, 13, 13, 13]
    # FusedAdamW takes the groups as they are (binding to the flat buffer needs the GPU)
    from csmae_hip.optim import FusedAdamW
    opt = FusedAdamW(groups, lr=1e-3)
    assert len(opt.param_groups) == 8 and opt.param_groups[0]["lr_scale"] == 0.75 ** 3


def test_f1_from_the_confusion_matrix_matches_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from util.metrics import confusion_matrix, f1_scores
    rng = np.random.default_rng(0)
    for K, n in ((2, 40), (5, 64), (62, 300)):
        y, pred = rng.integers(0, K, n), rng.integers(0, K + 1, n)   # (a predicted class that never occurs in y_true, classes that never occur at all)
        macro, micro, per_class = f1_scores(y, pred)
        assert abs(macro - metrics.f1_score(y, pred, average="macro")) < 1e-12 and abs(micro - metrics.f1_score(y, pred, average="micro")) < 1e-12
        np.testing.assert_allclose(per_class, metrics.f1_score(y, pred, average=None), atol=1e-12)
        np.testing.assert_array_equal(confusion_matrix(y, pred, K + 1), metrics.confusion_matrix(y, pred, labels=list(range(K + 1))))
    assert f1_scores([1, 1], [1, 1])[:2] == (1.0, 1.0)


def test_refusals(monkeypatch):
    import main_finetune
    import models_vit
    vit = models_vit.vit_base_patch16(num_classes=3, **VIT_MICRO).finetune_mode()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vit(torch.zeros(2, 3, 64, 64), torch.zeros(2, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vit(torch.zeros(2, 3, 64, 64), torch.full((2, 3), 1 / 3))
    for kw in (dict(drop_path_rate=0.1), dict(drop_rate=0.1), dict(attn_drop_rate=0.1)):
        with pytest.raises(NotImplementedError):
            models_vit.vit_base_patch16(num_classes=3, **VIT_MICRO, **kw)
    with pytest.raises(RuntimeError, match="probe mode"):
        models_vit.vit_base_patch16(num_classes=3, **VIT_MICRO).probe_mode().finetune_mode()
    parse = main_finetune.get_args_parser().parse_args
    with pytest.raises(NotImplementedError, match="drop_path"):
        main_finetune.main(parse(["--dataset_type", "synthetic", "--drop_path", "0.1"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        main_finetune.main(parse(["--dataset_type", "synthetic"]))
