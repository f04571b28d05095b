"""The command lines of the four downstream drivers, which are assembled from the flag groups of util/downstream.py.

DEFAULTS was produced by the parsers of the commit BEFORE the drivers were rewritten onto those groups (each driver then carried its own copy
of the flag table), not by the parsers under test: `vars(get_args_parser().parse_args([]))`, pasted.  `local_rank` of main_finetune.py comes
from the environment variable LOCAL_RANK and is normalised to its value without that variable.  No kernel is launched."""
import importlib

import pytest

RGB = dict(train_path="./train_64.csv", test_path="/data2/HDD_16TB/fmow-rgb-preproc/val_224.csvv", dataset_type="rgb", masked_bands=None, dropped_bands=None,
           nb_classes=62, input_channels=None)
RUN = dict(output_dir=None, output_dir_base="./out", device="cuda:0", seed=0, num_workers=10, synthetic_len=64)
MODEL = dict(model="vit_base_patch16", patch_size=16, embed_dim=None, depth=None, num_heads=None, finetune="", transform_checkpoint_keys=False)
SCHEDULE = dict(accum_iter=1, lr=None, resume=None, save_every=1, start_epoch=0, eval=False, print_freq=20)

DEFAULTS = dict(
    main_linprobe=dict(batch_size=512, epochs=50, input_size=224, weight_decay=0.0, blr=0.1, min_lr=0.0, warmup_epochs=10, global_pool=False,
                       **MODEL, **SCHEDULE, **RGB, **RUN),
    main_finetune=dict(batch_size=512, epochs=100, model_type=None, input_size=128, drop_path=0.0, clip_grad=None, weight_decay=0.05, blr=0.001, layer_decay=0.75,
                       min_lr=1e-06, warmup_epochs=5, color_jitter=None, aa="rand-m9-mstd0.5-inc1", smoothing=0.1, reprob=0.25, remode="pixel", recount=1,
                       resplit=False, mixup=0.8, cutmix=1.0, cutmix_minmax=None, mixup_prob=1.0, mixup_switch_prob=0.5, mixup_mode="batch", use_psa=False,
                       global_pool=True, val_img_path="./images/", log_dir="./output_dir", wandb_entity="utk-iccv23", wandb_project=None, wandb_id=None,
                       dist_eval=False, pin_mem=True, world_size=1, local_rank=0, dist_on_itp=False, dist_url="env://", **MODEL, **SCHEDULE, **RGB, **RUN),
    main_knn=dict(batch_size=512, input_size=224, global_pool=False, knn_k=20, knn_t=0.07, knn_scales=[1.0, 0.5, 0.25, 0.125], bank_max=None, knn_dtype="bf16",
                  **MODEL, **RGB, **RUN),
    main_segprobe=dict(batch_size=64, epochs=50, input_size=224, weight_decay=0.0, blr=0.1, min_lr=0.0, warmup_epochs=0, train_path="./seg/train",
                       test_path="./seg/val", dataset_type="folder", nb_classes=6, **MODEL, **SCHEDULE, **RUN),
)

# one line per driver that touches every shared group the driver has: model geometry, checkpoint, pooling, data, run / output, schedule
LINES = dict(
    main_linprobe=("--global_pool --dataset_type synthetic --dropped_bands 0 9 --resume  --embed_dim 128 --lr 0.5 --finetune ck.pth --transform_checkpoint_keys --seed 3 --epochs 2",
                   dict(global_pool=True, dataset_type="synthetic", dropped_bands=[0, 9], resume=None, embed_dim=128, lr=0.5, finetune="ck.pth",
                        transform_checkpoint_keys=True, seed=3, epochs=2)),
    main_finetune=("--cls_token --dataset_type synthetic --dropped_bands 0 9 --resume  --embed_dim 128 --lr 0.5 --finetune ck.pth --transform_checkpoint_keys --seed 3 --epochs 2",
                   dict(global_pool=False, dataset_type="synthetic", dropped_bands=[0, 9], resume=None, embed_dim=128, lr=0.5, finetune="ck.pth",
                        transform_checkpoint_keys=True, seed=3, epochs=2)),
    main_knn=("--global_pool --dataset_type synthetic --dropped_bands 0 9 --embed_dim 128 --finetune ck.pth --transform_checkpoint_keys --seed 3 --batch_size 8",
              dict(global_pool=True, dataset_type="synthetic", dropped_bands=[0, 9], embed_dim=128, finetune="ck.pth", transform_checkpoint_keys=True, seed=3,
                   batch_size=8)),
    main_segprobe=("--dataset_type synthetic --resume  --embed_dim 128 --lr 0.5 --finetune ck.pth --transform_checkpoint_keys --seed 3 --epochs 2 --input_size 64",
                   dict(dataset_type="synthetic", resume=None, embed_dim=128, lr=0.5, finetune="ck.pth", transform_checkpoint_keys=True, seed=3, epochs=2,
                        input_size=64)),
)


def typed(namespace):
    """{flag: (value, type)}: 1 == 1.0 == True in Python, so equal values alone would let a flag's type drift"""
    return {k: (v, type(v)) for k, v in namespace.items()}


@pytest.mark.parametrize("driver", sorted(DEFAULTS))
def test_default_namespace_is_the_one_before_the_shared_flag_table(driver, monkeypatch):
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    p = importlib.import_module(driver).get_args_parser()
    assert p.add_help is False
    assert typed(vars(p.parse_args([]))) == typed(DEFAULTS[driver])


@pytest.mark.parametrize("driver", sorted(LINES))
def test_a_line_through_every_shared_group(driver, monkeypatch):
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    line, changed = LINES[driver]
    got = vars(importlib.import_module(driver).get_args_parser().parse_args(line.split(" ")))   # ("--resume", "": the empty string means none)
    assert typed(got) == typed({**DEFAULTS[driver], **changed})
