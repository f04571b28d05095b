"""CPU-side checks of the linear-probe surface: command line, parameter names against the checkpoint key mapping, probe head,
and the refusals (no CPU fallback, no multi-GPU probing).  No kernel is launched."""
import pytest
import torch

MICRO = dict(dim_model=128, encoder_num_layers=2, encoder_num_heads=2, decoder_embed_dim=64, decoder_num_layers=2, decoder_num_heads=2)
VIT_MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2)

# main_linprobe.py:64-356 of the reference, the flags kept here (--model aside: its reference default names no models_vit factory)
REFERENCE_DEFAULTS = dict(batch_size=512, epochs=50, accum_iter=1, input_size=224, patch_size=16, weight_decay=0.0, lr=None, blr=0.1, min_lr=0.0,
                          warmup_epochs=10, finetune="", global_pool=False, nb_classes=62, dataset_type="rgb", output_dir=None, output_dir_base="./out",
                          device="cuda:0", seed=0, resume=None, save_every=1, start_epoch=0, eval=False, transform_checkpoint_keys=False)


def test_cli_parses_the_reference_defaults():
    import main_linprobe
    import models_vit
    p = main_linprobe.get_args_parser()
    args = p.parse_args([])
    for k, v in REFERENCE_DEFAULTS.items():
        assert getattr(args, k) == v, (k, getattr(args, k), v)
    assert args.model in models_vit.__dict__
    assert p.parse_args(["--global_pool"]).global_pool is True and p.parse_args(["--global_pool", "--cls_token"]).global_pool is False
    assert p.parse_args(["--resume", ""]).resume is None
    a = p.parse_args(["--dataset_type", "synthetic", "--lr", "0.5", "--eval"])
    assert a.dataset_type == "synthetic" and a.lr == 0.5 and a.eval is True


@pytest.mark.parametrize("global_pool", [False, True])
def test_factory_keys_match_the_checkpoint_mapping(global_pool):
    import models_mae
    import models_vit
    from util.checkpoint_keys import to_vit_keys
    pre = models_mae.MAE_ViT_MsLdCeCd(**MICRO, input_size=64, patch_size="16", predictor_hidden_size=128)
    mapped = to_vit_keys(pre.state_dict())
    vit = models_vit.vit_base_patch16(num_classes=5, global_pool=global_pool, in_chans=3, **VIT_MICRO)
    own = vit.state_dict()
    norm = "fc_norm" if global_pool else "norm"
    assert set(own) == (set(mapped) - {"norm.weight", "norm.bias"}) | {f"{norm}.weight", f"{norm}.bias", "head.weight", "head.bias"}
    for k, v in mapped.items():
        if k in own:
            assert own[k].shape == v.shape, k
    assert own["head.weight"].shape == (5, 128) and own[f"{norm}.weight"].shape == (128,)
    msg = vit.load_state_dict(mapped, strict=False)
    assert set(msg.missing_keys) == {"head.weight", "head.bias"} | ({"fc_norm.weight", "fc_norm.bias"} if global_pool else set())
    assert torch.equal(vit.pos_embed, pre.encoder_pos_embed)   # both are the sin-cos table
    # the full-size factories carry the reference's geometry
    for name, (D, depth, heads) in dict(vit_base_patch16=(768, 12, 12), vit_large_patch16=(1024, 24, 16), vit_huge_patch14=(1280, 32, 16)).items():
        m = models_vit.__dict__[name](depth=1, img_size=28, patch_size=14, num_classes=2)
        assert (m.embed_dim, m.num_heads) == (D, heads) and m.head.weight.shape == (2, D)
    assert len(models_vit.vit_base_patch16(img_size=32, num_classes=2).blocks) == 12


def test_probe_mode_head_and_frozen_trunk():
    import models_vit
    torch.manual_seed(0)
    vit = models_vit.vit_base_patch16(num_classes=62, global_pool=True, **VIT_MICRO).probe_mode()
    assert isinstance(vit.head[0], torch.nn.BatchNorm1d) and vit.head[0].affine is False and vit.head[0].eps == 1e-6
    w = vit.head[1].weight.detach()
    assert w.shape == (62, 128) and abs(float(w.std()) / 2e-5 - 1) < 0.05 and float(vit.head[1].bias.abs().max()) == 0   # trunc_normal_(std=2e-5) over 7936 draws
    assert sorted(n for n, p in vit.named_parameters() if p.requires_grad) == ["head.1.bias", "head.1.weight"]
    assert {"head.0.running_mean", "head.0.running_var", "head.0.num_batches_tracked", "head.1.weight", "head.1.bias"} <= set(vit.state_dict())


def test_model_and_lars_refuse_cpu_tensors():
    import models_vit
    from util.lars import LARS
    vit = models_vit.vit_base_patch16(num_classes=3, **VIT_MICRO).probe_mode()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vit(torch.zeros(2, 3, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vit(torch.zeros(2, 3, 64, 64), torch.zeros(2, dtype=torch.long))
    p = torch.nn.Parameter(torch.ones(3, 4))
    p.grad = torch.ones(3, 4)
    opt = LARS([p], lr=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(3, 4))
    assert opt.defaults == dict(lr=0.1, weight_decay=0, momentum=0.9, trust_coefficient=0.001)


def test_trunk_gradients_and_multi_gpu_are_refused(monkeypatch):
    import main_linprobe
    import models_vit
    vit = models_vit.vit_base_patch16(num_classes=3, **VIT_MICRO)   # not in probe mode: the trunk asks for gradients
    with pytest.raises(NotImplementedError, match="only the head is trainable"):
        vit(torch.zeros(2, 3, 64, 64), torch.zeros(2, dtype=torch.long))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        main_linprobe.main(main_linprobe.get_args_parser().parse_args(["--dataset_type", "synthetic"]))
